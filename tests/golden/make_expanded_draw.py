#!/usr/bin/env python3
"""Regenerates tests/golden/proofs_expanded_draw.json: proofs under the EXPANDED blinding draw (include/bbp.h bbp_set_blinding_draw)
from the big-int oracle with tests/expanded_draw_model.py in place of its transcript, under FIXED entropy.  An offline step: one proof
takes about 20 s.  Usage:  python tests/golden/make_expanded_draw.py

The N = 1 and N = 8 cases take the inputs of proofs_full.json (make_golden.py's full_n1 / full_n8), so their commitments can be compared
with the merlin-draw records of the same inputs; the second and third N = 8 cases differ in their entropy alone.  N = 202 is the list
length at which the circuit has 2048 multipliers: no padding, 4099 draws."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_golden import stream  # noqa: E402
from oracle.ref_py import blindbid as bb, ristretto as rs  # noqa: E402
from tests import expanded_draw_model as model  # noqa: E402

CASES = (("xd_n1", "full_n1", 1, 0, b"/ent"), ("xd_n8_a", "full_n8", 8, 3, b"/ent"), ("xd_n8_b", "full_n8", 8, 3, b"/xd-ent-b"),
         ("xd_n8_c", "full_n8", 8, 3, b"/xd-ent-c"), ("xd_n202", "xd_n202", 202, 117, b"/ent"))


def inputs(src, N, toggle, ent_tag):
    """make_golden.case's inputs for the name `src`, the entropy from `ent_tag`"""
    s = src.encode()
    d = int.from_bytes(stream(s + b"/d", 8), "little")
    k = rs.sc_wide(stream(s + b"/k", 64))
    seed = rs.sc_wide(stream(s + b"/seed", 64))
    w = bb.witness(d, k, seed)
    pub = [rs.sc_wide(stream(s + b"/pub%d" % i, 64)) for i in range(N)]
    pub[toggle] = w["x"]
    ent = stream(s + ent_tag, 32 * (4 + N) + 32)
    ent = b"".join(rs.sc_bytes(rs.sc_wide(ent[32 * i:32 * i + 32] + bytes(32))) for i in range(4 + N)) + ent[32 * (4 + N):]
    return d, k, seed, w, pub, ent


def prove_expanded(d, k, seed, w, pub, toggle, ent):
    """the record and the draw key of the EXPANDED prover"""
    made = []

    def new_transcript():
        made.append(model.ExpandedDrawTranscript())
        return made[-1]

    old, bb.new_transcript = bb.new_transcript, new_transcript
    try:
        pr = bb.prove(d, k, w["y"], w["y_inv"], w["q"], w["z_img"], seed, pub, toggle, ent)
    finally:
        bb.new_transcript = old
    return pr.to_record(), made[-1].last_rng.key


def case(name, src, N, toggle, ent_tag):
    d, k, seed, w, pub, ent = inputs(src, N, toggle, ent_tag)
    t0 = time.time()
    rec, key = prove_expanded(d, k, seed, w, pub, toggle, ent)
    t1 = time.time()
    assert bb.verify(bb.Proof.from_record(rec, N), w["q"], w["z_img"], seed, pub, bytes(32))
    print(name, "prove %.1fs verify %.1fs" % (t1 - t0, time.time() - t1), flush=True)
    sc = lambda v: rs.sc_bytes(v).hex()
    return dict(name=name, inputs_of=src, N=N, toggle=toggle, n_mul=model.n_mul_of(N), d=sc(d), k=sc(k), seed=sc(seed), y=sc(w["y"]), y_inv=sc(w["y_inv"]),
                q=sc(w["q"]), z_img=sc(w["z_img"]), pub_list=[sc(p) for p in pub], entropy=ent.hex(), draw_key=key.hex(), record=rec.hex())


def main():
    out = {"expanded_draw": [case(*c) for c in CASES]}
    json.dump(out, open(os.path.join(HERE, "proofs_expanded_draw.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
