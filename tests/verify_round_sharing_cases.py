"""Shared by tests/test_gpu_verify_round_sharing.py and its child process: the rounds the tests verify against, and the child that
runs bursts with round sharing on in an environment of its own (e.g. BBP_VERIFY_AGGREGATE).  A request is (record, score, z_img, seed,
pub_list), as in tests/verify_combine_cases.py."""
import hashlib
import json
import sys

from tests.verify_combine_cases import burst, from_json

L = 2 ** 252 + 27742317777372353535851937790883648493


def _h(tag, *ids):
    return hashlib.sha512(b"bbp-round-sharing-v1" + b"".join(i.to_bytes(8, "little") for i in ids) + tag).digest()


def _sc(b64):
    return (int.from_bytes(b64, "little") % L).to_bytes(32, "little")


def seed_of(rid):
    return _sc(_h(b"seed", rid))


class Round:
    """One round: seed, bid list and `k` valid requests (bids at list positions 0..k-1), proved by the engine under fixed entropy.
    `like`: take that round's bids, and its seed and the other list items unless `seed` / `patch` say otherwise -- patch = (item, byte,
    xor) changes one raw byte of a list item that is no bid's own."""

    def __init__(self, ctx, oc, bbp, rid, N, k=3, like=None, seed=None, patch=None):
        src = like.rid if like else rid
        self.rid, self.N = rid, N
        self.seed = seed if seed is not None else like.seed if like else seed_of(rid)
        k = min(N, k)
        pub = [_sc(_h(b"pub", src, j)) for j in range(N)]
        wit = []
        for i in range(k):
            d, kk = _h(b"d", src, i)[:8] + bytes(24), _sc(_h(b"k", src, i))
            w = oc.witness(d + kk + self.seed)
            m, x, y, yi, q, z = [w[32 * j:32 * j + 32] for j in range(6)]
            pub[i] = x
            wit.append((d, kk, y, yi, q, z))
        if patch:
            item, byte, xor = patch
            assert item >= k
            b = bytearray(pub[item])
            b[byte] ^= xor
            pub[item] = bytes(b)
        self.pub = b"".join(pub)
        ins = b"".join(d + kk + y + yi + q + z + self.seed + self.pub + i.to_bytes(8, "little") for i, (d, kk, y, yi, q, z) in enumerate(wit))
        ents = b"".join(b"".join(_sc(_h(b"ent", rid, i, j)) for j in range(4 + N)) + _h(b"es", rid, i)[:32] for i in range(k))
        out, st = ctx.prove_batch(k, N, ins, ents)
        assert st == [0] * k
        rsz = bbp.record_size(N)
        self.reqs = [(out[i * rsz:(i + 1) * rsz], wit[i][4], wit[i][5], self.seed, self.pub) for i in range(k)]

    def req(self, i=0):
        return self.reqs[i % len(self.reqs)]


def with_round(req, other):
    """req's proof, score and z_img against another round's seed and list"""
    return req[:3] + (other[3], other[4])


def child_main(path_in, path_out):
    """Child process of the GPU tests (its environment carries what the test is about): one context, a 100 ms window, round sharing on,
    every burst of the input file; writes statuses, the sharing counters after each burst and the engine's description."""
    try:
        import torch  # noqa: F401  (its HIP runtime first: tests/conftest.py)
    except ImportError:
        pass
    import dusk_blindbidproof_amd as bbp
    job = json.load(open(path_in))
    c = bbp.Context(0)
    c.set_batching(100000, 4096)
    c.set_verify_round_sharing(True)
    res = []
    for rows in job["bursts"]:
        before = c.verify_round_sharing_stats()
        st = burst(c, from_json(rows))
        after = c.verify_round_sharing_stats()
        res.append({"status": st, "shared": [a - b for a, b in zip(after, before)]})
    json.dump({"bursts": res, "describe": c.describe(), "health": c.health()}, open(path_out, "w"))
    c.close()


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2])
