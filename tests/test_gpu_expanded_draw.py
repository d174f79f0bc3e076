"""GPU tier: the EXPANDED blinding draw (include/bbp.h bbp_set_blinding_draw) through every prove entry point, against the records of
tests/golden/proofs_expanded_draw.json (the big-int oracle under tests/expanded_draw_model.py).  A proof's draw key depends on its
transcript, blindings and seed, never on its row index, so a batch whose rows cycle over the fixture cases must return the fixture
records in that order whatever its size, path or schedule.  Back under MERLIN the same context returns the C oracle's bytes."""
import os
import re
import signal
import subprocess
import tempfile
import time

import pytest

from tests import oracle_c, uds_client as uc

pytestmark = pytest.mark.gpu
KEY = bytes((0xA7 ^ (3 * i)) & 0xFF for i in range(32))


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


class Case:
    def __init__(self, c):
        h = lambda k: bytes.fromhex(c[k])
        self.name, self.N, self.toggle = c["name"], c["N"], c["toggle"]
        self.s7 = b"".join(h(k) for k in ["d", "k", "y", "y_inv", "q", "z_img", "seed"])
        self.pub = b"".join(bytes.fromhex(p) for p in c["pub_list"])
        self.row = self.s7 + self.pub + self.toggle.to_bytes(8, "little")
        self.ent, self.record = h("entropy"), h("record")
        self.tail = h("q") + h("z_img") + h("seed") + self.pub  # what follows a record in a verify row
        self.d, self.k, self.seed = h("d"), h("k"), h("seed")


@pytest.fixture(scope="module")
def cases(golden):
    cs = [Case(c) for c in golden("proofs_expanded_draw.json")["expanded_draw"]]
    return {1: cs[:1], 8: cs[1:4], 202: cs[4:]}


@pytest.fixture(scope="module")
def xctx(ctx, bbp):
    """this module's context, EXPANDED (after `ctx`, so torch's HIP runtime is initialised first); a test that changes the mode puts it back"""
    c = bbp.Context(0)
    assert c.blinding_draw() == bbp.BLINDING_DRAW_MERLIN and "blinding draw: merlin" in c.describe()
    c.set_blinding_draw("expanded")
    assert c.blinding_draw() == bbp.BLINDING_DRAW_EXPANDED and "blinding draw: expanded" in c.describe()
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


def _batch(cs, B):
    """B rows cycling over the cases cs: (inputs, entropy, expected records, verify rows)"""
    pick = [cs[i % len(cs)] for i in range(B)]
    return (b"".join(c.row for c in pick), b"".join(c.ent for c in pick), b"".join(c.record for c in pick),
            b"".join(c.record + c.tail for c in pick))


def _first_diff(got, want, rs_):
    return next((i for i in range(len(want) // rs_) if got[i * rs_:(i + 1) * rs_] != want[i * rs_:(i + 1) * rs_]), None)


def test_setter_refuses_other_modes(xctx, bbp):
    for mode in (2, -1, 7):
        with pytest.raises(bbp.BbpError) as e:
            xctx.set_blinding_draw(mode)
        assert e.value.status == 4 and xctx.blinding_draw() == bbp.BLINDING_DRAW_EXPANDED
    with pytest.raises(ValueError):
        xctx.set_blinding_draw("chacha")


@pytest.mark.parametrize("N", [1, 8, 202])
def test_one_proof_bytes_and_back_to_merlin(xctx, oc, cases, N):
    for c in cases[N]:
        assert xctx.prove(c.s7, c.pub, c.toggle, c.ent) == c.record, c.name  # one proof: the wavefront-per-proof prefix
    c = cases[N][0]
    xctx.set_blinding_draw("merlin")
    try:
        rc, want = oc.prove(c.s7, c.pub, c.toggle, c.ent)
        assert rc == 0 and xctx.prove(c.s7, c.pub, c.toggle, c.ent) == want != c.record
    finally:
        xctx.set_blinding_draw("expanded")
    assert xctx.prove(c.s7, c.pub, c.toggle, c.ent) == c.record


@pytest.mark.parametrize("N,B", [(8, 33), (8, 130), (202, 3)], ids=["lane-prefix-partial-wave", "sliced", "n202"])
def test_batches_give_the_fixture_records(xctx, oc, bbp, cases, N, B):
    ins, ents, want, vin = _batch(cases[N], B)
    out, st = xctx.prove_batch(B, N, ins, ents)
    assert st == [0] * B and _first_diff(out, want, bbp.record_size(N)) is None
    assert xctx.verify_batch(B, N, vin) == [0] * B
    assert oc.verify_many(vin, B, N, threads=8) == [0] * B


def test_no_plan_threshold_leaks_in(bbp, cases, capfd):
    """B = 769, one above rng_coop_below, where MERLIN takes the pair chain"""
    N, B = 8, 769
    os.environ["BBP_TRACE_PROVE"] = "1"
    try:
        c = bbp.Context(0)
    finally:
        del os.environ["BBP_TRACE_PROVE"]
    try:
        c.set_blinding_draw(bbp.BLINDING_DRAW_EXPANDED)
        ins, ents, want, vin = _batch(cases[N], B)
        capfd.readouterr()
        out, st = c.prove_batch(B, N, ins, ents)
        lines = [l for l in capfd.readouterr().err.split("\n") if l.startswith("prove call")]
        rs_ = bbp.record_size(N)
        assert st == [0] * B and out[:rs_] == want[:rs_] and out[-rs_:] == want[-rs_:]
        assert c.verify_batch(B, N, b"".join(out[i * rs_:(i + 1) * rs_] + cases[N][i % 3].tail for i in range(B))) == [0] * B
        assert len(lines) == 1 and " B 769 " in lines[0] and lines[0].endswith(" coop 0 draw expanded"), lines
        c.set_blinding_draw(bbp.BLINDING_DRAW_MERLIN)
        c.prove_batch(2, N, ins[:2 * len(cases[N][0].row)], ents[:2 * len(cases[N][0].ent)])
        lines = [l for l in capfd.readouterr().err.split("\n") if l.startswith("prove call")]
        assert len(lines) == 1 and re.search(r" coop 1$", lines[0]), lines
        assert c.health() == 0
    finally:
        c.close()


def test_prove_batch_dev_rotating_and_sliced(xctx, bbp, cases):
    import torch
    N, dev = 8, torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    rs_ = bbp.record_size(N)
    for B, calls in ((64, 3), (130, 1)):
        ins, ents, want, _ = _batch(cases[N], B)
        d_in = torch.frombuffer(bytearray(ins), dtype=torch.uint8).to(dev)
        d_ent = torch.frombuffer(bytearray(ents), dtype=torch.uint8).to(dev)
        outs = [torch.zeros(B * rs_, dtype=torch.uint8, device=dev) for _ in range(calls)]
        torch.cuda.synchronize()
        for o in outs:  # in flight together: no synchronisation between the calls
            xctx.prove_batch_dev(B, N, d_in.data_ptr(), d_ent.data_ptr(), o.data_ptr(), s)
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            assert _first_diff(bytes(o.cpu().numpy().tobytes()), want, rs_) is None, (B, k)


def test_prove_round_equals_prove_batch(xctx, bbp, cases):
    N, B = 8, 5
    cs = cases[N]
    table = cs[0].seed + cs[0].pub  # the three cases share inputs: one round, one bidder, three entropy rows
    ents = b"".join(cs[i % 3].ent for i in range(B))
    rows, toggles, st = xctx.prove_round(N, table, bbp.pack_round_bids([(cs[0].d, cs[0].k)] * B), ents)
    assert st == [0] * B and toggles == [cs[0].toggle] * B
    rr, rs_ = bbp.round_row_size(N), bbp.record_size(N)
    for i in range(B):
        assert rows[i * rr:i * rr + rs_] == cs[i % 3].record, i
    assert xctx.verify_rounds([N], table, None, rows) == [0] * B


def test_pool_of_two_members(ctx, bbp, cases):
    N, B = 8, 7
    ins, ents, want, vin = _batch(cases[N], B)
    p = bbp.Pool([0, 0])
    try:
        p.set_blinding_draw("expanded")
        assert p.blinding_draw() == 1 and [p.member(i).blinding_draw() for i in range(len(p))] == [1, 1]
        out, st = p.prove_batch(B, N, ins, ents)
        assert st == [0] * B and out == want
        with pytest.raises(bbp.BbpError):
            p.set_blinding_draw(5)
        assert [p.member(i).blinding_draw() for i in range(len(p))] == [1, 1]
        p.set_blinding_draw("merlin")
        assert p.blinding_draw() == 0 and [p.member(i).blinding_draw() for i in range(len(p))] == [0, 0]
    finally:
        p.close()


def test_checked_proving_reproves_the_fixture_record(xctx, bbp, cases):
    N, B, i = 8, 6, 4
    ins, ents, want, _ = _batch(cases[N], B)
    xctx.set_prove_check(True)
    try:
        n0 = xctx.prove_check_stats()
        xctx.debug_corrupt_next_proof(i)
        out, st = xctx.prove_batch(B, N, ins, ents)
        n1 = xctx.prove_check_stats()
        assert st == [0] * B and out == want
        assert n1[2] - n0[2] == 1  # record i failed its check and was proved again
    finally:
        xctx.set_prove_check(False)


@pytest.mark.parametrize("source", ["device", "hedged"])
def test_deterministic_under_a_debug_key(xctx, bbp, cases, source):
    N, B = 8, 5
    ins, _, _, _ = _batch(cases[N], B)
    rs_ = bbp.record_size(N)
    xctx.set_entropy_source(source)
    try:
        outs = []
        for _ in range(2):
            xctx.debug_next_entropy_key(KEY)
            out, st = xctx.prove_batch(B, N, ins, None)
            assert st == [0] * B
            outs.append(out)
        assert outs[0] == outs[1]
        assert xctx.verify_batch(B, N, b"".join(outs[0][i * rs_:(i + 1) * rs_] + cases[N][i % 3].tail for i in range(B))) == [0] * B
    finally:
        xctx.set_entropy_source("os")


def test_poisoned_scratch_and_secret_wipe(ctx, bbp, cases):
    N, B = 8, 33
    ins, ents, want, _ = _batch(cases[N], B)
    c = bbp.Context(0)
    try:
        c.set_blinding_draw("expanded")
        c.prove_batch(130, N, *_batch(cases[N], 130)[:2])  # the buffers exist, larger than the call under test carves them
        c.prove_batch(B, N, ins, ents)
        for word in (0xFFFFFFFF, 0x6E6E6E6E):
            assert c.debug_poison_scratch(word)[0] > 0
            out, st = c.prove_batch(B, N, ins, ents)
            assert st == [0] * B and out == want, hex(word)
        c.set_secret_wipe(True)
        out, st = c.prove_batch(B, N, ins, ents)
        assert st == [0] * B and out == want
        assert c.debug_secret_residue() == (0, 0, "")
        assert c.health() == 0
    finally:
        c.close()


def _allocs(c):
    m = re.search(r"in (\d+) allocation\(s\) since bbp_init", c.describe())
    assert m
    return int(m.group(1))


@pytest.mark.parametrize("reserved,then", [("merlin", "expanded"), ("expanded", "merlin")])
def test_a_context_reserved_in_one_mode_allocates_nothing_in_the_other(ctx, bbp, cases, reserved, then):
    N, B = 8, 192
    ins, ents, _, _ = _batch(cases[N], B)
    c = bbp.Context(0)
    try:
        c.set_blinding_draw(reserved)
        c.reserve(B, N)
        a0 = _allocs(c)
        assert a0 > 0
        c.set_blinding_draw(then)
        for k in range(7):
            out, st = c.prove_batch(B, N, ins, ents)
            assert st == [0] * B, k
        assert _allocs(c) == a0, (a0, _allocs(c))
    finally:
        c.close()


def test_server_with_the_flag(ctx, oc, built, bbp, cases):
    built.build_server()
    d = tempfile.mkdtemp(prefix="bbp-uds-xd-")
    path = os.path.join(d, "sock")
    err = open(os.path.join(d, "log"), "w+")
    p = subprocess.Popen([built.SERVER_BIN, "-b", path, "-l", "info", "--engine", bbp.lib_path, "--device", "0", "--blinding-draw", "expanded"], stderr=err)
    try:
        for _ in range(1500):
            if os.path.exists(path) or p.poll() is not None:
                break
            time.sleep(0.02)
        assert os.path.exists(path), "server did not bind: " + open(err.name).read()[-800:]
        c = cases[8][0]
        blob = uc.prove(path, c.s7, c.pub, c.toggle)
        proof, cm, t = uc.decode_proof(blob)
        record = proof + b"".join(cm) + b"".join(t)
        q, z, seed = c.tail[:32], c.tail[32:64], c.tail[64:96]
        assert uc.verify(path, blob, q, z, seed, c.pub) == b"\x01"
        assert oc.verify(record, q, z, seed, c.pub) == 0
    finally:
        if p.poll() is None:
            p.send_signal(signal.SIGTERM)
            p.wait(timeout=30)
    log = open(err.name).read()
    assert "blinding draw expanded" in log and "engine: blinding draw: expanded" in log, log[-1200:]
