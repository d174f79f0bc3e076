"""GPU tier: the device verifiers against forged proofs (tests/forgery_cases.py; the CPU-tier model that justifies the rows is
tests/test_verify_forgery_model.py).

Valid rows come from the device prover at N in {1, 3, 8, 202}.  The expected status of every row is the C oracle's, compared
exactly: a cancelling row must be VERIFY (1) on every path, a swept row what the oracle says (0, 1 or 3).  Paths: the plain
calls below and above the 4096-proof rule of csrc/verifier.inc (k_varprep + k_varsum below it, k_varbase with Q > 1 from it on),
the aggregated calls at several group sizes under both entropy sources with the exact number of individually checked proofs,
the mixed-N calls, and the call combiner (both record layouts; the batch calls take the compact layout only).

One CONTROL of the test itself, not a promise of the API: two members of a cancelling pair that are handed the SAME entropy row
draw the same weight, and the group check then passes (test_control_...).  It shows that the forged rows reach the group sum
intact, which is what makes the rejections elsewhere in this file meaningful."""
import math
import os
import random
import time

import pytest

from oracle.ref_py import ristretto as rs
from tests import forgery_cases as fc, oracle_c
from tests import verify_combine_cases as vc
from tests.test_gpu_prove_verify import _synth_batch
from tests.test_gpu_verify_combine import _child

pytestmark = pytest.mark.gpu
OK, VERIFY, FORMAT = fc.OK, fc.VERIFY, fc.FORMAT
NS = (1, 3, 8, 202)
PER_N = 6
THREADS = 16


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def valid(ctx, bbp):
    """PER_N valid rows per N from the device prover; row i has its own item at pub_list[i mod N]."""
    out = {}
    for n in NS:
        ins, ents, vins = _synth_batch(ctx, PER_N, n, seed=9100 + n)
        rec, st = ctx.prove_batch(PER_N, n, b"".join(ins), b"".join(ents))
        assert st == [0] * PER_N
        rs_ = bbp.record_size(n)
        out[n] = [(rec[i * rs_:(i + 1) * rs_],) + tuple(vins[i]) for i in range(PER_N)]
    return out


class Expect:
    """The C oracle's status of a row, evaluated once per distinct row (both layouts)."""

    def __init__(self, oc):
        self.oc, self.cache, self.seconds = oc, {}, 0.0

    def __call__(self, rows):
        todo = {}
        for r in rows:
            k = fc.join(r)
            if k not in self.cache and k not in todo:
                todo[k] = r
        by_shape = {}
        for k, r in todo.items():
            by_shape.setdefault((fc.n_of(r), len(r[0])), []).append(k)
        t0 = time.time()
        for (n, rec_len), keys in by_shape.items():
            st = self.oc.verify_many(b"".join(keys), len(keys), n, THREADS, rec_len=rec_len)
            for k, s in zip(keys, st):
                self.cache[k] = s
        self.seconds += time.time() - t0
        return [self.cache[fc.join(r)] for r in rows]


@pytest.fixture(scope="module")
def expect(oc):
    e = Expect(oc)
    yield e
    print("oracle: %d distinct rows in %.1f s" % (len(e.cache), e.seconds))


@pytest.fixture(scope="module")
def sweeps(valid, expect):
    """{N: (rows, expected statuses, rejected before the group sum)}: the valid row, its whole sweep and every cancelling set."""
    out = {}
    for n in NS:
        base, donor = valid[n][0], valid[n][1]
        cases = fc.sweep(base, donor, 0)
        sets = fc.cancelling_sets(base, random.Random(500 + n))
        rows = [base] + [c.row for c in cases] + [m for ms in sets.values() for m in ms]
        exp = expect(rows)
        assert exp[0] == OK
        for c, s in zip(cases, exp[1:]):
            assert (s != OK) == c.differs, (n, c.label, s)
        assert exp[1 + len(cases):] == [VERIFY] * (len(rows) - 1 - len(cases)), n   # every cancelling row alone is rejected
        early = [fc.rejected_before_the_sum(r, s, rs.decode, base) for r, s in zip(rows, exp)]
        print("N %d: %d sweep rows (+1 valid, +%d cancelling), oracle OK %d VERIFY %d FORMAT %d, decided before the sum %d"
              % (n, len(cases), len(rows) - 1 - len(cases), exp.count(OK), exp.count(VERIFY), exp.count(FORMAT), sum(early)))
        assert len(cases) >= 8 * (35 + 4 + n) and exp.count(FORMAT) >= 16
        out[n] = (rows, exp, early)
    return out


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _status_tensor(B):
    import torch
    return torch.full((B,), -7, dtype=torch.int32, device="cuda")


def _blob(rows):
    return b"".join(fc.join(r) for r in rows)


@pytest.mark.parametrize("n", NS)
def test_plain_sweep_below_and_above_the_varbase_rule(ctx, sweeps, n):
    import torch
    rows, exp, _ = sweeps[n]
    B = len(rows)
    blob = _blob(rows)
    assert ctx.verify_batch(B, n, blob) == exp
    d_in, d_ent, st = _dev(blob), _dev(os.urandom(32 * B)), _status_tensor(B)   # caller entropy rows: distinct
    torch.cuda.synchronize()
    ctx.verify_batch_dev(B, n, d_in.data_ptr(), d_ent.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    assert st.cpu().tolist() == exp
    reps = math.ceil(4096 / B)
    # either side of the rule `vb2 = B < 4096` (csrc/verifier.inc), and nothing in the environment that overrides it: both sum
    # shapes ran (Q = varbase_lanes / B > 1 above the rule: 65536 / 4462 = 14 at the largest tiled call)
    assert B < 4096 <= B * reps and "BBP_VARBASE_V1" not in os.environ and "BBP_VARBASE_LANES" not in os.environ
    assert ctx.verify_batch(B * reps, n, blob * reps) == exp * reps
    d_in, d_ent, st = _dev(blob * reps), _dev(os.urandom(32 * B * reps)), _status_tensor(B * reps)
    torch.cuda.synchronize()
    ctx.verify_batch_dev(B * reps, n, d_in.data_ptr(), d_ent.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    assert st.cpu().tolist() == exp * reps
    assert ctx.health() == 0


def _designed(valid, n):
    """203 rows, honest but for: a set of 32 filling rows 32..63; a pair at 6, 7 and one at 95, 96 (group boundaries for G = 7 and
    for G = 2 / 32); a triple at 128..130 beside an ordinary bad row at 131; a pair at 160, 161 whose first member is also a
    FormatError; a pair at 201, 202 (the ragged last group for G = 32 and 1024)."""
    base = valid[n][0]
    sets = fc.cancelling_sets(base, random.Random(900 + n))
    f = fc.fields_by_name(base)
    rows = [valid[n][i % PER_N] for i in range(203)]
    cancelling = set()

    def place(at, members):
        for k, m in enumerate(members):
            rows[at + k] = m
            cancelling.add(at + k)
    place(32, sets["a:set32"])
    place(6, sets["b:pair_small"])
    place(95, sets["a:pair_252"])
    place(128, sets["b:triple"])
    rows[131] = fc.put(base, f["t_x"], fc.b32((fc.i32(fc.get(base, f["t_x"])) + 1) % fc.L))
    place(160, sets["a:pair_small"])
    rows[160] = fc.put(rows[160], f["t_x_blinding"], b"\xff" * 32)
    cancelling.discard(160)
    place(201, sets["b:pair_252"])
    return rows, cancelling


AGG = [(3, G, src) for G in (1, 2, 7, 32, 1024) for src in ("os", "device")] + [(n, 32, "os") for n in (1, 8, 202)] + [(202, 7, "device")]


@pytest.mark.parametrize("n,G,source", AGG)
def test_aggregated_rejects_cancelling_sets_and_counts_its_fallback_exactly(ctx, valid, sweeps, expect, n, G, source):
    import torch
    ctx.set_entropy_source(source)
    try:
        honest = [valid[n][i % PER_N] for i in range(203)]
        got, nfb = ctx.verify_batch_aggregated(len(honest), n, _blob(honest), G)
        assert got == [OK] * len(honest) and nfb == 0

        rows, cancelling = _designed(valid, n)
        exp = expect(rows)
        assert all(exp[i] == VERIFY for i in cancelling) and exp[160] == FORMAT and exp[131] == VERIFY
        assert [i for i, s in enumerate(exp) if s != OK] == sorted(cancelling | {131, 160})
        early = [s == FORMAT for s in exp]   # every other bad row of this batch is found by the mega-check only
        blob = _blob(rows)
        plain = ctx.verify_batch(len(rows), n, blob)
        got, nfb = ctx.verify_batch_aggregated(len(rows), n, blob, G)
        print("designed: G %d fallback %d" % (G, nfb))
        assert got == exp and got == plain
        assert nfb == fc.expected_fallback(exp, early, G)
        d_in, d_ent, st = _dev(blob), _dev(os.urandom(32 * len(rows))), _status_tensor(len(rows))
        torch.cuda.synchronize()
        nfb_dev = ctx.verify_batch_aggregated_dev(len(rows), n, d_in.data_ptr(), d_ent.data_ptr(), st.data_ptr(), G)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == exp and nfb_dev == nfb

        if (n, G, source) == (3, 32, "os"):
            # the same batch tiled past the 4096 rule: k_varbase with Q > 1 and the weights multiplied in, k_var_sum over Q partial
            # sums.  Tile 0 keeps its alignment (the set of 32 fills group 1), the later tiles shift by 203 mod 32 each.
            reps = math.ceil(4096 / len(rows))
            assert "BBP_VARBASE_V1" not in os.environ and len(rows) * reps >= 4096
            got, nfb = ctx.verify_batch_aggregated(len(rows) * reps, n, blob * reps, G)
            assert got == exp * reps and nfb == fc.expected_fallback(exp * reps, early * reps, G)

        # a cancelling pair as the only bad rows of a batch, inside one group
        only = list(honest[:40])
        only[10:12] = fc.cancelling_sets(valid[n][2], random.Random(77))["b:pair_252"]
        exp_only = [VERIFY if i in (10, 11) else OK for i in range(40)]
        assert expect(only) == exp_only
        got, nfb = ctx.verify_batch_aggregated(40, n, _blob(only), G)
        assert got == exp_only and nfb == fc.expected_fallback(exp_only, [False] * 40, G)

        # the whole sweep of this N with its cancelling sets
        srows, sexp, searly = sweeps[n]
        got, nfb = ctx.verify_batch_aggregated(len(srows), n, _blob(srows), G)
        assert got == sexp
        assert nfb == fc.expected_fallback(sexp, searly, G)
        assert ctx.health() == 0
    finally:
        ctx.set_entropy_source("os")


def test_control_members_given_the_same_entropy_row_cancel(ctx, valid, expect):
    """CONTROL of this test file, not a promise of the API (module doc).  include/bbp.h asks for distinct, unpredictable entropy
    rows; should the weights ever mix in the row index, this control stops holding and the CPU-tier model takes its place."""
    import torch
    n, G, B = 3, 32, 64
    rows = [valid[n][i % PER_N] for i in range(B)]
    rows[40], rows[45] = fc.cancelling_sets(valid[n][1], random.Random(5))["a:pair_252"]
    exp = expect(rows)
    assert [i for i, s in enumerate(exp) if s] == [40, 45] and exp[40] == exp[45] == VERIFY
    d_in = _dev(_blob(rows))
    ent = bytearray(os.urandom(32 * B))
    d_distinct, st = _dev(ent), _status_tensor(B)
    torch.cuda.synchronize()
    nfb = ctx.verify_batch_aggregated_dev(B, n, d_in.data_ptr(), d_distinct.data_ptr(), st.data_ptr(), G)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == exp and nfb == 32          # distinct rows: rejected
    ent[32 * 45:32 * 46] = ent[32 * 40:32 * 41]            # the pair shares one entropy row: equal weights by construction
    d_shared, st = _dev(ent), _status_tensor(B)
    torch.cuda.synchronize()
    nfb = ctx.verify_batch_aggregated_dev(B, n, d_in.data_ptr(), d_shared.data_ptr(), st.data_ptr(), G)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [OK] * B and nfb == 0      # the residuals cancelled inside the group sum
    st = _status_tensor(B)
    ctx.verify_batch_dev(B, n, d_in.data_ptr(), d_shared.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    assert st.cpu().tolist() == exp                        # the plain path judges every proof alone
    assert ctx.health() == 0


def test_mixed_n_interleaved_sweeps(ctx, bbp, sweeps):
    """The sweeps of all four N dealt round-robin: the members of every cancelling set are separated by rows of other N."""
    import torch
    order = []
    for k in range(max(len(sweeps[n][0]) for n in NS)):
        order += [(n, k) for n in NS if k < len(sweeps[n][0])]
    rows = [sweeps[n][0][k] for n, k in order]
    exp = [sweeps[n][1][k] for n, k in order]
    early = [sweeps[n][2][k] for n, k in order]
    Ns, blob = bbp.pack_mixed_rows(rows)
    assert len(set(Ns[:8])) == 4
    assert ctx.verify_batch_mixed(Ns, blob) == exp
    for n in NS:                                           # the uniform call's statuses
        rws, e, _ = sweeps[n]
        assert ctx.verify_batch(len(rws), n, _blob(rws)) == e
    for G in (7, 32):
        got, nfb = ctx.verify_batch_mixed_aggregated(Ns, blob, G)
        assert got == exp
        assert nfb == fc.expected_fallback(exp, early, G)
    d_in, d_ent = _dev(blob), _dev(os.urandom(32 * len(Ns)))
    st = _status_tensor(len(Ns))
    torch.cuda.synchronize()
    ctx.verify_batch_mixed_dev(Ns, d_in.data_ptr(), d_ent.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    assert st.cpu().tolist() == exp
    st = _status_tensor(len(Ns))
    torch.cuda.synchronize()
    nfb = ctx.verify_batch_mixed_aggregated_dev(Ns, d_in.data_ptr(), d_ent.data_ptr(), st.data_ptr(), 32)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == exp and nfb == fc.expected_fallback(exp, early, 32)
    assert ctx.health() == 0


def _honest_mixed(valid):
    return [valid[(3, 1, 8, 202)[i % 4]][(i // 4) % PER_N] for i in range(201)]


def _designed_mixed(valid):
    """201 rows, honest rows of all four N in turn (N = 3 at every fourth, even position), but for forged rows of N = 3 whose neighbours are honest rows of other N:
      F  a pair at 10, 12 whose first member is also a FormatError (it stays out of the sum; its partner must still be VERIFY)
      A  a pair at 36, 38: the only bad rows of their group for G = 7 (35..41) and for G = 32 (32..63)
      B  a pair at 94, 96: inside 91..97 for G = 7, across the boundary 95 | 96 for G = 32
      C  a triple at 98, 100, 102 beside an ordinary bad row (t_x + 1, N = 8) at 101: one group for G = 7 (98..104) and G = 32
      D  a set of 32 at 128, 130 .. 190: across many boundaries for G = 7, half in 128..159 and half in 160..191 for G = 32
      E  a pair at 196, 200: the only bad rows of the ragged last group, 196..200 for G = 7 and 192..200 for G = 32
    A verifier whose groups are summed unweighted accepts A and E at both group sizes (and B at G = 7)."""
    rows = _honest_mixed(valid)
    sets = fc.cancelling_sets(valid[3][0], random.Random(1234))
    cancelling = set()

    def place(positions, members):
        assert len(positions) == len(members)
        for at, m in zip(positions, members):
            rows[at] = m
            cancelling.add(at)
    place((10, 12), sets["b:pair_small"])
    f = fc.fields_by_name(rows[10])
    rows[10] = fc.put(rows[10], f["t_x_blinding"], b"\xff" * 32)
    cancelling.discard(10)
    place((36, 38), sets["a:pair_small"])
    place((94, 96), sets["a:pair_252"])
    place((98, 100, 102), sets["b:triple"])
    g = fc.fields_by_name(valid[8][2])
    rows[101] = fc.put(valid[8][2], g["t_x"], fc.b32((fc.i32(fc.get(valid[8][2], g["t_x"])) + 1) % fc.L))
    place(range(128, 192, 2), sets["a:set32"])
    place((196, 200), sets["b:pair_252"])
    for i in sorted(cancelling):   # every member's neighbours are honest rows of another N (or the ordinary bad row of N = 8)
        assert all(fc.n_of(rows[j]) != 3 for j in (i - 1, i + 1) if j < len(rows))
    return rows, cancelling


@pytest.mark.parametrize("G", [7, 32])
def test_mixed_n_aggregated_rejects_cancelling_sets_between_rows_of_other_n(ctx, bbp, valid, expect, G):
    """The mixed-N verifier draws and applies its weights in kernels of its own (csrc/verifier_mixed.inc k_vtranscript_mx,
    k_vscalars_mx, k_varprep_mx / k_varbase_mx): the designed batch holds groups whose only bad rows are a whole cancelling set."""
    import torch
    rows, cancelling = _designed_mixed(valid)
    exp = expect(rows)
    assert [i for i, s in enumerate(exp) if s != OK] == sorted(cancelling | {10, 101})
    assert all(exp[i] == VERIFY for i in cancelling | {101}) and exp[10] == FORMAT
    early = [s == FORMAT for s in exp]   # every other bad row of this batch is found by the mega-check only
    for members in ((36, 38), (196, 200)):   # groups (cut by index) that an unweighted sum would pass
        g0 = members[0] // G * G
        assert members[1] // G * G == g0 and [i for i in range(g0, min(len(rows), g0 + G)) if exp[i] != OK] == list(members)
    Ns, blob = bbp.pack_mixed_rows(rows)
    assert set(Ns) == set(NS)
    honest = _honest_mixed(valid)
    hNs, hblob = bbp.pack_mixed_rows(honest)
    got, nfb = ctx.verify_batch_mixed_aggregated(hNs, hblob, G)
    assert got == [OK] * len(honest) and nfb == 0
    assert ctx.verify_batch_mixed(Ns, blob) == exp
    got, nfb = ctx.verify_batch_mixed_aggregated(Ns, blob, G)
    print("designed mixed: G %d fallback %d" % (G, nfb))
    assert got == exp
    assert nfb == fc.expected_fallback(exp, early, G)
    d_in, d_ent, st = _dev(blob), _dev(os.urandom(32 * len(Ns))), _status_tensor(len(Ns))   # caller entropy rows: distinct
    torch.cuda.synchronize()
    nfb_dev = ctx.verify_batch_mixed_aggregated_dev(Ns, d_in.data_ptr(), d_ent.data_ptr(), st.data_ptr(), G)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == exp and nfb_dev == nfb
    assert ctx.health() == 0


def _aggregated_burst(valid):
    """64 compact requests in queue order, honest ones of all four N but for forged ones of N = 8 placed for groups of 8 cut by
    queue position: a pair at 2, 3 (the only bad rows of 0..7), a triple at 10, 11, 12 (the only bad rows of 8..15) and a set of 32
    at 16..47.  One request that misses the batching window and leaves ahead of the rest moves every position down by one and
    leaves the pair and the triple inside their groups."""
    reqs = [valid[NS[i % 4]][(i // 4) % PER_N] for i in range(64)]
    sets = fc.cancelling_sets(valid[8][3], random.Random(31))
    reqs[2:4] = sets["a:pair_small"]
    reqs[10:13] = sets["b:triple"]
    reqs[16:48] = sets["a:set32"]
    assert len(reqs) == 64
    return reqs


def _burst_requests(valid):
    """Honest requests of several N and both layouts around a cancelling pair, a triple and a set of 32 (compact)."""
    reqs = []
    for i in range(48):
        r = valid[NS[i % 4]][(i // 4) % PER_N]
        reqs.append(fc.two_phase(r) if i % 5 == 4 else r)
    sets = fc.cancelling_sets(valid[8][3], random.Random(31))
    forged = {}
    for at, name in ((5, "a:pair_small"), (20, "b:triple"), (30, "a:set32")):
        for k, m in enumerate(sets[name]):
            forged[at + 2 * k] = m
    for at in sorted(forged):
        reqs.insert(at, forged[at])
    two = fc.cancelling_sets(fc.two_phase(valid[3][4]), random.Random(32))["b:pair_252"]
    reqs += two
    return reqs


def test_combiner_bursts_with_cancelling_sets_and_two_phase_sweeps(ctx, valid, expect):
    ctx.set_batching(100000, 4096)
    try:
        reqs = _burst_requests(valid)
        for n in NS:                                       # the two-phase layout reaches the device through the combiner only
            base, donor = fc.two_phase(valid[n][0]), fc.two_phase(valid[n][1])
            cases = fc.sweep(base, donor, 0)
            assert len(cases) >= 8 * (38 + 4 + n) - 3      # the identity is what A_I2, A_O2 and S2 already hold
            reqs += [c.row for c in cases]
        exp = expect(reqs)
        assert exp.count(VERIFY) > 1000 and exp.count(OK) > 40 and exp.count(FORMAT) >= 64
        print("combiner burst: %d requests" % len(reqs))
        for mixing in (True, False):
            ctx.set_verify_mixing(mixing)
            assert vc.burst(ctx, reqs, timeout=600.0) == exp, mixing
        assert ctx.health() == 0
    finally:
        ctx.set_verify_mixing(True)
        ctx.set_batching(0, 0)


def test_combiner_with_the_aggregated_engine_and_through_a_pool(bbp, valid, expect):
    """BBP_VERIFY_AGGREGATE=8 in a child process: a burst of several N that shares one device call runs the mixed aggregated
    verifier in groups of 8 (the host path aggregates from 16 rows on).  The call count of the warmed second burst shows that
    the requests did share a call, so the pair and the triple sat in one group each with honest requests only."""
    reqs = _aggregated_burst(valid)
    exp = expect(reqs)
    assert [i for i, s in enumerate(exp) if s != OK] == [2, 3, 10, 11, 12] + list(range(16, 48)) and exp.count(VERIFY) == 37
    res = _child({"bursts": [vc.to_json(reqs), vc.to_json(reqs)]}, {"BBP_VERIFY_AGGREGATE": "8"})
    print([b["calls"] for b in res["bursts"]])
    assert "aggregate groups of 8" in res["describe"] and "aggregate groups of 8 (off)" not in res["describe"]
    assert [b["status"] for b in res["bursts"]] == [exp, exp]
    assert res["bursts"][1]["calls"] <= 2 and res["health"] == 0
    pool = bbp.Pool([0, 0])
    try:
        pool.set_batching(100000, 4096)
        assert vc.burst(pool, reqs) == exp
        assert pool.health() == 0
    finally:
        pool.close()
