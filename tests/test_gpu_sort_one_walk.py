"""GPU tier: the staged MSM sort that recodes every scalar once and keeps its digits in registers (csrc/msm.hip k_msm_sort_staged).

Launches of 130 MSMs (unsplit geometry: one 1024-lane sort workgroup per MSM) through bbp_msm_batch_dev, every output point compared
with the C oracle.  Term counts: lanes with no, one, two, three and five scalars, the prover's shapes, both sides of the switch to the
wide image, the verifier's width (tests/sort_cases.py says why 2999 and 4097 stand for 3000 and 4098).  Scalar rows, each at each
count: uniform; all equal (one random value; nineteen digits of one magnitude, a bucket larger than the image: the direct pass); all
zero (no entry at all); the ends of the scalar range; a launch under BBP_SORT_STAGED=7 sends the wide counts through the 128 KB image.

The generator-fold pass (the kernel's composite-key instance) and the merged bases of the prover's index lists (MSM_SKIP_BASE) are
reached through the prover only: four proofs against the oracle's records (the fold pass in its split geometry), and 130 proofs in
one call -- every MSM and the fold pass unsplit, the A_I1 / S1 lists with their runs of skipped terms -- against the same proofs made
five at a time (split launches, the plain small-geometry sort) and, for a sample, against the oracle."""
import ctypes
import os

import pytest

from tests import msm_cases as mc
from tests import oracle_c
from tests import sort_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def planlib(built):
    return ctypes.CDLL(built.build_hostcheck())


@pytest.fixture(scope="module")
def wide_ctx(bbp, ctx):
    """a context whose plan sends MSMs wider than SORT_WIDE_FROM through the staged kernel too (made as test_gpu_msm_paths.py makes them)"""
    old = os.environ.get("BBP_SORT_STAGED")
    os.environ["BBP_SORT_STAGED"] = "7"
    try:
        c = bbp.Context(0)
    finally:
        if old is None:
            os.environ.pop("BBP_SORT_STAGED", None)
        else:
            os.environ["BBP_SORT_STAGED"] = old
    yield c
    flags = c.health()
    c.close()
    assert flags == 0


class Expected:
    """the oracle's point per distinct row, computed once per module"""

    def __init__(self, oc):
        self.oc, self.point = oc, {}

    def points(self, n, name):
        key = (n, name)
        if key not in self.point:
            rows = sc.rows(n)[name]
            canon = [mc.row_bytes([v % sc.L for v in row]) for row in rows]
            out = self.oc.msm_layout_many(canon, [n] * len(rows), [sc.layout(n)] * len(rows), threads=8)
            self.point[key] = [out[32 * i:32 * i + 32] for i in range(len(rows))]
        return self.point[key]


@pytest.fixture(scope="module")
def expected(oc):
    return Expected(oc)


def _launch(c, n, rows):
    import torch
    raw = [sc.row_bytes_raw(r) for r in rows]
    scal = torch.frombuffer(bytearray(b"".join(raw[b % len(raw)] for b in range(sc.B))), dtype=torch.uint8).cuda()
    out = torch.zeros(32 * sc.B, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the engine runs on a stream of its own)
    c.msm_batch_dev(sc.B, n, scal.data_ptr(), sc.layout(n), out.data_ptr())
    torch.cuda.synchronize()
    return bytes(out.cpu().numpy())


def _check(c, expected, n, name):
    rows = sc.rows(n)[name]
    got = _launch(c, n, rows)
    exp = expected.points(n, name)
    wrong = [b for b in range(sc.B) if got[32 * b:32 * b + 32] != exp[b % len(rows)]]
    assert not wrong, (n, name, wrong[:8])


@pytest.mark.parametrize("n", sc.TERMS)
def test_unsplit_launch_matches_the_oracle(ctx, planlib, expected, n):
    p = mc.plan(planlib, sc.B, n)
    assert p.split == 1 and p.geom == mc.LARGE and p.sort == (mc.STAGED if n <= 3000 else mc.PLAIN)
    for name in ("uniform", "equal", "zero", "extremes"):
        _check(ctx, expected, n, name)
    assert expected.points(n, "zero")[0] == bytes(32)  # the identity: an MSM without entries
    if n >= 1132:  # the second `equal` row's bucket 1 is larger than the image: it takes the direct pass
        hist, _ = mc.histogram(planlib, 12, sc.rows(n)["equal"][1], 1024)
        assert p.sort != mc.STAGED or hist[1] > p.sort_cap
    assert ctx.health() == 0


@pytest.mark.parametrize("n", [t for t in sc.TERMS if t > 3000])
def test_wide_launch_through_the_staged_kernel(wide_ctx, planlib, expected, n):
    p = mc.plan(planlib, sc.B, n, {"BBP_SORT_STAGED": "7"})
    assert p.split == 1 and p.sort == mc.STAGED_WIDE
    for name in ("uniform", "equal", "zero", "extremes"):
        _check(wide_ctx, expected, n, name)
    hist, _ = mc.histogram(planlib, 12, sc.rows(n)["equal"][1], 1024)
    assert hist[1] > p.sort_cap
    assert wide_ctx.health() == 0


def test_fold_pass_of_four_proofs_matches_the_oracle(ctx, oc, bbp):
    from tests.test_gpu_prove_verify import _synth_batch
    B, N = 4, 8
    ins, ents, _ = _synth_batch(ctx, B, N, seed=1604)
    out, st = ctx.prove_batch(B, N, b"".join(ins), b"".join(ents))
    cout, cst = oc.prove_many(b"".join(ins), b"".join(ents), B, N, threads=4)
    assert st == [0] * B == cst
    assert out == cout


def test_unsplit_prove_with_merged_bases_and_unsplit_fold_pass(ctx, oc, bbp):
    from tests.test_gpu_prove_verify import _synth_batch
    B, N, chunk = sc.B, 8, 5
    rs_ = bbp.record_size(N)
    ins, ents, _ = _synth_batch(ctx, B, N, seed=1605)
    out, st = ctx.prove_batch(B, N, b"".join(ins), b"".join(ents))
    assert st == [0] * B
    for b0 in range(0, B, chunk):
        part, pst = ctx.prove_batch(chunk, N, b"".join(ins[b0:b0 + chunk]), b"".join(ents[b0:b0 + chunk]))
        assert pst == [0] * chunk
        assert part == out[b0 * rs_:(b0 + chunk) * rs_], b0
    sample = [0, 64, 65, 129]
    cout, cst = oc.prove_many(b"".join(ins[i] for i in sample), b"".join(ents[i] for i in sample), len(sample), N, threads=4)
    assert cst == [0] * len(sample)
    for j, i in enumerate(sample):
        assert out[i * rs_:(i + 1) * rs_] == cout[j * rs_:(j + 1) * rs_], i
    assert ctx.health() == 0
