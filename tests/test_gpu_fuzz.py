"""GPU tier: randomised differential runs against the C oracle -- MSM shapes / scalar patterns that stress the recoding, the split
into sub-MSMs and empty buckets, and prove / verify over random batch geometries and list lengths.  Seeds are fixed: a failure
reproduces."""
import hashlib
import random

import pytest

from tests import msm_cases as mc
from tests import oracle_c
from tests.test_gpu_prove_verify import _synth_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.mark.parametrize("seed", mc.FUZZ_SEEDS)
def test_msm_fuzz(ctx, bbp, oc, seed):
    """fourteen random shapes per seed (tests/msm_cases.py fuzz_cases): launches of fewer than 700 terms with up to 200 MSMs -- split
    or through the staged sort, no bucket near its image -- and wider ones of at most 9 MSMs, all split"""
    for case, layout, n_terms, B, int_rows in mc.fuzz_cases(seed):
        rows = [mc.row_bytes(row) for row in int_rows]
        got = ctx.msm_batch(B, n_terms, b"".join(rows), layout)
        exp = oc.msm_layout_many(rows, [n_terms] * B, [layout] * B, threads=8)
        assert got == exp, (seed, case, layout, n_terms, B)


def test_msm_fuzz_half_wavefront_fold(bbp, oc):
    """k_msm_fold_half (two MSMs per wavefront, 32 lanes x 32 buckets) serves launches of 512 MSMs and more by default; with
    BBP_FOLD_HALF_FROM=1 every unsplit launch uses it: odd MSM counts (idle upper half), one-term and empty MSMs, every term in one
    bucket (runs of chunk-leading partial sums), and the full-width 4097-term shape as a launch of 128 MSMs -- all against the C
    oracle.  The list's split shapes (tests/msm_cases.py HALF_FOLD_SHAPES names each shape's fold) fold with k_msm_fold<2> as ever:
    the knob must not disturb them."""
    import os
    old = os.environ.get("BBP_FOLD_HALF_FROM")
    os.environ.update(mc.HALF_FOLD_KNOBS)
    try:
        c2 = bbp.Context(0)
    finally:
        if old is None:
            os.environ.pop("BBP_FOLD_HALF_FROM", None)
        else:
            os.environ["BBP_FOLD_HALF_FROM"] = old
    try:
        for layout, n_terms, B, int_rows in mc.half_fold_cases():
            rows = [mc.row_bytes(row) for row in int_rows]
            got = c2.msm_batch(B, n_terms, b"".join(rows), layout)
            exp = oc.msm_layout_many(rows, [n_terms] * B, [layout] * B, threads=8)
            assert got == exp, (layout, n_terms, B)
        assert c2.health() == 0
    finally:
        c2.close()


def test_msm_sort_oversized_bucket(bbp, oc):
    """Giant buckets in the SPLIT geometry: the scalar sum_j 2^(13 j) has 19 digits of magnitude 1 at width 9 as at width 12, so with
    every term equal to it bucket 1 of every sub-MSM holds all its entries (19 n_sub) and every other bucket is empty; a second
    pattern puts two thirds of the terms there and spreads the rest.  All three launches are cut 16 ways into the small geometry
    (k_msm_sort<2>: the plain scatter, whatever BBP_SORT_STAGED says -- the ledger in test_msm_plan_host.py shows it), so the knob is
    not varied here; the staged sort's direct pass and its images are test_gpu_msm_paths.py's."""
    c2 = bbp.Context(0)
    try:
        for n_terms, B, int_rows in mc.oversized_split_cases():
            rows = [mc.row_bytes(row) for row in int_rows]
            got = c2.msm_batch(B, n_terms, b"".join(rows), bbp.LAYOUT_BLIND_G_H)
            exp = oc.msm_layout_many(rows, [n_terms] * B, [bbp.LAYOUT_BLIND_G_H] * B, threads=8)
            assert got == exp, n_terms
        assert c2.health() == 0
    finally:
        c2.close()


@pytest.mark.parametrize("seed", [11, 12])
def test_prove_verify_fuzz(ctx, bbp, oc, seed):
    rnd = random.Random(seed)
    for case in range(5):
        N = rnd.choice([1, 2, 3, 5, 8, 13, 21, 40]) if case else rnd.choice([101, 202])
        B = rnd.choice([1, 2, 3, 7, 19]) if N < 100 else rnd.choice([1, 3])
        ins, ents, vins = _synth_batch(ctx, B, N, seed=seed * 100 + case)
        rs_ = bbp.record_size(N)
        out, st = ctx.prove_batch(B, N, b"".join(ins), b"".join(ents))
        assert st == [0] * B
        cout, cst = oc.prove_many(b"".join(ins), b"".join(ents), B, N, threads=8)
        assert cst == [0] * B and out == cout, (seed, case, N, B)
        vin = bytearray(b"".join(out[i * rs_:(i + 1) * rs_] + v[0] + v[1] + v[2] + v[3] for i, v in enumerate(vins)))
        bad = rnd.randrange(B)
        vin[bad * (rs_ + 96 + 32 * N) + 1 + rnd.randrange(1100)] ^= 1 << rnd.randrange(8)
        got = ctx.verify_batch(B, N, bytes(vin))
        exp = oc.verify_many(bytes(vin), B, N, threads=8)
        assert [g != 0 for g in got] == [e != 0 for e in exp] and got[bad] != 0, (seed, case, N, B, got, exp)
