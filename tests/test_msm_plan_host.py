"""not-gpu tier: which kernels an MSM launch takes (csrc/msm_plan.h: MsmKnobs, msm_split, plan_msm), compiled for the host by
tests/host_check.cpp -- and the coverage ledger of the MSM GPU tests: every case of tests/msm_cases.py is held against the plan of its
launch and, for the bucket cases, against the histogram the product's own recoder gives its scalars.  The plan table's expected values
are literals worked out from the rules as msm_plan.h states them, never a second call of the header; the ledger takes capacities from
the plan alone."""
import ctypes

import pytest

from tests import msm_cases as mc
from tests.msm_cases import HALF, LANES128, LARGE, PLAIN, SMALL, SMALL_FOLD, STAGED, STAGED_WIDE, plan


@pytest.fixture(scope="module")
def lib(built):
    return ctypes.CDLL(built.build_hostcheck())


SMALL_PLAN = dict(geom=SMALL, sort=PLAIN, sort_cap=0, fold=SMALL_FOLD, reduce=1, K=128, W=29, naf=9)
LARGE_PLAN = dict(geom=LARGE, reduce=0, K=1024, W=22, naf=12)


def check(p, **want):
    got = {k: getattr(p, k) for k in want}
    assert got == want, (p, want)


def test_launches_below_128_msms_are_split_into_the_small_geometry(lib):
    check(plan(lib, 127, 2933), split=4, n_sub=734, n_work=508, **SMALL_PLAN)  # 512 / 127 = 4 workgroups per MSM
    check(plan(lib, 128, 2933), split=1, n_sub=2933, n_work=128, sort=STAGED, sort_cap=21504, fold=LANES128, **LARGE_PLAN)
    check(plan(lib, 1, 2933), split=16, n_sub=184, n_work=16, **SMALL_PLAN)
    check(plan(lib, 3, 2933), split=16, n_sub=184, n_work=48, **SMALL_PLAN)
    check(plan(lib, 9, 1467), split=11, n_sub=134, n_work=99, **SMALL_PLAN)  # 1467 / 12 = 122 < 128, / 11 = 133
    check(plan(lib, 65, 2049), split=7, n_sub=293, n_work=455, **SMALL_PLAN)
    check(plan(lib, 2, 4097), split=16, n_sub=257, n_work=32, **SMALL_PLAN)


def test_an_msm_is_split_only_into_sub_msms_of_128_terms_or_more(lib):
    check(plan(lib, 3, 255), split=1, n_sub=255, n_work=3, sort=STAGED, sort_cap=21504, fold=LANES128, **LARGE_PLAN)
    check(plan(lib, 3, 256), split=2, n_sub=128, n_work=6, **SMALL_PLAN)
    check(plan(lib, 1, 383), split=2, n_sub=192, **SMALL_PLAN)
    check(plan(lib, 1, 384), split=3, n_sub=128, **SMALL_PLAN)
    check(plan(lib, 1, 2047), split=15, n_sub=137, **SMALL_PLAN)
    check(plan(lib, 1, 2048), split=16, n_sub=128, **SMALL_PLAN)
    check(plan(lib, 1, 65535), split=16, n_sub=4096, **SMALL_PLAN)
    check(plan(lib, 100, 639), split=4, n_sub=160, n_work=400, **SMALL_PLAN)  # 512 / 100 = 5, but 639 / 5 = 127
    check(plan(lib, 100, 640), split=5, n_sub=128, n_work=500, **SMALL_PLAN)
    check(plan(lib, 127, 511), split=3, n_sub=171, **SMALL_PLAN)
    check(plan(lib, 127, 512), split=4, n_sub=128, **SMALL_PLAN)
    check(plan(lib, 127, 129), split=1, n_sub=129, n_work=127, sort=STAGED, fold=LANES128, **LARGE_PLAN)
    check(plan(lib, 1, 1), split=1, n_sub=1, n_work=1, sort=STAGED, fold=LANES128, **LARGE_PLAN)


@pytest.mark.parametrize("staged,narrow,wide", [
    ("0", (PLAIN, 0), (PLAIN, 0)), ("1", (STAGED, 21504), (PLAIN, 0)), ("2", (PLAIN, 0), (PLAIN, 0)), ("3", (STAGED, 21504), (PLAIN, 0)),
    ("4", (PLAIN, 0), (PLAIN, 0)), ("5", (STAGED, 21504), (STAGED_WIDE, 32768)), ("7", (STAGED, 21504), (STAGED_WIDE, 32768))])
def test_the_staged_sort_and_its_image(lib, staged, narrow, wide):
    """bit 0 stages MSMs of at most 3000 terms through an image of 21 504 entries; beyond, bit 2 as well gives the image of 32 768"""
    knobs = {"BBP_SORT_STAGED": staged}
    for n_terms, (sort, cap) in ((3000, narrow), (3001, wide), (2933, narrow), (4097, wide), (4098, wide)):
        check(plan(lib, 128, n_terms, knobs), split=1, n_sub=n_terms, sort=sort, sort_cap=cap, fold=LANES128, **LARGE_PLAN)
    # a split MSM in the large geometry is judged by its sub-MSMs' terms: 48 016 / 16 = 3001
    big = dict(knobs, BBP_MSM_SMALL="0")
    check(plan(lib, 1, 48016, big), split=16, n_sub=3001, sort=wide[0], sort_cap=wide[1], geom=LARGE, reduce=1, K=1024, W=22)
    check(plan(lib, 1, 48000, big), split=16, n_sub=3000, sort=narrow[0], sort_cap=narrow[1], geom=LARGE, reduce=1)
    check(plan(lib, 3, 2933, knobs), **SMALL_PLAN)  # the small geometry has the plain scatter only


def test_the_fold_kernel(lib):
    check(plan(lib, 511, 100), n_work=511, fold=LANES128, sort=STAGED, **LARGE_PLAN)
    check(plan(lib, 512, 100), n_work=512, fold=HALF, sort=STAGED, **LARGE_PLAN)
    check(plan(lib, 1024, 4098), fold=HALF, sort=PLAIN, sort_cap=0, **LARGE_PLAN)
    check(plan(lib, 511, 100, {"BBP_FOLD_HALF_FROM": "511"}), fold=HALF)
    check(plan(lib, 1, 100, {"BBP_FOLD_HALF_FROM": "1"}), fold=HALF)
    check(plan(lib, 1, 100, {"BBP_FOLD_HALF_FROM": "0"}), fold=HALF)  # clamped to 1
    check(plan(lib, 3, 2933, {"BBP_FOLD_HALF_FROM": "1"}), **SMALL_PLAN)  # split launches fold with k_msm_fold<2> whatever the knob says
    # ... unless they keep the large geometry: then the workgroups count, not the MSMs
    large = {"BBP_MSM_SMALL": "0"}
    check(plan(lib, 3, 2933, large), split=16, n_sub=184, n_work=48, geom=LARGE, sort=STAGED, sort_cap=21504, fold=LANES128, reduce=1, K=1024, W=22, naf=12)
    check(plan(lib, 31, 2049, large), split=16, n_sub=129, n_work=496, fold=LANES128, reduce=1)
    check(plan(lib, 32, 2049, large), split=16, n_sub=129, n_work=512, fold=HALF, reduce=1)


def test_device_sized_launches_are_never_split(lib):
    check(plan(lib, 3, 2933, device_sized=True), split=1, n_sub=2933, n_work=3, sort=STAGED, sort_cap=21504, fold=LANES128, **LARGE_PLAN)
    check(plan(lib, 1, 4098, device_sized=True), split=1, n_sub=4098, n_work=1, sort=PLAIN, sort_cap=0, fold=LANES128, **LARGE_PLAN)
    check(plan(lib, 1024, 4098, device_sized=True), split=1, n_work=1024, sort=PLAIN, fold=HALF, **LARGE_PLAN)
    check(plan(lib, 127, 4098, {"BBP_SORT_STAGED": "7"}, device_sized=True), split=1, sort=STAGED_WIDE, sort_cap=32768, fold=LANES128, **LARGE_PLAN)


def test_split_knobs_and_clamps(lib):
    check(plan(lib, 3, 2933, {"BBP_MSM_SPLIT_BELOW": "0"}), split=1, n_sub=2933, **LARGE_PLAN)
    check(plan(lib, 200, 2933, {"BBP_MSM_SPLIT_BELOW": "256"}), split=2, n_sub=1467, n_work=400, **SMALL_PLAN)
    check(plan(lib, 3, 2933, {"BBP_MSM_SPLIT_TARGET": "8"}), split=2, n_sub=1467, n_work=6, **SMALL_PLAN)
    check(plan(lib, 3, 2933, {"BBP_MSM_SPLIT_TARGET": "2"}), split=1, n_sub=2933, **LARGE_PLAN)  # 2 / 3 = 0 workgroups: one
    check(plan(lib, 3, 2933, {"BBP_MSM_SPLIT_TARGET": "100000"}), split=16, n_sub=184, **SMALL_PLAN)
    for name, member, cases in (("BBP_SORT_STAGED", "sort_staged", {"0": 0, "3": 3, "7": 7, "8": 0, "15": 7}),
                                ("BBP_FOLD_HALF_FROM", "fold_half_from", {"-4": 1, "0": 1, "1": 1, "512": 512, "1000000": 1000000}),
                                ("BBP_MSM_SMALL", "msm_small", {"0": 0, "1": 1, "5": 1})):
        for text, want in cases.items():
            assert mc.knob_from_env(lib, name, text, member) == want, (name, text)
    defaults = dict(sort_staged=3, fold_half_from=512, msm_small=1, split_below=128, split_target=512)
    for member, want in defaults.items():
        assert mc.knob_from_env(lib, "BBP_NOT_A_KNOB", "1", member) == want, member
    with pytest.raises(AssertionError):
        plan(lib, 1, 1, {"BBP_SLICES": "2"})  # a prove knob is no MSM knob


def test_every_split_covers_its_terms(lib):
    """every n_msm in 1..127 and n_terms in 1..4097: split * n_sub >= n_terms, (split - 1) * n_sub < n_terms (no sub-MSM lies wholly
    past the end), split <= 16, and n_sub >= 128 whenever split > 1 -- looped in C"""
    bad, top = (ctypes.c_uint32 * 2)(), ctypes.c_uint32()
    n_bad = lib.hc_msm_split_sweep(127, 4097, bad, ctypes.byref(top))
    assert n_bad == 0, "first at n_msm %d, n_terms %d" % (bad[0], bad[1])
    assert top.value == 16


# ---- the coverage ledger ---------------------------------------------------------------------------------------------------------
def _check_counts(row, hist, neg, where):
    ops = {"==": lambda a, b: a == b, ">": lambda a, b: a > b, "<": lambda a, b: a < b, ">=": lambda a, b: a >= b}
    for bucket, rel, value in row.counts:
        assert ops[rel](hist[bucket], value), (where, bucket, hist[bucket], rel, value)
    if row.only is not None:
        assert {k for k, c in enumerate(hist) if c} == row.only, where
    if row.neg_half is not None:
        assert 2 * neg[row.neg_half] == hist[row.neg_half], where


@pytest.mark.parametrize("n_terms", sorted(mc.SHAPE_LAYOUT))
def test_ledger_bucket_rows_fill_the_image_as_named(lib, n_terms):
    """the bucket rows against the image capacity their launch's plan states: exact, one more, the window boundary, the direct passes"""
    p = plan(lib, mc.UNSPLIT_B, n_terms, mc.SETTINGS[mc.CAP_SETTING[n_terms]])
    assert p.split == 1 and p.sort in (STAGED, STAGED_WIDE) and p.naf == 12
    assert p.sort == (STAGED_WIDE if n_terms == 4097 else STAGED)
    cap = p.sort_cap
    rows = mc.unsplit_rows(lib, n_terms)
    assert set(rows) == set(mc.ROW_NAMES) - ({"adjacent_oversized"} if mc.SHAPE_LAYOUT[n_terms] == mc.LAYOUT_G else set()) | {"uniform"}
    for name, row in rows.items():
        assert len(row.scalars) == n_terms and all(0 <= v < mc.L for v in row.scalars), name
        hist, neg = mc.histogram(lib, p.naf, row.scalars, p.K)
        _check_counts(row, hist, neg, (n_terms, name))
        passes = mc.walk(hist, cap)
        if row.walk is not None:
            assert passes == row.walk, (n_terms, name, passes[:4])
        if name == "two_thirds_ones19":
            assert passes[0][0] == mc.two_thirds_first_pass(n_terms, cap) and passes[0][1][0] == 1, (n_terms, passes[0][0])
            assert n_terms == 1467 or passes[0] == ("direct", [1])  # oversized in both G || H shapes
        if name == "uniform":  # uniformly random scalars never outgrow the image: windows of many buckets only
            assert all(kind == "staged" for kind, _ in passes) and max(hist) < cap // 8 and len(passes) >= 2
    # what the rows are named for, in one place: the exact-capacity window, the smallest direct pass, a direct pass between two windows
    assert max(mc.histogram(lib, 12, rows["exact_capacity"].scalars, p.K)[0]) == cap
    assert max(mc.histogram(lib, 12, rows["capacity_plus_1"].scalars, p.K)[0]) == cap + 1
    if n_terms == 2933:
        assert 2.5 * cap < 19 * n_terms < 2.7 * cap  # the all-ones row: one bucket about 2.6 x the image


def test_ledger_every_new_case_takes_the_path_it_is_named_for(lib):
    reached = set()
    for c in mc.UNSPLIT_CASES:
        p = plan(lib, mc.UNSPLIT_B, c.n_terms, mc.SETTINGS[c.setting])
        assert mc.path(p) == c.path and p.split == 1 and not p.reduce, mc.case_id(c)
        assert c.row in mc.unsplit_rows(lib, c.n_terms), mc.case_id(c)
        reached.add((c.setting, c.n_terms, p.sort))
    assert len({mc.case_id(c) for c in mc.UNSPLIT_CASES}) == len(mc.UNSPLIT_CASES)
    # the direct pass and the exact-capacity window, the wide image, the unsplit plain scatter (knob off, and wide under the default)
    assert {("default", 2933, STAGED), ("default", 1467, STAGED), ("staged_wide", 4097, STAGED_WIDE), ("plain", 4097, PLAIN),
            ("default", 4097, PLAIN), ("staged_wide_half_fold", 4097, STAGED_WIDE)} == reached
    named = {(c.setting, c.n_terms, c.row) for c in mc.UNSPLIT_CASES}
    for setting, n_terms in (("default", 2933), ("default", 1467), ("staged_wide", 4097), ("plain", 4097), ("default", 4097)):
        for row in ("all_ones19", "exact_capacity", "capacity_plus_1", "boundary_between_1_and_2", "oversized_in_the_middle", "half_negative",
                    "two_thirds_ones19"):
            assert (setting, n_terms, row) in named
    assert ("default", 2933, "adjacent_oversized") in named and ("default", 1467, "adjacent_oversized") not in named
    assert ("staged_wide", 4097, "uniform") in named
    # the adversarial slots are the first, a middle and the last MSM of the smallest launch that is never split
    assert mc.ADVERSARIAL_AT[0] == 0 and 0 < mc.ADVERSARIAL_AT[1] < mc.UNSPLIT_B - 1 and mc.ADVERSARIAL_AT[2] == mc.UNSPLIT_B - 1
    assert plan(lib, mc.UNSPLIT_B - 1, 2933).split > 1 and plan(lib, mc.UNSPLIT_B, 2933).split == 1
    fill = mc.filler_rows(1467)
    assert sorted(set(fill) | set(mc.ADVERSARIAL_AT)) == list(range(mc.UNSPLIT_B)) and not set(mc.RANDOM_AT) & set(mc.ADVERSARIAL_AT)
    assert sum(1 for b, r in fill.items() if not any(r)) == 61 and sum(1 for r in fill.values() if sum(1 for v in r if v) == 1) == 60


def test_ledger_split_cases(lib):
    layout, n_terms, B = mc.SPLIT_SHAPE
    p = plan(lib, B, n_terms)
    check(p, split=16, n_sub=184, **SMALL_PLAN)
    rows = mc.split_rows(n_terms, p.n_sub)
    assert len(rows) == B and all(len(r) == n_terms and all(0 <= v < mc.L for v in r) for r in rows.values())
    assert not any(rows["all_zero"])
    live = [i for i, v in enumerate(rows["one_sub_msm"]) if v]
    assert len(live) == p.n_sub and {i // p.n_sub for i in live} == {mc.SPLIT_ONE_SUB} and mc.SPLIT_ONE_SUB < p.split
    hist, neg = mc.histogram(lib, p.naf, rows["width9_limits"], p.K)
    assert hist[p.K] > 200 and 0 < neg[p.K] < hist[p.K] and 0 < neg[1] < hist[1]  # digits +-255 and +-1, the width-9 limits
    for v, digits in ((0xFF, [255]), (0x101, [-255, 1]), (0x1FF, [-1, 1])):
        pos, dig = (ctypes.c_int32 * 32)(), (ctypes.c_int32 * 32)()
        n = lib.hc_sc_naf(9, v.to_bytes(32, "little"), pos, dig)
        assert list(dig[:n]) == digits, hex(v)
    kinds = {i % 7 for i in range(n_terms)}
    assert kinds == set(range(7))
    # every sub-MSM of the limits row holds terms (none is empty), the last one fewer than n_sub
    assert n_terms - (p.split - 1) * p.n_sub == 173


def test_ledger_existing_fuzz_lists(lib):
    """what the three lists of test_gpu_fuzz.py reach -- their docstrings say no more than this"""
    # the giant buckets of test_msm_sort_oversized_bucket: all split, whatever BBP_SORT_STAGED says
    for n_terms, B in mc.OVERSIZED_SPLIT_SHAPES:
        for staged in ("0", "3", "7"):
            p = plan(lib, B, n_terms, {"BBP_SORT_STAGED": staged})
            check(p, **SMALL_PLAN)
            assert p.split == 16
    for n_terms, B, rows in mc.oversized_split_cases():
        p = plan(lib, B, n_terms)
        hist, _ = mc.histogram(lib, 12, rows[0], 1024)
        assert hist[1] == 19 * n_terms and sum(hist) == hist[1]  # the width-12 view the rows were written for
        hist9, _ = mc.histogram(lib, p.naf, rows[0], p.K)
        assert hist9[1] == 19 * n_terms and sum(hist9) == hist9[1]  # ... and at the width the split launch recodes at: one giant bucket
    # test_msm_fuzz_half_wavefront_fold: the fold each shape is listed with; the last shape makes the full-width claim true
    reached = set()
    for layout, n_terms, B, fold in mc.HALF_FOLD_SHAPES:
        p = plan(lib, B, n_terms, mc.HALF_FOLD_KNOBS)
        assert p.fold == fold and (p.split > 1) == (fold == SMALL_FOLD), (n_terms, B)
        reached.add(mc.path(p))
    assert mc.HALF_FOLD_SHAPES[-1][1:] == (4097, 128, HALF)
    assert reached == {(LARGE, STAGED, HALF), (LARGE, PLAIN, HALF), (SMALL, PLAIN, SMALL_FOLD)}
    # test_msm_fuzz: launches of 700 terms and more have at most 9 MSMs and are split; the others reach the staged sort unsplit
    fuzz = set()
    for seed in mc.FUZZ_SEEDS:
        shapes = [(n_terms, B) for _, _, n_terms, B, _ in mc.fuzz_cases(seed)]
        assert len(shapes) == 14
        for n_terms, B in shapes:
            p = plan(lib, B, n_terms)
            assert n_terms < 700 or (B <= 9 and p.geom == SMALL), (seed, n_terms, B)
            assert p.sort != STAGED or 19 * n_terms < p.sort_cap  # ... with no bucket that could outgrow the image
            fuzz.add(mc.path(p))
    assert fuzz == {(LARGE, STAGED, LANES128), (SMALL, PLAIN, SMALL_FOLD)}


def test_ledger_union_reaches_every_combination(lib):
    """geometry x sort x fold: the combinations any knobs and shape can reach, and the cases that reach each"""
    reachable = set()
    for staged in range(8):
        for half_from in ("1", "512"):
            for small in ("0", "1"):
                knobs = {"BBP_SORT_STAGED": str(staged), "BBP_FOLD_HALF_FROM": half_from, "BBP_MSM_SMALL": small}
                for n_msm in (1, 3, 127, 128, 512):
                    for n_terms in (1, 255, 256, 2933, 3001, 4097, 65535):
                        reachable.add(mc.path(plan(lib, n_msm, n_terms, knobs)))
    assert reachable == {(SMALL, PLAIN, SMALL_FOLD)} | {(LARGE, s, f) for s in (PLAIN, STAGED, STAGED_WIDE) for f in (LANES128, HALF)}
    reached = {mc.path(plan(lib, mc.UNSPLIT_B, c.n_terms, mc.SETTINGS[c.setting])) for c in mc.UNSPLIT_CASES}
    reached.add(mc.path(plan(lib, mc.SPLIT_SHAPE[2], mc.SPLIT_SHAPE[1])))
    reached |= {mc.path(plan(lib, B, n_terms, mc.HALF_FOLD_KNOBS)) for _, n_terms, B, _ in mc.HALF_FOLD_SHAPES}
    assert reached == reachable
