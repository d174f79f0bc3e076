"""not-gpu tier: the staged MSM sort's one-walk recoding on the CPU (tests/sort_digits_check.cpp compiles csrc/scalar.h's packed digits
next to the callback recoder they restate).  The kernel keeps a scalar's digits in registers, one 16-bit slot per digit: every digit
the recoding can emit must survive the packing, the slots must hold exactly the callback recoder's digits, and no scalar may have
more digits than the sorted scratch reserves per term (MSM_W / SMALL_W)."""
import random

import pytest

from tests import msm_cases as mc
from tests import sort_cases as sc


@pytest.fixture(scope="module")
def lib(built):
    return sc.load(built.build_sortcheck())


@pytest.fixture(scope="module")
def planlib(built):
    import ctypes
    return ctypes.CDLL(built.build_hostcheck())


@pytest.mark.parametrize("width", [9, 12])
def test_every_digit_survives_the_packing(lib, width):
    # positions 0..253, odd magnitudes below 2^(width - 1), both signs
    assert lib.sd_roundtrip(width) == 254 * (1 << (width - 2)) * 2


def test_slots_and_scratch_bounds(lib):
    b = sc.bounds(lib)
    assert b["MSM_W"] <= b["slots12"] == 24 and b["SMALL_W"] <= b["slots9"] == 32
    assert b["staged_max_terms"] == 5 * 1024 >= 4098


@pytest.mark.parametrize("n", sc.TERMS)
def test_gpu_case_rows_recode_alike_and_within_the_reserved_digits(lib, n):
    b = sc.bounds(lib)
    for name, rows in sc.rows(n).items():
        for row in rows:
            for width, most_allowed in ((12, b["MSM_W"]), (9, b["SMALL_W"])):
                rc, most = sc.compare(lib, width, row)
                assert rc == 0, (name, width, rc - 1)
                assert most <= most_allowed, (name, width, most)


def test_limit_patterns_recode_alike(lib):
    """the recoding's limits at every bit offset (digits at the magnitude limit around a carry, long carry chains, the ends of the
    range), the fuzz tests' pattern scalars, and the densest rows: digits exactly `width` + 1 bits apart"""
    b = sc.bounds(lib)
    rnd = random.Random(1612)
    row = [mc.width9_limit_scalar(i) for i in range(3000)] + [mc.pattern_scalar(rnd) for _ in range(3000)]
    row += [(0x7FF << s) % mc.L for s in range(242)] + [(0x801 << s) % mc.L for s in range(242)] + [(0xFFF << s) % mc.L for s in range(242)]
    row += [sum(1 << (13 * j + o) for j in range(19)) for o in range(7)] + [sum(1 << (10 * j + o) for j in range(25)) for o in range(4)]
    row += [(1 << k) - 1 for k in range(1, 254)] + [1 << k for k in range(254)]
    for width, most_allowed in ((12, b["MSM_W"]), (9, b["SMALL_W"])):
        rc, most = sc.compare(lib, width, row)
        assert rc == 0, (width, rc - 1)
        assert most <= most_allowed, (width, most)


def test_plan_stages_only_what_the_lanes_hold(lib, planlib):
    """the staged kernel holds at most five scalars on each of its 1024 lanes: a longer (sub-)MSM is planned onto the plain scatter,
    whatever the knob says"""
    cap = sc.bounds(lib)["staged_max_terms"]
    for knobs in ({}, {"BBP_SORT_STAGED": "7"}):
        assert mc.plan(planlib, 128, cap + 1, knobs).sort == mc.PLAIN
        assert mc.plan(planlib, 128, 65535, knobs).sort == mc.PLAIN
    assert mc.plan(planlib, 128, cap, {"BBP_SORT_STAGED": "7"}).sort == mc.STAGED_WIDE
    assert mc.plan(planlib, 128, 2933).sort == mc.STAGED
