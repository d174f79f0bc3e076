"""CPU tier: csrc/scalarmul.h compiled for the host (tests/host_check.cpp) against the big-int oracle, with the batteries of
tests/scalarmul_cases.py -- the host twin of tests/test_gpu_scalarmul.py, same cases, same checks.  What the device does with wave
shuffles is a loop over the lanes' partial sums here."""
import ctypes

import pytest

from tests import scalarmul_cases as sm
from tests.scalarmul_run import Runner


@pytest.fixture(scope="module")
def run(built):
    return Runner(ctypes.CDLL(built.build_hostcheck()), "hc", "host")


def test_comb(run):
    assert sm.check_comb(run) > 1000


def test_comb_table(run):
    assert sm.check_comb_table(run) == 4 * 512


def test_tail(run):
    assert sm.check_tail(run) > 1000


def test_tail_pair(run):
    assert sm.check_tail_pair(run) > 1000


def test_straus(run):
    assert sm.check_straus(run) > 1000
