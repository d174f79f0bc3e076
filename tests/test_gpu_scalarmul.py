"""gpu tier: csrc/scalarmul.h as hipcc compiles it for gfx950 (tests/device_check.hip) against the big-int oracle: the Pedersen comb
on one lane and on eight, the comb table, the tail tables with their carry-mask walk (whole, by shares, and two terms on one doubling
chain) and the verifier's Straus steps walked from the top digit and spread over 32 lanes.  The scalars are the battery of
tests/scalarmul_cases.py, whose ledger tests/test_scalarmul_cases_host.py asserts; tests/test_scalarmul_host.py runs the same cases
on the CPU.  Every output is compared byte for byte: these are group elements, there is no tolerance.  Both device-check variants."""
import ctypes

import pytest

from tests import scalarmul_cases as sm
from tests.scalarmul_run import Runner

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=("chain", "nochain"))
def run(request, built, bbp):  # bbp: torch's HIP runtime loads first (conftest.py)
    return Runner(ctypes.CDLL(built.build_devcheck(request.param)), "dc", request.param)


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
