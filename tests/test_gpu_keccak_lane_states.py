"""GPU: the one-lane Keccak-f[1600] of csrc/keccak.h as compiled for gfx950 (every Boolean step one v_bitop3_b32 per half-word)
against the Python permutation, on states that reach each of the 170 three-input sites of a round with a pattern of their own:
the 1600 single-bit states, their 1600 complements, all-zero, all-ones and 64 seeded random states.  A wrong operand order or
table in any site flips at least one of them."""
import ctypes
import random

import pytest

from oracle.ref_py import merlin
from tests.test_gpu_device_arith import load

pytestmark = pytest.mark.gpu


def _states():
    ones = (1 << 1600) - 1
    single = [1 << bit for bit in range(1600)]
    rnd = random.Random(0x6B656363)
    vals = single + [ones ^ s for s in single] + [0, ones] + [rnd.getrandbits(1600) for _ in range(64)]
    return [v.to_bytes(200, "little") for v in vals]


def _ref(st):
    s = bytearray(st)
    merlin.keccak_f1600(s)
    return bytes(s)


@pytest.fixture(scope="module")
def cases():
    sts = _states()
    return sts, [_ref(s) for s in sts]


@pytest.fixture(scope="module")
def lib(built, bbp):  # bbp: torch's HIP runtime loads first (conftest.py)
    return load(built.build_devcheck("chain"))


def test_case_list(cases):
    sts, want = cases
    assert len(sts) == 1600 + 1600 + 2 + 64 and len(set(sts)) == len(sts)
    assert sts[0] == b"\x01" + bytes(199) and sts[1600] == b"\xfe" + b"\xff" * 199
    assert sts[3200] == bytes(200) and sts[3201] == b"\xff" * 200
    # Keccak-f[1600] of the zero state, first lane (the Keccak team's test vector): the Python reference is the permutation
    assert want[3200][:8] == bytes.fromhex("e7dde140798f25f1")


def test_one_lane_permutation_on_every_state(lib, cases):
    sts, want = cases
    n = len(sts)
    buf = ctypes.create_string_buffer(b"".join(sts), 200 * n)
    assert lib.dc_keccak_f(n, buf) == 0
    raw = buf.raw
    bad = [i for i in range(n) if raw[200 * i:200 * i + 200] != want[i]]
    assert not bad, (len(bad), bad[:10])
