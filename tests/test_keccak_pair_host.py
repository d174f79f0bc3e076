"""not-gpu tier: the pair form of Keccak-f[1600] and of the steady-state TranscriptRng draws (csrc/keccak.h: a state split over two
lanes, low words in one, high words in the other) as its plain-C model, which is built from the phase functions the device runs.
tests/keccak_pair_check.cpp is a stand-alone program under AddressSanitizer + UBSan; nothing is loaded into this process.

The permutation against the Python one: the zero state, all-ones, a single set bit at positions 0, 31, 32 and 63 (the edges of the
two halves) of each of the 25 lanes (lanes 0 and 24 among them), and 64 seeded random states.  The draw loop: 5 draws against the
one-lane merlin_rng_fill64_bulk compiled for the host, raw bytes and final state."""
import random
import subprocess

import pytest

from oracle.ref_py import merlin


def _states():
    ones = (1 << 1600) - 1
    single = [1 << (64 * lane + bit) for lane in range(25) for bit in (0, 31, 32, 63)]
    rnd = random.Random(0x70616972)
    return [v.to_bytes(200, "little") for v in [0, ones] + single + [rnd.getrandbits(1600) for _ in range(64)]]


def _ref(st):
    s = bytearray(st)
    merlin.keccak_f1600(s)
    return bytes(s)


@pytest.fixture(scope="module")
def binary(built):
    return built.build_keccak_pair_check()


def test_pair_model_permutation_equals_the_python_permutation(binary):
    sts = _states()
    assert len(sts) == 2 + 100 + 64 and len(set(sts)) == len(sts)
    r = subprocess.run([binary, "perm"], input=b"".join(sts), capture_output=True, timeout=300)
    assert r.returncode == 0 and len(r.stdout) == 200 * len(sts), (r.returncode, len(r.stdout), r.stderr[-2000:])
    got = [r.stdout[200 * i:200 * i + 200] for i in range(len(sts))]
    assert got[0][:8] == bytes.fromhex("e7dde140798f25f1")  # Keccak-f[1600] of the zero state, first lane
    bad = [i for i, s in enumerate(sts) if got[i] != _ref(s)]
    assert not bad, (len(bad), bad[:10])


def test_pair_model_draws_equal_the_one_lane_chain(binary):
    r = subprocess.run([binary, "draws"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "keccak_pair_check ok" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
