"""GPU: the pair form of the serial draw chain (csrc/keccak.h "pair form": two adjacent lanes per proof, half a Keccak state each,
the partner's word through a DPP move).

The permutation as compiled for gfx950 (tests/device_check_pair.hip dc_keccak_f_pair) on the 3266 states of
tests/test_gpu_keccak_lane_states.py -- a wrong operand order in any of the 29 rotation sites or 85 three-input sites of a half
flips at least one single-bit state -- and on n = 1, 31, 32, 33 states, where the last wavefront (32 states) is partial.

Proving through k_open_serial's whole-chain form on a context created under BBP_RNG_COOP=0 BBP_TR_WAVE_BELOW=0: B = 1, and 32 | 33
and 65 on either side of a wavefront (32 proofs) and of the 64-proof workgroup; records byte-equal to the C oracle's, all valid,
one flipped byte invalid, health() 0 at the end."""
import ctypes
import os

import pytest

from tests import oracle_c
from tests.test_gpu_keccak_lane_states import _ref, _states
from tests.test_gpu_prove_verify import _synth_batch

pytestmark = pytest.mark.gpu
N, BMAX = 8, 65
KNOBS = {"BBP_RNG_COOP": "0", "BBP_TR_WAVE_BELOW": "0", "BBP_TRACE_PROVE": "1"}


@pytest.fixture(scope="module")
def cases():
    sts = _states()
    return sts, [_ref(s) for s in sts]


@pytest.fixture(scope="module")
def lib(built, bbp):  # bbp: torch's HIP runtime loads first (conftest.py)
    lib = ctypes.CDLL(built.build_devcheck_pair())
    lib.dc_keccak_f_pair.argtypes = [ctypes.c_int, ctypes.c_char_p]
    lib.dc_keccak_f_pair.restype = ctypes.c_int
    return lib


def _run(lib, sts):
    buf = ctypes.create_string_buffer(b"".join(sts), 200 * len(sts))
    assert lib.dc_keccak_f_pair(len(sts), buf) == 0
    return [buf.raw[200 * i:200 * i + 200] for i in range(len(sts))]


def test_pair_permutation_on_every_state(lib, cases):
    sts, want = cases
    assert len(sts) == 3266
    got = _run(lib, sts)
    bad = [i for i in range(len(sts)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_pair_permutation_with_a_partial_last_wavefront(lib, cases, n):
    sts, want = cases
    first = 3202  # the seeded random states
    assert _run(lib, sts[first:first + n]) == want[first:first + n]


@pytest.fixture(scope="module")
def serial_ctx(bbp):
    old = {k: os.environ.get(k) for k in KNOBS}
    os.environ.update(KNOBS)
    try:
        c = bbp.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


@pytest.fixture(scope="module")
def batch(built, serial_ctx):
    """65 rows and the C oracle's records for them, computed once: row i does not depend on the batch it is in"""
    oc = oracle_c.load(built.build_oracle())
    ins, ents, vins = _synth_batch(serial_ctx, BMAX, N, seed=2727)
    cout, cst = oc.prove_many(b"".join(ins), b"".join(ents), BMAX, N, threads=8)
    assert cst == [0] * BMAX
    return ins, ents, vins, cout


@pytest.mark.parametrize("B", [1, 32, 33, 65])
def test_pair_chain_records_equal_the_oracle(bbp, serial_ctx, batch, capfd, B):
    ins, ents, vins, cout = batch
    rs_ = bbp.record_size(N)
    capfd.readouterr()
    out, st = serial_ctx.prove_batch(B, N, b"".join(ins[:B]), b"".join(ents[:B]))
    trace = [l for l in capfd.readouterr().err.splitlines() if l.startswith("prove call")]
    assert st == [0] * B
    assert len(trace) == 1 and trace[0].rstrip().endswith("coop 0"), trace  # the whole serial chain was taken
    bad = [i for i in range(B) if out[i * rs_:(i + 1) * rs_] != cout[i * rs_:(i + 1) * rs_]]
    assert not bad, bad[:10]
    rows = [out[i * rs_:(i + 1) * rs_] + b"".join(vins[i]) for i in range(B)]
    assert serial_ctx.verify_batch(B, N, b"".join(rows)) == [0] * B
    flipped = B - 1
    row = bytearray(rows[flipped])
    row[200] ^= 0x10
    rows[flipped] = bytes(row)
    exp = [0] * B
    exp[flipped] = 1
    assert serial_ctx.verify_batch(B, N, b"".join(rows)) == exp
    assert serial_ctx.health() == 0
