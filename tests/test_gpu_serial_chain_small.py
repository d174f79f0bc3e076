"""GPU: the single-lane TranscriptRng draw chain (k_open_serial) and the one-lane transcript kernels on batches small enough for a
test.  By default batches this small take the cooperative chain and the wavefront transcripts and never reach the one-lane
permutation of csrc/keccak.h; a context created under BBP_RNG_COOP=0 BBP_TR_WAVE_BELOW=0 sends them through it.  B = 1, and 64 | 65
on either side of the serial kernels' 64-lane workgroup (`serial_blk`): records byte-equal to the C oracle's, all valid on the
same context, one flipped byte invalid."""
import os

import pytest

from tests import oracle_c
from tests.test_gpu_prove_verify import _synth_batch

pytestmark = pytest.mark.gpu
N, BMAX = 8, 65
KNOBS = {"BBP_RNG_COOP": "0", "BBP_TR_WAVE_BELOW": "0", "BBP_TRACE_PROVE": "1"}


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
    ins, ents, vins = _synth_batch(serial_ctx, BMAX, N, seed=2934)
    cout, cst = oc.prove_many(b"".join(ins), b"".join(ents), BMAX, N, threads=8)
    assert cst == [0] * BMAX
    return ins, ents, vins, cout


@pytest.mark.parametrize("B", [1, 64, 65])
def test_serial_chain_records_equal_the_oracle(bbp, serial_ctx, batch, capfd, B):
    ins, ents, vins, cout = batch
    rs_ = bbp.record_size(N)
    capfd.readouterr()
    out, st = serial_ctx.prove_batch(B, N, b"".join(ins[:B]), b"".join(ents[:B]))
    trace = [l for l in capfd.readouterr().err.splitlines() if l.startswith("prove call")]
    assert st == [0] * B
    assert len(trace) == 1 and trace[0].rstrip().endswith("coop 0"), trace  # the single-lane chain was taken
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
