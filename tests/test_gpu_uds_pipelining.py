"""GPU tier: pipelined requests on one connection of bbp-uds-server with the REAL engine on cuda:0 (--pipeline-depth 64, no
--reserve).  Replies come back in request order, every proof is accepted by Context.verify in this process and by the server's
own opcode 2, tampered ones are refused in their place; large verify frames (N = 202) written ahead are served, not dropped;
one connection's requests shared device batches.  The CPU tier has the same client against the stub (tests/test_uds_pipelining.py).
One server process for the module, started as a fresh child with its own time limit, never restarted."""
import os
import re
import signal
import subprocess
import tempfile
import time

import pytest

from tests import uds_client as uc
from tests.test_gpu_prove_verify import _synth_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def server(built, bbp):
    built.build_server()
    d = tempfile.mkdtemp(prefix="bbp-uds-gpu-pipe-")
    path = os.path.join(d, "sock")
    err = open(os.path.join(d, "log"), "w+")
    p = subprocess.Popen([built.SERVER_BIN, "-b", path, "-l", "info", "--engine", bbp.lib_path, "--device", "0", "--window-us", "500", "--pipeline-depth", "64"],
                         stderr=err)
    for _ in range(1500):  # 30 s for the engine to come up
        if os.path.exists(path) or p.poll() is not None:
            break
        time.sleep(0.02)
    assert os.path.exists(path), "server did not bind: " + open(err.name).read()[-800:]
    yield {"path": path, "proc": p, "log": err}
    if p.poll() is None:
        p.send_signal(signal.SIGTERM)
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()


def _blob(record, n):
    """raw record (R1CSProof || 4 commitments || N t_c) -> the wire's proof blob"""
    pts = [record[1121 + 32 * i:1121 + 32 * (i + 1)] for i in range(4 + n)]
    return uc.tlv(record[:1121]) + uc.tlv_list(pts[:4]) + uc.tlv_list(pts[4:])


def _tampered(blob, i):
    bad = bytearray(blob)
    bad[300 + i] ^= 0x04
    return bytes(bad)


def test_pipelined_proves_then_verifies_on_one_connection(ctx, server):
    N, B = 8, 32
    ins, _, vins = _synth_batch(ctx, B, N, seed=8140)
    c = uc.Conn(server["path"])
    for i in range(B):  # every frame written before anything is read
        c.send(uc.prove_request(ins[i][:224], ins[i][224:224 + 32 * N], int.from_bytes(ins[i][-8:], "little")))
    blobs = [c.recv_frame() for _ in range(B)]
    assert all(b is not None for b in blobs)
    for i, blob in enumerate(blobs):  # in request order: blob i proves bid i and no other
        proof, cm, t = uc.decode_proof(blob)
        assert len(proof) == 1121 and len(cm) == 4 and len(t) == N
        assert ctx.verify(proof + b"".join(cm) + b"".join(t), *vins[i]) == 0, i
    bad_at = {3: 5, 11: 11, 20: 0, 35: 31}  # position in the pipeline -> the proof that is sent there tampered
    frames, want, nxt = [], [], 0
    for pos in range(B + len(bad_at)):
        if pos in bad_at:
            frames.append(uc.verify_request(_tampered(blobs[bad_at[pos]], pos), *vins[bad_at[pos]]))
            want.append(b"\x00")
        else:
            frames.append(uc.verify_request(blobs[nxt], *vins[nxt]))
            want.append(b"\x01")
            nxt += 1
    for f in frames:
        c.send(f)
    assert [c.recv_frame() for _ in frames] == want
    c.close()


def test_large_verify_frames_written_ahead_are_served(ctx, server):
    """12 verify frames of ~14 KB each: more than the parent's per-connection buffer, which used to end in a dropped connection."""
    N, B = 202, 12
    ins, _, vins = _synth_batch(ctx, B, N, seed=8141)
    recs, status = ctx.prove_batch(B, N, b"".join(ins))
    assert status == [0] * B
    rs = len(recs) // B
    blobs = [_blob(recs[rs * i:rs * (i + 1)], N) for i in range(B)]
    frames = [uc.verify_request(_tampered(blobs[i], i) if i in (4, 9) else blobs[i], *vins[i]) for i in range(B)]
    assert sum(map(len, frames)) > 2 * (1 << 16) + 16
    c = uc.Conn(server["path"])
    for f in frames:
        c.send(f)
    assert [c.recv_frame() for _ in range(B)] == [b"\x00" if i in (4, 9) else b"\x01" for i in range(B)]
    c.close()


def test_shutdown_line_shows_batches_from_one_connection(server):
    """Last test of the module: stop the server and read its shutdown line."""
    server["proc"].send_signal(signal.SIGTERM)
    assert server["proc"].wait(timeout=30) == 0
    server["log"].seek(0)
    log = server["log"].read()
    m = re.search(r"served (\d+) requests \((\d+) errors\) in (\d+) device calls, largest batch (\d+), deepest pipeline (\d+)", log)
    assert m, log[-800:]
    served, errs, calls, biggest, deepest = map(int, m.groups())
    assert served == 32 + 36 + 12 and errs == 0, m.group(0)  # the tampered verifies are served, not errors
    assert biggest >= 4 and calls < served and 4 <= deepest <= 64, m.group(0)
