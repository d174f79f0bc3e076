"""not-gpu tier: pipelined requests on ONE connection of bbp-uds-server (--pipeline-depth, --max-inflight) against the stub engine --
replies strictly in request order whatever order the engine finishes in, reads paused instead of the connection dropped, the
reference's per-request error rule applied at the request's position ("poisoning"), half-close, abandoned pipelines, a device
failure inside a pipeline, the global bound; the same cases against stand-alone sanitizer builds of the server; the load
generator's --depth.  The GPU tier runs the real engine behind the same client (tests/test_gpu_uds_pipelining.py)."""
import json
import os
import platform
import re
import shutil
import signal
import socket
import subprocess
import sys
import tempfile
import threading
import time

import pytest

from tests import uds_client as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHUTDOWN_LINE = r"served (\d+) requests \((\d+) errors\) in (\d+) device calls, largest batch (\d+), deepest pipeline (\d+)"
SANITIZER_REPORT = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "WARNING: ThreadSanitizer")


def _bid(i, n):
    s7 = b"".join(bytes([(7 * i + k) & 0xff]) * 31 + b"\x01" for k in range(7))
    pub = b"".join(bytes([(11 * i + j) & 0xff]) * 31 + b"\x02" for j in range(n))
    return s7, pub, i % n


def _qzs(s7):
    return s7[128:160], s7[160:192], s7[192:224]


class Server:
    """one server process on a socket of its own; flavour None = the shipped binary, "asan" / "tsan" = the sanitizer builds"""

    def __init__(self, built, flags=(), env=None, flavour=None):
        built.build_server()
        exe = built.SERVER_BIN if flavour is None else built.build_server_san(flavour)
        stub = built.build_stub_engine_refusing(flavour)
        cmd = [exe]
        if flavour == "tsan":  # ThreadSanitizer's fixed shadow addresses: no address randomisation for this child (see test_uds_server.py)
            setarch = shutil.which("setarch")
            if setarch and subprocess.run([setarch, platform.machine(), "-R", "true"], capture_output=True).returncode == 0:
                cmd = [setarch, platform.machine(), "-R", exe]
        d = tempfile.mkdtemp(prefix="bbp-uds-pipe-")
        self.path = os.path.join(d, "sock")
        self.log = open(os.path.join(d, "log"), "w+")
        self.proc = subprocess.Popen(cmd + ["-b", self.path, "-l", "info", "--engine", stub] + list(flags), stderr=self.log,
                                     env=dict(os.environ, **(env or {})))
        for _ in range(500):
            if os.path.exists(self.path) or self.proc.poll() is not None:
                break
            time.sleep(0.02)
        assert os.path.exists(self.path), "server did not bind: " + self.text()[-800:]

    def text(self):
        self.log.seek(0)
        return self.log.read()

    def stop(self, timeout=10):
        """SIGTERM -> (exit status, log)"""
        if self.proc.poll() is None:
            self.proc.send_signal(signal.SIGTERM)
        try:
            rc = self.proc.wait(timeout=timeout)
        except subprocess.TimeoutExpired:
            self.proc.kill()
            self.proc.wait()
            raise
        return rc, self.text()

    def kill(self):
        if self.proc.poll() is None:
            self.proc.kill()
            self.proc.wait()


def _stats(text):
    m = re.search(SHUTDOWN_LINE, text)
    assert m, text[-800:]
    return dict(zip(("served", "errors", "calls", "biggest", "deepest"), map(int, m.groups())))


def _pipeline(path, frames, half_close=False):
    """write every frame on one connection without waiting, reading on a second thread -> the replies up to EOF (at most one
    more than the frames, so that a reply nobody asked for would show)"""
    c = uc.Conn(path)
    replies = []

    def reader():
        for _ in range(len(frames) + 1):
            r = c.recv_frame()
            if r is None:
                return
            replies.append(r)

    t = threading.Thread(target=reader)
    t.start()
    try:
        for f in frames:
            c.send(f)
        if half_close:
            c.s.shutdown(socket.SHUT_WR)
    except (BrokenPipeError, ConnectionResetError):
        pass  # the server closed a poisoned connection while the rest was being written
    return c, t, replies


def _finish(c, t, timeout=60):
    t.join(timeout)
    assert not t.is_alive(), "the connection neither answered everything nor closed"
    c.close()


def _proved(path, i, n):
    s7, pub, toggle = _bid(i, n)
    blob = uc.prove(path, s7, pub, toggle)
    assert blob is not None
    return s7, pub, blob


def _tampered(blob):
    bad = bytearray(blob)
    bad[100] ^= 1
    return bytes(bad)


# ---- the cases, written once and run against whichever server they are given ---------------------------------------------------------
def _case_large_verify_pipeline(srv):
    """64 verify frames at N = 202 (~0.9 MB) written before anything is read, every third tampered"""
    s7, pub, blob = _proved(srv.path, 5, 202)
    q, z, seed = _qzs(s7)
    frames = [uc.verify_request(_tampered(blob) if i % 3 == 2 else blob, q, z, seed, pub) for i in range(64)]
    assert sum(map(len, frames)) > 800 * 1024 and len(frames[0]) < (1 << 16)
    c = uc.Conn(srv.path)
    for f in frames:  # nothing is read until every byte is written: the 64 three-byte replies fit the socket buffer unread, and the
        c.send(f)     # server keeps taking frames as completed requests make room (a send that stalls for good ends in the timeout)
    replies = [c.recv_frame() for _ in range(64)]
    assert replies == [b"\x00" if i % 3 == 2 else b"\x01" for i in range(64)], replies
    c.s.settimeout(0.2)
    with pytest.raises(socket.timeout):  # exactly 64: nothing follows
        c.s.recv(1)
    c.close()
    assert uc.verify(srv.path, blob, q, z, seed, pub) == b"\x01"  # still serving


POISON_FRAMES = {
    "prove parse error": lambda s7, pub: uc.tlv(b"\x01" + b"".join(uc.tlv(s7[32 * i:32 * i + 32]) for i in range(6))),
    "prove refused by the engine at once": lambda s7, pub: uc.prove_request(*_bid(90, 5)),           # STUB_REFUSE_ITEMS=5
    "prove completes with an error": lambda s7, pub: uc.prove_request(s7[:31] + b"\xff" + s7[32:], pub, 0),  # non-canonical d
    "undefined opcode": lambda s7, pub: uc.tlv(b"\x07hello"),
    "empty request": lambda s7, pub: uc.tlv(b""),
    "unreadable frame header": lambda s7, pub: b"\x03\x00\x00\x00",
    "frame over MAX_FRAME": lambda s7, pub: b"\x04" + ((1 << 16) + 1).to_bytes(4, "little") + b"\x01" * 64,
}


def _case_poisoning(srv):
    """[good prove, good verify, BAD, good verify, good prove] -> two replies, then EOF; a malformed verify is an ordinary 0x00.
    -> (replies written, errors) as the server must have counted them"""
    s7, pub, blob = _proved(srv.path, 31, 4)
    q, z, seed = _qzs(s7)
    s7b, pubb, togb = _bid(32, 4)
    good_p, good_v = uc.prove_request(s7b, pubb, togb), uc.verify_request(blob, q, z, seed, pub)
    want_blob = uc.prove(srv.path, s7b, pubb, togb)
    served, errors = 2, 0
    for name, bad in POISON_FRAMES.items():
        c, t, replies = _pipeline(srv.path, [good_p, good_v, bad(s7, pub), good_v, good_p])
        _finish(c, t)
        assert replies == [want_blob, b"\x01"], (name, [r[:8] for r in replies])
        assert uc.verify(srv.path, blob, q, z, seed, pub) == b"\x01", name  # a fresh connection is served
        served, errors = served + 3, errors + 1
    c, t, replies = _pipeline(srv.path, [good_p, good_v, uc.tlv(b"\x02"), good_v, good_p], half_close=True)
    _finish(c, t)
    assert replies == [want_blob, b"\x01", b"\x00", b"\x01", want_blob]
    return served + 5, errors


def _case_abandoned_pipelines(srv):
    """20 connections write 64 prove frames each and close without reading; a bystander is served meanwhile"""
    frames = b"".join(uc.prove_request(*_bid(200 + i, 8)) for i in range(64))
    for _ in range(20):
        c = uc.Conn(srv.path)
        c.send(frames)
        c.close()
    s7, pub, blob = _proved(srv.path, 7, 8)
    assert uc.verify(srv.path, blob, *_qzs(s7), pub) == b"\x01"


# ---- case 1 ------------------------------------------------------------------------------------------------------------------------
def test_large_verify_frames_pipelined_are_not_dropped(built):
    """The connection used to be dropped once ~131 KB were buffered behind a request that was with the engine."""
    srv = Server(built)
    try:
        _case_large_verify_pipeline(srv)
        rc, text = srv.stop()
    finally:
        srv.kill()
    assert rc == 0 and _stats(text)["errors"] == 0, text[-600:]


# ---- cases 2 and 3 -------------------------------------------------------------------------------------------------------------------
def _prove_burst(built, depth):
    srv = Server(built, ["--pipeline-depth", str(depth), "--window-us", "2000"])
    try:
        c, t, replies = _pipeline(srv.path, [uc.prove_request(*_bid(300 + i, 8)) for i in range(256)], half_close=True)
        _finish(c, t, timeout=120)
        assert len(replies) == 256 and all(len(uc.decode_proof(r)[2]) == 8 for r in replies)
        rc, text = srv.stop()
    finally:
        srv.kill()
    assert rc == 0, text[-600:]
    assert "pipeline depth %d" % depth in text
    return _stats(text)


def test_one_connection_fills_batches(built):
    """256 proves back to back on ONE connection become batches: the thresholds test_concurrent_connections_are_micro_batched
    asks of 48 connections.  (Every batch from one connection used to have size 1.)"""
    s = _prove_burst(built, 256)
    assert s["served"] == 256 and s["errors"] == 0, s
    assert s["calls"] < s["served"] // 2 and s["biggest"] >= 4, s
    assert 4 <= s["deepest"] <= 256, s


def test_pipeline_depth_1_is_one_request_at_a_time(built):
    s = _prove_burst(built, 1)
    assert s["served"] == 256 and s["errors"] == 0, s
    assert s["biggest"] == 1 and s["calls"] == 256 and s["deepest"] == 1, s


# ---- case 4 ------------------------------------------------------------------------------------------------------------------------
def test_replies_keep_request_order_when_completions_do_not(built):
    """prove(i), verify, prove(i+1), verify, ..: a prove takes 20 ms in the stub, a verify 1 ms on the other combiner lane, so
    every verify is done before the prove written ahead of it.  The peer still sees blob, 0x01, blob, 0x01, .. and every blob is
    the one of its own inputs."""
    srv = Server(built, ["--window-us", "200"], env={"STUB_PROVE_US": "20000"})
    try:
        s7, pub, blob = _proved(srv.path, 3, 4)
        vframe = uc.verify_request(blob, *_qzs(s7), pub)
        bids, want = [], []
        for i in range(40, 120):  # the stub's tag is one byte of its inputs: take bids whose blobs differ from each other
            b = _bid(i, 4)
            w = uc.prove(srv.path, *b)
            if w not in want:
                bids.append(b)
                want.append(w)
            if len(want) == 8:
                break
        assert len(want) == 8
        frames = []
        for b in bids:
            frames += [uc.prove_request(*b), vframe]
        c, t, replies = _pipeline(srv.path, frames, half_close=True)
        _finish(c, t)
        assert replies == [x for w in want for x in (w, b"\x01")]
        rc, text = srv.stop()
    finally:
        srv.kill()
    assert rc == 0 and _stats(text)["errors"] == 0


# ---- case 5 ------------------------------------------------------------------------------------------------------------------------
def test_a_bad_request_poisons_its_connection_at_its_position(built):
    srv = Server(built, ["--window-us", "500"], env={"STUB_REFUSE_ITEMS": "5"})
    try:
        served, errors = _case_poisoning(srv)
        rc, text = srv.stop()
    finally:
        srv.kill()
    s = _stats(text)
    assert rc == 0 and "still with the engine" not in text, text[-600:]
    # one error per poisoned request, one served per reply written (what was dispatched behind a poisoned request is discarded)
    assert s["errors"] == errors == len(POISON_FRAMES) and s["served"] == served, (s, served, errors)


# ---- case 6 ------------------------------------------------------------------------------------------------------------------------
def test_half_close_serves_every_complete_frame(built):
    srv = Server(built, ["--window-us", "500"])
    try:
        s7, pub, blob = _proved(srv.path, 9, 4)
        vframe = uc.verify_request(blob, *_qzs(s7), pub)
        frames = [vframe if i % 2 else uc.prove_request(*_bid(60 + i, 4)) for i in range(32)]
        c, t, replies = _pipeline(srv.path, frames, half_close=True)
        _finish(c, t)
        assert len(replies) == 32 and all(r == b"\x01" for r in replies[1::2]) and all(len(uc.decode_proof(r)[2]) == 4 for r in replies[0::2])
        assert "unreadable frame" not in srv.text()
        c, t, replies = _pipeline(srv.path, frames[:31] + [frames[31][:-7]], half_close=True)  # the stream ends inside the 32nd frame
        _finish(c, t)
        assert len(replies) == 31 and replies[1::2] == [b"\x01"] * 15
        rc, text = srv.stop()
    finally:
        srv.kill()
    s = _stats(text)
    assert rc == 0 and text.count("unreadable frame") == 1 and s["errors"] == 1 and s["served"] == 1 + 32 + 31, (s, text[-600:])


# ---- case 7 ------------------------------------------------------------------------------------------------------------------------
def test_abandoned_pipelines_cost_nothing(built):
    srv = Server(built)
    try:
        _case_abandoned_pipelines(srv)
        t0 = time.time()
        rc, text = srv.stop(timeout=10)
    finally:
        srv.kill()
    assert rc == 0 and time.time() - t0 < 10 and "still with the engine" not in text, text[-600:]


# ---- case 8 ------------------------------------------------------------------------------------------------------------------------
def test_device_failure_inside_a_pipeline_answers_nothing_unjudged(built):
    """The third engine call and every later one report a dead device.  64 verifies are in flight on one connection: whatever is
    answered is a verdict of a call that ran, in order; nothing is answered for a request of a failed call; exit status 3."""
    srv = Server(built, ["--window-us", "2000", "--max-batch", "16"], env={"STUB_DEVICE_FAIL_AFTER": "3"})  # 64 verifies = four calls at least
    try:
        s7, pub, blob = _proved(srv.path, 21, 4)                                                    # call 1
        q, z, seed = _qzs(s7)
        want = [b"\x00" if i % 3 == 2 else b"\x01" for i in range(64)]
        c, t, replies = _pipeline(srv.path, [uc.verify_request(_tampered(blob) if i % 3 == 2 else blob, q, z, seed, pub) for i in range(64)])
        _finish(c, t)
        assert srv.proc.wait(timeout=15) == 3
        text = srv.text()
    finally:
        srv.kill()
    assert len(replies) < 64 and replies == want[:len(replies)], replies  # call 2 judged a first batch at the most
    assert "device failure" in text and "exiting with status 3" in text, text[-600:]
    assert _stats(text)["served"] == 1 + len(replies)


# ---- case 9 ------------------------------------------------------------------------------------------------------------------------
def test_max_inflight_bounds_requests_with_the_engine(built):
    srv = Server(built, ["--max-inflight", "8", "--pipeline-depth", "64", "--window-us", "500"])
    try:
        runs = [_pipeline(srv.path, [uc.prove_request(*_bid(400 + 64 * k + i, 8)) for i in range(64)], half_close=True) for k in range(4)]
        for c, t, replies in runs:
            _finish(c, t)
            assert len(replies) == 64 and all(len(uc.decode_proof(r)[2]) == 8 for r in replies)
        rc, text = srv.stop()
    finally:
        srv.kill()
    m = re.search(r"peak requests with the engine at once: (\d+) \(max inflight 8\)", text)
    assert rc == 0 and m, text[-600:]
    assert 2 <= int(m.group(1)) <= 8 + 4, m.group(0)  # the bound, plus each connection's always-admitted first request
    assert _stats(text)["served"] == 256 and "max inflight 8" in text


# ---- case 10 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["asan", "tsan"])
def test_pipelining_under_sanitizers(built, flavour):
    """The server and the stub engine it dlopens, both built with -fsanitize=address,undefined (then -fsanitize=thread) as binaries
    of their own: the large-frame pipeline, the poisoning sequences and the abandoned pipelines, a clean exit, no report."""
    srv = Server(built, ["--window-us", "500"], env={"STUB_REFUSE_ITEMS": "5"}, flavour=flavour)
    try:
        _case_large_verify_pipeline(srv)
        _case_poisoning(srv)
        _case_abandoned_pipelines(srv)
        rc, text = srv.stop(timeout=30)
    finally:
        srv.kill()
    assert rc == 0, text[-3000:]
    assert not any(s in text for s in SANITIZER_REPORT), text[-3000:]
    assert _stats(text)["errors"] == len(POISON_FRAMES)


# ---- case 11 -----------------------------------------------------------------------------------------------------------------------
def test_load_generator_keeps_ops_outstanding_per_connection(built):
    tool = os.path.join(ROOT, "tools", "uds_bench.py")
    p = subprocess.run([sys.executable, tool, "--stub", "--connections", "2", "--depth", "16", "--pipeline-depth", "16", "--ops", "200"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-800:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["mode"] == "closed-loop" and d["ops"] == 200 and d["failed"] == 0 and d["rejected"] == 0 and d["depth"] == 16, d
    assert d["connections"] == 2 and d["server"]["errors"] == 0 and d["server"]["deepest_pipeline"] > 1, d
    assert d["server"]["device_calls"] < d["server"]["requests"], d
