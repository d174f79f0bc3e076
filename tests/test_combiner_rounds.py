"""not-gpu tier: the call combiner's round sharing (csrc/submit.cpp).  With Combiner::set_round_sharing on and a rounds runner installed,
concurrent bbp_verify / bbp_verify_async requests whose seed || pub_list is byte-equal leave as one rounds call whose table holds every
distinct round once; tests/combiner_rounds.cpp links the product's submit.cpp against a stand-in engine that records every call it is
handed.  Also here: the public switch and its counters are exported and bound, and the UDS server's --verify-rounds flag against an
engine that lacks the setting."""
import ctypes
import os
import platform
import shutil
import signal
import subprocess
import tempfile
import time

from tests import uds_client as uc

SCENARIOS = ("one_round_32_requests", "three_rounds_interleaved", "hash_does_not_decide", "fallback_all_distinct", "fallback_all_distinct_one_n",
             "fallback_batch_of_one", "fallback_two_phase_member", "fallback_no_runner", "fallback_sharing_off", "mixing_off_one_n_still_shares",
             "failing_round_call", "max_batch_is_respected", "stress_1_target", "stress_3_targets")


def _check(p):
    assert p.returncode == 0, p.stdout + p.stderr[-3000:]
    for name in SCENARIOS:
        assert "PASS " + name in p.stdout, p.stdout
    assert "RESULT failed 0" in p.stdout, p.stdout


def test_round_sharing_rules(built):
    """One round, 32 requests: one rounds call with R = 1, the table holds the round once, short rows in queue order, every request its
    own row's status.  Three interleaved rounds, two of equal N: numbered by first appearance, round_of per row, the table their
    concatenation, and the rows rebuilt from the table byte-equal to the requests.  Requests given the same hash whose bytes differ in
    one bit of the last list item, or of the seed, are separate rounds; equal bytes under different hashes still meet their own
    bytes.  Fallbacks -- no two requests share, a batch of one, a two-phase member, no runner, sharing off -- make exactly the calls
    of a run with sharing off and move no counter.  Mixing off: a batch is one N and still shares.  A failing rounds call fails every
    member with its code and message.  max_batch holds.  Then 32 threads of blocking and asynchronous requests over five rounds, on
    one engine and on a pool of three, the counters agreeing with the calls the stand-in saw."""
    exe = built.build_combiner_rounds()
    _check(subprocess.run([exe], capture_output=True, text=True, timeout=300))


def test_round_sharing_under_thread_sanitizer(built):
    """The same source with -fsanitize=thread, as a stand-alone program: every scenario passes and the sanitizer reports no data race."""
    exe = built.build_combiner_rounds(tsan=True)
    # ThreadSanitizer aborts before main on kernels that randomise mmap with more bits than its runtime expects: run the binary
    # with address randomisation off for its own process wherever setarch is there and allowed to (tests/test_combiner_mixed.py)
    cmd = [exe]
    setarch = shutil.which("setarch")
    if setarch and subprocess.run([setarch, platform.machine(), "-R", "true"], capture_output=True).returncode == 0:
        cmd = [setarch, platform.machine(), "-R", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    _check(p)
    assert "WARNING: ThreadSanitizer" not in p.stderr, p.stderr[-3000:]


def test_library_exports_the_switch_and_its_counters(bbp):
    L = ctypes.CDLL(bbp.lib_path)
    for name in ("bbp_set_verify_round_sharing", "bbp_verify_round_sharing_stats"):
        assert hasattr(L, name), name
        assert name in bbp.SIGNATURES, name
    for cls in (bbp.Context, bbp.Pool):
        assert hasattr(cls, "set_verify_round_sharing") and hasattr(cls, "verify_round_sharing_stats")
    assert bbp.lib.bbp_set_verify_round_sharing(None, 1) == 4  # BBP_ERR_BAD_ARG: no context
    assert bbp.lib.bbp_verify_round_sharing_stats(None, None, None, None) == 4


def _bid(i, n):
    s7 = b"".join(bytes([(7 * i + k) & 0xff]) * 31 + b"\x01" for k in range(7))
    pub = b"".join(bytes([(11 * i + j) & 0xff]) * 31 + b"\x02" for j in range(n))
    return s7, pub, i % n


def test_server_flag_against_an_engine_without_the_setting(built):
    """The server resolves bbp_set_verify_round_sharing only when --verify-rounds is given.  The tests' stub engine does not have it:
    with `on` (and with `off`) the server starts, says in its log that the engine lacks the setting, and serves an opcode-2 request;
    without the flag the log does not mention it; any other value is a usage error."""
    built.build_server()
    stub = built.build_stub_engine()
    assert not hasattr(ctypes.CDLL(stub), "bbp_set_verify_round_sharing")
    for flags in (("--verify-rounds", "on"), ("--verify-rounds", "off"), ()):
        d = tempfile.mkdtemp(prefix="bbp-uds-rounds-")
        path = os.path.join(d, "sock")
        err = open(os.path.join(d, "log"), "w+")
        p = subprocess.Popen([built.SERVER_BIN, "-b", path, "-l", "info", "--engine", stub] + list(flags), stderr=err)
        try:
            for _ in range(300):
                if os.path.exists(path) or p.poll() is not None:
                    break
                time.sleep(0.02)
            assert os.path.exists(path) and p.poll() is None, open(err.name).read()[-800:]
            s7, pub, toggle = _bid(3, 8)
            blob = uc.prove(path, s7, pub, toggle)
            assert blob is not None
            assert uc.verify(path, blob, s7[128:160], s7[160:192], s7[192:224], pub) == b"\x01"
            assert uc.verify(path, blob, s7[160:192], s7[160:192], s7[192:224], pub) == b"\x00"
        finally:
            if p.poll() is None:
                p.send_signal(signal.SIGTERM)
                p.wait(timeout=10)
        log = open(err.name).read()
        if flags:
            assert "--verify-rounds " + flags[1] in log and "bbp_set_verify_round_sharing" in log and "has no such setting" in log, log[-800:]
        else:
            assert "verify-rounds" not in log and "bbp_set_verify_round_sharing" not in log, log[-800:]
    q = subprocess.run([built.SERVER_BIN, "--verify-rounds", "maybe"], capture_output=True, text=True, timeout=10)
    assert q.returncode == 2 and "--verify-rounds on|off" in q.stderr
