"""not-gpu tier: the call combiner's merged verify class (csrc/submit.cpp).  Concurrent bbp_verify / bbp_verify_async requests of any
bid-list length and record layout leave as one batch once the engine's mixed-N runner is installed; tests/combiner_mixed.cpp
links the product's submit.cpp against a stand-in engine that records every batch it is handed.  Also here: the public switch
(bbp_set_verify_mixing) is exported, and the UDS server's --verify-mixing flag against an engine that lacks the switch."""
import ctypes
import os
import platform
import shutil
import subprocess
import tempfile
import time

SCENARIOS = ("one_mixed_batch", "uniform_goes_uniform", "prove_stays_per_class", "no_runner_is_per_class", "mixing_off_is_per_class",
             "failing_mixed_call", "blocking_and_async", "stress_1_target_mixing_on", "stress_3_targets_mixing_on", "stress_1_target_mixing_off")


def _check(p):
    assert p.returncode == 0, p.stdout + p.stderr[-3000:]
    for name in SCENARIOS:
        assert "PASS " + name in p.stdout, p.stdout
    assert "RESULT failed 0" in p.stdout, p.stdout


def test_merged_verify_class_rules(built):
    """Three list lengths and both layouts in one window: one mixed batch, Ns / vers / packed bytes in queue order, every request
    its own row's status.  One list length: verify_batch_locked, the runner is not called.  Prove requests: one class per batch.
    No runner, or mixing off: per class as before.  A failing mixed call fails every member with its status and message.  Blocking
    and asynchronous requests share a batch.  Then 32 threads of prove and verify requests on one engine and on a pool of three."""
    exe = built.build_combiner_mixed()
    _check(subprocess.run([exe], capture_output=True, text=True, timeout=300))


def test_merged_verify_class_under_thread_sanitizer(built):
    """The same source with -fsanitize=thread: every scenario passes and the sanitizer reports no data race."""
    exe = built.build_combiner_mixed(tsan=True)
    # ThreadSanitizer aborts before main on kernels that randomise mmap with more bits than its runtime expects: run the binary
    # with address randomisation off for its own process wherever setarch is there and allowed to (tests/test_uds_server.py)
    cmd = [exe]
    setarch = shutil.which("setarch")
    if setarch and subprocess.run([setarch, platform.machine(), "-R", "true"], capture_output=True).returncode == 0:
        cmd = [setarch, platform.machine(), "-R", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    _check(p)
    assert "WARNING: ThreadSanitizer" not in p.stderr, p.stderr[-3000:]


def test_library_exports_the_switch(bbp):
    L = ctypes.CDLL(bbp.lib_path)
    assert hasattr(L, "bbp_set_verify_mixing")
    assert "bbp_set_verify_mixing" in bbp.SIGNATURES
    assert hasattr(bbp.Context, "set_verify_mixing") and hasattr(bbp.Pool, "set_verify_mixing")
    assert bbp.lib.bbp_set_verify_mixing(None, 1) == 4  # BBP_ERR_BAD_ARG: no context


def _start(built, stub, *flags):
    d = tempfile.mkdtemp(prefix="bbp-uds-mix-")
    path = os.path.join(d, "sock")
    err = open(os.path.join(d, "log"), "w+")
    p = subprocess.Popen([built.SERVER_BIN, "-b", path, "-l", "info", "--engine", stub] + list(flags), stderr=err)
    for _ in range(300):
        if os.path.exists(path) or p.poll() is not None:
            break
        time.sleep(0.02)
    return p, path, err


def test_server_flag_against_an_engine_without_the_switch(built):
    """The server resolves bbp_set_verify_mixing only when --verify-mixing is given.  The tests' stub engine does not have it:
    without the flag and with `on` the server serves (the engine's own grouping applies), `off` cannot be honoured and the server
    refuses to start and says why; any other value is a usage error."""
    built.build_server()
    stub = built.build_stub_engine()
    for flags in ((), ("--verify-mixing", "on")):
        p, path, err = _start(built, stub, *flags)
        try:
            assert os.path.exists(path) and p.poll() is None, open(err.name).read()[-800:]
        finally:
            p.terminate()
            p.wait(timeout=10)
    p, path, err = _start(built, stub, "--verify-mixing", "off")
    assert p.wait(timeout=10) == 2 and not os.path.exists(path)
    log = open(err.name).read()
    assert "--verify-mixing off" in log and "bbp_set_verify_mixing" in log, log[-800:]
    q = subprocess.run([built.SERVER_BIN, "--verify-mixing", "maybe"], capture_output=True, text=True, timeout=10)
    assert q.returncode == 2 and "--verify-mixing on|off" in q.stderr
