"""not-gpu tier: the blinding-draw setting's two entry points exist, are declared and bound, and refuse what they can refuse without a
device (a context needs one: what a live context refuses is tests/test_gpu_expanded_draw.py's)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 4


def test_symbols_declared_exported_and_bound(bbp):
    header = open(os.path.join(ROOT, "include", "bbp.h")).read()
    assert re.search(r"#define BBP_BLINDING_DRAW_MERLIN 0\b", header) and re.search(r"#define BBP_BLINDING_DRAW_EXPANDED 1\b", header)
    L = ctypes.CDLL(bbp.lib_path)
    for name in ("bbp_set_blinding_draw", "bbp_blinding_draw"):
        assert re.search(r"int32_t %s\(bbp_ctx\* ctx" % name, header), name
        assert hasattr(L, name) and name in bbp.SIGNATURES, name
    assert (bbp.BLINDING_DRAW_MERLIN, bbp.BLINDING_DRAW_EXPANDED) == (0, 1)
    assert callable(bbp.Context.set_blinding_draw) and callable(bbp.Context.blinding_draw)
    assert bbp.Pool.set_blinding_draw is not bbp.Context.set_blinding_draw  # the pool documents its own: every member


def test_refusals_without_a_context(bbp):
    for mode in (0, 1, 2, -1, 1 << 20):
        assert bbp.lib.bbp_set_blinding_draw(None, mode) == BAD_ARG, mode
    assert bbp.lib.bbp_blinding_draw(None) == -1  # no mode: 0 and 1 are modes


def test_the_setting_has_no_environment_name(bbp):
    """the mode changes a record's bytes: it is an API setting of the context, never read from the environment"""
    blob = open(bbp.lib_path, "rb").read()
    assert b"BBP_BLINDING_DRAW" not in blob and b"BBP_RNG_COOP_BELOW" in blob


def test_server_flag_against_an_engine_without_the_setting(built):
    """The server resolves bbp_set_blinding_draw only when --blinding-draw is given.  The tests' stub engine does not have it: the server
    starts, says so at warn level and serves; without the flag the log does not mention it; any other value is a usage error."""
    import signal
    import subprocess
    import tempfile
    import time

    from tests import uds_client as uc
    built.build_server()
    stub = built.build_stub_engine()
    assert not hasattr(ctypes.CDLL(stub), "bbp_set_blinding_draw")
    for flags in (("--blinding-draw", "expanded"), ("--blinding-draw", "merlin"), ()):
        d = tempfile.mkdtemp(prefix="bbp-uds-draw-")
        path = os.path.join(d, "sock")
        err = open(os.path.join(d, "log"), "w+")
        p = subprocess.Popen([built.SERVER_BIN, "-b", path, "-l", "info", "--engine", stub] + list(flags), stderr=err)
        try:
            for _ in range(300):
                if os.path.exists(path) or p.poll() is not None:
                    break
                time.sleep(0.02)
            assert os.path.exists(path) and p.poll() is None, open(err.name).read()[-800:]
            s7 = b"".join(bytes([(7 * 3 + k) & 0xff]) * 31 + b"\x01" for k in range(7))
            pub = b"".join(bytes([(11 * 3 + j) & 0xff]) * 31 + b"\x02" for j in range(8))
            blob = uc.prove(path, s7, pub, 3)
            assert blob is not None and uc.verify(path, blob, s7[128:160], s7[160:192], s7[192:224], pub) == b"\x01"
        finally:
            if p.poll() is None:
                p.send_signal(signal.SIGTERM)
                p.wait(timeout=10)
        log = open(err.name).read()
        if flags:
            assert "--blinding-draw " + flags[1] in log and "bbp_set_blinding_draw" in log and "has no such setting" in log, log[-800:]
        else:
            assert "blinding" not in log, log[-800:]
    q = subprocess.run([built.SERVER_BIN, "--blinding-draw", "maybe"], capture_output=True, text=True, timeout=10)
    assert q.returncode == 2 and "--blinding-draw merlin|expanded" in q.stderr
