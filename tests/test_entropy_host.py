"""not-gpu tier: on-device entropy (csrc/chacha.h), compiled for the host, against RFC 8439's known answer and a Python restatement
of the expansion (tests/entropy_ref.py); the server's --entropy flag against the stub engine."""
import ctypes
import os
import signal
import subprocess
import tempfile
import time

import pytest

from tests import entropy_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dusk_blindbidproof_amd", "csrc")

_SHIM = r"""
#include <string.h>
#include "chacha.h"
using namespace bbp;
extern "C" void cc_block(const unsigned char* key, unsigned counter, const unsigned char* nonce, unsigned char* out64) {
    u32 n[3], w[16];
    memcpy(n, nonce, 12);
    chacha20_block(chacha_key_from_bytes(key), counter, n[0], n[1], n[2], w);
    memcpy(out64, w, 64);
}
extern "C" void cc_prove_row(const unsigned char* key, unsigned N, unsigned row, unsigned char* out) {
    entropy_prove_row_bytes(chacha_key_from_bytes(key), N, row, out);
}
extern "C" void cc_verify_row(const unsigned char* key, unsigned row, unsigned char* out32) {
    u32 w[8];
    entropy_verify_row(chacha_key_from_bytes(key), row, w);
    memcpy(out32, w, 32);
}
"""


@pytest.fixture(scope="module")
def cc():
    d = tempfile.mkdtemp(prefix="bbp-cc-")
    src, so = os.path.join(d, "cc.cpp"), os.path.join(d, "libcc.so")
    with open(src, "w") as f:
        f.write(_SHIM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.cc_block.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p]
    lib.cc_prove_row.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p]
    lib.cc_verify_row.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    return lib


_KAT_KEY = bytes(range(32))
_KAT_NONCE = bytes.fromhex("000000090000004a00000000")
_KAT_BLOCK = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                           "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")


def test_rfc8439_block_function_known_answer(cc):
    """RFC 8439 2.3.2: the header's block function and the Python restatement both give the published block."""
    out = ctypes.create_string_buffer(64)
    cc.cc_block(_KAT_KEY, 1, _KAT_NONCE, out)
    assert out.raw == _KAT_BLOCK
    assert er.chacha20_block(_KAT_KEY, 1, _KAT_NONCE) == _KAT_BLOCK


@pytest.mark.parametrize("N", [1, 8, 202])
def test_expansion_matches_the_python_restatement(cc, N):
    key = bytes((7 * i + N) & 0xFF for i in range(32))
    size = 32 * (4 + N) + 32
    for row in (0, 1, 2, 4095):
        out = ctypes.create_string_buffer(size)
        cc.cc_prove_row(key, N, row, out)
        want = er.prove_row(key, N, row)
        assert out.raw == want, (N, row)
        for k in range(4 + N):  # every blinding canonical
            assert int.from_bytes(want[32 * k:32 * k + 32], "little") < er.L
        v = ctypes.create_string_buffer(32)
        cc.cc_verify_row(key, row, v)
        assert v.raw == er.verify_row(key, row), row
    # rows, list lengths and kinds draw from distinct streams
    assert er.prove_row(key, N, 0) != er.prove_row(key, N, 1)
    assert er.prove_row(key, N, 0)[:32] != er.prove_row(key, N + 1, 0)[:32]
    assert er.verify_row(key, 0) != er.prove_row(key, N, 0)[32 * (4 + N):]


def _start(built, extra):
    d = tempfile.mkdtemp(prefix="bbp-uds-ent-")
    path = os.path.join(d, "sock")
    log = open(os.path.join(d, "log"), "w+")
    p = subprocess.Popen([built.SERVER_BIN, "-b", path, "--engine", built.build_stub_engine(), "--window-us", "0"] + extra, stderr=log)
    for _ in range(500):
        if os.path.exists(path) or p.poll() is not None:
            break
        time.sleep(0.02)
    return p, path, log


def test_server_entropy_flag_against_the_stub_engine(built):
    """--entropy device needs bbp_set_entropy_source, which the stub engine does not export: the server refuses to start.  Without
    the flag (and with --entropy os) it starts as before; a value other than os / device is a usage error."""
    built.build_server()
    assert not hasattr(ctypes.CDLL(built.build_stub_engine()), "bbp_set_entropy_source")
    p, path, log = _start(built, ["--entropy", "device"])
    try:
        assert p.wait(timeout=30) == 2
        assert not os.path.exists(path)
        assert "bbp_set_entropy_source" in open(log.name).read()
    finally:
        if p.poll() is None:
            p.kill()
    for extra in ([], ["--entropy", "os"]):
        p, path, log = _start(built, extra)
        try:
            assert os.path.exists(path) and p.poll() is None, open(log.name).read()[-800:]
        finally:
            if p.poll() is None:
                p.send_signal(signal.SIGTERM)
                p.wait(timeout=30)
    bad = subprocess.run([built.SERVER_BIN, "--engine", built.build_stub_engine(), "--entropy", "urandom"], capture_output=True, text=True,
                         timeout=30)
    assert bad.returncode == 2 and "--entropy os|device" in bad.stderr
