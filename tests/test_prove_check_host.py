"""not-gpu tier: checked proving's witness check (csrc/witness_check.h), compiled for the host, against the C oracle's ground truth
-- a witness is satisfied exactly when oc.prove followed by oc.verify accepts -- and the C-ABI / binding surface of the feature."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from tests import oracle_c
from tests import prove_check_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dusk_blindbidproof_amd", "csrc")

_SHIM = r"""
#include <string.h>
#include <vector>
#include "witness_check.h"
using namespace bbp;
extern "C" unsigned wc_row(unsigned N, const unsigned char* row, const unsigned char* mimc90) {
    std::vector<u32> w(7 * 8 + (size_t)N * 8 + 2);
    memcpy(w.data(), row, 4 * w.size());
    std::vector<sc> c(BBP_MIMC_ROUNDS);
    memcpy(c.data(), mimc90, 32 * BBP_MIMC_ROUNDS);
    return witness_check_row(N, w.data(), c.data());
}
extern "C" const char* wc_text(unsigned mask) { return witness_check_text(mask); }
"""


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def wc(oc):
    d = tempfile.mkdtemp(prefix="bbp-wc-")
    src, so = os.path.join(d, "wc.cpp"), os.path.join(d, "libwc.so")
    with open(src, "w") as f:
        f.write(_SHIM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.wc_row.restype = ctypes.c_uint32
    lib.wc_row.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p]
    lib.wc_text.restype = ctypes.c_char_p
    lib.wc_text.argtypes = [ctypes.c_uint32]
    mimc = b"".join(oc.mimc_constant(i) for i in range(90))
    return lambda N, row: lib.wc_row(N, row, mimc), lambda m: lib.wc_text(m).decode()


def _oracle_accepts(oc, c, N, seed):
    rc, rec = oc.prove(pc.scalars7(c), b"".join(c["pub"]), c["toggle"], pc.entropy(seed, N))
    if rc != 0:
        return False
    f = c["f"]
    return oc.verify(rec, pc.b32(f[pc.Q]), pc.b32(f[pc.Z]), pc.b32(f[pc.SEED]), b"".join(c["pub"])) == 0


@pytest.mark.parametrize("N", [1, 8, 202])
def test_witness_check_matches_the_oracle(oc, wc, N):
    """About 40 cases over N in {1, 8, 202}: the header's verdict (mask == 0) is the oracle's prove + verify verdict on every one."""
    check, text = wc
    seed = 100 + N
    cases = pc.variants(oc, seed, N)
    for name, c, expect in cases:
        mask = check(N, pc.row(c))
        truth = _oracle_accepts(oc, c, N, seed)
        assert truth == expect, (N, name, "oracle")          # the case list says what the circuit does ...
        assert (mask == 0) == truth, (N, name, mask)         # ... and the header agrees with the oracle
        if mask:
            assert text(mask) != "witness satisfied"


def test_witness_check_bits_name_the_broken_relation(oc, wc):
    check, text = wc
    N = 8
    got = {name: check(N, pc.row(c)) for name, c, _ in pc.variants(oc, 77, N)}
    assert got["list_wrong"] == 4 and "pub_list[toggle]" in text(got["list_wrong"])
    assert got["z_img_wrong"] == 8 and "z_img" in text(got["z_img_wrong"])
    assert got["y_inv_wrong"] == 16 and "y_inv != 1" in text(got["y_inv_wrong"])
    assert got["q_wrong"] == 32 and "q != d * y_inv" in text(got["q_wrong"])
    assert got["toggle_is_n"] == 1 and text(1) == "toggle >= N"
    c = pc.honest(oc, 77, N)
    c["f"][pc.Y] = pc.L  # l itself: not a canonical encoding
    assert check(N, pc.row(c)) == 2 and text(2) == "non-canonical scalar input"
    c = pc.honest(oc, 77, N)
    c["toggle"] = 1 << 40  # never used as an index
    assert check(N, pc.row(c)) == 1


def test_entry_points_refuse_a_null_context(bbp):
    lib = bbp.lib
    assert lib.bbp_set_prove_check(None, 1) == 4
    assert lib.bbp_prove_check_stats(None, None, None, None, None) == 4
    assert lib.bbp_prove_batch_checked_dev(None, 1, 8, 1, 1, 1, 1, 1, None) == 4
    assert lib.bbp_debug_corrupt_next_proof(None, 0) == 4
    for name in ("set_prove_check", "prove_check_stats", "prove_batch_checked_dev", "debug_corrupt_next_proof"):
        assert callable(getattr(bbp.Context, name)), name


def test_server_refuses_check_proofs_without_engine_support(built):
    """--check-proofs needs bbp_set_prove_check in the engine; the stub engine has none, so the server refuses to start."""
    built.build_server()
    stub = built.build_stub_engine()
    d = tempfile.mkdtemp(prefix="bbp-uds-chk-")
    p = subprocess.run([built.SERVER_BIN, "-b", os.path.join(d, "sock"), "--engine", stub, "--check-proofs"], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 2 and "bbp_set_prove_check" in p.stderr, p.stderr[-600:]
    assert not os.path.exists(os.path.join(d, "sock"))
