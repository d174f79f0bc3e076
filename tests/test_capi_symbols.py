"""not-gpu tier: the C-ABI library loads and exports every symbol include/bbp.h declares; no compute without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "bbp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(bbp_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(bbp):
    names = _declared()
    assert len(names) >= 15
    L = ctypes.CDLL(bbp.lib_path)
    for n in names:
        assert hasattr(L, n), n
    assert sorted(bbp.SIGNATURES) == names  # the Python binding covers exactly the header


def test_no_cpu_fallback(bbp):
    """Without a gfx950 device the engine refuses to start (and says so) instead of computing on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(bbp.BbpError) as e:
        bbp.Context(0)
    assert e.value.status == 5


def test_sizes(bbp):
    assert bbp.lib.bbp_proof_record_size(8) == 1121 + 32 * 12 == bbp.record_size(8)
    assert bbp.lib.bbp_entropy_size(8) == 32 * 12 + 32 == bbp.entropy_size(8)


def test_product_does_not_reference_oracle():
    """The shipped package must never import, link or execute anything under oracle/."""
    pkg = os.path.join(ROOT, "dusk_blindbidproof_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".h", ".hip", ".cpp", ".hpp")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "oracle/" not in txt and "from oracle" not in txt and "import oracle" not in txt and "bbp_oracle" not in txt, f


def test_no_verdict_changing_knobs_in_the_product(bbp):
    """a knock-out mask read from the environment turned the verifier into accept-stale.  Verdict-changing
    experiment knobs exist only in -DBBP_EXPERIMENTS builds (tools/build_variant.py); the product library must not even carry
    their names, neither as getenv strings nor as compile-time knock-outs."""
    blob = open(bbp.lib_path, "rb").read()
    for name in (b"BBP_KO_VERIFY", b"BBP_KO_", b"BBP_EXP_ROWMASK"):
        assert name not in blob, name
    assert b"BBP_SLICES" in blob  # (the scheduling knobs are there: the scan does see getenv strings)


def test_init_exports_the_hardware_queue_setting_before_touching_hip(bbp):
    """Round 4: bbp_init owns GPU_MAX_HW_QUEUES.  Without a GPU the call fails (status 5, no CPU path) -- but the variable must have
    been exported BEFORE the first HIP call, which is what makes it effective on a GPU box; a value the caller set is left alone.
    Fresh processes that load only the library (the GPU tier checks the three cases on hardware through bbp_describe)."""
    import subprocess
    import sys
    code = (
        "import ctypes, sys\n"
        "L = ctypes.CDLL(sys.argv[1])\n"
        "h = ctypes.c_void_p()\n"
        "L.bbp_init.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]\n"
        "rc = L.bbp_init(0, ctypes.byref(h))\n"
        "libc = ctypes.CDLL(None)\n"
        "libc.getenv.restype = ctypes.c_char_p\n"
        "print('RC', rc, 'ENV', libc.getenv(b'GPU_MAX_HW_QUEUES'))\n")
    for preset, expect in ((None, b"2"), ("1", b"1")):
        env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
        if preset:
            env["GPU_MAX_HW_QUEUES"] = preset
        p = subprocess.run([sys.executable, "-c", code, bbp.lib_path], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-1500:]
        assert ("ENV %r" % expect) in p.stdout, (preset, p.stdout, p.stderr[-300:])


def test_circuit_synthesis_sizes_and_statuses(bbp):
    """Host-only synthesis through the C ABI (no device): n_mul = 1442 + 3N, n_cons = 2 n_mul + 3 + 3N; the states
    the reference panics on / rejects come back as statuses."""
    from dusk_blindbidproof_amd._native import compile_circuit
    for n in (1, 3, 8, 40, 202):
        rc, n_mul, n_cons = compile_circuit(n)
        assert (rc, n_mul, n_cons) == (0, 1442 + 3 * n, 2 * (1442 + 3 * n) + 3 + 3 * n), n
    assert compile_circuit(0)[0] == 4      # empty list: the reference panics at src/gadgets.rs:103
    assert compile_circuit(203)[0] == 2    # R1CSError::InvalidGeneratorsLength


def test_exception_barrier_turns_a_throw_into_a_status(bbp, monkeypatch):
    """include/bbp.h promises that nothing throws across the boundary: force circuit::compile to throw (the same code path
    bbp_prove / bbp_verify take for a list length they have not compiled yet) and see BBP_ERR_INTERNAL, not a crash."""
    from dusk_blindbidproof_amd._native import compile_circuit
    monkeypatch.setenv("BBP_FAULT_INJECT", "compile")
    assert compile_circuit(8)[0] == 6
    monkeypatch.delenv("BBP_FAULT_INJECT")
    assert compile_circuit(8)[0] == 0


def test_device_check_libraries_export_every_entry_point(built, bbp):
    """tests/device_check.hip (the gpu tier's view of the product headers) cross-compiles for gfx950 in both field variants, and both
    libraries load and export every dc_* entry point the source defines, each one bound in tests/test_gpu_device_arith.py or, for
    the scalar multiplications of csrc/scalarmul.h, in tests/scalarmul_run.py, for the table audit in tests/table_run.py"""
    from tests.scalarmul_run import SIGNATURES as SCALARMUL
    from tests.table_run import SIGNATURES as TABLES
    from tests.test_gpu_device_arith import SIGNATURES, VARIANTS
    src = open(os.path.join(ROOT, "tests", "device_check.hip")).read()
    defined = sorted(set(re.findall(r"^int (dc_[a-z0-9_]+)\(", src, flags=re.M)))
    bound = sorted(list(SIGNATURES) + ["dc_" + name for name in SCALARMUL] + ["dc_" + name for name in TABLES])
    assert len(defined) >= 13 + 6 + 5 and defined == bound
    for v in VARIANTS:
        path = built.build_devcheck(v)
        blob = open(path, "rb").read()
        assert b"gfx950" in blob, v
        L = ctypes.CDLL(path)
        for n in defined:
            assert hasattr(L, n), (v, n)
