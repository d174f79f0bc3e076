"""CPU tier: secret wiping's host side (include/bbp.h "Secret wiping").  csrc/secret_map.h over the real circuits' layouts
(tests/secret_map_check.cpp), the host erase helpers and the call combiner's erase of its gathered rows (tests/secret_wipe_san.cpp),
both stand-alone programs under AddressSanitizer + UBSan; the header, the binding and the server flag agree."""
import os
import re
import subprocess
import tempfile
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ge():
    import __graft_entry__ as ge
    return ge


def test_secret_map_classes_alignment_and_tiling(ge):
    r = subprocess.run([ge.build_secret_map_check()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "secret_map_check ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "FAILED" not in r.stdout
    for want in ("B = 3, N = 1:", "B = 64, N = 8:", "B = 2, N = 202:", "N = 1", "N = 8", "N = 202", "classed exactly once"):
        assert want in r.stdout, want


def test_host_erase_helpers_and_combiner_vectors_under_asan(ge):
    r = subprocess.run([ge.build_secret_wipe_san()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "secret_wipe_san ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "FAILED" not in r.stdout
    assert "wiping off: records right" in r.stdout and "wiping on: records right" in r.stdout


def test_every_batch_array_of_the_issue_is_secret():
    """The arrays the contract names SECRET are in BBP_BATCH_SECRET, and only the seven it allows are PUBLIC."""
    src = open(os.path.join(ROOT, "dusk_blindbidproof_amd", "csrc", "secret_map.h")).read()

    def names(macro):
        body = src.split("#define %s(X)" % macro)[1].split("\n//")[0]
        return re.findall(r"X\((\w+),", body)
    secret, public = names("BBP_BATCH_SECRET"), names("BBP_BATCH_PUBLIC")
    must = "cst v vb ai1 ao1 s1 tr rng misc wv l1 r0 r1 r3 a b g h lr pts lrpts fpts entropy".split()
    assert sorted(secret) == sorted(must)
    assert sorted(public) == sorted("zpow ypow yipow wl wr wo enc".split())


POISON_EXEMPT = ["stand"]  # what bbp_debug_poison_scratch leaves alone: a new buffer is poisoned by default, exempting one changes this line


def test_poison_exempt_list_is_the_expected_one_and_names_real_buffers(ge):
    """BBP_POISON_EXEMPT (csrc/secret_map.h): every name occurs exactly once in the context's buffer lists (the stand-alone program
    expands the macros), and the list is the literal above, both as compiled and as written."""
    r = subprocess.run([ge.build_secret_map_check()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ok: every poison-exempt buffer is one buffer of the context, exempted once, with a reason" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("poison exempt: ")]
    assert len(line) == 1 and line[0] == "poison exempt: [%s]" % " ".join(POISON_EXEMPT), line
    src = open(os.path.join(ROOT, "dusk_blindbidproof_amd", "csrc", "secret_map.h")).read()
    body = src.split("#define BBP_POISON_EXEMPT(X)")[1].split("\ninline")[0]
    assert re.findall(r'X\("([\w.]+)",', body) == POISON_EXEMPT
    buffers = re.findall(r'^\s*X\("([\w.]+)",', src.split("#define BBP_POISON_EXEMPT(X)")[0], flags=re.M)
    assert len(buffers) >= 30 and all(buffers.count(n) == 1 for n in POISON_EXEMPT)
    hdr = open(os.path.join(ROOT, "include", "bbp.h")).read()
    assert re.search(r"\bbbp_debug_poison_scratch\s*\(", hdr) and "BBP_POISON_EXEMPT" in hdr and "No call of the context may be in flight" in hdr


def test_header_and_binding_name_the_entry_points():
    """The four entry points of the contract and the cost hook that goes with them (bbp_debug_wipe_cost)"""
    hdr = open(os.path.join(ROOT, "include", "bbp.h")).read()
    py = open(os.path.join(ROOT, "dusk_blindbidproof_amd", "_native.py")).read()
    for sym in ("bbp_set_secret_wipe", "bbp_wipe_secrets", "bbp_debug_secret_residue", "bbp_debug_secret_scan", "bbp_debug_wipe_cost"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert '"%s"' % sym in py, sym
    assert "Secret wiping" in hdr
    for said in ("does not scrub caches", "caller's own buffers", "not a constant-time claim"):
        assert said in hdr, said


def test_server_refuses_to_start_when_the_engine_cannot_wipe(ge):
    """--wipe-secrets resolves bbp_set_secret_wipe only when given; the stub engine lacks it, so the server does not serve unwiped."""
    ge.build_server()
    stub = ge.build_stub_engine()
    d = tempfile.mkdtemp(prefix="bbp-uds-wipe-")
    path = os.path.join(d, "sock")
    r = subprocess.run([ge.SERVER_BIN, "-b", path, "--engine", stub, "--wipe-secrets"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stderr[-1000:])
    assert "--wipe-secrets" in r.stderr and "bbp_set_secret_wipe" in r.stderr
    assert not os.path.exists(path)
    # without the flag the same engine serves (the symbol is not asked for)
    p = subprocess.Popen([ge.SERVER_BIN, "-b", path, "--engine", stub], stderr=subprocess.PIPE, text=True)
    try:
        for _ in range(500):
            if os.path.exists(path) or p.poll() is not None:
                break
            time.sleep(0.02)
        assert os.path.exists(path) and p.poll() is None
    finally:
        p.terminate()
        p.wait(timeout=30)
