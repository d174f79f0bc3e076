"""not-gpu tier: the per-proof batch buffer as csrc/batch_layout.h states it once (BBP_BATCH_ARRAYS: the carve, the views of slices, the
strides, the encoding slots), compiled for the host by tests/host_check.cpp.  Every expected value comes from the formula written out
here -- the list of (name, element bytes, elements per proof) that batch_reserve used to spell out -- never from the header under test."""
import ctypes

import pytest

NS = (1, 8, 202)
BS = (1, 3, 7, 8, 9, 64, 640)  # 1: arrays shorter than one 256-byte unit; 7, 8, 9 straddle 8 x 32 = 256
MS_COUNT, FOLD_CLS = 32, 32    # csrc/batch_layout.h


@pytest.fixture(scope="module")
def lib(built):
    lib = ctypes.CDLL(built.build_hostcheck())
    lib.hc_slice_first.restype = ctypes.c_uint32
    return lib


@pytest.fixture(scope="module")
def sizes(lib):
    out = (ctypes.c_uint64 * 3)()
    lib.hc_batch_elem_sizes(out)
    sc, ge, tr = (int(x) for x in out)
    assert sc == 32 and ge == 160  # a scalar of eight words, a point of four field elements of ten limbs
    assert tr >= 200 + 12          # the Keccak state and three counters at the least
    return sc, ge, tr


def _up(n):
    return (n + 255) // 256 * 256


def dims(lib, N):
    """(m, n_mul, n_cons, n_cst) of circuit::compile(N)"""
    out = (ctypes.c_uint32 * 4)()
    lib.hc_circuit_dims(N, out)
    d = tuple(int(x) for x in out)
    assert d[0] == 4 + N and d[1] == 1442 + 3 * N and d[3] == 95 + N  # SURVEY.md F7; circuit.h CST_ITEM0
    return d


def widened(lib):
    """the largest of each count over N = 1, 8, 202, as a mixed verify call reserves"""
    return tuple(max(col) for col in zip(*(dims(lib, n) for n in NS)))


def parent_arrays(d, sizes):
    """the batch buffer as batch_reserve carved it before the table: (name, element bytes, elements per proof), in the order of its take() calls"""
    (m, n1, n_cons, n_cst), (S, GE, TR) = d, sizes
    return [("cst", S, n_cst), ("v", S, m), ("vb", S, m), ("ai1", S, 1 + 2 * n1), ("ao1", S, 1 + n1), ("s1", S, 1 + 2 * n1), ("tr", TR, 1), ("rng", TR, 1),
            ("misc", S, MS_COUNT), ("zpow", S, n_cons + 1), ("ypow", S, 2049), ("yipow", S, 2048), ("wl", S, 2048), ("wr", S, 2048), ("wo", S, 2048),
            ("wv", S, m), ("l1", S, n1), ("r0", S, n1), ("r1", S, n1), ("r3", S, n1), ("a", S, 2048), ("b", S, 2048), ("g", S, 2048), ("h", S, 2048),
            ("lr", S, 2 * 2049), ("pts", GE, m + 8), ("lrpts", GE, 2), ("fpts", GE, 2 * FOLD_CLS), ("enc", 4, (m + 8 + 22) * 8), ("entropy", 1, 32 * m + 32)]


def layout(lib, B, d):
    off, stride, elem = ((ctypes.c_uint64 * 64)() for _ in range(3))
    total, names = ctypes.c_uint64(), ctypes.create_string_buffer(512)
    n = lib.hc_batch_layout(B, (ctypes.c_uint32 * 4)(*d), off, stride, elem, ctypes.byref(total), names, len(names))
    return names.value.decode().split(), [int(x) for x in off[:n]], [int(x) for x in stride[:n]], [int(x) for x in elem[:n]], int(total.value)


def view(lib, B, d, first):
    delta = (ctypes.c_uint64 * 64)()
    n = lib.hc_batch_view(B, (ctypes.c_uint32 * 4)(*d), first, delta)
    return [int(x) for x in delta[:n]]


def cases(lib):
    return [(B, dims(lib, N)) for N in NS for B in BS] + [(B, widened(lib)) for B in BS]


def test_offsets_and_total_are_the_parents(lib, sizes):
    """every offset and the total equal the running sum of align256(bytes per proof x B) over the written-out list"""
    assert widened(lib) == (206, 2048, max(dims(lib, n)[2] for n in NS), 297)
    for B, d in cases(lib):
        want = parent_arrays(d, sizes)
        names, off, stride, elem, total = layout(lib, B, d)
        assert names == [w[0] for w in want] and len(names) == 30
        assert elem == [w[1] for w in want] and stride == [w[2] for w in want], (B, d)
        end = 0
        for (name, e, count), o in zip(want, off):
            assert o == end, (B, d, name)
            end += _up(e * count * B)
        assert total == end, (B, d)


def test_regions_are_aligned_ordered_and_disjoint(lib, sizes):
    for B, d in cases(lib):
        names, off, stride, elem, total = layout(lib, B, d)
        ends = off[1:] + [total]
        for name, o, s, e, nxt in zip(names, off, stride, elem, ends):
            assert o % 256 == 0 and o + s * e * B <= nxt <= total and o < nxt, (B, d, name)  # in list order: each ends before the next starts
        assert total % 256 == 0


@pytest.mark.parametrize("B", (9, 640))
def test_views_of_slices(lib, sizes, B):
    """a view's pointers are first x stride elements in; the slices of a call cover every array's B rows exactly once, inside its region"""
    for d in [dims(lib, N) for N in NS] + [widened(lib)]:
        names, off, stride, elem, total = layout(lib, B, d)
        ends = off[1:] + [total]
        assert view(lib, B, d, 0) == off
        for slices in (2, 3, 4):
            bounds = [int(lib.hc_slice_first(B, slices, i)) for i in range(slices + 1)]
            assert bounds == [B * i // slices for i in range(slices + 1)] and bounds[0] == 0 and bounds[-1] == B
            assert all(lo < hi for lo, hi in zip(bounds, bounds[1:]))  # no empty slice: the ranges are disjoint and cover [0, B)
            views = [view(lib, B, d, f) for f in bounds]
            for k, (name, o, s, e, nxt) in enumerate(zip(names, off, stride, elem, ends)):
                for i in range(slices):
                    lo, hi = views[i][k], views[i + 1][k]
                    assert lo == o + bounds[i] * s * e, (d, slices, name)        # first * stride elements in
                    assert hi - lo == (bounds[i + 1] - bounds[i]) * s * e        # the slice's rows end where the next slice's begin
                assert views[slices][k] == o + B * s * e <= nxt, (d, name)       # ... and the last inside the carved region


@pytest.mark.parametrize("m", (5, 12, 206))
def test_encoding_slots_are_the_record_order(lib, m):
    """V[m], A_I1, A_O1, S1, T_1, T_3, T_4, T_5, T_6, then (L_j, R_j) for j = 1..11, eight words each (k_assemble's order)"""
    out = (ctypes.c_uint64 * 18)()
    lib.hc_enc_slots(m, out)
    got = [int(x) for x in out]
    order = ["V%d" % i for i in range(m)] + ["A_I1", "A_O1", "S1", "T_1", "T_3", "T_4", "T_5", "T_6"] + [s % j for j in range(1, 12) for s in ("L_%d", "R_%d")]
    word = {name: 8 * i for i, name in enumerate(order)}
    assert got[0] == 8 * len(order) == (m + 30) * 8
    assert got[1] == word["V0"] == 0 and got[2] == word["V%d" % (m - 1)]
    assert got[3] == word["A_I1"] and got[4] == word["T_1"]
    for r in range(1, 12):
        assert got[4 + r] == word["L_%d" % r] == 8 * (m + 8 + 2 * (r - 1)) and word["R_%d" % r] == got[4 + r] + 8
    assert got[16] == m + 8 and got[17] == m + 3  # the point block: V[m], A_I1, A_O1, S1, T_1 ...


def test_case_grid_under_the_sanitizers(built):
    """tests/batch_layout_san.cpp: the exports above and the index lists over their grids, with batches up to 32768, in a stand-alone
    program built with -fsanitize=address,undefined"""
    import subprocess
    p = subprocess.run([built.build_batch_layout_san()], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "sanitizer report or failed expectation:\n" + (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("0 failures")
