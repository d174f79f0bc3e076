"""not-gpu tier: the row-layout descriptor every verify call passes from the entry points to the launches (csrc/verify_rows.h),
compiled for the host by tests/host_check.cpp.  Every expected size comes from the Python packers of the binding (verify_row_size,
mixed_row_offsets, round_row_size, round_table_offsets) or from bbp_proof_record_size, never from the header under test."""
import ctypes
import itertools

import pytest

UNIFORM, MIXED, ROUNDS = 0, 1, 2
NS7 = [1, 8, 202, 8, 1, 202, 202]  # seven rows, list lengths from {1, 8, 202}
VERS7 = [0, 1, 0, 0, 1, 1, 0]
ROUND_NS = [8, 1, 202]
ROUND_OF7 = [2, 0, 1, 1, 2, 0, 2]
WHOLE = (1, 0)  # lo > hi: the call itself, not a slice


@pytest.fixture(scope="module")
def lib(built):
    return ctypes.CDLL(built.build_hostcheck())


class Rows:
    """One probe call: the descriptor of (kind, ...) cut to [lo, hi), as plain Python values."""

    def __init__(self, lib, kind, B, N=0, rec_ver=0, ns=None, vers=None, round_ns=None, round_of=None, cut=WHOLE, table=0x7000):
        u32s = lambda v: None if v is None else (ctypes.c_uint32 * max(len(v), 1))(*v)
        self._keep = a_ns, a_vers, a_rns, a_rof = u32s(ns), None if vers is None else (ctypes.c_uint8 * max(len(vers), 1))(*vers), u32s(round_ns), u32s(round_of)
        n = B if cut == WHOLE else cut[1] - cut[0]
        out_n, out_ver, out_off, info = (ctypes.c_uint32 * (n + 1))(), (ctypes.c_uint32 * (n + 1))(), (ctypes.c_uint64 * (n + 1))(), (ctypes.c_uint64 * 11)()
        lib.hc_verify_rows(kind, B, N, rec_ver, a_ns, a_vers, len(round_ns or []), a_rns, ctypes.c_void_p(table), a_rof, cut[0], cut[1],
                           out_n, out_ver, out_off, info)
        self.B, self.rec_ver, self.has_vers, self.mixed_front, self.front_n, self.R, self.table, self.table_bytes = [int(x) for x in info[:8]]
        self.has_round_of, self.round_of_at, self.first_n = int(info[8]), int(info[9]), int(info[10])
        assert self.B == n
        self.n, self.ver, self.off = list(out_n)[:n], list(out_ver)[:n], list(out_off)
        self.aggregable = not self.rec_ver  # the host path aggregates a call only when no row is two-phase


def _cum(sizes):
    return list(itertools.accumulate(sizes, initial=0))


def test_row_bytes_and_offsets_agree_with_the_packers(lib, bbp):
    for n in (1, 8, 202):
        assert bbp.verify_row_size(n) == bbp.lib.bbp_proof_record_size(n) + 96 + 32 * n
        for ver in (0, 1):
            r = Rows(lib, UNIFORM, 5, N=n, rec_ver=ver)
            assert r.off == [i * (bbp.verify_row_size(n) + 96 * ver) for i in range(6)]
            assert r.n == [n] * 5 and r.ver == [ver] * 5 and r.first_n == n and r.table_bytes == 0
    r = Rows(lib, MIXED, 7, ns=NS7)
    assert r.off == bbp.mixed_row_offsets(NS7) and r.n == NS7 and r.ver == [0] * 7 and r.first_n == NS7[0]
    r = Rows(lib, MIXED, 7, ns=NS7, vers=VERS7)
    assert r.off == _cum(bbp.verify_row_size(n) + 96 * v for n, v in zip(NS7, VERS7)) and r.ver == VERS7
    r = Rows(lib, ROUNDS, 7, round_ns=ROUND_NS, round_of=ROUND_OF7)
    ns = [ROUND_NS[k] for k in ROUND_OF7]
    assert r.n == ns and r.ver == [0] * 7 and r.first_n == ns[0]
    assert r.off == _cum(bbp.round_row_size(n) for n in ns) == _cum(bbp.lib.bbp_proof_record_size(n) + 64 for n in ns)
    assert r.table_bytes == bbp.round_table_offsets(ROUND_NS)[-1]
    r = Rows(lib, ROUNDS, 4, round_ns=[202])
    assert r.off == [i * bbp.round_row_size(202) for i in range(5)] and r.n == [202] * 4 and r.table_bytes == 32 * 203


CALLS = {
    "uniform": dict(kind=UNIFORM, N=8),
    "uniform-two-phase": dict(kind=UNIFORM, N=202, rec_ver=1),
    "mixed": dict(kind=MIXED, ns=NS7),
    "mixed-vers": dict(kind=MIXED, ns=NS7, vers=VERS7),
    "rounds": dict(kind=ROUNDS, round_ns=ROUND_NS, round_of=ROUND_OF7),
    "one-round": dict(kind=ROUNDS, round_ns=[8]),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_every_slice_is_the_parents_rows(lib, name):
    call = CALLS[name]
    parent = Rows(lib, B=7, **call)
    for lo in range(8):
        for hi in range(lo, 8):
            s = Rows(lib, B=7, cut=(lo, hi), **call)
            assert s.off == [o - parent.off[lo] for o in parent.off[lo:hi + 1]], (lo, hi)
            assert s.n == parent.n[lo:hi] and s.ver == parent.ver[lo:hi]
            assert (s.R, s.table, s.table_bytes) == (parent.R, parent.table, parent.table_bytes) and s.table == (0x7000 if call["kind"] == ROUNDS else 0)
            assert s.has_round_of == parent.has_round_of == (name == "rounds") and s.round_of_at == (lo if name == "rounds" else 0)
            assert s.mixed_front == parent.mixed_front and s.has_vers == parent.has_vers
            # what the launch geometry of the slice's own call reads: a uniform call's layout, else whether one of ITS rows is two-phase
            assert s.rec_ver == (parent.rec_ver if call["kind"] == UNIFORM else 1 if any(parent.ver[lo:hi]) else 0)


def test_normalisation(lib):
    r = Rows(lib, MIXED, 3, ns=[8, 1, 8], vers=[0, 0, 0])  # every row compact: the call the public mixed entry points make
    assert not r.has_vers and r.aggregable and r.mixed_front
    r = Rows(lib, MIXED, 3, ns=[8, 1, 8], vers=[0, 1, 0])
    assert r.has_vers and not r.aggregable and r.ver == [0, 1, 0]
    r = Rows(lib, MIXED, 3, ns=[8, 8, 8])  # equal Ns: still the mixed kernels
    assert r.mixed_front and r.aggregable
    r = Rows(lib, UNIFORM, 3, N=8)
    assert not r.mixed_front and r.front_n == 8 and r.aggregable
    assert not Rows(lib, UNIFORM, 3, N=8, rec_ver=1).aggregable
    r = Rows(lib, ROUNDS, 3, round_ns=[202])  # one round: the uniform front end with that N
    assert not r.mixed_front and r.front_n == 202 and r.aggregable and not r.has_round_of
    r = Rows(lib, ROUNDS, 3, round_ns=[202], round_of=[0, 0, 0])
    assert not r.mixed_front and r.front_n == 202
    r = Rows(lib, ROUNDS, 3, round_ns=[8, 8], round_of=[0, 1, 0])  # two rounds of equal N: the mixed front end
    assert r.mixed_front and r.aggregable and r.n == [8, 8, 8]
