"""not-gpu tier: the base-index lists of the fixed-base MSMs (csrc/msm_index.h: index_ai, index_s1, index_ao, index_ipa, index_ver over
circuit::compile(N)), compiled for the host by tests/host_check.cpp.  A wrong entry is a wrong proof; tests/test_gpu_tables.py only
sees that the entries stay inside the tables.  Every expected entry comes from a formula written out here."""
import ctypes

import pytest

NS = (1, 8, 202)
BBLIND, G0, H0, BASE_B, N_PUBLIC = 0, 1, 2049, 4097, 4098  # include/bbp.h
PAD_BASE0, MRG_BASE0, TAB_BASES, SKIP = 4098, 4300, 8396, 0xffffffff  # csrc/msm_index.h
AI, S1, AO, IPA, VER = range(5)


@pytest.fixture(scope="module")
def lib(built):
    return ctypes.CDLL(built.build_hostcheck())


def _words(call):
    n = call(None, 0)
    buf = (ctypes.c_uint32 * n)()
    assert call(buf, n) == n
    return [int(x) for x in buf]


@pytest.fixture(scope="module")
def lists(lib):
    """{N: {which: list}} with n_ai_terms under "n_ai", and the gadget program under "w_terms" / "w_loff" / "w_roff" """
    out = {}
    for N in NS:
        n_ai = ctypes.c_uint32()
        d = {w: _words(lambda buf, cap, w=w: lib.hc_index_lists(N, w, buf, cap, ctypes.byref(n_ai))) for w in (S1, AO, IPA, VER, AI)}
        d["n_ai"] = int(n_ai.value)
        for k, name in enumerate(("w_terms", "w_loff", "w_roff")):
            d[name] = _words(lambda buf, cap, k=k: lib.hc_circuit_wires(N, k, buf, cap))
        out[N] = d
    return out


def n_mul(N):
    return 1442 + 3 * N


def test_lengths(lists):
    """what tests/test_gpu_tables.py reads back from the device"""
    for N in NS:
        n, d = n_mul(N), lists[N]
        assert [len(d[w]) for w in (AI, AO, S1, IPA, VER)] == [1 + 2 * n, 1 + n, 1 + 2 * n, 11 * 2 * 2049, N_PUBLIC]
        assert len(d["w_loff"]) == n + 1 and len(d["w_roff"]) == n and d["w_loff"][n] == len(d["w_terms"])


def test_unmerged_lists(lists):
    for N in NS:
        n, d = n_mul(N), lists[N]
        assert d[S1] == [BBLIND] + [G0 + i for i in range(n)] + [H0 + i for i in range(n)]
        assert d[AO] == [BBLIND] + [G0 + i for i in range(n)]
        assert d[VER] == [G0 + i for i in range(2048)] + [H0 + i for i in range(2048)] + [BASE_B, BBLIND]


def test_ai_expands_to_every_base_once(lists):
    """MRG_BASE0 + i stands for G[i] + H[i] + H[i+1], MRG_BASE0 + 2048 + i for G[i] + G[i+1] + H[i+1]; the skip marks carry nothing"""
    for N in NS:
        expanded = []
        for e in lists[N][AI]:
            if e == SKIP:
                continue
            if MRG_BASE0 <= e < MRG_BASE0 + 2048:
                i = e - MRG_BASE0
                expanded += [G0 + i, H0 + i, H0 + i + 1]
            elif MRG_BASE0 + 2048 <= e < TAB_BASES:
                i = e - MRG_BASE0 - 2048
                expanded += [G0 + i, G0 + i + 1, H0 + i + 1]
            else:
                assert e < N_PUBLIC, (N, e)
                expanded.append(e)
        assert sorted(expanded) == sorted(lists[N][S1]), N
        assert len(set(expanded)) == len(expanded), N


def test_ai_merged_triples_share_one_wire(lists):
    for N in NS:
        n, d = n_mul(N), lists[N]
        ai, terms, loff, roff = d[AI], d["w_terms"], d["w_loff"], d["w_roff"]
        left = lambda i: terms[loff[i]:roff[i]]
        right = lambda i: terms[roff[i]:loff[i + 1]]
        merged = skipped = 0
        for pos, e in enumerate(ai):
            if e == SKIP or e < MRG_BASE0:
                continue
            merged += 1
            i = pos - 1
            assert 0 <= i < n - 1, (N, pos)  # a merged base sits at the LEFT input of multiplier i, and i + 1 exists
            if e < MRG_BASE0 + 2048:  # {L_i, R_i, R_i+1}
                assert e == MRG_BASE0 + i and left(i) == right(i) == right(i + 1), (N, i)
                others = (1 + n + i, 1 + n + i + 1)
            else:                     # {L_i, L_i+1, R_i+1}
                assert e == MRG_BASE0 + 2048 + i and left(i) == left(i + 1) == right(i + 1), (N, i)
                others = (1 + i + 1, 1 + n + i + 1)
            assert all(ai[o] == SKIP for o in others), (N, i)
            skipped += 2
        assert merged >= 1 and skipped == ai.count(SKIP), N  # the merged bases are in use; every skip mark belongs to a triple
        assert d["n_ai"] == len(ai) - ai.count(SKIP), N
        assert MRG_BASE0 + 2047 not in ai and MRG_BASE0 + 2048 + 2047 not in ai, N  # the table promises no value there


def test_ipa_rounds(lists):
    """round r, n = 1024 >> (r - 1): generator k sits in block k // 2n, in its low half (i < n) or its high half, at rank blk n + io.
    L pairs the high G's (ranks 0..1023) with the low H's (ranks 1024..2047), R is the mirror; entry 2048 is B."""
    for N in NS:
        ipa, nm = lists[N][IPA], n_mul(N)
        for r in range(1, 12):
            n = 1024 >> (r - 1)
            L, R = ipa[(r - 1) * 2 * 2049:][:2049], ipa[(r - 1) * 2 * 2049 + 2049:][:2049]
            want_l, want_r = [None] * 2049, [None] * 2049
            for k in range(2048):
                blk, i = divmod(k, 2 * n)
                hi, io = i >= n, i % n
                rank = blk * n + io
                if hi:
                    want_l[rank], want_r[1024 + rank] = G0 + k, H0 + k
                else:
                    want_r[rank], want_l[1024 + rank] = G0 + k, H0 + k
            want_l[2048] = want_r[2048] = BASE_B
            pad = PAD_BASE0 + N - 1
            if r == 1 and N < 202:  # the first zero-padded multiplier's H carries the common scalar on the range-sum base
                assert want_l[1024 + (nm - 1024)] == H0 + (nm - 1024)
                want_l[1024 + (nm - 1024)] = pad
            assert L == want_l and R == want_r, (N, r)
            assert (L.count(pad), R.count(pad)) == ((1, 0) if r == 1 and N < 202 else (0, 0)), (N, r)
        assert all(e < N_PUBLIC or e == PAD_BASE0 + N - 1 for e in ipa), N
