"""not-gpu tier: the row sizes of the prove side and the staging layout of one host-pointer prove call (csrc/prove_io.h), compiled for
the host by tests/host_check.cpp.  Every expected size comes from the Python packers of the binding and the test cases
(prove_row_size, pack_round_bids, pack_rounds, pack_mixed_rows, Round.in_row), from the library's bbp_*_size functions or from a
formula written out here, never from the header under test."""
import ctypes
import itertools

import pytest

from tests import prove_round_cases as rc

NS, BS = (1, 2, 8, 202), (1, 3, 64, 640)
MODES = list(itertools.product((0, 1), repeat=3))  # (round, check, device-drawn entropy)
SIZES = ("prove_in_bytes prove_in_words in_q in_list in_list_word in_toggle in_toggle_word entropy_row verify_tail verify_tail_words "
         "tail_list_word round_bid round_table").split()
LAYOUT = ("in_stride ent_stride rec res_stride in_first_bytes in_tab in_tab_bytes in_scratch in_rows in_upload in_cap rs_end rs_rb ent_drawn "
          "ent_up_off ent_up_bytes ent_cap ent_check out_recs out_info out_status out_mask out_fail_n out_fail_idx out_tog out_pass_st out_fetch "
          "out_cap chk_vstatus chk_bytes h_in h_out").split()
RINGS = "c_vstatus c_scratch c_mask c_bytes r_pass_bytes r_rows r_recs r_bytes".split()


@pytest.fixture(scope="module")
def lib(built):
    return ctypes.CDLL(built.build_hostcheck())


class Probe:
    def __init__(self, lib, B, N, mode=(0, 0, 0), first=0):
        s, l, r = (ctypes.c_uint64 * len(SIZES))(), (ctypes.c_uint64 * len(LAYOUT))(), (ctypes.c_uint64 * len(RINGS))()
        lib.hc_prove_staging(B, N, mode[0], mode[1], mode[2], first, s, l, r)
        for names, vals in ((SIZES, s), (LAYOUT, l), (RINGS, r)):
            for k, v in zip(names, vals):
                setattr(self, k, int(v))


def _up(n):
    return (n + 255) // 256 * 256


def _disjoint_inside(regions, cap):
    """regions: (offset, bytes); the non-empty ones do not overlap and end inside cap"""
    at = 0
    for off, n in sorted(r for r in regions if r[1]):
        assert off >= at and off + n <= cap, (regions, cap)
        at = off + n


@pytest.mark.parametrize("N", NS)
def test_row_helpers_are_the_packers_row_lengths(lib, bbp, N):
    p = Probe(lib, 1, N)
    r = rc.honest(N, 1, tag=3)
    row = r.in_row(0)
    assert p.prove_in_bytes == len(row) == bbp.prove_row_size(N) and p.prove_in_words * 4 == len(row)
    assert row[p.in_q:p.in_q + 96] == r.tail(0) + r.seed and row[p.in_list:p.in_toggle] == b"".join(r.items)  # q, z_img, seed; the list
    assert (p.in_list, p.in_list_word * 4, p.in_toggle_word * 4) == (7 * 32, 7 * 32, p.in_toggle) and p.in_toggle + 8 == len(row)
    assert int.from_bytes(row[p.in_toggle:], "little") == r.toggles[0]
    assert p.entropy_row == bbp.lib.bbp_entropy_size(N) == bbp.entropy_size(N) == len(rc.entropy(1, 1, N))
    rec = bbp.lib.bbp_proof_record_size(N)
    _, vrow = bbp.pack_mixed_rows([(bytes(rec), r.tail(0)[:32], r.tail(0)[32:], r.seed, b"".join(r.items))])
    assert p.verify_tail == len(vrow) - rec == bbp.verify_row_size(N) - rec and p.verify_tail_words * 4 == p.verify_tail
    assert vrow[rec + 4 * p.tail_list_word:] == b"".join(r.items)
    assert p.round_bid == len(bbp.pack_round_bids([(bytes(32), bytes(32))])) == bbp.ROUND_BID_BYTES == len(r.bid_bytes)
    assert p.round_table == len(bbp.pack_rounds([(r.seed, b"".join(r.items))])[1]) == len(r.table)
    assert (p.in_stride, p.ent_stride, p.rec) == (len(row), p.entropy_row, rec)
    assert Probe(lib, 1, N, (1, 0, 0)).res_stride == bbp.round_row_size(N) == bbp.lib.bbp_round_row_size(N) and p.res_stride == rec


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_regions_of_every_mode(lib, bbp, B, N):
    rec, vrow, in_row, ent_row = bbp.lib.bbp_proof_record_size(N), bbp.verify_row_size(N), bbp.prove_row_size(N), bbp.entropy_size(N)
    for mode in MODES:
        rnd, chk, dd = mode
        p = Probe(lib, B, N, mode, first=B - 1)
        # slot `in`: rows alone, or bids, table, the pass's scratch and the rows it writes
        if rnd:
            scratch = 512 + _up(32 * (1 + N)) + _up(4 * 36 * B)  # two offsets, a flag, the reduced table, 36 words per bid
            assert p.rs_end == scratch and p.rs_rb == scratch - _up(4 * 36 * B)
            _disjoint_inside([(0, 64 * B), (p.in_tab, 32 * (1 + N)), (p.in_scratch, scratch), (p.in_rows, in_row * B)], p.in_cap)
            assert p.in_tab % 256 == 0 and p.in_scratch % 256 == 0 and p.in_rows % 256 == 0
            assert (p.in_first_bytes, p.in_tab_bytes, p.in_upload) == (64 * B, 32 * (1 + N), p.in_tab + 32 * (1 + N))
        else:
            assert (p.in_rows, p.in_first_bytes, p.in_upload, p.in_cap, p.in_tab_bytes) == (0, in_row * B, in_row * B, in_row * B, 0)
        assert p.in_cap == p.in_rows + in_row * B
        # slot `ent`: the prover's rows, drawn or uploaded, then the check's weights; the two spans make up the buffer
        assert p.ent_drawn == (ent_row * B if dd else 0) and p.ent_up_off == p.ent_drawn
        assert p.ent_up_bytes == (0 if dd else ent_row * B) + (32 * B if chk else 0)
        assert p.ent_drawn + p.ent_up_bytes == p.ent_cap
        assert p.ent_check == ent_row * B + 32 * (B - 1) and (not chk or p.ent_check + 32 == p.ent_cap)
        # slot `out`
        info = [(p.out_status, 4 * B), (p.out_mask, 4 * B), (p.out_fail_n, 4), (p.out_fail_idx, 4 * B)] if chk else []
        pass_out = [(p.out_tog, 8 * B), (p.out_pass_st, 4 * B)] if rnd else []
        _disjoint_inside([(0, p.res_stride * B)] + info + pass_out, p.out_fetch)
        _disjoint_inside([(0, p.out_fetch)] + ([(p.out_recs, rec * B)] if rnd else []), p.out_cap)
        last = (pass_out or info or [(0, p.res_stride * B)])[-1]
        assert p.out_fetch == last[0] + last[1]  # nothing is fetched that the host does not read
        if chk or rnd:
            assert p.out_info % 256 == 0 and p.out_info == p.out_status  # the info block holds 32-bit words, the toggles are u64
        if rnd:
            assert p.out_tog % 256 == 0 and p.out_pass_st % 4 == 0 and p.out_recs % 256 == 0 and p.out_cap == p.out_recs + rec * B
        else:
            assert p.out_recs == 0 and p.out_cap == p.out_fetch
        # slot `chk` and the mirrors
        if chk:
            _disjoint_inside([(0, vrow * B), (p.chk_vstatus, 4 * B)], p.chk_bytes)
            assert p.chk_vstatus % 256 == 0 and p.chk_bytes == p.chk_vstatus + 4 * B
        else:
            assert p.chk_bytes == 0
        assert p.h_in == p.in_upload + p.ent_up_bytes and p.h_out == p.out_fetch
    # the rings: scratch, then masks | the pass's scratch, the rows, the records
    p = Probe(lib, B, N)
    _disjoint_inside([(0, vrow * B), (p.c_vstatus, 4 * B), (p.c_mask, 4 * B)], p.c_bytes)
    assert p.c_vstatus % 256 == 0 and p.c_mask % 256 == 0 and p.c_bytes == p.c_mask + 4 * B
    assert (p.c_vstatus, p.c_scratch) == (Probe(lib, B, N, (0, 1, 0)).chk_vstatus, Probe(lib, B, N, (0, 1, 0)).chk_bytes)
    scratch = 512 + _up(32 * (1 + N)) + _up(4 * 36 * B)
    _disjoint_inside([(0, scratch), (p.r_rows, in_row * B), (p.r_recs, rec * B)], p.r_bytes)
    assert p.r_pass_bytes == scratch == p.r_rows and p.r_recs % 256 == 0 and p.r_bytes == p.r_recs + rec * B


# (B, N) = (64, 8) as the commit before this header laid it out (its formulas, evaluated by hand): the header renames arithmetic, it
# does not move anything.  Columns: in_tab in_scratch in_rows in_upload in_cap | ent_up_off ent_up_bytes ent_cap | out_recs out_info
# out_tog out_pass_st out_fetch out_cap | chk_bytes h_in h_out
BEFORE_64_8 = {
    (0, 0, 0): (0, 0, 0, 31232, 31232, 0, 26624, 26624, 0, 96320, 96320, 96320, 96320, 96320, 0, 57856, 96320),
    (0, 0, 1): (0, 0, 0, 31232, 31232, 26624, 0, 26624, 0, 96320, 96320, 96320, 96320, 96320, 0, 31232, 96320),
    (0, 1, 0): (0, 0, 0, 31232, 31232, 0, 28672, 28672, 0, 96512, 97284, 97284, 97284, 97284, 119296, 59904, 97284),
    (0, 1, 1): (0, 0, 0, 31232, 31232, 26624, 2048, 28672, 0, 96512, 97284, 97284, 97284, 97284, 119296, 33280, 97284),
    (1, 0, 0): (4096, 4608, 14848, 4384, 46080, 0, 26624, 26624, 101376, 100608, 100608, 101120, 101376, 197696, 0, 31008, 101376),
    (1, 0, 1): (4096, 4608, 14848, 4384, 46080, 26624, 0, 26624, 101376, 100608, 100608, 101120, 101376, 197696, 0, 4384, 101376),
    (1, 1, 0): (4096, 4608, 14848, 4384, 46080, 0, 28672, 28672, 102400, 100608, 101632, 102144, 102400, 198720, 119296, 33056, 102400),
    (1, 1, 1): (4096, 4608, 14848, 4384, 46080, 26624, 2048, 28672, 102400, 100608, 101632, 102144, 102400, 198720, 119296, 6432, 102400),
}


@pytest.mark.parametrize("mode", MODES)
def test_offsets_of_64_by_8_are_the_previous_ones(lib, mode):
    p = Probe(lib, 64, 8, mode)
    got = (p.in_tab, p.in_scratch, p.in_rows, p.in_upload, p.in_cap, p.ent_up_off, p.ent_up_bytes, p.ent_cap, p.out_recs, p.out_info, p.out_tog,
           p.out_pass_st, p.out_fetch, p.out_cap, p.chk_bytes, p.h_in, p.h_out)
    assert got == BEFORE_64_8[mode]
    assert (p.in_stride, p.ent_stride, p.rec, p.ent_check) == (488, 416, 1505, 26624)
    if mode[1]:  # the info block: statuses, masks, the fail counter, the fail indices
        assert (p.out_status, p.out_mask, p.out_fail_n, p.out_fail_idx) == (p.out_info, p.out_info + 256, p.out_info + 512, p.out_info + 516)
    assert (p.c_vstatus, p.c_scratch, p.c_mask, p.c_bytes) == (119040, 119296, 119296, 119552)
    assert (p.r_pass_bytes, p.r_rows, p.r_recs, p.r_bytes) == (10240, 10240, 41472, 137792)
