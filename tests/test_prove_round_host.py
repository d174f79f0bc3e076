"""not-gpu tier: bbp_prove_round's surface -- header formulas, the binding's packers -- and its per-row logic (csrc/round_bids.h: witness,
list search, status, expanded row, output row) compiled for the host by tests/round_bids_check.cpp, against the big-int oracle
(oracle/ref_py).  The expected values of the GPU tier (tests/test_gpu_prove_round.py) come from the same case builder."""
import ctypes
import random

import pytest

from tests import prove_round_cases as rc

u32 = ctypes.c_uint32
RB_Y, RB_YINV, RB_Q, RB_ZIMG, RB_TOGGLE, RB_STATUS, RB_WORDS = 0, 8, 16, 24, 32, 34, 36


@pytest.fixture(scope="module")
def rcheck(built):
    lib = ctypes.CDLL(built.build_roundcheck())
    lib.rc_round.restype = None
    lib.rc_round.argtypes = [u32, ctypes.c_char_p, u32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p,
                             ctypes.c_void_p]
    lib.rc_rb_words.restype = u32
    mimc = b"".join(rc.b32(c) for c in rc._C)

    def run(r, records=None):
        rb = (u32 * (RB_WORDS * r.B))()
        pin = (ctypes.c_uint8 * ((7 * 32 + 32 * r.N + 8) * r.B))()
        rows = (ctypes.c_uint8 * ((1121 + 32 * (4 + r.N) + 64) * r.B))()
        lib.rc_round(r.N, r.table, r.B, r.bid_bytes, mimc, rb, pin, records, rows if records is not None else None)
        return list(rb), bytes(pin), bytes(rows)
    assert lib.rc_rb_words() == RB_WORDS
    return run


def _words(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def _check_round(run, r):
    rnd = random.Random(r.N)
    rec = 1121 + 32 * (4 + r.N)
    records = bytes(rnd.getrandbits(8) for _ in range(rec * r.B))
    rb, pin, rows = run(r, records)
    for i in range(r.B):
        st, toggle, w = r.expect[i]
        o = rb[RB_WORDS * i:RB_WORDS * (i + 1)]
        assert o[RB_STATUS] == st, i
        if st != rc.OK:
            assert o[:RB_STATUS] == [0] * RB_STATUS, i  # a refused bid leaves nothing behind
            continue
        assert o[RB_Y:RB_Y + 8] == _words(w["y"]) and o[RB_YINV:RB_YINV + 8] == _words(w["y_inv"]), i
        assert o[RB_Q:RB_Q + 8] == _words(w["q"]) and o[RB_ZIMG:RB_ZIMG + 8] == _words(w["z_img"]), i
        assert o[RB_TOGGLE:RB_TOGGLE + 2] == [toggle, 0], i
    assert pin == r.in_rows()
    assert rows == r.rows(records)


def test_header_formulas_and_binding_surface(bbp):
    for n in (1, 3, 8, 202):
        assert bbp.lib.bbp_round_row_size(n) == bbp.record_size(n) + 64 == bbp.round_row_size(n)
    assert bbp.ROUND_BID_BYTES == 64
    hdr = open(bbp.lib_path.rsplit("/", 2)[0] + "/include/bbp.h").read()
    assert "#define BBP_ROUND_BID_BYTES 64u" in hdr
    for name in ("bbp_prepare_round_dev", "bbp_prove_round", "bbp_prove_round_dev"):
        assert name in bbp.SIGNATURES and hasattr(bbp.lib, name), name
    for name in ("prove_round", "prove_round_dev", "prepare_round_dev"):
        assert callable(getattr(bbp.Context, name)), name
    assert "prove_round" in vars(bbp.Pool)


def test_packers_against_hand_built_bytes(bbp):
    d, k = bytes(range(32)), bytes(range(32, 64))
    assert bbp.pack_round_bids([(d, k), (k, d)]) == bytes(range(64)) + k + d
    assert bbp.pack_round_bids([]) == b""
    with pytest.raises(ValueError):
        bbp.pack_round_bids([(d, k[:31])])
    seed, items = b"\x07" * 32, b"\x01" * 32 + b"\x02" * 32
    assert bbp.pack_rounds([(seed, items)]) == ([2], seed + items)  # the round-table packer the verify side uses


def test_null_and_pool_free_screening_without_a_device(bbp):
    """The checks that need no context: a NULL required pointer is BBP_ERR_BAD_ARG in every form."""
    lib = bbp.lib
    assert lib.bbp_prove_round(None, 8, 1, 1, 1, None, 1, None, 1) == 4
    assert lib.bbp_prove_round_dev(None, 8, 1, 1, 1, 1, 1, None, 1, None) == 4
    assert lib.bbp_prepare_round_dev(None, 8, 1, 1, 1, 1, None, None, 1, None) == 4


@pytest.mark.parametrize("N,B", [(1, 5), (3, 5), (8, 5), (202, 3)])
def test_row_logic_matches_the_oracle(rcheck, N, B):
    r = rc.honest(N, B, tag=1)
    assert all(s == rc.OK for s in r.status) and {0, N - 1} <= set(r.toggles)
    _check_round(rcheck, r)


def test_row_logic_statuses(rcheck):
    r = rc.status_round()
    assert r.status == [0, 4, 3, 3, 0, 0, 0, 0] and r.toggles == [2, 0, 0, 0, 0, 7, 1, 3]
    _check_round(rcheck, r)
    bad = rc.status_round(seed=rc.L)  # a non-canonical seed: every row FORMAT, everything zero
    assert bad.status == [3] * 8
    _check_round(rcheck, bad)
    assert rcheck(bad)[1] == bytes(len(bad.in_rows()))
