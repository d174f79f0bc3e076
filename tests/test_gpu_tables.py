"""gpu tier: the resident tables every kernel trusts, audited entry by entry against the big-int oracle.  bbp_debug_table hands out the
device pointers; the check kernels of tests/device_check.hip read the tables in place (same process, same HIP context).

  gens     all 8396 points encoded on the device: the 4098 public bases from blindbid.gens(2048), the 202 range sums of k_pad_sums,
           the 4094 merged bases of k_merge_sums; entry 2047 of either merged half is only promised to be a valid point and no index
           list may name it
  ptable   every one of the 8396 x 256 rows, consumed as the MSM consumes it (load_row_at + ge_madd_row, both signs), against a
           ge_dbl walk from gens[i] on the device: onto the identity, where only y+x and y-x count (T = 0 multiplies 2dxy away), and
           onto P itself, where all three fields count (P + row = 2P, P - row = 0) -- and, independent of ge_dbl, a sample of rows
           added to the identity and to the basepoint against Python's 2^b P and B + 2^b P
  comb     all 1024 entries against m 16^j Base, the third field of each against 2d x y of its point
  btab     every entry of the table the shipped k_tail_tables built at start-up against m 2^(w k) B

Points are compared by their encodings, byte for byte."""
import ctypes

import pytest

from oracle.ref_py import blindbid as bb, ristretto as rs
from tests.table_run import GE_BYTES, ROW_BYTES, COMB_BYTES, Tables

pytestmark = pytest.mark.gpu

N_PUBLIC, PAD_BASE0, PAD_BASES, MRG_BASE0, TAB_BASES, MSM_POS = 4098, 4098, 202, 4300, 8396, 256  # csrc/context.h
SKIP_BASE = 0xffffffff
LISTS = (1, 8, 202)  # list lengths whose index lists are read


@pytest.fixture(scope="module")
def tables(built, bbp):  # bbp: torch's HIP runtime loads first (conftest.py)
    return Tables(ctypes.CDLL(built.build_devcheck("chain")), "chain")


@pytest.fixture(scope="module")
def oracle_gens():
    """the 8396 bases as the oracle builds them (index 2047 of either merged half: None, the source promises no value)"""
    pc, bp = bb.gens(2048)
    G, H = bp.G, bp.H
    out = [pc.B_blinding] + list(G) + list(H) + [pc.B]
    pad, acc = {202: rs.IDENT}, rs.IDENT
    for k in range(1023, 420, -1):  # PAD_BASE0 + N - 1 = H[418 + 3N] + .. + H[1023]
        acc = rs.pt_add(acc, H[k])
        if (k - 418) % 3 == 0:
            pad[(k - 418) // 3] = acc
    assert sorted(pad) == list(range(1, 203))
    out += [pad[n] for n in range(1, 203)]
    out += [rs.pt_add(rs.pt_add(G[i], H[i]), H[i + 1]) for i in range(2047)] + [None]
    out += [rs.pt_add(rs.pt_add(G[i], G[i + 1]), H[i + 1]) for i in range(2047)] + [None]
    assert len(out) == TAB_BASES
    return out


@pytest.fixture(scope="module")
def device_gens(ctx, bbp, tables):
    dev, size = ctx.debug_table(bbp.TABLE_GENS)
    assert size == TAB_BASES * GE_BYTES
    return tables.points(dev, size)


def test_base_indices(bbp):
    assert (bbp.BASE_BBLIND, bbp.BASE_G0, bbp.BASE_H0, bbp.BASE_B, bbp.NUM_BASES) == (0, 1, 2049, 4097, N_PUBLIC)
    assert PAD_BASE0 + PAD_BASES == MRG_BASE0 and MRG_BASE0 + 2 * 2048 == TAB_BASES


def test_gens_every_entry(device_gens, oracle_gens):
    unspecified = {MRG_BASE0 + 2047, MRG_BASE0 + 2048 + 2047}
    bad = [i for i, p in enumerate(oracle_gens) if i not in unspecified and device_gens[i] != rs.encode(p)]
    assert not bad, (len(bad), bad[:5])
    assert device_gens[PAD_BASE0 + 202 - 1] == bytes(32)  # N = 202: the empty range
    for i in sorted(unspecified):  # "any valid point will do"
        assert rs.decode(device_gens[i]) is not None, i


def test_index_lists_stay_inside_the_tables(ctx, bbp, tables):
    """every entry of every base-index list names a base that has rows, or is the skip mark; none names the unspecified merged entry"""
    for n in LISTS:
        n_mul = 1442 + 3 * n
        sizes = {bbp.TABLE_IDX_AI: 1 + 2 * n_mul, bbp.TABLE_IDX_AO: 1 + n_mul, bbp.TABLE_IDX_S1: 1 + 2 * n_mul, bbp.TABLE_IDX_IPA: 11 * 2 * 2049,
                 bbp.TABLE_IDX_VER: N_PUBLIC}
        for which, count in sizes.items():
            dev, size = ctx.debug_table(which | (n << 8))
            assert size == 4 * count, (n, which)
            idx = tables.words(dev, size)
            assert all(i < TAB_BASES or (i == SKIP_BASE and which == bbp.TABLE_IDX_AI) for i in idx), (n, which)
            assert MRG_BASE0 + 2047 not in idx and MRG_BASE0 + 2048 + 2047 not in idx, (n, which)
            if which == bbp.TABLE_IDX_AI:
                assert any(MRG_BASE0 <= i < TAB_BASES for i in idx), n  # the merged bases are in use
            if which == bbp.TABLE_IDX_IPA:
                assert (PAD_BASE0 + n - 1 in idx) == (n < 202), n  # (N = 202 pads nothing)


def test_index_list_lengths_are_screened(ctx, bbp):
    for n, status in ((0, 4), (203, 2), (0xffffff, 2)):  # BAD_ARG, GENS_LEN: before anything is compiled
        with pytest.raises(bbp.BbpError) as e:
            ctx.debug_table(bbp.TABLE_IDX_AI | (n << 8))
        assert e.value.status == status, n
    for which in (9, 0xff, bbp.TABLE_GENS | (8 << 8)):  # no such table; N with a table that takes none
        with pytest.raises(bbp.BbpError) as e:
            ctx.debug_table(which)
        assert e.value.status == 4, which


def test_ptable_every_row(ctx, bbp, tables):
    gens, gsize = ctx.debug_table(bbp.TABLE_GENS)
    table, tsize = ctx.debug_table(bbp.TABLE_PTABLE)
    assert gsize == TAB_BASES * GE_BYTES and tsize == TAB_BASES * MSM_POS * ROW_BYTES
    bad, first = tables.walk(gens, gsize, table, tsize, TAB_BASES, MSM_POS)
    wrong = [(i, first[i], bad[i]) for i in range(TAB_BASES) if bad[i]]
    assert not wrong, "%d mismatching checks (four per row); first (base, bit, count): %r" % (sum(bad), wrong[:3])
    assert all(f == MSM_POS for f in first)


def test_ptable_sample_against_python(ctx, bbp, tables, oracle_gens):
    """independent of ge_dbl on the device: 2^b P by the oracle's doublings, and B + 2^b P (an accumulator with T != 0 reads 2dxy)"""
    table, tsize = ctx.debug_table(bbp.TABLE_PTABLE)
    bases = [0, N_PUBLIC - 1, PAD_BASE0, PAD_BASE0 + PAD_BASES - 1, MRG_BASE0, MRG_BASE0 + 2046, MRG_BASE0 + 2048, MRG_BASE0 + 2048 + 2046,
             PAD_BASE0 + 201 - 1, bbp.BASE_G0, bbp.BASE_G0 + 2047, bbp.BASE_H0, bbp.BASE_H0 + 2047, bbp.BASE_B, bbp.BASE_BBLIND]
    bits = [0, 15, 16, 17, 127, 128, 252, 255]
    assert PAD_BASE0 + 1 - 1 in bases and PAD_BASE0 + 202 - 1 in bases
    pairs = [(i, b) for i in sorted(set(bases)) for b in bits]
    got, got_b = tables.rows(table, tsize, [i * MSM_POS + b for i, b in pairs])
    at = 0
    for i in sorted(set(bases)):
        p, b_now = oracle_gens[i], 0
        for b in bits:
            while b_now < b:
                p, b_now = rs.pt_dbl(p), b_now + 1
            assert got[at] == rs.encode(p), (i, b)
            assert got_b[at] == rs.encode(rs.pt_add(rs.BASEPOINT, p)), (i, b)
            at += 1


def test_comb_every_entry(ctx, bbp, tables):
    dev, size = ctx.debug_table(bbp.TABLE_COMB)
    assert size == 2 * 64 * 8 * COMB_BYTES
    got, xy2d_ok = tables.comb(dev, size)
    assert all(f == 1 for f in xy2d_ok), [i for i, f in enumerate(xy2d_ok) if f != 1][:5]
    pc, _ = bb.gens(2048)
    for b, base in enumerate((pc.B, pc.B_blinding)):
        p = base
        for j in range(64):
            m = p
            for k in range(8):
                assert got[(b * 64 + j) * 8 + k] == rs.encode(m), (b, j, k)  # (k + 1) * 16^j * Base
                m = rs.pt_add(m, p)
            for _ in range(4):
                p = rs.pt_dbl(p)


def test_btab_every_entry(ctx, bbp, tables):
    pieces = tables.tail_pieces()  # the geometry the libraries were built with (csrc/scalarmul.h)
    bits = 256 // pieces
    dev, size = ctx.debug_table(bbp.TABLE_BTAB)
    assert size == 8 * pieces * GE_BYTES
    got = tables.points(dev, size)
    p = bb.gens(2048)[0].B
    for k in range(pieces):
        m = p
        for j in range(8):
            assert got[8 * k + j] == rs.encode(m), (k, j)  # (j + 1) * 2^(bits k) * B
            m = rs.pt_add(m, p)
        for _ in range(bits):
            p = rs.pt_dbl(p)

