"""not-gpu tier: how a verify call is laid out and launched (csrc/verify_plan.h: VerifyKnobs, VerifyDims, plan_verify, VerifyStaging),
compiled for the host by tests/host_check.cpp.  Every expected value comes from a formula written out here, from the Python packers
of the binding or from the library's bbp_*_size functions, never from the header under test."""
import ctypes
import itertools

import pytest

UNIFORM, MIXED, ROUND1, ROUNDS_MX = range(4)
GE, SC, VROW, TERMS, VC_COUNT = 160, 32, 16, 4098, 27  # bytes of a point (four field elements of ten limbs), a scalar, a row descriptor
GEO = ("front mixed rounds np npa Q vb2 one_phase vstride zstride zchunks n_tgt vtw ng agg_flag rd_S rd_nof rd_too_large m n_mul n_cons "
       "n_cst").split()
LAUNCHES = "fill_mimc round_consts vrows parse transcript powers_z powers_yinv flatten vscalars per_row group_sum group_final prep sum lanes compact".split()
MISC = "vpts vchal vs tab var fixed sp rows ns rof rblk rflag".split()
AGG = "vsg fixedg varsum gstatus".split()
AGG_IO = "fixed idx".split()
STAGING = "in_bytes tab_off tab_bytes ent_up_bytes ent_drawn out_bytes fetch_bytes group n_chunks chunk last_row_off sizeof_ge sizeof_vrow".split()
BS = (1, 2, 32, 33, 64, 65, 4095, 4096, 4097, 32768)
GS = (0, 2, 8, 64)


@pytest.fixture(scope="module")
def lib(built):
    return ctypes.CDLL(built.build_hostcheck())


def _up(n):
    return (n + 255) // 256 * 256


def _cdiv(a, b):
    return (a + b - 1) // b


def dims(N):
    """(m, n_mul, n_cons, n_cst) of circuit N: SURVEY.md F7 for the first three; n_cst is a stand-in that grows with N"""
    n_mul = 1442 + 3 * N
    return (4 + N, n_mul, 2 * n_mul + 3 + 3 * N, 100 + N)


class Rows:
    """the arguments of hc_verify_rows / hc_verify_plan / hc_verify_staging for one call"""

    def __init__(self, kind, B, N=0, rec_ver=0, ns=None, vers=None, round_ns=None, round_of=None):
        self.kind, self.B, self.N, self.rec_ver, self.ns, self.vers, self.round_ns, self.round_of = kind, B, N, rec_ver, ns, vers, round_ns, round_of
        arr = lambda t, v: (t * len(v))(*v) if v is not None else None
        self.args = (kind, B, N, rec_ver, arr(ctypes.c_uint32, ns), arr(ctypes.c_uint8, vers), len(round_ns or []), arr(ctypes.c_uint32, round_ns),
                     arr(ctypes.c_uint32, round_of))

    def n_of(self, i):
        return self.N if self.kind == 0 else self.ns[i] if self.kind == 1 else self.round_ns[self.round_of[i] if self.round_of else 0]

    def all_n(self):
        return sorted({self.n_of(i) for i in range(self.B)})


def uniform(B, N, rec_ver=0):
    return Rows(0, B, N=N, rec_ver=rec_ver)


def mixed(B, ns, two_phase_at=None):
    vers = None if two_phase_at is None else [1 if i == two_phase_at else 0 for i in range(B)]
    return Rows(1, B, ns=[ns[i % len(ns)] for i in range(B)], vers=vers)


def rounds(B, round_ns, with_round_of=True):
    return Rows(2, B, round_ns=list(round_ns), round_of=[i % len(round_ns) for i in range(B)] if with_round_of else None)


class Plan:
    def __init__(self, lib, rows, G=0, knobs=None, tr_wave_below=32, ds=None):
        flat = [x.encode() for kv in (knobs or {}).items() for x in kv]
        names = (ctypes.c_char_p * max(1, len(flat)))(*flat)
        ds = ds if ds is not None else [dims(n) for n in rows.all_n()]
        d = (ctypes.c_uint32 * (4 * len(ds)))(*itertools.chain(*ds))
        geo, lay = (ctypes.c_int64 * (len(GEO) + 2 * len(LAUNCHES)))(), (ctypes.c_uint64 * 39)()
        rd_off = (ctypes.c_uint32 * (len(rows.round_ns or []) + 1))()
        self.rc = lib.hc_verify_plan(names, len(flat) // 2, *rows.args, d, len(ds), G, tr_wave_below, geo, lay, rd_off)
        for k, v in zip(GEO, geo):
            setattr(self, k, int(v))
        self.launch = {k: (int(geo[len(GEO) + 2 * i]), int(geo[len(GEO) + 2 * i + 1])) for i, k in enumerate(LAUNCHES)}
        lay = [int(x) for x in lay]
        self.misc = {k: (lay[2 * i], lay[2 * i + 1]) for i, k in enumerate(MISC)}
        self.misc_bytes = lay[24]
        self.agg = {k: (lay[25 + 2 * i], lay[26 + 2 * i]) for i, k in enumerate(AGG)}
        self.agg_bytes = lay[33]
        self.agg_io = {k: (lay[34 + 2 * i], lay[35 + 2 * i]) for i, k in enumerate(AGG_IO)}
        self.agg_io_bytes = lay[38]
        self.rd_off = [int(x) for x in rd_off]


def _packed(regions, total):
    """the non-empty regions are 256-aligned, disjoint, end inside `total`, and nothing but alignment lies between them; an empty one is (0, 0)"""
    at = 0
    for off, n in sorted(r for r in regions.values() if r[1]):
        assert off % 256 == 0 and off == at and off + n <= total, (regions, total)
        at = off + _up(n)
    assert at == total and all(r == (0, 0) for r in regions.values() if not r[1])


def _check(p, rows, G, knobs=None, tr_wave_below=32):
    """every field of the plan of `rows` from the rules, written out"""
    knobs = knobs or {}
    B, ns = rows.B, rows.all_n()
    m, n_mul, n_cons, n_cst = dims(max(ns))  # a mixed call: the strides of its largest N
    two = rows.rec_ver if rows.kind == 0 else int(any(rows.vers or []))
    is_rounds, is_mixed = rows.kind == 2, rows.kind == 1 or (rows.kind == 2 and len(rows.round_ns) > 1)
    assert p.rc == 0
    assert (p.front, p.mixed, p.rounds) == ({(0, 0): UNIFORM, (1, 0): MIXED, (0, 1): ROUND1, (1, 1): ROUNDS_MX}[(is_mixed, is_rounds)], is_mixed, is_rounds)
    assert (p.m, p.n_mul, p.n_cons, p.n_cst) == (m, n_mul, n_cons, n_cst)
    np_ = 6 + m + 5 + 22
    assert (p.np, p.npa, p.one_phase) == (np_, np_ if two else np_ - 3, 0 if two else 1)
    v1 = knobs.get("BBP_VARBASE_V1")
    vb2 = B < 4096 if v1 is None else v1 == "0"
    lanes = max(64, int(knobs.get("BBP_VARBASE_LANES", 65536)))
    assert (p.vb2, p.Q) == (vb2, 1 if vb2 else min(max(lanes // B, 1), p.npa))
    assert (p.vstride, p.zstride, p.zchunks, p.n_tgt) == (8 * np_, n_cons + 1, _cdiv(n_cons + 1, 32), 3 * n_mul + m)
    assert p.vtw == (1 if tr_wave_below > 0 and B <= tr_wave_below else 0)
    assert (p.ng, p.agg_flag) == (_cdiv(B, G) if G else 0, 1 if G else 0)
    # every grid x block covers its work items, with less than one workgroup to spare
    rd_S = sum(1 + n for n in rows.round_ns) if is_rounds else 0
    work = dict(fill_mimc=(B * 90, 64), round_consts=(rd_S, 64), parse=(B, 64), powers_z=(B * p.zchunks, 64), powers_yinv=(B * 64, 64),
                flatten=(B * p.n_tgt, 128), per_row=(B, 64), group_sum=(TERMS, 256), group_final=(p.ng, 64), prep=(B * p.npa, 64), sum=(32 * B, 64),
                lanes=(B * p.Q, 64), transcript=(64 * B if p.vtw else B, 64))
    for name, (items, block) in work.items():
        grid, blk = p.launch[name]
        assert blk == block and items <= grid * blk < items + blk, (name, items, grid, blk)
    assert p.launch["vrows"] == (1, 1024) and p.launch["vscalars"] == (B, 256) and p.launch["compact"] == (1, 1024)
    # the round table
    assert (p.rd_S, p.rd_nof, p.rd_too_large) == (rd_S, B if is_rounds and is_mixed else 0, 0)
    if is_rounds:
        assert p.rd_off == [sum(1 + n for n in rows.round_ns[:r]) for r in range(len(rows.round_ns) + 1)]
    # the layouts: sizes by formula, a region is empty exactly when the front end has no use for it
    R = len(rows.round_ns) if is_rounds else 0
    want = dict(vpts=B * np_ * 32, vchal=B * VC_COUNT * 32, vs=B * TERMS * 32, tab=B * np_ * 8 * GE, var=B * np_ * GE, fixed=B * GE, sp=B * np_ * 32,
                rows=B * VROW if is_mixed else 0, ns=5 * B if is_mixed and not is_rounds else 0, rof=4 * (p.rd_nof + R + 1) if is_rounds else 0,
                rblk=rd_S * SC, rflag=4 * R)
    assert {k: v[1] for k, v in p.misc.items()} == want
    _packed(p.misc, p.misc_bytes)
    want = dict(vsg=p.ng * TERMS * 32, fixedg=p.ng * GE, varsum=B * GE, gstatus=4 * p.ng) if G else dict.fromkeys(AGG, 0)
    assert {k: v[1] for k, v in p.agg.items()} == want
    _packed(p.agg, p.agg_bytes)
    assert {k: v[1] for k, v in p.agg_io.items()} == (dict(fixed=B * GE, idx=4 * B) if G else dict(fixed=0, idx=0))
    _packed(p.agg_io, p.agg_io_bytes)


def _fronts(B):
    yield uniform(B, 8)
    yield uniform(B, 202, rec_ver=1)
    for ns in ((1,), (8,), (202,), (1, 8, 202)):
        yield mixed(B, ns)
        yield mixed(B, ns, two_phase_at=B - 1)
    yield rounds(B, (8,))
    yield rounds(B, (8,), with_round_of=False)  # round_of null with R = 1
    for round_ns in ((8, 8), (1, 202), (8, 8, 8), (1, 8, 202)):
        yield rounds(B, round_ns)


@pytest.mark.parametrize("B", BS)
def test_every_front_end_and_group_size(lib, B):
    for rows in _fronts(B):
        for G in GS:
            if G and (rows.rec_ver or any(rows.vers or [])):
                continue  # a call with a two-phase row is not aggregated
            _check(Plan(lib, rows, G), rows, G)


def test_point_count_is_what_the_packers_put_into_a_row(bbp):
    """np = 6 + m + 5 + 22: the 32-byte points of a two-phase record (A_I1 A_O1 S1 A_I2 A_O2 S2, T_1 T_3..T_6, 11 L and 11 R) and the
    m = 4 + N commitments -- what the record has besides its version byte and the three scalars t_x, t_x_blinding, e_blinding and the
    IPP's a and b"""
    for N in (1, 8, 202):
        rec2 = bbp.lib.bbp_proof_record_size(N) + 96  # three more points than the compact record
        assert (rec2 - 1 - 5 * 32) // 32 == 6 + (4 + N) + 5 + 22 and (rec2 - 1) % 32 == 0


def test_variable_base_rule_and_its_knobs(lib):
    for B, vb2 in ((4095, 1), (4096, 0)):
        assert Plan(lib, uniform(B, 8)).vb2 == vb2
        for v1 in ("0", "1"):
            knobs = {"BBP_VARBASE_V1": v1}
            p = Plan(lib, uniform(B, 8), knobs=knobs)
            assert p.vb2 == (v1 == "0")
            _check(p, uniform(B, 8), 0, knobs=knobs)
    for lanes in ("64", "1000", "65536"):
        for B in (1, 33, 4095, 4097, 32768):
            for v1 in ("0", "1"):
                knobs = {"BBP_VARBASE_LANES": lanes, "BBP_VARBASE_V1": v1}
                _check(Plan(lib, mixed(B, (1, 8, 202)), knobs=knobs), mixed(B, (1, 8, 202)), 0, knobs=knobs)
    p = Plan(lib, uniform(1, 8), knobs={"BBP_VARBASE_V1": "1"})
    assert (p.Q, p.npa) == (42, 42)  # 65536 lanes for one proof: a lane per active point, no more
    assert Plan(lib, uniform(1, 8, 1), knobs={"BBP_VARBASE_V1": "1"}).Q == 45
    assert Plan(lib, uniform(5000, 8)).Q == 13 and Plan(lib, uniform(5000, 8), knobs={"BBP_VARBASE_LANES": "10"}).Q == 1  # clamped to 64 lanes


def test_wavefront_per_proof_rule(lib):
    for below in (32, 7):
        for B, vtw in ((below, 1), (below + 1, 0)):
            p = Plan(lib, uniform(B, 8), tr_wave_below=below)
            assert p.vtw == vtw and p.launch["transcript"] == ((B, 64) if vtw else (1, 64))
    for B in BS:
        p = Plan(lib, mixed(B, (1, 8)), tr_wave_below=0)
        assert p.vtw == 0 and p.launch["transcript"] == (_cdiv(B, 64), 64)


def test_round_table_limit(lib):
    """the reduced table holds 1 + N scalars per round; the first total above 0x7fffffff is refused, the last below it is not"""
    for round_ns, too_large in (([0x7ffffffe], 0), ([0x7fffffff], 1), ([0x3fffffff, 0x3ffffffe], 0), ([0x3fffffff, 0x3fffffff], 1),
                                ([0xfffffffe, 0xfffffffe, 0xfffffffe], 1)):
        total = sum(1 + n for n in round_ns)
        assert (total > 0x7fffffff) == bool(too_large)
        p = Plan(lib, Rows(2, 2, round_ns=round_ns, round_of=[0, len(round_ns) - 1]), ds=[dims(8)])
        assert p.rc == 0 and p.rd_too_large == too_large
        if not too_large:
            assert p.rd_S == total and p.rd_off == [sum(1 + n for n in round_ns[:r]) for r in range(len(round_ns) + 1)]


def test_knob_names_and_clamps(lib):
    from tests.test_prove_plan_host import NOT_PROVE_KNOBS
    rows = uniform(64, 8)
    for name in ("BBP_VARBASE_LANES", "BBP_VERIFY_OVERLAP", "BBP_VERIFY_AGGREGATE", "BBP_VARBASE_V1", "BBP_V_FENCE", "BBP_HOST_CHUNK_VERIFY"):
        assert Plan(lib, rows, knobs={name: "1"}).rc == 0, name
    # a prove or an MSM knob is none of the verifier's, and the verdict-changing knock-out mask exists in experiment builds only
    for name in ("BBP_TR_WAVE_BELOW", "BBP_SERIAL_LDS", "BBP_SLICES", "BBP_FOLD_HALF_FROM", "BBP_SORT_STAGED", "BBP_HOST_CHUNK_PROVE", "BBP_KO_VERIFY"):
        assert Plan(lib, rows, knobs={name: "1"}).rc == -1, name
    assert {"BBP_VARBASE_LANES", "BBP_VERIFY_OVERLAP"} <= set(NOT_PROVE_KNOBS)  # (the prove plan's test refuses them from its side)
    lib.hc_verify_knob_from_env.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    env = lambda name, text, which: int(lib.hc_verify_knob_from_env(name.encode(), text.encode(), which))
    for text, want in {"0": 64, "63": 64, "64": 64, "1000": 1000, "65536": 65536}.items():
        assert env("BBP_VARBASE_LANES", text, 0) == want
    for text, want in {"0": 0, "1": 1, "5": 1}.items():
        assert env("BBP_VERIFY_OVERLAP", text, 1) == want
    for text, want in {"0": 0, "1": 0, "2": 2, "32": 32, "-4": 0}.items():
        assert env("BBP_VERIFY_AGGREGATE", text, 2) == want
    for text, want in {"0": 32768, "-1": 32768, "1": 1, "16": 16, "60": 60}.items():
        assert env("BBP_HOST_CHUNK_VERIFY", text, 5) == want
    # defaults; the two process-wide knobs were read before the variable was set, so a context made now does not see them
    assert [env("BBP_NOT_A_KNOB", "1", w) for w in range(6)] == [65536, 1, 0, -1, 0, 32768]
    assert env("BBP_VARBASE_V1", "1", 3) == -1 and env("BBP_V_FENCE", "1", 4) == 0


class Staging:
    def __init__(self, lib, rows, group=0, ctx_group=0, dev_draw=0, host_chunk=32768):
        out = (ctypes.c_uint64 * len(STAGING))()
        lib.hc_verify_staging(*rows.args, group, ctx_group, dev_draw, host_chunk, out)
        for k, v in zip(STAGING, out):
            setattr(self, k, int(v))


def test_sizes_the_formulas_above_rest_on(lib):
    s = Staging(lib, uniform(1, 8))
    assert (s.sizeof_ge, s.sizeof_vrow) == (GE, VROW)


@pytest.mark.parametrize("B", (1, 33, 640))
def test_staging_regions(lib, bbp, B):
    cases = [(uniform(B, 8), [bbp.verify_row_size(8)] * B, 0),
             (mixed(B, (1, 8, 202)), [bbp.verify_row_size((1, 8, 202)[i % 3]) for i in range(B)], 0),
             (rounds(B, (8,), with_round_of=False), [bbp.round_row_size(8)] * B, 32 * 9),
             (rounds(B, (1, 8, 202)), [bbp.round_row_size((1, 8, 202)[i % 3]) for i in range(B)], 32 * (2 + 9 + 203))]
    for rows, sizes, table in cases:
        for dd in (0, 1):
            s = Staging(lib, rows, dev_draw=dd)
            assert (s.in_bytes, s.tab_off, s.tab_bytes, s.last_row_off) == (sum(sizes), _up(sum(sizes)), table, sum(sizes[:-1]))
            assert (s.ent_up_bytes, s.ent_drawn) == ((0, 32 * B) if dd else (32 * B, 0))
            assert (s.out_bytes, s.fetch_bytes) == (4 * (B + 1), 4 * B)
            assert Staging(lib, rows, group=8, dev_draw=dd).fetch_bytes == 4 * (B + 1)  # ... with the fallback counter
    Ns = [(1, 8, 202)[i % 3] for i in range(B)]
    assert Staging(lib, mixed(B, (1, 8, 202))).in_bytes == bbp.mixed_row_offsets(Ns)[B]
    assert Staging(lib, mixed(B, (1, 8, 202), two_phase_at=0)).in_bytes == bbp.mixed_row_offsets(Ns)[B] + 96


def test_chunk_split(lib):
    # the first two: what tests/test_gpu_verify_rounds.py and tests/test_gpu_verify_mixed.py assert of BBP_HOST_CHUNK_VERIFY = 16 and 14
    for B, host_chunk, n_chunks, chunk in ((70, 16, 5, 14), (40, 14, 3, 14), (32768, 32768, 1, 32768), (32769, 32768, 2, 16385), (1, 32768, 1, 1),
                                           (60, 60, 1, 60), (61, 60, 2, 31)):
        s = Staging(lib, uniform(B, 8), host_chunk=host_chunk)
        assert (s.n_chunks, s.chunk) == (n_chunks, chunk), B
        cuts = list(range(0, B, chunk))
        assert len(cuts) == n_chunks and all(min(chunk, B - c) <= host_chunk for c in cuts)
    assert [min(14, 40 - c) for c in range(0, 40, 14)] == [14, 14, 12]


def test_group_rule(lib):
    # (the caller's group, the context's, B, a two-phase row) -> the group the call runs with
    table = {(0, 0, 64, 0): 0, (8, 0, 64, 0): 8, (8, 0, 3, 0): 8, (8, 32, 64, 0): 8, (1, 0, 64, 0): 1,
             (0, 32, 63, 0): 0, (0, 32, 64, 0): 32, (0, 32, 65, 0): 32, (0, 1, 64, 0): 0, (0, 2, 3, 0): 0, (0, 2, 4, 0): 2,
             (8, 0, 64, 1): 0, (0, 32, 64, 1): 0, (8, 32, 64, 1): 0}
    for (group, ctx_group, B, two), want in table.items():
        for rows in (uniform(B, 8, rec_ver=two), mixed(B, (1, 8), two_phase_at=B - 1 if two else None)):
            s = Staging(lib, rows, group=group, ctx_group=ctx_group)
            assert s.group == want and s.fetch_bytes == 4 * (B + (1 if want > 1 else 0)), (group, ctx_group, B, two)


def test_case_grid_under_the_sanitizers(built):
    """tests/verify_plan_san.cpp: the same exports over the grid above in a stand-alone program built with -fsanitize=address,undefined"""
    import subprocess
    p = subprocess.run([built.build_verify_plan_san()], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "sanitizer report or failed expectation:\n" + (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("0 failures")
