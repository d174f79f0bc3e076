"""Shapes and scalar rows of the MSM GPU tests, and the plan csrc/msm_plan.h makes for a launch (tests/host_check.cpp hc_msm_plan).
Shared by the GPU tests that launch the cases (test_gpu_msm_paths.py, test_gpu_fuzz.py) and the not-gpu ledger that proves, from the
plan and the product's own recoder, which kernel path every case takes (test_msm_plan_host.py): a shape list cannot miss its target
unseen.  No capacity is written down here: every count is derived from the plan of the launch."""
import collections
import ctypes
import functools
import random

from oracle.ref_py import ristretto as rs

L = rs.L
LAYOUT_G_H, LAYOUT_G = 0, 1  # include/bbp.h BBP_LAYOUT_BLIND_G_H (n_terms = 1 + 2m) / BBP_LAYOUT_BLIND_G (1 + m)
LARGE, SMALL = 0, 1                        # MsmPlan::Geom
PLAIN, STAGED, STAGED_WIDE = 0, 1, 2       # MsmPlan::Sort
LANES128, HALF, SMALL_FOLD = 0, 1, 2       # MsmPlan::Fold
KNOB_ORDER = ["sort_staged", "fold_half_from", "msm_small", "split_below", "split_target"]  # hc_msm_knob_from_env's `which`

Plan = collections.namedtuple("Plan", "split n_sub n_work geom sort sort_cap fold reduce K W naf")


def plan(lib, n_msm, n_terms, knobs=None, device_sized=False):
    """plan_msm(knobs, n_msm, n_terms, device_sized); knobs: {environment name: text} over the defaults"""
    flat = [s.encode() for kv in (knobs or {}).items() for s in kv]
    names = (ctypes.c_char_p * max(len(flat), 1))(*flat)
    out = (ctypes.c_int64 * 11)()
    lib.hc_msm_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    rc = lib.hc_msm_plan(names, len(flat) // 2, n_msm, n_terms, int(device_sized), out)
    assert rc == 0, "not an MSM knob among %r" % (knobs,)
    return Plan(*[int(x) for x in out])


def path(p):
    return (p.geom, p.sort, p.fold)


def knob_from_env(lib, name, text, member):
    """MsmKnobs::from_env().<member> with name=text in the environment"""
    return int(lib.hc_msm_knob_from_env(name.encode(), text.encode(), KNOB_ORDER.index(member)))


def row_bytes(row):
    return b"".join(rs.sc_bytes(v) for v in row)


def histogram(lib, width, row, K):
    """entries per bucket (|d| + 1) / 2 of one row's scalars under the product's recoder, and how many of them are negative digits"""
    hist, neg = (ctypes.c_uint32 * (K + 1))(), (ctypes.c_uint32 * (K + 1))()
    lib.hc_msm_histogram.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    rc = lib.hc_msm_histogram(width, len(row), row_bytes(row), K, hist, neg)
    assert rc == 0, "a digit fell outside the %d buckets" % K
    return list(hist), list(neg)


def walk(hist, cap):
    """k_msm_sort_staged's scatter by its stated rule: buckets in order, a window takes as many consecutive buckets as fit the image
    of `cap` entries, a bucket larger than the image a direct pass of its own.  -> [(kind, non-empty buckets)] of the passes that
    place anything"""
    K, out, kb = len(hist) - 1, [], 1
    while kb <= K:
        if hist[kb] > cap:
            kind, ke = "direct", kb + 1
        else:
            kind, ke, total = "staged", kb, 0
            while ke <= K and total + hist[ke] <= cap:
                total += hist[ke]
                ke += 1
        full = [k for k in range(kb, ke) if hist[k]]
        if full:
            out.append((kind, full))
        kb = ke
    return out


# ---- building blocks -----------------------------------------------------------------------------------------------------------
def ones(k):
    """k width-12 digits of magnitude 1 (bucket 1): bits 13 apart"""
    return sum(1 << (13 * j) for j in range(k))


ONES_19 = ones(19)                                  # the most such digits a scalar below L holds
NEG_POS_PAIRS = sum(0xFFF << (26 * j) for j in range(9))  # 0xFFF = 2^12 - 1: digits -1 and +1, nine pairs, all in bucket 1


def bucket1(count, n):
    """terms that put exactly `count` entries in bucket 1 and none elsewhere, at most n of them"""
    k = 16 if count // 16 + 2 <= n else 19
    full, rem = divmod(count, k)
    terms = [ones(k)] * full + ([ones(rem)] if rem else [])
    assert len(terms) <= n, (count, n)
    return terms


# ---- unsplit launches: 128 MSMs, the adversarial row at index 0, in the middle and at the end ------------------------------------
UNSPLIT_B = 128                # the smallest launch that is never split
ADVERSARIAL_AT = (0, 61, 127)
RANDOM_AT = (1, 40, 90, 126)   # uniformly random filler rows; the other fillers are all zero (odd index) or hold one term (even)

Row = collections.namedtuple("Row", "scalars counts only walk neg_half")
# counts: [(bucket, relation, entries)] the histogram must satisfy; only: the buckets that may hold anything (None: any);
# walk: the passes of the staged scatter (None: the ledger names what it checks of them); neg_half: this bucket is half negative digits


def bucket_rows(n, cap, layout):
    """name -> Row for an MSM of n terms whose staged sort has an image of `cap` entries"""
    rnd = random.Random(9000 + n)
    pad = lambda terms: terms + [0] * (n - len(terms))
    rows = collections.OrderedDict()
    rows["all_ones19"] = Row([ONES_19] * n, [(1, "==", 19 * n), (1, ">", cap)], {1}, [("direct", [1])], None)
    rows["exact_capacity"] = Row(pad(bucket1(cap, n)), [(1, "==", cap)], {1}, [("staged", [1])], None)
    rows["capacity_plus_1"] = Row(pad(bucket1(cap, n) + [1]), [(1, "==", cap + 1)], {1}, [("direct", [1])], None)
    rows["boundary_between_1_and_2"] = Row(pad(bucket1(cap - 3, n) + [3] * 7), [(1, "==", cap - 3), (2, "==", 7)], {1, 2},
                                           [("staged", [1]), ("staged", [2])], None)
    light = 5
    rows["oversized_in_the_middle"] = Row([ONES_19] * light + [999 * ONES_19] * (n - 2 * light) + [2047 * ONES_19] * light,
                                          [(500, "==", 19 * (n - 2 * light)), (500, ">", cap), (1, "==", 19 * light), (1024, "==", 19 * light)],
                                          {1, 500, 1024}, [("staged", [1]), ("direct", [500]), ("staged", [1024])], None)
    if layout == LAYOUT_G_H:
        rows["adjacent_oversized"] = Row([ONES_19 if i % 2 else 3 * ONES_19 for i in range(n)], [(1, ">", cap), (2, ">", cap)], {1, 2},
                                         [("direct", [1]), ("direct", [2])], None)
    rows["half_negative"] = Row([NEG_POS_PAIRS] * n, [(1, "==", 18 * n), (1, ">", cap)], {1}, [("direct", [1])], 1)
    # two thirds of the terms in bucket 1, the rest uniformly random: oversized where 19 * (2/3) n exceeds the image (the G || H
    # shapes), otherwise one bucket that takes most of the first window
    thirds = 19 * (n - (n + 2) // 3)
    rows["two_thirds_ones19"] = Row([ONES_19 if i % 3 else rnd.randrange(L) for i in range(n)],
                                    [(1, ">=", thirds), (1, ">" if thirds > cap else "<", cap), (1, ">", cap // 2)], None, None, None)
    return rows


def two_thirds_first_pass(n, cap):
    return "direct" if 19 * (n - (n + 2) // 3) > cap else "staged"


@functools.lru_cache(maxsize=None)
def filler_rows(n):
    """index -> scalars of the cheap rows of an unsplit launch (shared: not to be changed)"""
    rnd = random.Random(7000 + n)
    out = {}
    for b in range(UNSPLIT_B):
        if b in ADVERSARIAL_AT:
            continue
        if b in RANDOM_AT:
            out[b] = [rnd.randrange(L) for _ in range(n)]
        else:
            out[b] = [0] * n
            if b % 2 == 0:
                out[b][rnd.randrange(n)] = rnd.randrange(1, L)
    return out


def uniform_row(n):
    rnd = random.Random(8000 + n)
    return [rnd.randrange(L) for _ in range(n)]


SETTINGS = {
    "default": {},
    "staged_wide": {"BBP_SORT_STAGED": "7"},
    "plain": {"BBP_SORT_STAGED": "0"},
    "staged_wide_half_fold": {"BBP_SORT_STAGED": "7", "BBP_FOLD_HALF_FROM": "1"},
}
ROW_NAMES = ["all_ones19", "exact_capacity", "capacity_plus_1", "boundary_between_1_and_2", "oversized_in_the_middle", "adjacent_oversized",
             "half_negative", "two_thirds_ones19"]
# the setting whose plan gives the image capacity the rows of a shape are built for: the wide rows serve the plain settings too
CAP_SETTING = {2933: "default", 1467: "default", 4097: "staged_wide"}
SHAPE_LAYOUT = {2933: LAYOUT_G_H, 1467: LAYOUT_G, 4097: LAYOUT_G_H}

UnsplitCase = collections.namedtuple("UnsplitCase", "setting n_terms row path")


def _unsplit_cases():
    cases = []
    for n, want in ((2933, (LARGE, STAGED, LANES128)), (1467, (LARGE, STAGED, LANES128))):
        cases += [UnsplitCase("default", n, r, want) for r in ROW_NAMES if r != "adjacent_oversized" or SHAPE_LAYOUT[n] == LAYOUT_G_H]
    for setting, want in (("staged_wide", (LARGE, STAGED_WIDE, LANES128)), ("plain", (LARGE, PLAIN, LANES128)), ("default", (LARGE, PLAIN, LANES128))):
        cases += [UnsplitCase(setting, 4097, r, want) for r in ROW_NAMES]
        if setting == "staged_wide":
            cases.append(UnsplitCase(setting, 4097, "uniform", want))
    # the wide image under the half-wavefront fold: the one combination of sort and fold no other list reaches
    cases += [UnsplitCase("staged_wide_half_fold", 4097, r, (LARGE, STAGED_WIDE, HALF)) for r in ("uniform", "oversized_in_the_middle")]
    return cases


UNSPLIT_CASES = _unsplit_cases()


def case_id(c):
    return "%s-%d-%s" % (c.setting, c.n_terms, c.row)


def image_capacity(lib, n_terms):
    p = plan(lib, UNSPLIT_B, n_terms, SETTINGS[CAP_SETTING[n_terms]])
    assert p.sort_cap > 0, "the shape the bucket rows are built for takes no staged sort"
    return p.sort_cap


_rows_cache = {}


def unsplit_rows(lib, n_terms):
    """name -> Row of a shape, built once for the image capacity its staged plan states; `uniform` added for the wide shape"""
    if n_terms not in _rows_cache:
        rows = bucket_rows(n_terms, image_capacity(lib, n_terms), SHAPE_LAYOUT[n_terms])
        rows["uniform"] = Row(uniform_row(n_terms), [], None, None, None)
        _rows_cache[n_terms] = rows
    return _rows_cache[n_terms]


# ---- split launches: what the split tests lack ---------------------------------------------------------------------------------
SPLIT_SHAPE = (LAYOUT_G_H, 2933, 3)
SPLIT_ONE_SUB = 5  # the sub-MSM that holds every non-zero term of the second row


def width9_limit_scalar(i):
    """the width-9 recoding's limits (digit magnitudes 255 and 1 around a carry) at every bit offset, long carry chains, the ends of
    the scalar range"""
    kind, s = i % 7, (i * 5) % 241
    if kind == 0:
        return 0xFF << s
    if kind == 1:
        return 0x101 << s
    if kind == 2:
        return 0x1FF << s
    if kind == 3:
        return ((1 << (2 + i % 250)) - 1) % L  # run of ones
    if kind == 4:
        return L - 1 - (i % 3)
    if kind == 5:
        return 1 << 252
    return (0xFF << s | 0x101 << ((s + 100) % 241)) % L


def split_rows(n_terms, n_sub):
    rnd = random.Random(6000 + n_terms)
    one_sub = [0] * n_terms
    for i in range(SPLIT_ONE_SUB * n_sub, min((SPLIT_ONE_SUB + 1) * n_sub, n_terms)):
        one_sub[i] = rnd.randrange(1, L)
    return collections.OrderedDict([("all_zero", [0] * n_terms), ("one_sub_msm", one_sub),
                                    ("width9_limits", [width9_limit_scalar(i) for i in range(n_terms)])])


# ---- the lists of tests/test_gpu_fuzz.py ---------------------------------------------------------------------------------------
def pattern_scalar(rnd):
    k = rnd.randrange(12)
    if k == 0:
        return 0
    if k == 1:
        return 1
    if k == 2:
        return L - 1 - rnd.randrange(3)
    if k == 3:
        return 1 << rnd.randrange(252)
    if k == 4:
        return ((1 << rnd.randrange(2, 252)) - 1) % L            # run of ones: one long carry chain in the NAF
    if k == 5:
        return int("10" * 126, 2) >> rnd.randrange(8)             # alternating bits
    if k == 6:
        return (0x7FF << rnd.randrange(0, 240)) % L               # a digit at the NAF magnitude limit
    if k == 7:
        return (0x801 << rnd.randrange(0, 240)) % L
    if k == 8:
        return rnd.getrandbits(rnd.randrange(1, 64))              # small values (witness-like)
    return rnd.randrange(L)


FUZZ_SEEDS = [1, 2, 3]


def fuzz_cases(seed):
    """test_msm_fuzz: (case, layout, n_terms, B, rows) -- fourteen random shapes per seed"""
    rnd = random.Random(1000 + seed)
    for case in range(14):
        layout = rnd.choice([LAYOUT_G_H, LAYOUT_G])
        m = rnd.choice([1, 2, 3, 17, 63, 64, 65, 127, 128, 129, 300, 1023, 1466, 2048]) if case % 2 else rnd.randrange(1, 2049)
        n_terms = 1 + (2 * m if layout == LAYOUT_G_H else m)
        B = rnd.choice([1, 2, 3, 5, 31, 64, 127, 128, 129, 200]) if n_terms < 700 else rnd.choice([1, 2, 3, 5, 9])
        repeated = pattern_scalar(rnd)
        rows = []
        for b in range(B):
            style = rnd.randrange(4)
            if style == 0:
                row = [pattern_scalar(rnd) for _ in range(n_terms)]
            elif style == 1:
                row = [repeated] * n_terms                           # every term in one bucket
            elif style == 2:
                row = [0] * n_terms                                  # empty MSM -> identity
                row[rnd.randrange(n_terms)] = pattern_scalar(rnd)
            else:
                row = [rnd.randrange(L) for _ in range(n_terms)]
            rows.append(row)
        yield case, layout, n_terms, B, rows


HALF_FOLD_KNOBS = {"BBP_FOLD_HALF_FROM": "1"}
# test_msm_fuzz_half_wavefront_fold: (layout, n_terms, B, fold the launch takes).  Split launches fold with k_msm_fold<2> whatever the
# knob says; the last shape is the unsplit full-width one (its rows are mostly cheap: the oracle's share)
HALF_FOLD_SHAPES = [(LAYOUT_G_H, 1, 1, HALF), (LAYOUT_G_H, 3, 3, HALF), (LAYOUT_G, 34, 5, HALF), (LAYOUT_G_H, 129, 127, HALF),
                    (LAYOUT_G_H, 257, 200, HALF), (LAYOUT_G, 1467, 9, SMALL_FOLD), (LAYOUT_G_H, 2933, 3, SMALL_FOLD), (LAYOUT_G_H, 4097, 2, SMALL_FOLD),
                    (LAYOUT_G_H, 2049, 65, SMALL_FOLD), (LAYOUT_G_H, 4097, 128, HALF)]


def half_fold_cases():
    rnd = random.Random(77)
    for layout, n_terms, B, _ in HALF_FOLD_SHAPES:
        repeated = pattern_scalar(rnd)
        rows = []
        for b in range(B):
            style = (b + n_terms) % 4
            if B * n_terms > 200000 and b % 16 >= 4:
                style = 2 + 2 * (b % 2)  # the large unsplit launch: a dozen dense rows, the others one term or none
            if style == 0:
                row = [pattern_scalar(rnd) for _ in range(n_terms)]
            elif style == 1:
                row = [repeated] * n_terms
            elif style == 2:
                row = [0] * n_terms
                row[rnd.randrange(n_terms)] = pattern_scalar(rnd)
            elif style == 3:
                row = [rnd.randrange(L) for _ in range(n_terms)]
            else:
                row = [0] * n_terms
            rows.append(row)
        yield layout, n_terms, B, rows


OVERSIZED_SPLIT_SHAPES = ((2933, 3), (2049, 4), (4097, 2))  # test_msm_sort_oversized_bucket: (n_terms, B), layout G || H, all split


def oversized_split_cases():
    rnd = random.Random(5)
    for n_terms, B in OVERSIZED_SPLIT_SHAPES:
        rows = []
        for b in range(B):
            if b % 2 == 0:
                rows.append([ONES_19] * n_terms)
            else:
                rows.append([ONES_19 if i % 3 else rnd.randrange(L) for i in range(n_terms)])
        yield n_terms, B, rows
