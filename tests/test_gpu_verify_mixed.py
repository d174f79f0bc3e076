"""Mixed-N verification on the device (include/bbp.h bbp_verify_batch_mixed*): one call verifies rows of any mix of bid-list
lengths, and every row's status is what bbp_verify_batch reports for it with its own N.

Anchors: the C oracle's verdicts (oracle/c, proving and verifying on the CPU under fixed entropy) and the per-N uniform calls
on the same rows.  Tampered rows cover the transcript (t_x + 1), every public input (score, seed, one pub_list entry), the
serde screening of the public scalars (score + l, a FormatError in the reference and in both oracles) and the structural parse
(version byte)."""
import hashlib
import random

import pytest

from oracle.ref_py import ristretto as rs
from tests import oracle_c

pytestmark = pytest.mark.gpu
OK, VERIFY, GENS_LEN, FORMAT, BAD_ARG = 0, 1, 2, 3, 4
L = 2 ** 252 + 27742317777372353535851937790883648493
KINDS = ("tx", "score", "seed", "pub", "noncanon", "parse")


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


def _synth(oc, B, N, seed):
    """Prove inputs, fixed entropy and verify tails for B bids at list length N (witness from the C oracle, CPU)."""
    def stream(i, tag):
        return hashlib.sha512(b"bbp-mixed-v1" + seed.to_bytes(8, "little") + i.to_bytes(8, "little") + tag).digest()
    sd = rs.sc_bytes(rs.sc_wide(stream(0, b"seed")))
    ins, ents, tails = [], [], []
    for i in range(B):
        d, k = stream(i, b"d")[:8] + bytes(24), rs.sc_bytes(rs.sc_wide(stream(i, b"k")))
        m, x, y, yi, q, z = (lambda w: [w[32 * j:32 * j + 32] for j in range(6)])(oc.witness(d + k + sd))
        toggle = i % N
        pub = [rs.sc_bytes(rs.sc_wide(stream(i, b"pub%d" % j))) for j in range(N)]
        pub[toggle] = x
        ins.append(d + k + y + yi + q + z + sd + b"".join(pub) + toggle.to_bytes(8, "little"))
        ents.append(b"".join(rs.sc_bytes(rs.sc_wide(stream(i, b"ent%d" % j))) for j in range(4 + N)) + stream(i, b"entseed")[:32])
        tails.append(q + z + sd + b"".join(pub))
    return ins, ents, tails


def _tamper(row, N, kind):
    rs_ = 1121 + 32 * (4 + N)
    b = bytearray(row)
    if kind == "tx":        # t_x: after the version byte, A_I1 A_O1 S1 and T_1 T_3..T_6
        b[257:289] = ((int.from_bytes(b[257:289], "little") + 1) % L).to_bytes(32, "little")
    elif kind == "score":
        b[rs_] ^= 0x01
    elif kind == "seed":
        b[rs_ + 64] ^= 0x01
    elif kind == "pub":     # the LAST pub_list entry: a row-stride mistake would read past it into the next row
        b[rs_ + 96 + 32 * (N - 1)] ^= 0x01
    elif kind == "noncanon":
        b[rs_:rs_ + 32] = (int.from_bytes(b[rs_:rs_ + 32], "little") + L).to_bytes(32, "little")
    elif kind == "parse":   # version byte 1 on a compact-length record: FormatError
        b[0] ^= 0x01
    return bytes(b)


def _uniform(ctx, Ns, blob, bbp):
    """What bbp_verify_batch says for every row, one call per distinct N (what a caller does today)."""
    off = bbp.mixed_row_offsets(Ns)
    out = [None] * len(Ns)
    for n in sorted(set(Ns)):
        idx = [i for i, v in enumerate(Ns) if v == n]
        st = ctx.verify_batch(len(idx), n, b"".join(blob[off[i]:off[i + 1]] for i in idx))
        for i, s in zip(idx, st):
            out[i] = s
    return out


def _expected_fallback(Ns, st, G, tampered_verify):
    """Members of failing groups that reach the group check (FORMAT rows are rejected before it), groups cut by index."""
    if G <= 1:
        return 0
    total = 0
    for g0 in range(0, len(Ns), G):
        members = range(g0, min(len(Ns), g0 + G))
        if any(i in tampered_verify for i in members):
            total += sum(1 for i in members if st[i] != FORMAT)
    return total


@pytest.fixture(scope="module")
def anchor(oc, bbp):
    """Two oracle-proved rows at each N in {1, 5, 8, 40, 202} plus one tampered copy of each kind, shuffled."""
    rows, ns, oracle = [], [], []
    for n in (1, 5, 8, 40, 202):
        ins, ents, tails = _synth(oc, 2, n, seed=1000 + n)
        out, st = oc.prove_many(b"".join(ins), b"".join(ents), 2, n, threads=8)
        assert st == [0, 0]
        rs_ = bbp.record_size(n)
        good = [out[i * rs_:(i + 1) * rs_] + tails[i] for i in range(2)]
        bad = [_tamper(good[k % 2], n, kind) for k, kind in enumerate(KINDS)]
        group = good + bad
        verdicts = oc.verify_many(b"".join(group), len(group), n, threads=8)
        assert verdicts[2 + KINDS.index("noncanon")] == FORMAT  # serde screening (see the module doc)
        rows += group
        ns += [n] * len(group)
        oracle += verdicts
    order = list(range(len(rows)))
    random.Random(77).shuffle(order)
    Ns = [ns[i] for i in order]
    return Ns, b"".join(rows[i] for i in order), [oracle[i] for i in order]


@pytest.fixture(scope="module")
def scale(ctx, oc, bbp):
    """B = 1024, N uniform in 1..202 under a fixed seed, records from the engine's prove_batch under fixed entropy, 1 % tampered."""
    rnd = random.Random(4242)
    B = 1024
    Ns = [rnd.randint(1, 202) for _ in range(B)]
    rows = [None] * B
    for n in sorted(set(Ns)):
        idx = [i for i, v in enumerate(Ns) if v == n]
        ins, ents, tails = _synth(oc, len(idx), n, seed=n)
        out, st = ctx.prove_batch(len(idx), n, b"".join(ins), b"".join(ents))
        assert st == [0] * len(idx)
        rs_ = bbp.record_size(n)
        for j, i in enumerate(idx):
            rows[i] = out[j * rs_:(j + 1) * rs_] + tails[j]
    bad = rnd.sample(range(B), B // 100)
    kinds = {}
    for k, i in enumerate(bad):
        kinds[i] = KINDS[k % len(KINDS)]
        rows[i] = _tamper(rows[i], Ns[i], kinds[i])
    return Ns, b"".join(rows), kinds


def test_oracle_anchor(ctx, anchor, bbp):
    Ns, blob, oracle = anchor
    st = ctx.verify_batch_mixed(Ns, blob)
    assert st == oracle
    assert st == _uniform(ctx, Ns, blob, bbp)
    assert st.count(OK) == 10 and st.count(FORMAT) == 10 and st.count(VERIFY) == 20


def test_scale_random_n(ctx, scale, oc, bbp):
    Ns, blob, kinds = scale
    st = ctx.verify_batch_mixed(Ns, blob)
    uni = _uniform(ctx, Ns, blob, bbp)
    assert st == uni
    for i in range(len(Ns)):
        exp = OK if i not in kinds else FORMAT if kinds[i] in ("noncanon", "parse") else VERIFY
        assert st[i] == exp, (i, Ns[i], kinds.get(i))
    off = bbp.mixed_row_offsets(Ns)
    rnd = random.Random(9)
    sample = sorted(set(rnd.sample(range(len(Ns)), 28)) | set(list(kinds)[:4]))
    for i in sample:
        assert oc.verify_many(blob[off[i]:off[i + 1]], 1, Ns[i], threads=8) == [st[i]], i


def test_neighbour_isolation(ctx, oc, bbp):
    ins1, ents1, tails1 = _synth(oc, 4, 1, seed=31)
    out1, st1 = ctx.prove_batch(4, 1, b"".join(ins1), b"".join(ents1))
    ins2, ents2, tails2 = _synth(oc, 1, 202, seed=32)
    out2, st2 = ctx.prove_batch(1, 202, b"".join(ins2), b"".join(ents2))
    assert st1 == [OK] * 4 and st2 == [OK]
    r1 = [out1[i * bbp.record_size(1):(i + 1) * bbp.record_size(1)] + tails1[i] for i in range(4)]
    big = out2 + tails2[0]
    Ns = [1, 1, 202, 1, 1]
    good = b"".join([r1[0], r1[1], big, r1[2], r1[3]])
    assert ctx.verify_batch_mixed(Ns, good) == [OK] * 5
    blob = b"".join([r1[0], r1[1], _tamper(big, 202, "pub"), r1[2], r1[3]])
    assert ctx.verify_batch_mixed(Ns, blob) == [OK, OK, VERIFY, OK, OK]
    assert ctx.verify_batch_mixed_aggregated(Ns, blob, 2)[0] == [OK, OK, VERIFY, OK, OK]
    # and a short row tampered at its end between long ones
    Ns2 = [202, 1, 202]
    blob2 = b"".join([big, _tamper(r1[0], 1, "pub"), big])
    assert ctx.verify_batch_mixed(Ns2, blob2) == [OK, VERIFY, OK]


def test_single_n_is_the_uniform_call(ctx, oc, bbp):
    B, N = 256, 8
    ins, ents, tails = _synth(oc, B, N, seed=88)
    out, st = ctx.prove_batch(B, N, b"".join(ins), b"".join(ents))
    assert st == [OK] * B
    rs_ = bbp.record_size(N)
    rows = [out[i * rs_:(i + 1) * rs_] + tails[i] for i in range(B)]
    for k, i in enumerate((3, 50, 51, 130, 200, 255)):
        rows[i] = _tamper(rows[i], N, KINDS[k])
    blob = b"".join(rows)
    assert ctx.verify_batch_mixed([N] * B, blob) == ctx.verify_batch(B, N, blob)
    assert ctx.verify_batch_mixed_aggregated([N] * B, blob) == ctx.verify_batch_aggregated(B, N, blob)


@pytest.mark.parametrize("G", [1, 7, 32, 1024])
def test_aggregated_groups_span_n(ctx, scale, G):
    Ns, blob, kinds = scale
    plain = ctx.verify_batch_mixed(Ns, blob)
    st, nfb = ctx.verify_batch_mixed_aggregated(Ns, blob, G)
    assert st == plain
    assert len(set(Ns[:G])) > 1 or G == 1  # groups hold different N
    assert nfb == _expected_fallback(Ns, st, G, {i for i, k in kinds.items() if k not in ("noncanon", "parse")})


def test_dev_forms(ctx, anchor, scale, bbp):
    import torch
    dev = torch.device("cuda")

    def put(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    Ns, blob, oracle = anchor
    sNs, sblob, _ = scale
    expect_s = ctx.verify_batch_mixed(sNs, sblob)
    d_in, d_sin = put(blob), put(sblob)
    d_ent = torch.randint(0, 256, (32 * len(sNs),), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    st = torch.full((len(Ns),), -7, dtype=torch.int32, device=dev)
    ctx.verify_batch_mixed_dev(Ns, d_in.data_ptr(), d_ent.data_ptr(), st.data_ptr())  # BBP_STREAM_CONTEXT
    torch.cuda.synchronize()
    assert st.cpu().tolist() == oracle

    # two verifier lanes back to back with different N sets, and several calls queued on one lane (staging of their Ns)
    a = torch.full((len(Ns),), -7, dtype=torch.int32, device=dev)
    b = torch.full((len(sNs),), -7, dtype=torch.int32, device=dev)
    c = torch.full((len(Ns),), -7, dtype=torch.int32, device=dev)
    e = torch.full((len(sNs),), -7, dtype=torch.int32, device=dev)
    ctx.verify_batch_mixed_dev(Ns, d_in.data_ptr(), d_ent.data_ptr(), a.data_ptr(), stream=ctx.verify_stream(0))
    ctx.verify_batch_mixed_dev(sNs, d_sin.data_ptr(), d_ent.data_ptr(), b.data_ptr(), stream=ctx.verify_stream(1))
    ctx.verify_batch_mixed_dev(Ns, d_in.data_ptr(), d_ent.data_ptr(), c.data_ptr(), stream=ctx.verify_stream(1))
    assert ctx.verify_batch_mixed_aggregated_dev(sNs, d_sin.data_ptr(), d_ent.data_ptr(), e.data_ptr(), group=32,
                                                 stream=ctx.verify_stream(1), want_count=False) is None
    torch.cuda.synchronize()
    assert a.cpu().tolist() == oracle and c.cpu().tolist() == oracle
    assert b.cpu().tolist() == expect_s and e.cpu().tolist() == expect_s

    # a caller's stream
    s = torch.cuda.Stream()
    f = torch.full((len(sNs),), -7, dtype=torch.int32, device=dev)
    g = torch.full((len(Ns),), -7, dtype=torch.int32, device=dev)
    ctx.verify_batch_mixed_dev(sNs, d_sin.data_ptr(), d_ent.data_ptr(), f.data_ptr(), stream=s.cuda_stream)
    nfb = ctx.verify_batch_mixed_aggregated_dev(Ns, d_in.data_ptr(), d_ent.data_ptr(), g.data_ptr(), group=7, stream=s.cuda_stream)
    s.synchronize()
    assert f.cpu().tolist() == expect_s and g.cpu().tolist() == oracle
    assert nfb > 0


def test_argument_screening(ctx, bbp, anchor):
    import ctypes
    import torch
    Ns, blob, _ = anchor
    B = len(Ns)
    d_in = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_ent = torch.zeros(32 * B, dtype=torch.uint8, device="cuda")
    d_st = torch.full((B,), 55, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for bad_n, rc in ((0, BAD_ARG), (203, GENS_LEN)):
        ns = list(Ns)
        ns[B // 2] = bad_n
        arr = (ctypes.c_uint32 * B)(*ns)
        st = (ctypes.c_int32 * B)(*([55] * B))
        nfb = ctypes.c_uint32(9)
        buf = (ctypes.c_uint8 * len(blob)).from_buffer_copy(blob)
        assert bbp.lib.bbp_verify_batch_mixed(ctx._h, B, arr, buf, st) == rc
        assert list(st) == [55] * B
        assert bbp.lib.bbp_verify_batch_mixed_aggregated(ctx._h, B, arr, buf, st, 0, ctypes.byref(nfb)) == rc
        assert list(st) == [55] * B and nfb.value == 0
        assert bbp.lib.bbp_verify_batch_mixed_dev(ctx._h, B, arr, d_in.data_ptr(), d_ent.data_ptr(), d_st.data_ptr(), None) == rc
        assert bbp.lib.bbp_verify_batch_mixed_aggregated_dev(ctx._h, B, arr, d_in.data_ptr(), d_ent.data_ptr(), d_st.data_ptr(), 0,
                                                             ctypes.byref(nfb), None) == rc
        torch.cuda.synchronize()
        assert d_st.cpu().tolist() == [55] * B and nfb.value == 0
    # both at once: the 0 decides, as the uniform call with N = 0 would
    arr = (ctypes.c_uint32 * 3)(5, 203, 0)
    st = (ctypes.c_int32 * 3)()
    assert bbp.lib.bbp_verify_batch_mixed(ctx._h, 3, arr, b"\0", st) == BAD_ARG
    # B == 0 behaves as in the uniform calls
    st = (ctypes.c_int32 * 1)(55)
    assert bbp.lib.bbp_verify_batch(ctx._h, 0, 8, b"\0", st) == OK
    assert bbp.lib.bbp_verify_batch_mixed(ctx._h, 0, None, b"\0", st) == OK
    assert bbp.lib.bbp_verify_batch_mixed_aggregated(ctx._h, 0, None, b"\0", st, 0, None) == OK
    assert list(st) == [55]


@pytest.mark.parametrize("chunk", [16, 1])
def test_host_chunks_cut_a_mixed_call(ctx, anchor, monkeypatch, chunk):
    """BBP_HOST_CHUNK_VERIFY is read at every call.  The 40 shuffled rows of five list lengths in chunks of 14, 14 and 12 rows
    (40 / ceil(40 / 16)), every chunk edge between rows of different N and so at a byte offset no row stride gives; chunks of one
    row as the extreme.  The aggregated form cuts its groups per chunk: same statuses, no claim about its fallback count."""
    Ns, blob, oracle = anchor
    assert len(Ns) == 40 and Ns[13] != Ns[14] and Ns[27] != Ns[28]
    monkeypatch.setenv("BBP_HOST_CHUNK_VERIFY", str(chunk))
    assert ctx.verify_batch_mixed(Ns, blob) == oracle
    assert ctx.verify_batch_mixed_aggregated(Ns, blob, 4)[0] == oracle


def test_pool_matches_single_context(ctx, scale, anchor, bbp):
    p = bbp.Pool([0, 0])
    try:
        Ns, blob, kinds = scale
        assert p.verify_batch_mixed(Ns, blob) == ctx.verify_batch_mixed(Ns, blob)
        st, nfb = p.verify_batch_mixed_aggregated(Ns, blob, 32)
        assert st == ctx.verify_batch_mixed(Ns, blob)
        aNs, ablob, oracle = anchor
        assert p.verify_batch_mixed(aNs, ablob) == oracle
        with pytest.raises(bbp.BbpError):
            p.verify_batch_mixed_dev(aNs, 1, 1, 1)
        assert p.health() == 0
    finally:
        p.close()
