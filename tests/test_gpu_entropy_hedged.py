"""GPU tier: hedged on-device entropy (include/bbp.h "Hedged on-device entropy": BBP_ENTROPY_SOURCE_HEDGED, bbp_draw_entropy_hedged_dev).
A prove row's ChaCha20 key is SHA3-256 over the call key and the row's own inputs, on the device.  Drawn rows are the restatement's
bytes (tests/hedge_ref.py: hashlib.sha3_256 + the ChaCha20 block function); host-pointer calls under a known key return the records
of an explicit-entropy call with the restatement's rows (and the C oracle's); a call key used twice repeats a row's entropy only where
the whole row repeats; chunked calls, round calls, checked proving, the device pipeline, a pool and the server follow."""
import hashlib
import os
import signal
import subprocess
import tempfile
import time

import pytest

from tests import entropy_ref as er
from tests import hedge_ref as hr
from tests import oracle_c
from tests import prove_round_cases as rc
from tests import uds_client as uc
from tests.test_gpu_prove_verify import _synth_batch

pytestmark = pytest.mark.gpu
OK, VERIFY = 0, 1
KEY = bytes((0xA7 ^ (29 * i)) & 0xFF for i in range(32))


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def hctx(ctx, bbp):
    """A context of this module's own (the source is switched here; after `ctx`, so torch's HIP runtime is initialised first)."""
    c = bbp.Context(0)
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


@pytest.fixture
def hedged(hctx):
    hctx.set_entropy_source("hedged")
    yield hctx
    hctx.set_entropy_source("os")


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy().tobytes())


def _vin(out, vins, N, rows):
    rs_ = 1121 + 32 * (4 + N)
    return b"".join(out[i * rs_:(i + 1) * rs_] + b"".join(vins[i][:3]) + vins[i][3] for i in rows)


def _commitments(rec, N):
    return [rec[1121 + 32 * k:1121 + 32 * (k + 1)] for k in range(4 + N)]


def _random_rows(B, N, tag):
    n = B * hr.in_bytes(N)
    return b"".join(hashlib.sha512(b"hedge-rows" + bytes([tag]) + i.to_bytes(4, "little")).digest() for i in range((n + 63) // 64))[:n]


def test_describe_reports_the_source(hedged):
    assert "entropy source: hedged" in hedged.describe()


@pytest.mark.parametrize("B,N", [(3, 1), (65, 4), (3, 8), (3, 202)])
def test_device_draw_is_the_restatement(hctx, bbp, B, N):
    """65 rows cross a wavefront of row keys, 3 x 207 slots one of slots; N = 1 / 4 / 8 / 202 end the sponge at every kind of position."""
    import torch
    es = bbp.entropy_size(N)
    rows = _random_rows(B, N, N & 0xFF)
    d_in = _dev(rows)
    d = torch.zeros(B * es + 64, dtype=torch.uint8, device="cuda")
    d[B * es:] = 0xAB  # guard bytes behind the rows stay untouched
    torch.cuda.synchronize()
    hctx.draw_entropy_hedged_dev(B, N, d_in.data_ptr(), d.data_ptr(), key=KEY)
    torch.cuda.synchronize()
    got = _host(d)
    assert got[:B * es] == hr.expand_prove(KEY, N, rows)
    assert got[B * es:] == b"\xab" * 64
    assert _host(d_in) == rows
    # key = NULL: 32 fresh OS bytes per call -- two calls differ
    e = torch.zeros(B * es, dtype=torch.uint8, device="cuda")
    hctx.draw_entropy_hedged_dev(B, N, d_in.data_ptr(), d.data_ptr())
    hctx.draw_entropy_hedged_dev(B, N, d_in.data_ptr(), e.data_ptr())
    torch.cuda.synchronize()
    a, b = _host(d)[:B * es], _host(e)
    assert a != b and got[B * es:] == _host(d)[B * es:]
    for r in (a, b):
        for i in range(B):
            for k in range(4 + N):
                assert int.from_bytes(r[i * es + 32 * k:i * es + 32 * k + 32], "little") < er.L, (i, k)


def test_device_draw_reads_rows_that_are_only_4_byte_aligned(hctx, bbp):
    """The other load shape: rows at an address that is 4 mod 8 are read with 32-bit loads and give the same bytes."""
    import torch
    B, N = 3, 8
    rows = _random_rows(B, N, 77)
    buf = torch.zeros(len(rows) + 8, dtype=torch.uint8, device="cuda")
    buf[4:4 + len(rows)] = _dev(rows)
    d = torch.zeros(B * bbp.entropy_size(N), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert (buf.data_ptr() + 4) % 8 == 4
    hctx.draw_entropy_hedged_dev(B, N, buf.data_ptr() + 4, d.data_ptr(), key=KEY)
    torch.cuda.synchronize()
    assert _host(d) == hr.expand_prove(KEY, N, rows)


def test_device_draw_refuses_bad_arguments(hctx, bbp):
    import torch
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for B, N, i, o in ((1, 0, d.data_ptr(), d.data_ptr() + 2048), (1, 203, d.data_ptr(), d.data_ptr() + 2048),
                       (1, 8, None, d.data_ptr()), (1, 8, d.data_ptr(), None)):
        with pytest.raises(bbp.BbpError):
            hctx.draw_entropy_hedged_dev(B, N, i, o, key=KEY)
    pool = bbp.Pool([0])
    try:
        with pytest.raises(bbp.BbpError):
            pool.draw_entropy_hedged_dev(1, 8, d.data_ptr(), d.data_ptr() + 2048, key=KEY)
    finally:
        pool.close()
    with pytest.raises(bbp.BbpError):
        hctx.set_entropy_source(3)


@pytest.mark.parametrize("N,B", [(4, 3), (8, 3), (202, 2)])
def test_host_path_with_a_known_key_is_the_explicit_entropy_call(hedged, oc, bbp, N, B):
    ins, _, vins = _synth_batch(hedged, B, N, seed=8080 + N)
    ent = hr.expand_prove(KEY, N, ins)
    hedged.debug_next_entropy_key(KEY)
    out, st = hedged.prove_batch(B, N, b"".join(ins))
    assert st == [OK] * B
    ref, rst = hedged.prove_batch(B, N, b"".join(ins), ent)
    assert rst == [OK] * B and out == ref
    cout, cst = oc.prove_many(b"".join(ins), ent, B, N, threads=4)
    assert cst == [OK] * B and out == cout
    assert hedged.verify_batch(B, N, _vin(out, vins, N, range(B))) == [OK] * B
    assert oc.verify_many(_vin(out, vins, N, range(B)), B, N, threads=4) == [OK] * B
    # the key was consumed: the next call draws a fresh one
    again, _ = hedged.prove_batch(B, N, b"".join(ins))
    rs_ = bbp.record_size(N)
    assert again[:rs_] != out[:rs_]


def test_prove_round_is_prove_batch_on_the_expanded_rows(hedged, bbp):
    N, B = 8, 3
    r = rc.honest(N, B, tag=6)
    hedged.debug_next_entropy_key(KEY)
    rows, toggles, st = hedged.prove_round(N, r.table, r.bid_bytes, None)
    assert st == [OK] * B and toggles == r.toggles
    hedged.debug_next_entropy_key(KEY)
    pout, pst = hedged.prove_batch(B, N, r.in_rows())
    assert pst == [OK] * B and rows == r.rows(pout)
    ref, _ = hedged.prove_batch(B, N, r.in_rows(), hr.expand_prove(KEY, N, r.in_rows()))
    assert pout == ref


def test_a_repeated_key_repeats_entropy_only_where_the_row_repeats(hctx, bbp):
    """What the source is for.  Two calls under the same key differ in row 1's bid d (and what follows from it: x, y, y_inv, q and the
    list entry at the toggle).  Rows 0 and 2 return identical records; row 1 shares no entropy slot and no commitment between the
    calls, where under source DEVICE it shares every slot."""
    N, B = 8, 3
    ins, _, vins = _synth_batch(hctx, B, N, seed=9393)
    row = ins[1]
    d2 = (int.from_bytes(row[:8], "little") ^ 1).to_bytes(8, "little") + bytes(24)
    k, seed, toggle = row[32:64], row[192:224], 1 % N
    m, x, y, yi, q, z = (hctx.witness_batch(d2 + k + seed)[32 * j:32 * j + 32] for j in range(6))
    pub = bytearray(row[224:224 + 32 * N])
    pub[32 * toggle:32 * toggle + 32] = x
    row2 = d2 + k + y + yi + q + z + seed + bytes(pub) + row[-8:]
    assert z == row[160:192] and row2 != row and len(row2) == len(row)
    ins2, vins2 = [ins[0], row2, ins[2]], [vins[0], (q, z, seed, bytes(pub)), vins[2]]
    outs = []
    hctx.set_entropy_source("hedged")
    try:
        for rows_ in (ins, ins2):
            hctx.debug_next_entropy_key(KEY)
            out, st = hctx.prove_batch(B, N, b"".join(rows_))
            assert st == [OK] * B
            outs.append(out)
    finally:
        hctx.set_entropy_source("os")
    rs_ = bbp.record_size(N)
    a, b = ([o[i * rs_:(i + 1) * rs_] for i in range(B)] for o in outs)
    assert a[0] == b[0] and a[2] == b[2]
    assert not any(ca == cb for ca, cb in zip(_commitments(a[1], N), _commitments(b[1], N)))
    assert hctx.verify_batch(B, N, _vin(outs[0], vins, N, range(B))) == [OK] * B
    assert hctx.verify_batch(B, N, _vin(outs[1], vins2, N, range(B))) == [OK] * B
    e1, e2 = hr.prove_row(KEY, N, 1, row), hr.prove_row(KEY, N, 1, row2)
    assert not any(e1[32 * s:32 * s + 32] == e2[32 * s:32 * s + 32] for s in range(5 + N))
    assert outs[0] == hctx.prove_batch(B, N, b"".join(ins), hr.expand_prove(KEY, N, ins))[0]
    assert outs[1] == hctx.prove_batch(B, N, b"".join(ins2), hr.expand_prove(KEY, N, ins2))[0]
    # source DEVICE: the row's entropy does not depend on the row -- every slot is shared
    assert er.prove_row(KEY, N, 1) == er.expand_prove(KEY, N, B)[bbp.entropy_size(N):2 * bbp.entropy_size(N)]


def test_host_batches_cut_into_chunks_equal_the_unchunked_call(hedged, bbp, monkeypatch):
    """BBP_HOST_CHUNK_PROVE=2: a 5-proof call goes out as three engine calls; each hedges and draws its own rows under the call's key
    and the rows' indices in the call."""
    N, B = 8, 5
    ins, _, _ = _synth_batch(hedged, B, N, seed=4343)
    hedged.debug_next_entropy_key(KEY)
    whole, st = hedged.prove_batch(B, N, b"".join(ins))
    assert st == [OK] * B
    monkeypatch.setenv("BBP_HOST_CHUNK_PROVE", "2")
    hedged.debug_next_entropy_key(KEY)
    cut, st = hedged.prove_batch(B, N, b"".join(ins))
    monkeypatch.delenv("BBP_HOST_CHUNK_PROVE")
    assert st == [OK] * B and cut == whole
    assert whole == hedged.prove_batch(B, N, b"".join(ins), hr.expand_prove(KEY, N, ins))[0]


@pytest.mark.parametrize("form", ["rows", "round"])
def test_checked_reprove_uses_the_row_it_had(hedged, bbp, form):
    """A record that fails its check is proved again under its own entropy row: a rows call re-derives the row key on the host, a round
    call fetches it from the device.  The output is the unchecked call's under the same key."""
    N, B = 8, 3
    r = rc.honest(N, B, tag=7)

    def call():
        hedged.debug_next_entropy_key(KEY)
        if form == "rows":
            out, st = hedged.prove_batch(B, N, r.in_rows())
        else:
            out, _, st = hedged.prove_round(N, r.table, r.bid_bytes, None)
        return out, st
    ref, st = call()
    assert st == [OK] * B
    hedged.set_prove_check(True)
    try:
        n0 = hedged.prove_check_stats()
        hedged.debug_corrupt_next_proof(1)
        out, st = call()
        n1 = hedged.prove_check_stats()
    finally:
        hedged.set_prove_check(False)
    assert st == [OK] * B and out == ref
    assert n1[2] - n0[2] == 1
    assert hedged.health() == 0


def test_device_pipeline_orders_itself(hctx, bbp):
    """bbp_prepare_bids_dev, the hedged draw and bbp_prove_batch_dev on three streams, no ordering added by the caller: the draw waits
    for the prepare (it reads the rows), the prover for both.  The records are the host path's under the same key."""
    import torch
    N, B = 8, 3
    ins, _, _ = _synth_batch(hctx, B, N, seed=3131)
    bids = b"".join(r[:64] + r[192:224] for r in ins)
    lists = bytearray(b"".join(r[224:224 + 32 * N] for r in ins))
    toggles = [int.from_bytes(r[-8:], "little") for r in ins]
    for i, t in enumerate(toggles):
        lists[32 * (N * i + t):32 * (N * i + t + 1)] = b"\xee" * 32
    d_bids, d_lists = _dev(bids), _dev(lists)
    d_tog = torch.tensor(toggles, dtype=torch.int64, device="cuda")
    d_in = torch.zeros(B * hr.in_bytes(N), dtype=torch.uint8, device="cuda")
    d_ent = torch.zeros(B * bbp.entropy_size(N), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(B * bbp.record_size(N), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hctx.prepare_bids_dev(B, N, d_bids.data_ptr(), d_lists.data_ptr(), d_tog.data_ptr(), d_in.data_ptr(), None, stream=hctx.copy_stream)
    hctx.draw_entropy_hedged_dev(B, N, d_in.data_ptr(), d_ent.data_ptr(), key=KEY, stream=hctx.verify_stream(1))
    hctx.prove_batch_dev(B, N, d_in.data_ptr(), d_ent.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    assert _host(d_in) == b"".join(ins)
    assert _host(d_ent) == hr.expand_prove(KEY, N, ins)
    hctx.set_entropy_source("hedged")
    try:
        hctx.debug_next_entropy_key(KEY)
        ref, st = hctx.prove_batch(B, N, b"".join(ins))
    finally:
        hctx.set_entropy_source("os")
    assert st == [OK] * B and _host(d_out) == ref


def test_verify_statuses_do_not_depend_on_the_source(hctx, bbp):
    N, B = 8, 6
    ins, ents, vins = _synth_batch(hctx, B, N, seed=3838)
    out, _ = hctx.prove_batch(B, N, b"".join(ins), b"".join(ents))
    rs_ = bbp.record_size(N)
    stride = rs_ + 96 + 32 * N
    blob = bytearray(_vin(out, vins, N, range(B)))
    blob[1 * stride + 300] ^= 0x08   # a flipped proof byte
    blob[4 * stride + rs_] ^= 0x01   # a wrong score (still canonical)
    res = {}
    for src in ("os", "hedged"):
        hctx.set_entropy_source(src)
        try:
            res[src] = (hctx.verify_batch(B, N, bytes(blob)), hctx.verify_batch_aggregated(B, N, bytes(blob))[0])
        finally:
            hctx.set_entropy_source("os")
    assert res["hedged"] == res["os"]
    exp = [OK, VERIFY, OK, OK, VERIFY, OK]
    assert res["os"] == (exp, exp)


def test_pool_takes_the_source(hctx, bbp):
    N, B = 8, 3
    ins, _, vins = _synth_batch(hctx, B, N, seed=5151)
    pool = bbp.Pool([0])
    try:
        pool.set_entropy_source("hedged")
        assert "entropy source: hedged" in pool.member(0).describe()
        out, st = pool.prove_batch(B, N, b"".join(ins))
        assert st == [OK] * B
        assert pool.verify_batch(B, N, _vin(out, vins, N, range(B))) == [OK] * B
        pool.set_entropy_source("os")
    finally:
        pool.close()
    seen = [c for i in range(B) for c in _commitments(out[i * bbp.record_size(N):(i + 1) * bbp.record_size(N)], N)]
    assert len(set(seen)) == len(seen)


def test_server_entropy_hedged(ctx, built, bbp):
    built.build_server()
    N, K = 8, 4
    ins, _, vins = _synth_batch(ctx, K, N, seed=5454)
    d = tempfile.mkdtemp(prefix="bbp-uds-hedge-")
    path = os.path.join(d, "sock")
    log = open(os.path.join(d, "log"), "w+")
    p = subprocess.Popen([built.SERVER_BIN, "-b", path, "-l", "info", "--engine", bbp.lib_path, "--device", "0", "--window-us", "200",
                          "--entropy", "hedged"], stderr=log)
    try:
        for _ in range(1500):
            if os.path.exists(path) or p.poll() is not None:
                break
            time.sleep(0.02)
        assert os.path.exists(path), open(log.name).read()[-800:]
        blobs = [uc.prove(path, ins[j][:224], ins[j][224:224 + 32 * N], int.from_bytes(ins[j][-8:], "little")) for j in range(K)]
        for j in range(K):
            assert uc.verify(path, blobs[j], *vins[j]) == b"\x01"
        assert "entropy source: hedged" in open(log.name).read()
    finally:
        if p.poll() is None:
            p.send_signal(signal.SIGTERM)
            p.wait(timeout=30)
