"""GPU tier: on-device entropy (include/bbp.h bbp_draw_entropy_dev, bbp_set_entropy_source, bbp_debug_next_entropy_key).  Drawn rows are
the Python restatement's bytes (tests/entropy_ref.py); host-pointer calls with source DEVICE under a known key return exactly the records
of an explicit-entropy call with that key's expansion (and the C oracle's); without a key every record verifies and no two records share
a commitment; checked proving re-proves from the same key; verification statuses do not depend on the source; the device pipeline
orders itself after a prepare and a draw on two other streams."""
import os
import signal
import subprocess
import tempfile
import threading
import time

import pytest

from tests import entropy_ref as er
from tests import oracle_c
from tests import uds_client as uc
from tests.test_gpu_prove_verify import _synth_batch

pytestmark = pytest.mark.gpu
OK, VERIFY = 0, 1
KEY = bytes((0x5A ^ (13 * i)) & 0xFF for i in range(32))


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def ectx(ctx, bbp):
    """A context of this module's own (the source is switched here; after `ctx`, so torch's HIP runtime is initialised first)."""
    c = bbp.Context(0)
    c.fresh_report = c.describe()
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


@pytest.fixture
def device_source(ectx):
    ectx.set_entropy_source("device")
    yield ectx
    ectx.set_entropy_source("os")


def _dev_bytes(t):
    return bytes(t.cpu().numpy().tobytes())


def _commitments(rec, N):
    return [rec[1121 + 32 * k:1121 + 32 * (k + 1)] for k in range(4 + N)]


def _vin(out, vins, N, rows):
    rs_ = 1121 + 32 * (4 + N)
    return b"".join(out[i * rs_:(i + 1) * rs_] + b"".join(vins[i][:3]) + vins[i][3] for i in rows)


def test_default_source_is_os(ectx):
    assert "entropy source: os" in ectx.fresh_report


@pytest.mark.parametrize("kind,B,N", [(0, 1024, 8), (0, 130, 202), (1, 1024, 0)])
def test_draw_with_a_fixed_key_is_the_restatement(ectx, bbp, kind, B, N):
    import torch
    row = bbp.entropy_size(N) if kind == bbp.ENTROPY_PROVE else 32
    d = torch.zeros(B * row + 64, dtype=torch.uint8, device="cuda")
    d[B * row:] = 0xAB  # guard bytes behind the rows stay untouched
    torch.cuda.synchronize()
    ectx.draw_entropy_dev(B, N, kind, d.data_ptr(), key=KEY)
    torch.cuda.synchronize()
    got = _dev_bytes(d)
    want = er.expand_prove(KEY, N, B) if kind == bbp.ENTROPY_PROVE else er.expand_verify(KEY, B)
    assert got[:B * row] == want
    assert got[B * row:] == b"\xab" * 64
    # key = NULL: 32 fresh OS bytes per call -- two calls differ, blindings are canonical
    e = torch.zeros(B * row, dtype=torch.uint8, device="cuda")
    ectx.draw_entropy_dev(B, N, kind, d.data_ptr())
    ectx.draw_entropy_dev(B, N, kind, e.data_ptr())
    torch.cuda.synchronize()
    a, b = _dev_bytes(d)[:B * row], _dev_bytes(e)
    assert a != b
    if kind == bbp.ENTROPY_PROVE:
        for r in (a, b):
            for i in range(0, B, 7):
                for k in range(4 + N):
                    o = i * row + 32 * k
                    assert int.from_bytes(r[o:o + 32], "little") < er.L, (i, k)


def test_draw_refuses_bad_arguments(ectx, bbp):
    import torch
    d = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    for args in ((1, 0, 0), (1, 203, 0), (1, 8, 2)):  # N == 0 / N > 202 for prove rows, an unknown kind
        with pytest.raises(bbp.BbpError):
            ectx.draw_entropy_dev(*args, d.data_ptr(), key=KEY)
    pool = bbp.Pool([0])
    try:
        with pytest.raises(bbp.BbpError):
            pool.draw_entropy_dev(1, 8, 0, d.data_ptr(), key=KEY)
        with pytest.raises(bbp.BbpError):
            pool.debug_next_entropy_key(KEY)
    finally:
        pool.close()


@pytest.mark.parametrize("N,B", [(8, 256), (202, 128)])
def test_host_path_with_a_known_key_is_the_explicit_entropy_call(device_source, oc, bbp, N, B):
    ectx = device_source
    ins, _, vins = _synth_batch(ectx, B, N, seed=6060 + N)
    ent = er.expand_prove(KEY, N, B)
    ectx.debug_next_entropy_key(KEY)
    out, st = ectx.prove_batch(B, N, b"".join(ins))
    assert st == [OK] * B
    ref, rst = ectx.prove_batch(B, N, b"".join(ins), ent)
    assert rst == [OK] * B and out == ref
    rs_, es = bbp.record_size(N), bbp.entropy_size(N)
    rows = sorted({0, B - 1} | set(range(1, B - 1, max(1, (B - 2) // 16))))
    assert len(rows) >= 18
    cout, cst = oc.prove_many(b"".join(ins[i] for i in rows), b"".join(ent[i * es:(i + 1) * es] for i in rows), len(rows), N, threads=16)
    assert cst == [OK] * len(rows)
    for j, i in enumerate(rows):
        assert out[i * rs_:(i + 1) * rs_] == cout[j * rs_:(j + 1) * rs_], i
    assert ectx.verify_batch(B, N, _vin(out, vins, N, range(B))) == [OK] * B
    orows = range(B) if N == 8 else rows
    assert oc.verify_many(_vin(out, vins, N, orows), len(orows), N, threads=16) == [OK] * len(orows)
    # the key was consumed: the next call draws a fresh one
    again, _ = ectx.prove_batch(B, N, b"".join(ins))
    assert again[:rs_] != out[:rs_]


def test_host_batches_cut_into_chunks_draw_distinct_rows(device_source, bbp, monkeypatch):
    """BBP_HOST_CHUNK_PROVE=4: a 10-proof call goes out as three engine calls; each draws its own rows of the call's key."""
    ectx = device_source
    N, B = 2, 10
    ins, _, _ = _synth_batch(ectx, B, N, seed=4242)
    monkeypatch.setenv("BBP_HOST_CHUNK_PROVE", "4")
    ectx.debug_next_entropy_key(KEY)
    out, st = ectx.prove_batch(B, N, b"".join(ins))
    monkeypatch.delenv("BBP_HOST_CHUNK_PROVE")
    assert st == [OK] * B
    ref, _ = ectx.prove_batch(B, N, b"".join(ins), er.expand_prove(KEY, N, B))
    assert out == ref


def test_fresh_keys_never_repeat_a_commitment(device_source, bbp):
    """Source DEVICE without a key: single bbp_prove, bbp_prove_async, 32 concurrent combined callers and a two-member pool on one
    card.  Every record verifies and no two records of the test share a commitment."""
    ectx = device_source
    N, T = 8, 32
    ins, _, vins = _synth_batch(ectx, T, N, seed=7171)
    recs = [ectx.prove(ins[0][:224], ins[0][224:224 + 32 * N], 0)]
    done, ev = {}, threading.Event()

    def on_done(status, rec):
        done["r"] = (status, rec)
        ev.set()
    keep = ectx.prove_async(ins[1][:224], ins[1][224:224 + 32 * N], 1 % N, None, on_done)
    assert ev.wait(120)
    del keep
    assert done["r"][0] == OK
    recs.append(done["r"][1])
    res, errs = {}, []

    def worker(j):
        try:
            res[j] = ectx.prove(ins[j][:224], ins[j][224:224 + 32 * N], j % N)
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))
    th = [threading.Thread(target=worker, args=(j,)) for j in range(T)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not errs, errs
    recs += [res[j] for j in range(T)]
    rowof = [0, 1] + list(range(T))
    pool = bbp.Pool([0, 0])
    try:
        pool.set_entropy_source("device")
        assert all("entropy source: device" in pool.member(m).describe() for m in range(2))
        out, st = pool.prove_batch(T, N, b"".join(ins))
        assert st == [OK] * T
        rs_ = bbp.record_size(N)
        recs += [out[j * rs_:(j + 1) * rs_] for j in range(T)]
        rowof += list(range(T))
        pool.set_entropy_source("os")
    finally:
        pool.close()
    st = ectx.verify_batch(len(recs), N, b"".join(r + b"".join(vins[i][:3]) + vins[i][3] for r, i in zip(recs, rowof)))
    assert st == [OK] * len(recs)
    seen = [c for r in recs for c in _commitments(r, N)]
    assert len(set(seen)) == len(seen)


def test_checked_reprove_uses_the_same_key(device_source, bbp):
    ectx = device_source
    N, B = 8, 40
    ins, _, _ = _synth_batch(ectx, B, N, seed=9191)
    ref, _ = ectx.prove_batch(B, N, b"".join(ins), er.expand_prove(KEY, N, B))
    ectx.set_prove_check(True)
    try:
        n0 = ectx.prove_check_stats()
        ectx.debug_next_entropy_key(KEY)
        ectx.debug_corrupt_next_proof(17)
        out, st = ectx.prove_batch(B, N, b"".join(ins))
        n1 = ectx.prove_check_stats()
    finally:
        ectx.set_prove_check(False)
    assert st == [OK] * B and out == ref
    assert n1[2] - n0[2] == 1
    assert ectx.health() == 0


def test_verify_statuses_do_not_depend_on_the_source(ectx, bbp):
    N, B = 8, 96
    ins, ents, vins = _synth_batch(ectx, B, N, seed=3737)
    out, _ = ectx.prove_batch(B, N, b"".join(ins), b"".join(ents))
    rs_ = bbp.record_size(N)
    stride = rs_ + 96 + 32 * N
    blob = bytearray(_vin(out, vins, N, range(B)))
    blob[5 * stride + 300] ^= 0x08                                      # a flipped proof byte
    blob[70 * stride + rs_] ^= 0x01                                     # a wrong score (still canonical)
    res = {}
    for src in ("os", "device"):
        ectx.set_entropy_source(src)
        try:
            res[src] = (ectx.verify_batch(B, N, bytes(blob)), ectx.verify_batch_aggregated(B, N, bytes(blob))[0])
        finally:
            ectx.set_entropy_source("os")
    assert res["device"] == res["os"]
    exp = [OK] * B
    exp[5] = exp[70] = VERIFY
    assert res["os"] == (exp, exp)


def test_device_pipeline_waits_for_prepare_and_draw(ectx, oc, bbp):
    """bbp_prepare_bids_dev on the copy stream, bbp_draw_entropy_dev on a verifier lane's stream, bbp_prove_batch_dev on the context
    stream -- no host synchronisation in between: the prover waits for both by itself.  Then verify-kind rows feed
    bbp_verify_batch_dev."""
    import torch
    N, B = 8, 300
    ins, _, vins = _synth_batch(ectx, B, N, seed=2929)
    bids = b"".join(r[:64] + r[192:224] for r in ins)
    lists = bytearray(b"".join(r[224:224 + 32 * N] for r in ins))
    toggles = [int.from_bytes(r[-8:], "little") for r in ins]
    for i, t in enumerate(toggles):
        lists[32 * (N * i + t):32 * (N * i + t + 1)] = b"\xee" * 32
    in_stride, rs_, es = 224 + 32 * N + 8, bbp.record_size(N), bbp.entropy_size(N)
    d_bids = torch.frombuffer(bytearray(bids), dtype=torch.uint8).cuda()
    d_lists = torch.frombuffer(lists, dtype=torch.uint8).cuda()
    d_tog = torch.tensor(toggles, dtype=torch.int64, device="cuda")
    d_in = torch.zeros(B * in_stride, dtype=torch.uint8, device="cuda")
    d_vt = torch.zeros(B * (96 + 32 * N), dtype=torch.uint8, device="cuda")
    d_ent = torch.zeros(B * es, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(B * rs_, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ectx.prepare_bids_dev(B, N, d_bids.data_ptr(), d_lists.data_ptr(), d_tog.data_ptr(), d_in.data_ptr(), d_vt.data_ptr(),
                          stream=ectx.copy_stream)
    ectx.draw_entropy_dev(B, N, bbp.ENTROPY_PROVE, d_ent.data_ptr(), key=KEY, stream=ectx.verify_stream(1))
    ectx.prove_batch_dev(B, N, d_in.data_ptr(), d_ent.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    out = _dev_bytes(d_out)
    ref, st = ectx.prove_batch(B, N, b"".join(ins), er.expand_prove(KEY, N, B))
    assert st == [OK] * B and out == ref
    rc, exp = oc.prove(ins[B - 1][:224], ins[B - 1][224:224 + 32 * N], toggles[B - 1], er.prove_row(KEY, N, B - 1))
    assert rc == 0 and out[(B - 1) * rs_:] == exp
    vin = torch.frombuffer(bytearray(_vin(out, vins, N, range(B))), dtype=torch.uint8).cuda()
    vent = torch.zeros(B * 32, dtype=torch.uint8, device="cuda")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ectx.draw_entropy_dev(B, N, bbp.ENTROPY_VERIFY, vent.data_ptr())  # verify rows: ordered by the caller (same stream)
    ectx.verify_batch_dev(B, N, vin.data_ptr(), vent.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [OK] * B


def test_server_entropy_device(ctx, built, bbp):
    built.build_server()
    N, K = 8, 4
    ins, _, vins = _synth_batch(ctx, K, N, seed=5353)
    d = tempfile.mkdtemp(prefix="bbp-uds-ent-")
    path = os.path.join(d, "sock")
    log = open(os.path.join(d, "log"), "w+")
    p = subprocess.Popen([built.SERVER_BIN, "-b", path, "-l", "info", "--engine", bbp.lib_path, "--device", "0", "--window-us", "200",
                          "--entropy", "device"], stderr=log)
    try:
        for _ in range(1500):
            if os.path.exists(path) or p.poll() is not None:
                break
            time.sleep(0.02)
        assert os.path.exists(path), open(log.name).read()[-800:]
        blobs = [uc.prove(path, ins[j][:224], ins[j][224:224 + 32 * N], int.from_bytes(ins[j][-8:], "little")) for j in range(K)]
        for j in range(K):
            assert uc.verify(path, blobs[j], *vins[j]) == b"\x01"
        assert uc.verify(path, blobs[0], *vins[1]) != b"\x01"
        assert "entropy source: device" in open(log.name).read()
    finally:
        if p.poll() is None:
            p.send_signal(signal.SIGTERM)
            p.wait(timeout=30)
