"""GPU tier: checked proving (include/bbp.h bbp_set_prove_check, bbp_prove_batch_checked_dev).  Checked records are the unchecked
records byte for byte (and the C oracle's); rows whose witness the circuit rejects are refused instead of proved to records every
verifier rejects; a record corrupted on the device after the prover wrote it is caught, and proved again on the host path."""
import os
import signal
import subprocess
import tempfile
import threading
import time

import pytest

from tests import oracle_c
from tests import prove_check_cases as pc
from tests import uds_client as uc
from tests.test_gpu_prove_verify import _synth_batch

pytestmark = pytest.mark.gpu
OK, VERIFY, FORMAT, BAD_ARG = 0, 1, 3, 4


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def cctx(ctx, bbp):
    """A context of this module's own: checking is switched on and off here, and the hooks fire here (after `ctx`, so torch's
    HIP runtime is initialised first)."""
    c = bbp.Context(0)
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


def _prove(c, B, N, ins, ents, check):
    c.set_prove_check(check)
    try:
        return c.prove_batch(B, N, b"".join(ins), None if ents is None else b"".join(ents))
    finally:
        c.set_prove_check(False)


@pytest.mark.parametrize("N,B", [(8, 1), (8, 37), (8, 256), (8, 1024), (1, 64), (202, 64)])
def test_checked_records_are_the_unchecked_bytes(cctx, oc, bbp, N, B):
    """Single proof, small call, rotating and sliced heavy stages: with fixed entropy, checked == unchecked == C oracle (16 rows)."""
    ins, ents, vins = _synth_batch(cctx, B, N, seed=9000 + 7 * N + B)
    plain, st0 = _prove(cctx, B, N, ins, ents, False)
    n0 = cctx.prove_check_stats()
    checked, st1 = _prove(cctx, B, N, ins, ents, True)
    n1 = cctx.prove_check_stats()
    assert st0 == [OK] * B and st1 == [OK] * B
    assert checked == plain
    assert n1[0] - n0[0] == B and n1[1:] == n0[1:]
    rs_ = bbp.record_size(N)
    k = min(B, 16)
    cout, cst = oc.prove_many(b"".join(ins[:k]), b"".join(ents[:k]), k, N, threads=16)
    assert cst == [OK] * k and cout == checked[:k * rs_]


def _mixed_rows(oc, N):
    """honest rows with one row of each unsatisfied kind and the y-only row mixed in: (rows, entropies, {index: variant name})"""
    rows, ents, kinds = [], [], {}
    for name, c, _sat in pc.variants(oc, 31337, N):
        if name in ("honest", "item_bit255"):
            continue
        kinds[len(rows)] = name
        rows.append(c)
        ents.append(pc.entropy(len(rows), N))
        h = pc.honest(oc, 500 + len(rows), N)  # an honest row between every two variants
        rows.append(h)
        ents.append(pc.entropy(len(rows), N))
    return rows, ents, kinds


def test_unsatisfied_rows_are_refused(cctx, oc, bbp):
    N = 8
    rows, ents, kinds = _mixed_rows(oc, N)
    B, rs_ = len(rows), bbp.record_size(N)
    verdict = {n: s for n, _c, s in pc.variants(oc, 31337, N)}
    satisfied = {i: verdict[kinds[i]] if i in kinds else True for i in range(B)}
    plain, st0 = _prove(cctx, B, N, [pc.row(c) for c in rows], ents, False)
    n0 = cctx.prove_check_stats()
    checked, st1 = _prove(cctx, B, N, [pc.row(c) for c in rows], ents, True)
    err = bbp.lib.bbp_last_error(cctx.handle).decode()
    n1 = cctx.prove_check_stats()
    first_bad = min(i for i in range(B) if not satisfied[i])
    for i, c in enumerate(rows):
        f = c["f"]
        vt = (pc.b32(f[pc.Q]), pc.b32(f[pc.Z]), pc.b32(f[pc.SEED]), b"".join(c["pub"]))
        rec0, rec1 = plain[i * rs_:(i + 1) * rs_], checked[i * rs_:(i + 1) * rs_]
        if satisfied[i]:
            assert st0[i] == OK and st1[i] == OK, (i, kinds.get(i))
            assert rec1 == rec0 and cctx.verify(rec1, *vt) == 0, (i, kinds.get(i))
        else:
            if c["toggle"] < N:  # the gap this closes: unchecked, OK and a record every verifier rejects
                assert st0[i] == OK and cctx.verify(rec0, *vt) != 0, (i, kinds[i])
            assert st1[i] == BAD_ARG and rec1 == bytes(rs_), (i, kinds[i])
    assert ("row %d:" % first_bad) in err, err
    assert n1[0] - n0[0] == B and n1[1] - n0[1] == sum(1 for i in range(B) if not satisfied[i]) and n1[2:] == n0[2:]


def test_corruption_hook_host_path(cctx, bbp):
    N, B, i = 8, 8, 5
    ins, ents, vins = _synth_batch(cctx, B, N, seed=6060)
    rs_ = bbp.record_size(N)
    healthy, _ = _prove(cctx, B, N, ins, ents, False)
    cctx.debug_corrupt_next_proof(i)
    bad, st = _prove(cctx, B, N, ins, ents, False)
    assert st == [OK] * B and cctx.verify(bad[i * rs_:(i + 1) * rs_], *vins[i]) == 1
    assert bad[:i * rs_] == healthy[:i * rs_] and bad[(i + 1) * rs_:] == healthy[(i + 1) * rs_:]
    n0 = cctx.prove_check_stats()
    cctx.debug_corrupt_next_proof(i)
    out, st = _prove(cctx, B, N, ins, ents, True)
    n1 = cctx.prove_check_stats()
    assert st == [OK] * B and out == healthy
    assert n1[2] - n0[2] == 1 and n1[3] - n0[3] == 1
    cctx.debug_corrupt_next_proof(2)  # no entropy given: the second prove uses the entropy the call drew
    out, st = _prove(cctx, B, N, ins, None, True)
    assert st == [OK] * B and all(cctx.verify(out[j * rs_:(j + 1) * rs_], *vins[j]) == 0 for j in range(B))
    assert cctx.prove_check_stats()[2] - n1[2] == 1
    assert cctx.health() == 0


def test_device_path_statuses(cctx, oc, bbp):
    """Three checked _dev calls back to back, one synchronisation: the corrupted record is BBP_ERR_VERIFY, refused rows are
    BAD_ARG / FORMAT (device inputs are not screened: a toggle of 2^40 and a non-canonical y), every other row OK and byte-equal
    to the unchecked record."""
    import torch
    N, B, i = 8, 64, 17
    ins, ents, vins = _synth_batch(cctx, B, N, seed=7070)
    rs_ = bbp.record_size(N)
    plain, _ = _prove(cctx, B, N, ins, ents, False)
    ins3 = list(ins)
    bad = {}
    r = bytearray(ins3[3]); r[-8:] = (1 << 40).to_bytes(8, "little"); ins3[3] = bytes(r); bad[3] = BAD_ARG
    r = bytearray(ins3[4]); r[64:96] = pc.b32(pc.L); ins3[4] = bytes(r); bad[4] = FORMAT
    r = bytearray(ins3[5]); r[128:160] = pc.b32(int.from_bytes(r[128:160], "little") + 1); ins3[5] = bytes(r); bad[5] = BAD_ARG  # q
    dev = torch.device("cuda", 0)
    d_ent = torch.frombuffer(bytearray(b"".join(ents)), dtype=torch.uint8).to(dev)
    d_cent = torch.frombuffer(bytearray(os.urandom(32 * B)), dtype=torch.uint8).to(dev)
    d_ins = [torch.frombuffer(bytearray(b"".join(x)), dtype=torch.uint8).to(dev) for x in (ins, ins, ins3)]
    outs = [torch.full((B * rs_,), 0xAA, dtype=torch.uint8, device=dev) for _ in range(3)]
    sts = [torch.full((B,), -1, dtype=torch.int32, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    for k in range(3):
        if k == 1:
            cctx.debug_corrupt_next_proof(i)
        cctx.prove_batch_checked_dev(B, N, d_ins[k].data_ptr(), d_ent.data_ptr(), d_cent.data_ptr(), outs[k].data_ptr(), sts[k].data_ptr())
    torch.cuda.synchronize()
    for k in range(3):
        st = sts[k].cpu().tolist()
        out = bytes(outs[k].cpu().numpy().tobytes())
        want = {i: VERIFY} if k == 1 else bad if k == 2 else {}
        assert st == [want.get(j, OK) for j in range(B)], (k, [(j, s) for j, s in enumerate(st) if s])
        for j in range(B):
            rec = out[j * rs_:(j + 1) * rs_]
            assert rec == (bytes(rs_) if j in want else plain[j * rs_:(j + 1) * rs_]), (k, j)
    assert cctx.health() == 0


def test_combined_and_async_callers(cctx, oc, bbp):
    """Sixteen concurrent bbp_prove callers (combined into device batches), one of them unsatisfied: only that one fails, with
    BAD_ARG and the relation in its error text; prove_async likewise."""
    N, T = 8, 16
    ins, ents, vins = _synth_batch(cctx, T, N, seed=8080)
    bad = 9
    r = bytearray(ins[bad]); r[160:192] = pc.b32(int.from_bytes(r[160:192], "little") + 1); ins[bad] = bytes(r)  # z_img
    res, errs = {}, []
    cctx.set_prove_check(True)
    try:
        def worker(j):
            try:
                res[j] = ("ok", cctx.prove(ins[j][:224], ins[j][224:224 + 32 * N], j % N, ents[j]))
            except bbp.BbpError as e:
                res[j] = ("err", e.status, str(e))
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
        th = [threading.Thread(target=worker, args=(j,)) for j in range(T)]
        for t in th:
            t.start()
        for t in th:
            t.join(120)
        assert not errs, errs
        for j in range(T):
            if j == bad:
                assert res[j][0] == "err" and res[j][1] == BAD_ARG and "z_img" in res[j][2], res[j]
            else:
                assert res[j][0] == "ok" and cctx.verify(res[j][1], *vins[j]) == 0, j
        done = {}
        ev = threading.Event()

        def on_done(j):
            def f(status, record):
                done[j] = (status, record)
                if len(done) == 2:
                    ev.set()
            return f
        keep = [cctx.prove_async(ins[j][:224], ins[j][224:224 + 32 * N], j % N, ents[j], on_done(j)) for j in (bad, 0)]
        assert ev.wait(120)
        del keep
        assert done[bad][0] == BAD_ARG and done[0][0] == OK and cctx.verify(done[0][1], *vins[0]) == 0
    finally:
        cctx.set_prove_check(False)


def test_pool_members_take_the_setting_and_stats_sum(ctx, oc, bbp):
    pool = bbp.Pool([0, 0])
    try:
        N, B = 8, 10
        ins, ents, vins = _synth_batch(ctx, B, N, seed=1212)
        pool.set_prove_check(True)
        assert all("checked proving: on" in pool.member(m).describe() for m in range(2))
        out, st = pool.prove_batch(B, N, b"".join(ins), b"".join(ents))
        assert st == [OK] * B
        a, b, tot = pool.member(0).prove_check_stats(), pool.member(1).prove_check_stats(), pool.prove_check_stats()
        assert a[0] > 0 and b[0] > 0 and tot == tuple(x + y for x, y in zip(a, b)) and tot[0] == B
        assert pool.health() == 0
    finally:
        pool.close()


def test_checked_prove_beside_verify_on_one_context(cctx, oc, bbp):
    """Checked bbp_prove_batch from two threads while a third verifies on the same context: every record is the unchecked bytes
    and every verdict is right."""
    N, B = 8, 48
    ins, ents, vins = _synth_batch(cctx, B, N, seed=4545)
    rs_ = bbp.record_size(N)
    plain, _ = _prove(cctx, B, N, ins, ents, False)
    vin_ok = b"".join(plain[j * rs_:(j + 1) * rs_] + b"".join(vins[j][:3]) + vins[j][3] for j in range(B))
    tampered = bytearray(vin_ok)
    tampered[300] ^= 4
    errs, outs, verdicts = [], [], []
    cctx.set_prove_check(True)
    try:
        def prover():
            try:
                for _ in range(3):
                    outs.append(cctx.prove_batch(B, N, b"".join(ins), b"".join(ents)))
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))

        def verifier():
            try:
                for _ in range(4):
                    verdicts.append((cctx.verify_batch(B, N, vin_ok), cctx.verify_batch(B, N, bytes(tampered))))
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
        th = [threading.Thread(target=prover), threading.Thread(target=prover), threading.Thread(target=verifier)]
        for t in th:
            t.start()
        for t in th:
            t.join(180)
        assert not errs, errs
    finally:
        cctx.set_prove_check(False)
    assert len(outs) == 6 and len(verdicts) == 4
    for out, st in outs:
        assert st == [OK] * B and out == plain
    for ok, bad in verdicts:
        assert ok == [OK] * B and bad == [VERIFY] + [OK] * (B - 1)


def test_server_check_proofs(ctx, built, bbp):
    built.build_server()
    N = 8
    ins, _, vins = _synth_batch(ctx, 1, N, seed=3131)
    d = tempfile.mkdtemp(prefix="bbp-uds-chk-")
    path = os.path.join(d, "sock")
    log = open(os.path.join(d, "log"), "w+")
    p = subprocess.Popen([built.SERVER_BIN, "-b", path, "-l", "info", "--engine", bbp.lib_path, "--device", "0", "--window-us", "200",
                          "--check-proofs"], stderr=log)
    try:
        for _ in range(1500):
            if os.path.exists(path) or p.poll() is not None:
                break
            time.sleep(0.02)
        assert os.path.exists(path), open(log.name).read()[-800:]
        blob = uc.prove(path, ins[0][:224], ins[0][224:224 + 32 * N], int.from_bytes(ins[0][-8:], "little"))
        assert uc.verify(path, blob, *vins[0]) == b"\x01"
        assert "checked proving on" in open(log.name).read()
    finally:
        if p.poll() is None:
            p.send_signal(signal.SIGTERM)
            p.wait(timeout=30)
