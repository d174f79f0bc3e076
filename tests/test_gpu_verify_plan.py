"""The four front ends of a verify call (csrc/verify_plan.h VerifyPlan::Front: uniform, mixed, one round, several rounds) through the
plain and the aggregated engine at B = 32 and B = 33: the two sides of the wavefront-per-proof rule of the transcript replay
(BBP_TR_WAVE_BELOW, 32), the one choice of the plan that no other verify suite straddles.

Rows are proved by the C oracle on the CPU (tests/test_gpu_verify_mixed.py's builders), one per bid-list length, tiled to B with one
row tampered (t_x + 1: the check fails, the parse does not).  Expected: the oracle's verdict row by row, and for the aggregated calls
the fallback count -- the members of the one group that fails."""
import types

import pytest

from tests import test_gpu_verify_mixed as vm
from tests import test_gpu_verify_rounds as vr

pytestmark = pytest.mark.gpu
OK, VERIFY = 0, 1
NS = (1, 8, 202)
G = 8
oc = vm.oc


@pytest.fixture(scope="module")
def proved(oc, bbp):
    """N -> a round of one valid row and its tampered copy, as tests/test_gpu_verify_rounds.py's _batch takes rounds; .full: the two
    rows with seed and list behind them (a row of bbp_verify_batch)"""
    out = {}
    for n in NS:
        ins, ents, tails = vm._synth(oc, 1, n, seed=7000 + n)
        rec, st = oc.prove_many(ins[0], ents[0], 1, n, threads=8)
        assert st == [0]
        rsz = bbp.record_size(n)
        good = rec[:rsz] + tails[0]
        full = [good, vm._tamper(good, n, "tx")]
        verdict = oc.verify_many(b"".join(full), 2, n, threads=8)
        assert verdict == [OK, VERIFY]
        table = tails[0][64:]  # seed || pub_list
        out[n] = types.SimpleNamespace(N=n, full=full, variants=[r[:rsz + 64] for r in full], verdict=verdict, table=lambda t=table: t)
    return out


def _picks(B, n_rounds):
    """row i belongs to round i % n_rounds; the last row is the tampered one (B = 33 and G = 8: a group of its own)"""
    return [(i % n_rounds, 1 if i == B - 1 else 0) for i in range(B)]


def _check(B, want, plain, agg):
    assert plain == want
    st, nfb = agg
    assert st == want
    assert nfb == vm._expected_fallback([0] * B, want, G, {B - 1}) == (B - 1) % G + 1


@pytest.mark.parametrize("B", [32, 33])
@pytest.mark.parametrize("N", [1, 8])
def test_uniform(ctx, proved, N, B):
    blob = b"".join(proved[N].full[v] for _, v in _picks(B, 1))
    want = [OK] * (B - 1) + [VERIFY]
    _check(B, want, ctx.verify_batch(B, N, blob), ctx.verify_batch_aggregated(B, N, blob, G))


@pytest.mark.parametrize("B", [32, 33])
def test_mixed(ctx, proved, B):
    picks = _picks(B, len(NS))
    Ns = [NS[r] for r, _ in picks]
    blob = b"".join(proved[NS[r]].full[v] for r, v in picks)
    want = [OK] * (B - 1) + [VERIFY]
    _check(B, want, ctx.verify_batch_mixed(Ns, blob), ctx.verify_batch_mixed_aggregated(Ns, blob, G))


@pytest.mark.parametrize("B", [32, 33])
@pytest.mark.parametrize("N", [1, 8])
def test_one_round(ctx, proved, N, B):
    round_Ns, table, _, rows, want = vr._batch([proved[N]], _picks(B, 1))
    assert want == [OK] * (B - 1) + [VERIFY]
    _check(B, want, ctx.verify_rounds(round_Ns, table, None, rows), ctx.verify_rounds_aggregated(round_Ns, table, None, rows, G))


@pytest.mark.parametrize("B", [32, 33])
def test_several_rounds(ctx, proved, B):
    round_Ns, table, round_of, rows, want = vr._batch([proved[n] for n in NS], _picks(B, len(NS)))
    assert round_Ns == list(NS) and want == [OK] * (B - 1) + [VERIFY]
    _check(B, want, ctx.verify_rounds(round_Ns, table, round_of, rows), ctx.verify_rounds_aggregated(round_Ns, table, round_of, rows, G))
