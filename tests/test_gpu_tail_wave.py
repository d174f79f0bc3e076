"""gpu tier: the IPA tail on one wavefront per proof (prover.hip k_tail_lr: a 64-lane workgroup per proof, the B term dealt to the
lanes) and the composite bucket fold in front of it (msm.hip k_msm_fold<1>), through bbp_prove_batch_dev at N = 8.  Records are compared
byte for byte with the C oracle's, as bench_workloads.ProveWorkload.check does.  Batch sizes: 1 takes the split-MSM path in front of
the fold; 64 is the first unsplit launch (128 MSMs); 3, 4 and 5 straddle the earlier three-proofs-per-workgroup boundary; 65 has a lone
last workgroup.  Every row is checked at B <= 5, rows 0, 63 and 64 at B = 64 and 65.

By default a heavy stage of fewer than 65 proofs keeps all eleven IPA rounds on the fixed-base MSM kernels (prove_plan.h
tail_small_below), so every size runs twice: on the session's context (only B = 65 reaches the tail) and on a context created under
BBP_TAIL_SMALL_BELOW=0, where every size does."""
import os

import pytest

import bench_workloads as bw

pytestmark = pytest.mark.gpu
N = 8
SEED = 2101
SIZES = (1, 3, 4, 5, 64, 65)
ROWS = (0, 1, 2, 3, 4, 63, 64)  # the rows any size checks


@pytest.fixture(scope="module")
def bids(ctx):
    """65 synthetic bids (row i does not depend on the batch size: every size proves a prefix) and the oracle's records of ROWS"""
    lib = bw._oracle_lib()
    ins, ents, _, _ = bw.synth_bids(ctx, max(SIZES), N, SEED)
    want = {}
    for r in ROWS:
        rc, rec = lib.prove(ins[r][:224], ins[r][224:224 + 32 * N], int.from_bytes(ins[r][-8:], "little"), ents[r])
        assert rc == 0, r
        want[r] = rec
    return ins, ents, want


@pytest.fixture(scope="module")
def tail_ctx(ctx, bbp):
    """a context whose small heavy stages take the folded-generator tail as well (after `ctx`: torch's HIP runtime comes first)"""
    old = os.environ.get("BBP_TAIL_SMALL_BELOW")
    os.environ["BBP_TAIL_SMALL_BELOW"] = "0"
    try:
        c = bbp.Context(0)
    finally:
        if old is None:
            os.environ.pop("BBP_TAIL_SMALL_BELOW", None)
        else:
            os.environ["BBP_TAIL_SMALL_BELOW"] = old
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("which", ["default_plan", "tail_at_every_size"])
def test_records_equal_the_oracles(ctx, tail_ctx, bbp, bids, which, B):
    import torch
    ctx = ctx if which == "default_plan" else tail_ctx
    ins, ents, want = bids
    rs = bbp.record_size(N)
    dev = torch.device("cuda:0")
    d_in, d_ent = bw._to_dev(torch, dev, b"".join(ins[:B])), bw._to_dev(torch, dev, b"".join(ents[:B]))
    d_out = torch.zeros(B * rs, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.prove_batch_dev(B, N, d_in.data_ptr(), d_ent.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    out = bytes(d_out.cpu().numpy().tobytes())
    rows = range(B) if B <= 5 else [r for r in (0, 63, 64) if r < B]
    wrong = [r for r in rows if out[r * rs:(r + 1) * rs] != want[r]]
    assert not wrong, (B, wrong)
