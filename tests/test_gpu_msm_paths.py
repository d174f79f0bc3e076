"""GPU tier: the paths of the unsplit MSM kernels that only large launches reach -- k_msm_sort_staged's window walk, its direct pass
for a bucket larger than the LDS image, the 128 KB wide image, the unsplit plain scatter -- and three rows the split tests lacked.
Every case goes through bbp_msm_batch and is compared byte for byte with the C oracle.  The cases and their scalar rows are
tests/msm_cases.py's; the not-gpu ledger (test_msm_plan_host.py) proves from the plan of each launch and the product's own recoder
that a case reaches the path it is named for, and every test here asks the same plan before it launches.

A launch is 128 MSMs (the smallest that is never split): the adversarial row at index 0, in the middle and at index 127, the others
cheap (all zero, one term, four uniformly random rows).  The oracle computes every distinct row once per session."""
import ctypes
import os

import pytest

from tests import msm_cases as mc
from tests import oracle_c

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def lib(built):
    return ctypes.CDLL(built.build_hostcheck())


@pytest.fixture(scope="module")
def contexts(bbp, ctx):
    """setting -> context: the session's for the default knobs, else one made the way test_gpu_fuzz.py makes them (set the variables,
    construct, restore).  The cases come grouped by setting, so one such context lives at a time; it is closed, healthy, when another
    setting is asked for or the module is through."""
    assert (bbp.LAYOUT_BLIND_G_H, bbp.LAYOUT_BLIND_G) == (mc.LAYOUT_G_H, mc.LAYOUT_G)
    live = {}

    def retire():
        for setting, c in list(live.items()):
            flags = c.health()
            c.close()
            del live[setting]
            assert flags == 0, (setting, flags)

    def get(setting):
        if setting == "default":
            return ctx
        if setting not in live:
            retire()
            knobs = mc.SETTINGS[setting]
            old = {k: os.environ.get(k) for k in knobs}
            os.environ.update(knobs)
            try:
                live[setting] = bbp.Context(0)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        return live[setting]
    yield get
    retire()


class Reference:
    """row bytes and the oracle's result per distinct row, computed once"""

    def __init__(self, oc):
        self.oc, self.bytes, self.point = oc, {}, {}

    def row(self, key, scalars):
        if key not in self.bytes:
            self.bytes[key] = mc.row_bytes(scalars)
        return self.bytes[key]

    def expect(self, keys, layout, n_terms):
        todo = [k for k in dict.fromkeys(keys) if k not in self.point]
        if todo:
            out = self.oc.msm_layout_many([self.bytes[k] for k in todo], [n_terms] * len(todo), [layout] * len(todo), threads=8)
            for i, k in enumerate(todo):
                self.point[k] = out[32 * i:32 * i + 32]
        return b"".join(self.point[k] for k in keys)


@pytest.fixture(scope="module")
def ref(oc):
    return Reference(oc)


@pytest.mark.parametrize("case", mc.UNSPLIT_CASES, ids=mc.case_id)
def test_unsplit_launch(contexts, lib, ref, case):
    n, layout = case.n_terms, mc.SHAPE_LAYOUT[case.n_terms]
    p = mc.plan(lib, mc.UNSPLIT_B, n, mc.SETTINGS[case.setting])
    assert mc.path(p) == case.path and p.split == 1
    keys = [None] * mc.UNSPLIT_B
    for b, scalars in mc.filler_rows(n).items():
        keys[b] = (n, "filler", b)
        ref.row(keys[b], scalars)
    for b in mc.ADVERSARIAL_AT:
        keys[b] = (n, case.row)
        ref.row(keys[b], mc.unsplit_rows(lib, n)[case.row].scalars)
    c = contexts(case.setting)
    got = c.msm_batch(mc.UNSPLIT_B, n, b"".join(ref.bytes[k] for k in keys), layout)
    exp = ref.expect(keys, layout, n)
    wrong = [b for b in range(mc.UNSPLIT_B) if got[32 * b:32 * b + 32] != exp[32 * b:32 * b + 32]]
    assert not wrong, (mc.case_id(case), wrong)
    assert c.health() == 0


def test_split_launch_rows_the_split_tests_lacked(ctx, lib, ref):
    """the small geometry (3 MSMs of 2933 terms, 16 sub-MSMs each): an all-zero row (every sub-MSM empty, k_msm_reduce over
    identities), a row whose non-zero terms all lie in one sub-MSM, a row of the width-9 recoding's limit patterns"""
    layout, n, B = mc.SPLIT_SHAPE
    p = mc.plan(lib, B, n)
    assert mc.path(p) == (mc.SMALL, mc.PLAIN, mc.SMALL_FOLD) and p.split == 16 and p.reduce
    rows = mc.split_rows(n, p.n_sub)
    keys = [(n, "split", name) for name in rows]
    for k, scalars in zip(keys, rows.values()):
        ref.row(k, scalars)
    got = ctx.msm_batch(B, n, b"".join(ref.bytes[k] for k in keys), layout)
    exp = ref.expect(keys, layout, n)
    assert got == exp, [name for i, name in enumerate(rows) if got[32 * i:32 * i + 32] != exp[32 * i:32 * i + 32]]
    assert got[:32] == bytes(32)  # the identity's encoding
    assert ctx.health() == 0
