"""gpu tier: the verifier's variable-base kernels AS SHIPPED -- k_varbase, k_varprep + k_varsum and their mixed-N twins, from the
product's own code object, launched by the verify path's launcher through bbp_debug_varbase -- against the big-int oracle.  Rows,
launches and expected values come from tests/varbase_cases.py (ledger: tests/test_varbase_cases_host.py).  Per row and launch: the
status, the eight digit words of every point slot (s + 0x88..8 computed in Python; 0x88888888 for a point that does not decode; zero
for a slot the kernels must not touch) and every partial sum, byte for byte.  A uniform launch also runs through the mixed kernels."""
import time

import pytest

from tests import varbase_cases as vc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", vc.groups())
def test_shipped_kernels(ctx, group):
    t0, o0 = time.perf_counter(), vc.ORACLE_SECONDS[0]
    runs = sums = 0
    for la in vc.launches():
        if la.group == group:
            for form in vc.forms_of(la):
                sums += vc.check_launch(ctx, la, form)
                runs += 1
    print("varbase %s: %d kernel runs, %d partial sums, %.2f s of which oracle %.2f s" % (group, runs, sums, time.perf_counter() - t0,
                                                                                        vc.ORACLE_SECONDS[0] - o0))
    assert runs >= 4


def _plain_row(n, ver=0):
    """a row of list length n as the binding packs it: identity points, every scalar 1"""
    return (n, ver, [bytes(32)] * (6 + 4 + n + 5 + 22), (1, 1, 1, 1), (1,) * (4 + n), (1,) * 22)


def test_rejects_what_it_cannot_size(ctx, bbp):
    """the entry point screens every count and scalar before it allocates or launches: BBP_ERR_BAD_ARG, through the native call"""
    ok = _plain_row(8)
    n, ver, pts, scal, wv, uj = ok
    refused = [
        ("form", 4, [ok], 1),
        ("B = 0", vc.LANES, [], 1),
        ("B = 1025", vc.PREP_SUM, [_plain_row(1)] * 1025, 1),
        ("Q = 0", vc.LANES, [ok], 0),
        ("Q = 1025", vc.MX_LANES, [ok], 1025),
        ("N = 0", vc.LANES, [_plain_row(0)], 1),
        ("N = 203", vc.MX_PREP_SUM, [_plain_row(203)], 1),
        ("two N in a uniform form", vc.LANES, [ok, _plain_row(1)], 1),
        ("two versions in a uniform form", vc.PREP_SUM, [ok, _plain_row(8, 1)], 1),
        ("version 2", vc.LANES, [(n, 2, pts, scal, wv, uj)], 1),
        ("x = l", vc.LANES, [(n, ver, pts, (vc.L, 1, 1, 1), wv, uj)], 1),
        ("rho = l", vc.LANES, [(n, ver, pts, (1, 1, 1, vc.L), wv, uj)], 1),
        ("wv = l", vc.MX_LANES, [(n, ver, pts, scal, (1,) * 11 + (vc.L,), uj)], 1),
        ("u_j^-1 = 2^256 - 1", vc.PREP_SUM, [(n, ver, pts, scal, wv, (1,) * 21 + (2**256 - 1,))], 1),
    ]
    for what, form, rows, Q in refused:
        with pytest.raises(bbp.BbpError) as e:
            ctx.debug_varbase(form, rows, Q, 0)
        assert e.value.status == 4, what
    (sums, digits, status), = ctx.debug_varbase(vc.LANES, [ok], 1, 0)  # and the row they were cut from is taken
    assert status == 0 and sums == [bytes(32)]
