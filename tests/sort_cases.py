"""Term counts and scalar rows of the one-walk staged sort's tests (test_gpu_sort_one_walk.py launches them, test_sort_digits_host.py
checks the recoder's bounds on the same rows), and the binding of tests/sort_digits_check.cpp."""
import ctypes
import functools
import random

from oracle.ref_py import ristretto as rs
from tests import msm_cases as mc

L = rs.L
B = 130  # MSMs per launch: launches of 128 and more are never split, so every case runs the unsplit kernels

# lanes with 0 / 1 / 2 scalars (1023, 1024, 1025 terms on 1024 lanes), the prover's shapes (2049, 2933), both sides of the switch to
# the wide image (SORT_WIDE_FROM = 3000) and the verifier's width.  bbp_msm_batch takes 1 + m terms (m <= 2048) or 1 + 2m: an even
# count above 2049 cannot be asked of it, so 2999 stands on the near side of the switch for 3000 and 4097 for the verifier's 4098
# (as in msm_cases.py); 3001 and 4097 have lanes with 3 / 5 scalars.
TERMS = [1, 2, 1023, 1024, 1025, 2049, 2933, 2999, 3001, 4097]


def layout(n):
    return mc.LAYOUT_G if n <= 2049 else mc.LAYOUT_G_H


EXTREMES = [L - 1, L - 2, 1 << 252, (1 << 253) - 1]  # the last is not canonical: it goes to the device as it is, to the oracle mod L


@functools.lru_cache(maxsize=None)
def rows(n):
    """name -> list of distinct rows (each a list of n scalars); a launch cycles through a set's rows"""
    rnd = random.Random(16000 + n)
    uniform = [[rnd.randrange(L) for _ in range(n)] for _ in range(3)]
    # all scalars equal: every digit's bucket takes n entries; nineteen digits of one magnitude make one bucket of 19 n entries, larger
    # than the image from 1132 terms on (21 504 entries) and from 1725 on the wide image (32 768)
    equal = [[rnd.randrange(L)] * n, [mc.ONES_19] * n]
    zero = [[0] * n]
    extremes = [[EXTREMES[(i + r) % 4] for i in range(n)] for r in range(2)]
    return {"uniform": uniform, "equal": equal, "zero": zero, "extremes": extremes}


def row_bytes_raw(row):
    return b"".join(int(v).to_bytes(32, "little") for v in row)


def load(path):
    lib = ctypes.CDLL(path)
    lib.sd_roundtrip.restype = ctypes.c_int64
    lib.sd_roundtrip.argtypes = [ctypes.c_int]
    lib.sd_compare.restype = ctypes.c_int
    lib.sd_compare.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)]
    lib.sd_bounds.argtypes = [ctypes.POINTER(ctypes.c_uint32)]
    return lib


def compare(lib, width, row):
    """(0 when the packed slots are the callback recoder's digits, most digits of one scalar)"""
    most = ctypes.c_uint32()
    return lib.sd_compare(width, len(row), row_bytes_raw(row), ctypes.byref(most)), most.value


def bounds(lib):
    out = (ctypes.c_uint32 * 5)()
    lib.sd_bounds(out)
    return dict(zip(("MSM_W", "SMALL_W", "slots12", "slots9", "staged_max_terms"), out))
