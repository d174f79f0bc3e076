"""Mixed-N verification, the parts that need no GPU: the four C entry points are exported and declared, and the Python row
size / offset / packing helpers lay rows out back to back in request order (include/bbp.h bbp_verify_batch_mixed)."""
import ctypes
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = ["bbp_verify_batch_mixed", "bbp_verify_batch_mixed_aggregated", "bbp_verify_batch_mixed_dev",
         "bbp_verify_batch_mixed_aggregated_dev"]


@pytest.mark.parametrize("name", MIXED)
def test_library_exports_and_header_declares(bbp, name):
    so = ctypes.CDLL(bbp.lib_path)
    assert hasattr(so, name), name
    assert name in bbp.SIGNATURES
    with open(os.path.join(ROOT, "include", "bbp.h")) as f:
        assert ("int32_t %s(" % name) in f.read()


def test_verify_row_size(bbp):
    for n in range(1, 203):
        assert bbp.verify_row_size(n) == bbp.record_size(n) + 96 + 32 * n
        assert bbp.verify_row_size(n) == bbp.lib.bbp_proof_record_size(n) + 96 + 32 * n  # the library's record size


def _row(bbp, n, tag):
    rec = bytes([0]) + bytes((tag + i) & 0xFF for i in range(bbp.record_size(n) - 1))
    return (rec, bytes([tag]) * 32, bytes([tag ^ 1]) * 32, bytes([tag ^ 2]) * 32, bytes((tag * 7 + j) & 0xFF for j in range(32 * n)))


def test_packer_lays_rows_out_in_request_order(bbp):
    rnd = random.Random(20261016)
    ns = [rnd.randint(1, 202) for _ in range(40)] + [1, 202, 1]
    rows = [_row(bbp, n, i) for i, n in enumerate(ns)]
    Ns, blob = bbp.pack_mixed_rows(rows)
    assert Ns == ns
    off = bbp.mixed_row_offsets(Ns)
    assert len(off) == len(ns) + 1 and off[0] == 0 and off[-1] == len(blob)
    for i, (n, r) in enumerate(zip(ns, rows)):
        assert off[i + 1] - off[i] == bbp.verify_row_size(n)
        assert blob[off[i]:off[i + 1]] == b"".join(r), i
        # the fields where a verifier looks for them: score right after the record, pub_list last
        rs_ = bbp.record_size(n)
        assert blob[off[i] + rs_:off[i] + rs_ + 32] == r[1]
        assert blob[off[i] + rs_ + 96:off[i + 1]] == r[4]


def test_packer_refuses_rows_of_the_wrong_layout(bbp):
    rec, sc, zi, sd, pub = _row(bbp, 5, 3)
    with pytest.raises(ValueError):
        bbp.pack_mixed_rows([(rec, sc, zi, sd, pub[:-1])])
    with pytest.raises(ValueError):
        bbp.pack_mixed_rows([(rec + b"\0", sc, zi, sd, pub)])
