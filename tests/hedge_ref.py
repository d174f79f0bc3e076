"""Python restatement of the hedged on-device entropy (include/bbp.h "Hedged on-device entropy", csrc/hedge.h): a prove row's ChaCha20
key is SHA3-256 over a domain tag, the call key, the list length and the row's own input bytes; the row is then chacha.h's prove row
under that key and the nonce word "BBPH".  Built from hashlib.sha3_256 and tests/entropy_ref.chacha20_block.  Shared by the CPU tier
(tests/test_hedge_host.py) and the GPU tier (tests/test_gpu_entropy_hedged.py)."""
import hashlib
import struct

from tests.entropy_ref import L, chacha20_block

TAG = b"BBP-hedge-v1"


def in_bytes(N):
    return 232 + 32 * N


def row_key(key, N, row):
    """row: scalars7 || pub_list || toggle(u64 LE), 232 + 32 N raw bytes as bbp_prove_batch takes them."""
    assert len(key) == 32 and len(row) == in_bytes(N)
    return hashlib.sha3_256(TAG + key + struct.pack("<I", N) + row).digest()


def prove_row(key, N, i, row):
    """Entropy row of prove row i (its index in the host call) under call key `key`: (4+N) blindings mod l, then the rng seed."""
    rk, m = row_key(key, N, row), 4 + N
    nonce = b"BBPH" + struct.pack("<II", N, i)
    out = b"".join((int.from_bytes(chacha20_block(rk, k, nonce), "little") % L).to_bytes(32, "little") for k in range(m))
    return out + chacha20_block(rk, m, nonce)[:32]


def expand_prove(key, N, rows, first=0):
    """rows: a list of input rows, or their concatenation."""
    if isinstance(rows, (bytes, bytearray)):
        s = in_bytes(N)
        rows = [bytes(rows[o:o + s]) for o in range(0, len(rows), s)]
    return b"".join(prove_row(key, N, first + j, r) for j, r in enumerate(rows))
