"""Python restatement of the on-device entropy (include/bbp.h "On-device entropy", csrc/chacha.h): the RFC 8439 ChaCha20 block
function and the expansion of one 32-byte key into prove rows (bbp_entropy_size(N) bytes) and verify rows (32 bytes).  Shared by
the CPU tier (tests/test_entropy_host.py) and the GPU tier (tests/test_gpu_entropy.py)."""
import struct

L = 2 ** 252 + 27742317777372353535851937790883648493  # the ristretto255 group order l
_M = 0xFFFFFFFF


def _rotl(x, n):
    return ((x << n) & _M) | (x >> (32 - n))


def _quarter(s, a, b, c, d):
    s[a] = (s[a] + s[b]) & _M; s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & _M; s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b]) & _M; s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & _M; s[b] = _rotl(s[b] ^ s[c], 7)


def chacha20_block(key, counter, nonce):
    """RFC 8439 2.3: 32-byte key, 32-bit block counter, 12-byte nonce -> 64 bytes."""
    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(struct.unpack("<8I", key)) + [counter] + list(struct.unpack("<3I", nonce))
    s = list(init)
    for _ in range(10):
        _quarter(s, 0, 4, 8, 12); _quarter(s, 1, 5, 9, 13); _quarter(s, 2, 6, 10, 14); _quarter(s, 3, 7, 11, 15)
        _quarter(s, 0, 5, 10, 15); _quarter(s, 1, 6, 11, 12); _quarter(s, 2, 7, 8, 13); _quarter(s, 3, 4, 9, 14)
    return struct.pack("<16I", *((a + b) & _M for a, b in zip(s, init)))


def prove_row(key, N, i):
    """Row i of a prove-kind expansion for list length N: (4+N) blindings mod l, then the 32-byte rng seed."""
    m = 4 + N
    nonce = b"BBPE" + struct.pack("<II", N, i)
    out = b"".join((int.from_bytes(chacha20_block(key, k, nonce), "little") % L).to_bytes(32, "little") for k in range(m))
    return out + chacha20_block(key, m, nonce)[:32]


def verify_row(key, i):
    return chacha20_block(key, 0, b"BBPV" + struct.pack("<II", 0, i))[:32]


def expand_prove(key, N, B, first=0):
    return b"".join(prove_row(key, N, i) for i in range(first, first + B))


def expand_verify(key, B, first=0):
    return b"".join(verify_row(key, i) for i in range(first, first + B))
