"""MODEL (test infrastructure, never shipped): the EXPANDED blinding draw of include/bbp.h (bbp_set_blinding_draw) in Python, on top
of the oracle's merlin restatement.

The prover's TranscriptRng is built exactly as merlin builds it (clone of the transcript, rekeyed with every v_blinding, finalised
with the external 32 bytes).  Then
  key = rng.fill_bytes(32)
  draw j < 3 + 2 n1 = sc_wide(ChaCha20 block(key, counter j, nonce words ("BBPX", 0, 0)))        (RFC 8439 section 2.3)
and every later draw (the five t blindings) comes from the same TranscriptRng, continuing after the key squeeze.

Put ExpandedDrawTranscript in place of oracle.ref_py.blindbid.new_transcript (monkeypatch, or the `patched()` context manager):
oracle.ref_py.blindbid.prove is then the EXPANDED prover, and the unmodified verify its verifier."""
import contextlib
import struct

from oracle.ref_py.merlin import Transcript

NONCE0 = int.from_bytes(b"BBPX", "little")
_M32 = 0xFFFFFFFF


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & _M32


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & _M32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & _M32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & _M32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & _M32; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_block(key32, counter, nonce_words):
    """RFC 8439 2.3: the 64 bytes of block `counter` under (key, nonce); nonce as three little-endian words"""
    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(struct.unpack("<8I", key32)) + [counter & _M32] + list(nonce_words)
    x = list(init)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return struct.pack("<16I", *[(a + b) & _M32 for a, b in zip(x, init)])


def n_mul_of(n_items):
    """multipliers of the blind-bid circuit with a bid list of n_items: four MiMC gadgets of 4 x 90, 3 per item, 2"""
    return 1442 + 3 * n_items


def draw_bytes(key32, j):
    """the 64 bytes that draw j is reduced from"""
    return chacha20_block(key32, j, (NONCE0, 0, 0))


class ExpandedRng:
    """steps 2-4 of the draw over the real TranscriptRng"""

    def __init__(self, rng, n_draws):
        self.rng, self.n_draws, self.j = rng, n_draws, 0
        self.key = rng.fill_bytes(32)

    def fill_bytes(self, n):
        if self.j < self.n_draws:
            assert n == 64
            self.j += 1
            return draw_bytes(self.key, self.j - 1)
        return self.rng.fill_bytes(n)


class ExpandedDrawTranscript(Transcript):
    """The prover's transcript under EXPANDED.  The number of expanded draws, 3 + 2 n1, follows from the "m" message the prover appends
    before it builds its rng (m = 4 + N, n1 = n_mul_of(N)) unless n1 is given.  A verifier builds its rng without witnesses and keeps
    merlin's draws (include/bbp.h: the verifier's draws do not change)."""

    def __init__(self, label=b"BlindBidProofGadget", n1=None):
        super().__init__(label)
        self.n1, self.last_rng = n1, None

    def append_message(self, label, msg):
        if label == b"m" and self.n1 is None:
            self.n1 = n_mul_of(struct.unpack("<Q", msg)[0] - 4)
        super().append_message(label, msg)

    def build_rng(self, witnesses, entropy32):
        rng = super().build_rng(witnesses, entropy32)
        if not witnesses:
            return rng
        self.last_rng = ExpandedRng(rng, 3 + 2 * self.n1)
        return self.last_rng


@contextlib.contextmanager
def patched(blindbid):
    """oracle.ref_py.blindbid with ExpandedDrawTranscript as its new_transcript, for callers without pytest's monkeypatch"""
    old = blindbid.new_transcript
    blindbid.new_transcript = ExpandedDrawTranscript
    try:
        yield
    finally:
        blindbid.new_transcript = old
