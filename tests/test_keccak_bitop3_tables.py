"""CPU tier: the two truth tables csrc/keccak.h hands to v_bitop3_b32 (keccak_xor3, keccak_chi) against the plain expressions
of their host branches.  The instruction computes, per bit position, table[(s0 << 2) | (s1 << 1) | s2]; the tables are read from
the header, so a changed literal there fails here before it reaches a GPU."""
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "dusk_blindbidproof_amd", "csrc", "keccak.h")
M32 = 0xFFFFFFFF


def _tables():
    src = open(HEADER).read()
    return {name: int(val, 16) for name, val in re.findall(r"^#define (BBP_BITOP3_\w+) (0x[0-9a-fA-F]+)\b", src, re.M)}


def bitop3(s0, s1, s2, table):
    """v_bitop3_b32 on 32-bit words, bit by bit"""
    out = 0
    for i in range(32):
        idx = ((s0 >> i & 1) << 2) | ((s1 >> i & 1) << 1) | (s2 >> i & 1)
        out |= (table >> idx & 1) << i
    return out


PLAIN = {
    "BBP_BITOP3_XOR3": lambda a, b, c: a ^ b ^ c,
    "BBP_BITOP3_CHI": lambda a, b, c: a ^ (~b & c & M32),
}


def test_header_defines_the_two_tables():
    assert _tables() == {"BBP_BITOP3_XOR3": 0x96, "BBP_BITOP3_CHI": 0xD2}


def test_tables_equal_the_plain_expressions_on_all_eight_inputs():
    t = _tables()
    for name, plain in PLAIN.items():
        for s0, s1, s2 in itertools.product((0, 1), repeat=3):
            assert (t[name] >> ((s0 << 2) | (s1 << 1) | s2)) & 1 == plain(s0, s1, s2) & 1, (name, s0, s1, s2)


def test_tables_on_words():
    """whole words, each of the eight input combinations in four bit positions, and the all-ones / all-zero words"""
    t = _tables()
    s0, s1, s2 = 0xF0F0F0F0, 0xCCCCCCCC, 0xAAAAAAAA
    for name, plain in PLAIN.items():
        assert bitop3(s0, s1, s2, t[name]) == plain(s0, s1, s2) & M32, name
        for a, b, c in itertools.product((0, M32), repeat=3):
            assert bitop3(a, b, c, t[name]) == plain(a, b, c) & M32, (name, a, b, c)


def test_every_boolean_step_of_the_round_goes_through_the_helpers():
    """keccak_f1600_body holds no plain ^ ~ & between state lanes besides iota: 10 + 25 xor3 sites and 25 chi sites, two halves each
    = the 120 three-input instructions of a round"""
    src = open(HEADER).read()
    body = src[src.index("BBP_HD void keccak_f1600_body"):src.index("BBP_HD_NOINLINE void keccak_f1600")]
    loop = re.sub(r"//[^\n]*", "", body[body.index("for (int r = 0"):body.index("s[0] = a00")])
    assert loop.count("keccak_xor3(") == 35 and loop.count("keccak_chi(") == 25
    assert re.findall(r"[\^~&]", loop) == ["^"] and "a00 ^= RC[r];" in loop
