"""ctypes front end of the scalar-multiplication entry points that tests/host_check.cpp (hc_*) and tests/device_check.hip (dc_*) share:
the same arguments and outputs in both, so tests/scalarmul_cases.py checks both tiers with one set of functions."""
import ctypes

from tests.scalarmul_cases import STRAUS_MAX

_u8p, _u32p, _i32p = ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
_int = ctypes.c_int
SIGNATURES = {
    "comb": [_int, _u8p, _int, _u32p, _u32p, _u8p, _u8p, _u8p, _u8p, _i32p],
    "comb_table": [_int, _u8p, _u8p, _i32p],
    "tail_pieces": [],
    "tail": [_int, _u8p, _int, _u32p, _u8p, _i32p, _i32p, _u8p, _i32p],
    "tail_pair": [_int, _u8p, _int, _u32p, _u8p, _u32p, _u8p, _u8p, _i32p],
    "straus": [_int, _u8p, _int, _i32p, _u32p, _u8p, _u8p, _u8p, _u32p, _i32p],
}


def _sc(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def _u32(vals):
    return (ctypes.c_uint32 * len(vals))(*vals)


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _split32(buf, n):
    return [buf.raw[32 * i:32 * i + 32] for i in range(n)]


class Runner:
    """prefix: "hc" (host) or "dc" (device); a non-zero return value (a hipError_t on the device) or an undecodable point fails the test"""

    def __init__(self, lib, prefix, name):
        self.name = name
        self.fn = {}
        for short, argtypes in SIGNATURES.items():
            f = getattr(lib, "%s_%s" % (prefix, short))
            f.argtypes, f.restype = argtypes, _int
            self.fn[short] = f

    def _done(self, what, rc, ok):
        assert rc == 0, "%s (%s): returned %d" % (what, self.name, rc)
        assert all(x == 1 for x in ok), "%s (%s): a point did not decode" % (what, self.name)

    def tail_pieces(self):
        return self.fn["tail_pieces"]()

    def comb(self, encs, items):
        n, ok = len(items), _i32([0] * len(encs))
        one, split = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n)
        rc = self.fn["comb"](len(encs), b"".join(encs), n, _u32([it[0] for it in items]), _u32([it[1] for it in items]),
                             _sc([it[2] for it in items]), _sc([it[3] for it in items]), one, split, ok)
        self._done("comb", rc, ok)
        return _split32(one, n), _split32(split, n)

    def comb_table(self, encs):
        ok, out = _i32([0] * len(encs)), ctypes.create_string_buffer(32 * 512 * len(encs))
        self._done("comb_table", self.fn["comb_table"](len(encs), b"".join(encs), out, ok), ok)
        return _split32(out, 512 * len(encs))

    def tail(self, encs, items):
        n, ok, out = len(items), _i32([0] * len(encs)), ctypes.create_string_buffer(32 * len(items))
        rc = self.fn["tail"](len(encs), b"".join(encs), n, _u32([it[1] for it in items]), _sc([it[0] for it in items]),
                             _i32([it[2] for it in items]), _i32([it[3] for it in items]), out, ok)
        self._done("tail", rc, ok)
        return _split32(out, n)

    def tail_pair(self, encs, items):
        n, ok, out = len(items), _i32([0] * len(encs)), ctypes.create_string_buffer(32 * len(items))
        rc = self.fn["tail_pair"](len(encs), b"".join(encs), n, _u32([it[1] for it in items]), _sc([it[0] for it in items]),
                                  _u32([it[3] for it in items]), _sc([it[2] for it in items]), out, ok)
        self._done("tail_pair", rc, ok)
        return _split32(out, n)

    def straus(self, encs, items):
        n, ok = len(items), _i32([0] * len(encs))
        pad = [list(it) + [(0, 0)] * (STRAUS_MAX - len(it)) for it in items]
        top, lanes = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n)
        words = (ctypes.c_uint32 * (8 * STRAUS_MAX * n))()
        rc = self.fn["straus"](len(encs), b"".join(encs), n, _i32([len(it) for it in items]), _u32([i for it in pad for _, i in it]),
                               _sc([s for it in pad for s, _ in it]), top, lanes, words, ok)
        self._done("straus", rc, ok)
        w = list(words)
        return _split32(top, n), _split32(lanes, n), [[w[8 * (STRAUS_MAX * i + a):8 * (STRAUS_MAX * i + a) + 8] for a in range(STRAUS_MAX)]
                                                       for i in range(n)]
