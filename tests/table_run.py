"""ctypes front end of the table-audit entry points of tests/device_check.hip (dc_points_encode, dc_comb_entries, dc_ptable_walk,
dc_ptable_rows, dc_read_u32): they read the engine's resident tables in place, through the device pointers bbp_debug_table hands out,
so the library must be loaded into the process that holds the context."""
import ctypes

_vp, _int, _u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
_u8p, _u32p = ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)
SIGNATURES = {
    "points_encode": [_vp, _int, _u8p],
    "comb_entries": [_vp, _int, _u8p, ctypes.POINTER(ctypes.c_int32)],
    "ptable_walk": [_vp, _u64, _vp, _u64, _int, _int, _u32p, _u32p],
    "ptable_rows": [_vp, _u64, _int, _u32p, _u8p, _u8p],
    "read_u32": [_vp, _int, _u32p],
}
GE_BYTES, ROW_BYTES, COMB_BYTES = 160, 128, 96


class Tables:
    def __init__(self, lib, name):
        self.name = name
        self.fn = {}
        for short, argtypes in SIGNATURES.items():
            f = getattr(lib, "dc_" + short)
            f.argtypes, f.restype = argtypes, _int
            self.fn[short] = f
        self.tail_pieces = lib.dc_tail_pieces  # (bound in tests/scalarmul_run.py as well)

    def _encodings(self, what, dev, n):
        out = ctypes.create_string_buffer(32 * n)
        rc = self.fn[what](dev, n, out)
        assert rc == 0, "%s (%s): returned %d" % (what, self.name, rc)
        return [out.raw[32 * i:32 * i + 32] for i in range(n)]

    def points(self, dev, size):
        assert size % GE_BYTES == 0
        return self._encodings("points_encode", dev, size // GE_BYTES)

    def comb(self, dev, size):
        """(encodings of the entries' points, flags: the entry's third field is 2d x y of that point)"""
        assert size % COMB_BYTES == 0
        n = size // COMB_BYTES
        out, ok = ctypes.create_string_buffer(32 * n), (ctypes.c_int32 * n)()
        rc = self.fn["comb_entries"](dev, n, out, ok)
        assert rc == 0, "comb_entries (%s): returned %d" % (self.name, rc)
        return [out.raw[32 * i:32 * i + 32] for i in range(n)], list(ok)

    def walk(self, gens, gens_size, table, table_size, n_bases, n_pos):
        bad, first = (ctypes.c_uint32 * n_bases)(), (ctypes.c_uint32 * n_bases)()
        rc = self.fn["ptable_walk"](gens, gens_size, table, table_size, n_bases, n_pos, bad, first)
        assert rc == 0, "ptable_walk (%s): returned %d" % (self.name, rc)
        return list(bad), list(first)

    def rows(self, table, table_size, idx):
        """(identity + row, basepoint + row) of every listed row, as encodings"""
        out, out_b = ctypes.create_string_buffer(32 * len(idx)), ctypes.create_string_buffer(32 * len(idx))
        rc = self.fn["ptable_rows"](table, table_size // ROW_BYTES, len(idx), (ctypes.c_uint32 * len(idx))(*idx), out, out_b)
        assert rc == 0, "ptable_rows (%s): returned %d" % (self.name, rc)
        return [out.raw[32 * i:32 * i + 32] for i in range(len(idx))], [out_b.raw[32 * i:32 * i + 32] for i in range(len(idx))]

    def words(self, dev, size):
        assert size % 4 == 0
        out = (ctypes.c_uint32 * (size // 4))()
        rc = self.fn["read_u32"](dev, size // 4, out)
        assert rc == 0, "read_u32 (%s): returned %d" % (self.name, rc)
        return list(out)
