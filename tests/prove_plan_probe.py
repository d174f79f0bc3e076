"""Python side of tests/host_check.cpp's hc_prove_plan: the plan csrc/prove_plan.h makes for one prove call, as plain values.
Shared by the not-gpu table (test_prove_plan_host.py) and the GPU test that holds the library's trace lines against it."""
import ctypes

SERIAL, LANES25, WORD, HALFWORD = 0, 1, 2, 3  # ProvePlan::Chain
FOLD_ROUND = 7
KNOB_ORDER = ["slices", "rotate_below", "rotate_deep_max", "deep_from", "mixed_from", "dual_open_below", "rng_coop", "rng_coop_below", "rng_coop_idle_below",
              "rng_dpp", "rng_block", "serial_block", "serial_lds", "tr_wave_below", "ipa_wide_below", "commit_split_below", "witness_native",
              "tail_small_below", "tail_round", "stagger_mode", "trace_prove"]  # hc_prove_knob_from_env's `which`


class Plan:
    """plan_prove(knobs, state, B, inflight, sliced_busy) and plan_heavy(knobs, B).  knobs: {environment name: text} over the defaults;
    state: deep_mode, deep_idle_seen, force_deep, last_sliced, calls -- `state_out` is the same after the call."""

    def __init__(self, lib, B, inflight=0, knobs=None, busy=False, deep_mode=0, deep_idle_seen=0, force_deep=0, last_sliced=0, calls=0):
        flat = [s.encode() for kv in (knobs or {}).items() for s in kv]
        names = (ctypes.c_char_p * max(len(flat), 1))(*flat)
        state = (ctypes.c_int32 * 5)(deep_mode, deep_idle_seen, force_deep, last_sliced, calls)
        out, trace = (ctypes.c_int64 * 27)(), ctypes.create_string_buffer(256)
        lib.hc_prove_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_char_p, ctypes.c_size_t]
        rc = lib.hc_prove_plan(names, len(flat) // 2, state, B, inflight, int(busy), out, trace, len(trace))
        assert rc == 0, "not a prove knob among %r" % (knobs,)
        (self.call, self.deep, self.behind_sliced, self.dual, self.open_stream, self.par, self.coop, self.chain, self.prefix_form, self.serial_blk,
         self.cblk, self.cblk_wave, self.rotate, self.heavy_stream, self.slices, self.busy_asked) = [int(x) for x in out[:16]]
        self.bounds = [int(x) for x in out[16:21] if x >= 0]
        self.tw, self.tgrid, self.wide_ipa, self.split_T, self.tail_from, self.stagger_after = [int(x) for x in out[21:27]]
        self.trace = trace.value.decode()
        self.state_out = dict(zip(("deep_mode", "deep_idle_seen", "force_deep", "last_sliced", "calls"), (int(x) for x in state)))


def knob_from_env(lib, name, text, member):
    """ProveKnobs::from_env().<member> with name=text in the environment"""
    return int(lib.hc_prove_knob_from_env(name.encode(), text.encode(), KNOB_ORDER.index(member)))
