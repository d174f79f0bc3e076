"""not-gpu tier: how a prove call is scheduled (csrc/prove_plan.h: ProveKnobs, ProveRuleState, plan_prove, plan_heavy), compiled for
the host by tests/host_check.cpp.  Every expected value is a literal worked out from the rules as DESIGN.md section 4 states them,
never a second call of the header."""
import ctypes

import pytest

from tests.prove_plan_probe import FOLD_ROUND, HALFWORD, LANES25, SERIAL, WORD, Plan, knob_from_env


@pytest.fixture(scope="module")
def lib(built):
    return ctypes.CDLL(built.build_hostcheck())


# B: prefix_form, cblk, tw, tgrid, wide_ipa, split_T, tail_from -- defaults: a wavefront per proof for the transcripts and the wide
# IPA round up to 32 proofs, all rounds fixed-base below 65, T commitments split while 5 B <= 1024, workgroups of 64 / 128 / 256
SMALL = {
    1: (2, 64, 1, 1, 1, 1, 12), 32: (2, 64, 1, 32, 1, 1, 12), 33: (1, 64, 0, 1, 0, 1, 12), 64: (1, 64, 0, 1, 0, 1, 12),
    65: (1, 64, 0, 2, 0, 1, 7), 127: (1, 64, 0, 2, 0, 1, 7), 128: (1, 64, 0, 2, 0, 1, 7), 191: (1, 128, 0, 3, 0, 1, 7),
    192: (1, 128, 0, 3, 0, 1, 7), 204: (1, 128, 0, 4, 0, 1, 7), 205: (1, 128, 0, 4, 0, 0, 7), 768: (1, 256, 0, 12, 0, 0, 7),
    769: (1, 256, 0, 13, 0, 0, 7), 1023: (1, 256, 0, 16, 0, 0, 7),
}


@pytest.mark.parametrize("call", [0, 7, 14])
def test_calls_below_1024_open_on_two_streams_and_rotate(lib, call):
    for B, (prefix, cblk, tw, tgrid, wide, split, tail) in SMALL.items():
        p = Plan(lib, B, calls=call)
        assert (p.call, p.deep, p.behind_sliced, p.dual, p.rotate, p.slices, p.bounds) == (call, 0, 0, 1, 1, 0, []), B
        assert (p.open_stream, p.par, p.heavy_stream) == ({0: 0, 7: 1, 14: 0}[call], {0: 0, 7: 2, 14: 4}[call], {0: 1, 7: 2, 14: 3}[call]), B
        assert (p.coop, p.chain, p.prefix_form, p.cblk, p.cblk_wave) == (1, HALFWORD, prefix, cblk, 2 * cblk), B
        assert (p.tw, p.tgrid, p.wide_ipa, p.split_T, p.tail_from) == (tw, tgrid, wide, split, tail), B
        assert p.busy_asked == 0 and p.state_out == dict(deep_mode=0, deep_idle_seen=1, force_deep=0, last_sliced=0, calls=call + 1)


def test_the_cooperative_chain_above_768_needs_an_idle_device(lib):
    for B in (769, 1023):
        p = Plan(lib, B, inflight=1)
        assert (p.coop, p.chain, p.prefix_form, p.serial_blk) == (0, SERIAL, 0, 64) and (p.dual, p.rotate) == (1, 1)
    assert Plan(lib, 768, inflight=2).coop == 1


LARGE = {1024: [0, 341, 682, 1024], 2300: [0, 766, 1533, 2300], 2301: [0, 767, 1534, 2301], 4096: [0, 1365, 2730, 4096], 4097: [0, 1365, 2731, 4097]}


@pytest.mark.parametrize("call", [0, 7])
def test_calls_from_1024_are_sliced_on_the_callers_stream(lib, call):
    for B, bounds in LARGE.items():
        for inflight in (0, 1, 2):
            p = Plan(lib, B, inflight=inflight, calls=call)
            assert (p.deep, p.dual, p.rotate, p.open_stream, p.par, p.heavy_stream) == (0, 0, 0, 0, call & 1, 0), B
            assert (p.slices, p.bounds) == (3, bounds), B
            assert p.coop == (1 if inflight == 0 and B <= 2300 else 0), (B, inflight)
            assert (p.tw, p.wide_ipa, p.split_T, p.tail_from) == (0, 0, 0, 7)


def test_three_calls_in_flight_enter_deep_mode(lib):
    for B in (1024, 4096):
        p = Plan(lib, B, inflight=3, calls=8)
        assert (p.deep, p.dual, p.rotate, p.slices, p.open_stream, p.par, p.heavy_stream, p.coop) == (1, 1, 1, 0, 0, 3, 3, 0), B
        assert p.state_out["deep_mode"] == 1 and p.state_out["deep_idle_seen"] == 0
    p = Plan(lib, 4097, inflight=3, calls=8)  # beyond BBP_ROTATE_DEEP_MAX: sliced, though the caller is in deep mode
    assert (p.deep, p.dual, p.rotate, p.slices, p.par, p.bounds) == (0, 0, 0, 3, 0, LARGE[4097]) and p.state_out["deep_mode"] == 1
    assert Plan(lib, 1024, inflight=2).deep == 0
    p = Plan(lib, 1024, inflight=2, knobs={"BBP_ROTATE_DEEP_FROM": "2"})
    assert (p.deep, p.rotate) == (1, 1)


def test_deep_mode_is_left_by_the_sixth_idle_call(lib):
    state = dict(deep_mode=1, deep_idle_seen=0, force_deep=0, last_sliced=0, calls=0)
    for k in range(1, 6):
        p = Plan(lib, 1024, inflight=2, **state)
        assert (p.deep, p.rotate, p.slices, p.par) == (1, 1, 0, (k - 1) % 5), k
        state = p.state_out
        assert state == dict(deep_mode=1, deep_idle_seen=k, force_deep=0, last_sliced=0, calls=k)
    p = Plan(lib, 1024, inflight=2, **state)
    assert (p.deep, p.rotate, p.slices, p.par) == (0, 0, 3, 1)
    assert p.state_out == dict(deep_mode=0, deep_idle_seen=6, force_deep=0, last_sliced=0, calls=6)
    p = Plan(lib, 1024, inflight=3, **state)  # ... and a call that finds three in flight starts the count again
    assert p.deep == 1 and p.state_out["deep_idle_seen"] == 0


def test_force_deep_and_one_slice(lib):
    p = Plan(lib, 1024, force_deep=1)
    assert (p.deep, p.dual, p.rotate, p.slices) == (1, 1, 1, 0)
    assert p.state_out == dict(deep_mode=0, deep_idle_seen=1, force_deep=1, last_sliced=0, calls=1)  # the hysteresis as after any idle call
    assert Plan(lib, 4097, force_deep=1).deep == 0
    for kw in (dict(inflight=3), dict(force_deep=1), dict(deep_mode=1)):
        p = Plan(lib, 1024, knobs={"BBP_SLICES": "1"}, **kw)
        assert (p.deep, p.dual, p.rotate, p.slices, p.bounds) == (0, 0, 0, 1, [0, 1024]), kw
    assert Plan(lib, 1024, inflight=3, knobs={"BBP_ROTATE_DEEP_MAX": "0"}).deep == 0


def test_a_call_behind_a_sliced_heavy_stage_is_sliced_too(lib):
    p = Plan(lib, 870, last_sliced=1, busy=True, calls=5)
    assert (p.behind_sliced, p.busy_asked, p.dual, p.rotate, p.open_stream, p.par, p.slices, p.bounds) == (1, 1, 0, 0, 0, 1, 3, [0, 290, 580, 870])
    p = Plan(lib, 870, last_sliced=1, busy=False, calls=5)  # the slices have left the device
    assert (p.behind_sliced, p.busy_asked, p.dual, p.rotate, p.par) == (0, 1, 1, 1, 0)
    p = Plan(lib, 511, last_sliced=1, busy=True, calls=5)  # a small call is not asked
    assert (p.behind_sliced, p.busy_asked, p.dual, p.rotate, p.par) == (0, 0, 1, 1, 0)
    p = Plan(lib, 870, last_sliced=1, busy=True, knobs={"BBP_ROTATE_MIXED_FROM": "0"})
    assert (p.behind_sliced, p.busy_asked, p.rotate) == (0, 0, 1)
    assert Plan(lib, 870, last_sliced=0, busy=True).busy_asked == 0           # the last call rotated
    p = Plan(lib, 1024, last_sliced=1, busy=True, inflight=3)                  # a deep call is not asked either
    assert (p.deep, p.busy_asked, p.behind_sliced) == (1, 0, 0)


def test_slice_counts(lib):
    p = Plan(lib, 200, knobs={"BBP_ROTATE_BELOW": "0"})  # would be three slices; two opening streams leave room for two
    assert (p.dual, p.rotate, p.heavy_stream, p.slices, p.bounds) == (1, 0, 0, 2, [0, 100, 200])
    p = Plan(lib, 127, knobs={"BBP_ROTATE_BELOW": "0"})
    assert (p.dual, p.rotate, p.slices, p.bounds) == (1, 0, 1, [0, 127])
    # four slices from 256 proofs; below 1024 only with one opening stream (two cap the slices at two)
    four = {"BBP_SLICES": "4", "BBP_DUAL_OPEN_BELOW": "0"}
    p = Plan(lib, 255, knobs=four)
    assert (p.dual, p.rotate, p.slices, p.bounds) == (0, 0, 2, [0, 127, 255])
    p = Plan(lib, 256, knobs=four)
    assert (p.dual, p.rotate, p.slices, p.bounds) == (0, 0, 4, [0, 64, 128, 192, 256])
    p = Plan(lib, 256, knobs={"BBP_SLICES": "4", "BBP_ROTATE_BELOW": "0"})
    assert (p.dual, p.slices) == (1, 2)
    assert Plan(lib, 4096, knobs={"BBP_SLICES": "4"}).bounds == [0, 1024, 2048, 3072, 4096]


# the knob sets of test_engine_schedules_give_identical_bytes, by position, at its B = 261: what differs from the default plan
# (dual, rotating, half-word chain on 256-thread workgroups doubled to 512, prefix form 1, tail from round 7)
DEFAULT_261 = dict(dual=1, rotate=1, slices=0, coop=1, chain=HALFWORD, prefix_form=1, cblk=256, cblk_wave=512, serial_blk=64, tail_from=7, stagger_after=0)
ENGINE_SETS = [
    dict(tail_from=12), dict(), dict(serial_blk=256), dict(stagger_after=1), dict(dual=0, rotate=0, slices=3), dict(),
    dict(coop=0, chain=SERIAL, prefix_form=0), dict(cblk=64, cblk_wave=128), dict(cblk=1024, cblk_wave=1024), dict(),
    dict(chain=WORD), dict(chain=WORD, cblk=64, cblk_wave=128), dict(chain=LANES25), dict(chain=LANES25, cblk=64, cblk_wave=128), dict(), dict(), dict(),
]
NOT_PROVE_KNOBS = ("BBP_VARBASE_LANES", "BBP_VERIFY_OVERLAP", "BBP_FOLD_HALF_FROM")  # the verifier's and the MSM's own


def test_knob_sets_of_the_engine_schedule_test(lib):
    from tests import test_gpu_prove_verify as gpu
    sets = [m for m in gpu.test_engine_schedules_give_identical_bytes.pytestmark if m.name == "parametrize"][0].args[1]
    assert len(sets) == len(ENGINE_SETS)
    for knobs, diff in zip(sets, ENGINE_SETS):
        p = Plan(lib, 261, knobs={k: v for k, v in knobs.items() if k not in NOT_PROVE_KNOBS})
        assert {k: getattr(p, k) for k in DEFAULT_261} == {**DEFAULT_261, **diff}, knobs
    assert Plan(lib, 64, knobs={"BBP_TAIL_SMALL_BELOW": "0", "BBP_SLICES": "1"}).tail_from == 7  # (what that set changes: small heavy stages)
    assert Plan(lib, 261, knobs={"BBP_SERIAL_LDS": "0", "BBP_SERIAL_BLOCK": "256"}).serial_blk == 64  # not fenced: plain 64-thread workgroups


@pytest.mark.parametrize("name,member,cases", [
    ("BBP_ROTATE_DEEP_FROM", "deep_from", {"0": 2, "1": 2, "2": 2, "5": 5}),
    ("BBP_TAIL_ROUND", "tail_round", {"7": FOLD_ROUND, "12": 12, "6": 12, "0": 12}),
    ("BBP_SERIAL_BLOCK", "serial_block", {"64": 64, "128": 128, "256": 256, "100": 256, "0": 256}),
    ("BBP_SERIAL_LDS", "serial_lds", {"-5": 0, "0": 0, "4096": 4096, "163840": 163840, "200000": 163840}),
    ("BBP_SLICES", "slices", {"0": 1, "1": 1, "2": 2, "4": 4, "9": 4}),
    ("BBP_RNG_BLOCK", "rng_block", {"0": 64, "100": 64, "128": 128, "300": 256, "512": 512, "1023": 512, "4096": 1024}),
    ("BBP_RNG_COOP", "rng_coop", {"0": 0, "1": 1, "7": 1}),
    ("BBP_TRACE_PROVE", "trace_prove", {"1": 1, "0": 1, "": 1}),
    ("BBP_ROTATE_BELOW", "rotate_below", {"0": 0, "300": 300}),
])
def test_from_env_clamps(lib, name, member, cases):
    for text, want in cases.items():
        assert knob_from_env(lib, name, text, member) == want, (name, text)


def test_defaults_and_trace_line(lib):
    defaults = dict(slices=3, rotate_below=1023, rotate_deep_max=4096, deep_from=3, mixed_from=512, dual_open_below=1024, rng_coop=-1, rng_coop_below=768,
                    rng_coop_idle_below=2300, rng_dpp=2, rng_block=0, serial_block=64, serial_lds=163840, tr_wave_below=32, ipa_wide_below=32,
                    commit_split_below=1024, witness_native=1, tail_small_below=65, tail_round=7, stagger_mode=0, trace_prove=0)
    for member, want in defaults.items():
        assert knob_from_env(lib, "BBP_NOT_A_KNOB", "1", member) == want, member
    assert Plan(lib, 870, inflight=2, last_sliced=1, busy=True, calls=41).trace == \
        "prove call 41: B 870 inflight 2 deep 0 behind_sliced 1 dual 0 rotate 0 par 1 coop 0\n"
    assert Plan(lib, 33, calls=13).trace == "prove call 13: B 33 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 3 coop 1\n"
