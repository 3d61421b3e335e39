"""The filter envelope without a device: tests/fenv_model.py against a plain per-voice loop that steps 64 frames at a time, the three
block cuttings, the release arriving in every stage, stages that land at once and chain, relative levels on a tracked base under a
bend, clamps and withheld records, the pedal scene (and its failure on a model that does not read the release clock), the clear rule
(and its failure without it), and every refusal with its return code through tests/c_fenv_host.c, a program of its own built with
skred_amd/csrc/skred_bank_fenv.c under -fsanitize=address,undefined.  Nothing loaded into Python runs under a sanitizer.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import bend_model as BM
import chan_model as CHM
import cutoff_model as M
import fenv_model as FM
import owner_model as OM
import owner_scenes as OS
import pedal_model as PM
from skred_amd import device

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
f32 = np.float32
QM = M.SET_Q | M.SET_MODE
SYMBOLS = ("skred_bank_fenv_match", "skred_bank_fenv_owned_each", "skred_bank_fenv_tags_each", "skred_bank_download_fenv")
B = M.bits


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    L = device.load()
    for s in SYMBOLS + ("skred_fenv_check",):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in device.ABI_SYMBOLS + device.HOST_ABI_SYMBOLS
    assert "filter envelope" in text and "ENTERING A STAGE" in text and "WHO ENDS AN ENVELOPE" in text and "THE STATED PROPERTY" in text
    assert (device.FENV_ABS, device.FENV_REL, device.FENV_START) == (FM.ABS, FM.REL, FM.START)
    assert C_sizeof_fenv() == 32


def C_sizeof_fenv():
    import ctypes
    return ctypes.sizeof(device.FenvC)


# ---------------------------------------------------------------------------------------------- the model against a plain loop

def bank(n, w=None, q=0.9, mode=1):
    """n voices that all have a cutoff word (w: one value or an array)"""
    cut, filt = M.new(n), np.zeros(n, [(c, f32) for c in M.COEFFS])
    cut[:, M.W] = B(np.broadcast_to(np.asarray(0.1 if w is None else w, f32), (n,)))
    cut[:, M.Q], cut[:, M.MODE] = B(f32(q)), mode
    M.store(filt, np.arange(n), M.coeffs(cut[:, M.MODE], M.flt(cut[:, M.W]), M.flt(cut[:, M.Q])))
    return cut, FM.new(n), filt, np.zeros(n, np.uint64)


def brute_voice_step(s):
    """one 64-frame step of one voice: s = dict(stage, w, target, rate, peak, sus, end, ra, rd, rr), floats; returns arrived"""
    if s["target"] == 0.0:
        return False
    up = s["w"] < s["target"]
    s["w"] = f32(s["w"] * s["rate"])
    if not ((up and s["w"] >= s["target"]) or (not up and s["w"] <= s["target"])):
        return False
    s["w"] = s["target"]
    brute_next(s)
    return True


def brute_aim(s, stage, level, rate):
    if s["w"] == level or (rate > 1 and s["w"] > level) or (rate < 1 and s["w"] < level):
        s["w"] = level
        return False
    s["stage"], s["target"], s["rate"] = stage, level, rate
    return True


def brute_next(s):
    """the stage behind the one that just landed"""
    if s["stage"] == 1 and brute_aim(s, 2, s["sus"], s["rd"]):
        return
    if s["stage"] in (1, 2):
        s["stage"], s["target"], s["rate"] = 3, f32(0), f32(0)
        return
    s["stage"], s["target"], s["rate"] = 0, f32(0), f32(0)           # behind the release


def brute_advance(cut, fenv, release, filt, first, count, frames):
    res = [0, 0]
    for v in range(first, first + count):
        if fenv[v, 0] == 0:
            c, f = cut[v:v + 1].copy(), filt[v:v + 1].copy()
            r = M.advance(c, f, 0, 1, frames)                        # (cutoff_model has its own plain loop in tests/test_cutoff_cpu.py)
            cut[v], filt[v] = c[0], f[0]
            res = [res[0] + r[0], res[1] + r[1]]
            continue
        fl = M.flt(fenv[v])
        s = dict(stage=int(fenv[v, 0]), w=M.flt(cut[v, M.W]), target=M.flt(cut[v, M.TARGET]), rate=M.flt(cut[v, M.RATE_UP]), peak=fl[1], sus=fl[2],
                 end=fl[3], ra=fl[4], rd=fl[5], rr=fl[6])
        moving, arrived, entered = s["target"] != 0, False, False
        if release[v] != 0 and s["stage"] in (1, 2, 3):
            entered = True
            w0 = s["w"]
            if not brute_aim(s, 4, s["end"], s["rr"]):
                s["stage"], s["target"], s["rate"] = 0, f32(0), f32(0)
                arrived = True
            assert s["w"] == w0 or arrived
        total = int(cut[v, M.CARRY]) + frames
        for _ in range(total // 64):
            arrived |= brute_voice_step(s)
        cut[v, :4] = [B(s["w"]), B(s["target"]) if s["target"] else 0, B(s["rate"]) if s["rate"] else 0, B(s["rate"]) if s["rate"] else 0]
        cut[v, M.CARRY] = total % 64 if s["stage"] else 0
        if s["stage"]:
            fenv[v, 0] = s["stage"]
        else:
            fenv[v] = 0
        if moving or entered:
            M.store(filt, [v], M.coeffs(cut[v, M.MODE], M.flt(cut[v, M.W]), M.flt(cut[v, M.Q])).reshape(5, 1))
        res[0] += s["target"] != 0
        res[1] += arrived
    return [int(res[0]), int(res[1])]


def contours(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        up, down = f32(rng.uniform(1.02, 2.5)), f32(rng.uniform(0.4, 0.98))
        kind = k % 5
        if kind == 0:
            out.append(FM.Rec(FM.ABS, 2.0, 0.5, 0.05, up, down, down))
        elif kind == 1:
            out.append(FM.Rec(FM.REL | FM.START, 8.0, 2.0, 1.0, up, down, down, start=0.5))
        elif kind == 2:
            out.append(FM.Rec(FM.ABS | FM.START, 0.02, 0.3, 1.5, down, up, up, start=1.0))     # a contour upside down
        elif kind == 3:
            out.append(FM.Rec(FM.REL, 1e4, 1e-4, 1.0, 16.0, 1.0 / 16.0, 2.0))                  # clamped both ways, the fastest rates
        else:
            out.append(FM.Rec(FM.ABS, 1.0, 1.0, 1.0, up, up, down))                            # peak == sustain: the decay lands at once
    return out


def test_model_against_a_plain_loop():
    n = 240
    rng = np.random.default_rng(5)
    cut, fenv, filt, release = bank(n, rng.uniform(0.01, 2.5, n).astype(f32))
    cut[3::11, M.TARGET], cut[3::11, M.RATE_UP], cut[3::11, M.RATE_DOWN] = B(f32(1.0)), B(f32(1.1)), B(f32(0.9))   # plain sweeps beside the contours
    cut[::17] = 0                                                    # voices without a cutoff word
    recs = contours(n, 6)
    enveloped = np.flatnonzero(np.arange(n) % 3 != 0)
    started = withheld = 0
    for v in enveloped:
        a = FM.apply(cut, fenv, filt, [v], recs[v])
        started, withheld = started + a[0], withheld + a[1]
    assert started > 100 and withheld > 5 and (fenv[:, 0] == 3).any() and (fenv[:, 0] == 1).any() and (fenv[:, 0] == 2).any()
    moved, stages = [0, 0], set()
    for step, frames in enumerate([64, 37, 200, 64, 1, 26, 128, 64, 640, 64, 64, 4096, 65536]):
        if step == 3:
            release[enveloped[::4]] = 1000                           # note-offs while some attack, some decay, some rest
        if step == 7:
            release[enveloped[1::4]] = 2000
        if step == 10:
            release[:] = 3000
        ca, cb, ea, eb, fa, fb = cut.copy(), cut.copy(), fenv.copy(), fenv.copy(), filt.copy(), filt.copy()
        got = FM.advance(ca, ea, release, fa, 0, n, frames)
        want = brute_advance(cb, eb, release, fb, 0, n, frames)
        assert got == want and ca.tobytes() == cb.tobytes() and ea.tobytes() == eb.tobytes() and fa.tobytes() == fb.tobytes(), (step, got, want)
        cut, fenv, filt = ca, ea, fa
        moved = [x + y for x, y in zip(moved, got)]
        stages |= set(fenv[:, 0].tolist())
        assert (fenv[fenv[:, 0] == 0] == 0).all() and (cut[:, M.CARRY] < 64).all()
    assert all(moved) and stages == {0, 1, 2, 3, 4}, (moved, stages)
    assert not fenv.any() and not cut[enveloped, M.TARGET].any(), "every contour ended behind its release"
    w = M.flt(cut[cut[:, M.W] != 0, M.W])
    assert (w >= M.W_MIN).all() and (w <= M.W_MAX).all()


# ---------------------------------------------------------------------------------------------- cuttings

CUTTINGS = [(64,) * 24, (512, 1024), (100, 412, 300, 724)]


def performance(cutting, read_clock=True):
    """a record at frame 0, a note-off at frame 512 (a block cut in every cutting), 1536 frames in all: w at every multiple of 64"""
    cut, fenv, filt, release = bank(8, np.linspace(0.02, 0.2, 8).astype(f32))
    FM.apply(cut, fenv, filt, range(8), FM.Rec(FM.REL, 9.0, 3.0, 0.5, 1.3, 0.91, 0.8))
    at, seen = 0, {}
    for f in cutting:
        if at == 512:
            release[:] = 512
        FM.advance(cut, fenv, release, filt, 0, 8, f)
        at += f
        if at % 64 == 0:
            seen[at] = (cut.copy(), fenv.copy(), filt.copy())
    return seen


def test_three_block_cuttings_agree_at_every_common_multiple_of_64():
    states = [performance(c) for c in CUTTINGS]
    assert len(states[0]) == 24 and set(states[1]) == {512, 1536} and set(states[2]) == {512, 1536}
    for other in states[1:]:
        for at, got in other.items():
            for x, y in zip(got, states[0][at]):
                assert x.tobytes() == y.tobytes(), at
    stages = [set(states[0][at][1][:, 0].tolist()) for at in sorted(states[0])]
    assert {1} in stages and {4} in stages and stages[-1] == {0}, stages
    # the release did not start on a fresh grid: w at 576 is ONE step below w at 512 -- and the carry ran on through the cut at 100 + 412
    c512, c576 = states[0][512][0], states[0][576][0]
    assert (c576[:, M.W] == B(M.flt(c512[:, M.W]) * f32(0.8))).all() or (states[0][512][1][:, 0] != 3).any()


# ---------------------------------------------------------------------------------------------- the release in every stage

@pytest.mark.parametrize("during,blocks", [("attack", 2), ("decay", 8), ("sustain", 40)])
def test_release_arrives_during(during, blocks):
    cut, fenv, filt, release = bank(2, 0.1)
    rec = FM.Rec(FM.ABS, 1.6, 0.4, 0.05, 2.0, 0.75, 0.5)
    assert FM.apply(cut, fenv, filt, [0, 1], rec) == [2, 0, 0]
    for _ in range(blocks):
        FM.advance(cut, fenv, release, filt, 0, 2, 64)
    assert fenv[0, 0] == {"attack": 1, "decay": 2, "sustain": 3}[during], fenv[0]
    w_before = cut[0, M.W]
    release[0] = 77                                                   # voice 1 is the twin whose key stays down
    res = FM.advance(cut, fenv, release, filt, 0, 2, 64)
    assert fenv[0, 0] == 4 and cut[0, M.TARGET] == B(f32(0.05)) and cut[0, M.RATE_UP] == cut[0, M.RATE_DOWN] == B(f32(0.5))
    assert cut[0, M.W] == B(M.flt(w_before) * f32(0.5)), "the release's first step is taken in the pass that sees the clock"
    assert res[0] == 1 + int(fenv[1, 0] != 3)                         # (the twin moves on by itself)
    for _ in range(12):
        res = FM.advance(cut, fenv, release, filt, 0, 2, 64)
    assert not fenv[0].any() and cut[0].tolist() == [int(B(f32(0.05))), 0, 0, 0, 0, int(B(f32(0.9))), 1, 0]
    assert filt[0].tobytes() == M.coeffs(1, [f32(0.05)], [f32(0.9)])[:, 0].tobytes(), "a landed release is a voice set with ABS at w_end"
    assert fenv[1, 0] == 3 and cut[1, M.W] == B(f32(0.4)) and res == [0, 0]
    # a trigger stamp alone restarts nothing: the clock back at 0, the ended contour stays ended, the resting one rests
    release[:] = 0
    assert FM.advance(cut, fenv, release, filt, 0, 2, 64) == [0, 0] and not fenv[0].any() and fenv[1, 0] == 3


def test_a_trigger_stamp_does_not_restart_a_releasing_contour():
    cut, fenv, filt, release = bank(1, 1.0)
    FM.apply(cut, fenv, filt, [0], FM.Rec(FM.ABS, 2.0, 1.5, 0.01, 1.5, 0.9, 0.9))
    release[0] = 5
    FM.advance(cut, fenv, release, filt, 0, 1, 64)
    assert fenv[0, 0] == 4
    release[0] = 0                                                    # struck again without a new record
    w = cut[0, M.W]
    FM.advance(cut, fenv, release, filt, 0, 1, 64)
    assert fenv[0, 0] == 4 and cut[0, M.W] == B(M.flt(w) * f32(0.9))


# ---------------------------------------------------------------------------------------------- landing at once, chains

def test_stages_that_land_at_once_chain_at_the_record():
    cut, fenv, filt, release = bank(6, 0.5)
    before = filt.copy()
    # voice 0: already at the peak -> decay.  1: above the peak with a rising attack -> w = peak, decay.  2: peak == sustain -> sustain at
    # once.  3: a falling "attack" from below -> lands, decay rate points away too -> sustain.  4: nothing lands.  5: START moves w.
    FM.apply(cut, fenv, filt, [0], FM.Rec(FM.ABS, 0.5, 0.2, 0.1, 1.5, 0.9, 0.8))
    FM.apply(cut, fenv, filt, [1], FM.Rec(FM.ABS, 0.25, 0.2, 0.1, 1.5, 0.9, 0.8))
    FM.apply(cut, fenv, filt, [2], FM.Rec(FM.ABS, 0.5, 0.5, 0.1, 1.5, 0.9, 0.8))
    FM.apply(cut, fenv, filt, [3], FM.Rec(FM.ABS, 1.0, 2.0, 0.1, 0.9, 0.9, 0.8))
    FM.apply(cut, fenv, filt, [4], FM.Rec(FM.ABS, 1.0, 0.2, 0.1, 1.5, 0.9, 0.8))
    FM.apply(cut, fenv, filt, [5], FM.Rec(FM.ABS | FM.START, 1.0, 0.2, 0.1, 1.5, 0.9, 0.8, start=0.125))
    assert fenv[:, 0].tolist() == [2, 2, 3, 3, 1, 1]
    assert cut[:, M.W].tolist() == [int(B(f32(x))) for x in (0.5, 0.25, 0.5, 2.0, 0.5, 0.125)]
    assert cut[:, M.TARGET].tolist() == [int(B(f32(0.2))), int(B(f32(0.2))), 0, 0, int(B(f32(1.0))), int(B(f32(1.0)))]
    assert cut[2, M.RATE_UP] == 0 and cut[0, M.RATE_UP] == cut[0, M.RATE_DOWN] == B(f32(0.9))
    same = [0, 2, 4]                                                  # w did not change: the coefficients were not computed
    assert filt[same].tobytes() == before[same].tobytes()
    for v in (1, 3, 5):
        assert filt[v].tobytes() == M.coeffs(1, M.flt(cut[v:v + 1, M.W]), [f32(0.9)])[:, 0].tobytes() != before[v].tobytes()
    assert FM.advance(cut, fenv, release, filt, 0, 6, 64) == [4, 0]


def test_stages_chain_inside_an_advance_and_count_once():
    cut, fenv, filt, release = bank(3, 0.5)
    # voice 0: attack, decay and release all land inside ONE pass of 8 steps; 1: the attack lands and the decay (peak == sustain) lands
    # at once; 2: released while it rests, w == w_end: the release lands at once and the contour ends without a step
    FM.apply(cut, fenv, filt, [0], FM.Rec(FM.ABS, 2.0, 1.0, 0.25, 2.0, 0.5, 0.5))
    FM.apply(cut, fenv, filt, [1], FM.Rec(FM.ABS, 1.0, 1.0, 0.25, 2.0, 0.5, 0.5))
    FM.apply(cut, fenv, filt, [2], FM.Rec(FM.ABS, 0.5, 0.5, 0.5, 2.0, 0.5, 0.5))
    assert fenv[:, 0].tolist() == [1, 1, 3]
    release[0], release[2] = 9, 9
    cut2, fenv2, filt2 = cut.copy(), fenv.copy(), filt.copy()
    assert FM.advance(cut, fenv, release, filt, 0, 3, 512) == [0, 3], "three voices arrived, each counted once"
    assert not fenv[0].any() and cut[0, M.W] == B(f32(0.25)) and not cut[0, 1:5].any()
    assert fenv[1, 0] == 3 and cut[1, M.W] == B(f32(1.0)) and cut[1, M.CARRY] == 0
    assert not fenv[2].any() and cut[2, M.W] == B(f32(0.5))
    # one step is enough for all three: voice 0 is released first (the clock is read ahead of the steps), so its attack never runs
    # and 0.5 -> 0.25 is one step of the release; voice 1's attack 0.5 -> 1.0 is one step too
    assert FM.advance(cut2, fenv2, release, filt2, 0, 3, 64) == [0, 3]
    assert cut2.tobytes() == cut.tobytes() and fenv2.tobytes() == fenv.tobytes() and filt2.tobytes() == filt.tobytes()


# ---------------------------------------------------------------------------------------------- relative levels on a tracked base

def test_relative_levels_on_a_tracked_base_under_a_bend():
    n = 4
    cut, fenv, filt, release = M.new(n), FM.new(n), np.zeros(n, [(c, f32) for c in M.COEFFS]), np.zeros(n, np.uint64)
    owner = OM.new(n)
    owner[:] = 5
    key = np.array([0.01, 0.02, 0.04, 0.08], f32)
    inc, bend = key.copy(), BM.new(n)
    BM.apply(bend, inc, [1, 3], B(f32(1.5)))                          # voices 1, 3 bent: the sounding increment is key * 1.5
    assert M.cutoff_match(owner, cut, bend, inc, filt, 0, n, 1, 1, (0, 0), M.Rec(M.TRACK | QM, 4.0, 0.9, 1)) == [n, 0, 0, 0]
    assert (cut[:, M.W] == B(key * f32(4.0))).all(), "the base tracks the key, not the wheel"
    base = M.flt(cut[:, M.W]).copy()
    assert FM.fenv_match(owner, cut, fenv, filt, 0, n, 1, 1, (0, 0), FM.Rec(FM.REL, 8.0, 2.0, 1.0, 1.4, 0.9, 0.8)) == [n, 0, 0, 0]
    assert (fenv[:, FM.W_PEAK] == B(base * f32(8.0))).all() and (fenv[:, FM.W_SUSTAIN] == B(base * f32(2.0))).all()
    assert (fenv[:, FM.W_END] == cut[:, M.W]).all() and len(set(fenv[:, FM.W_PEAK].tolist())) == n, "a tracked base gives a tracked contour"
    for _ in range(60):
        FM.advance(cut, fenv, release, filt, 0, n, 64)
    assert (fenv[:, 0] == 3).all() and (cut[:, M.W] == B(base * f32(2.0))).all()
    release[:] = 1
    for _ in range(8):
        FM.advance(cut, fenv, release, filt, 0, n, 64)
    assert not fenv.any() and (cut[:, M.W] == B(base)).all(), "the release closes to the base's bits"


# ---------------------------------------------------------------------------------------------- clamps, withheld records

def test_clamps_and_withheld_records_are_counted():
    cut, fenv, filt, release = bank(6, [0.001, 0.1, 2.9, 0.1, 0.1, 0.1])
    cut[4] = 0
    owner = OM.new(6)
    owner[:] = 5
    owner[5] = 0
    before_c, before_f = cut.copy(), filt.copy()
    res = FM.fenv_match(owner, cut, fenv, filt, 0, 6, 1, 1, (0, 0), FM.Rec(FM.REL | FM.START, 4.0, 2.0, 1.0, 1.5, 0.9, 0.8, start=0.5))
    assert res == [4, 1, 1, 2], res                                   # voice 4 withheld, slot 5 untagged; voices 0 and 2 clamped, counted ONCE each
    assert cut[0, M.W] == B(M.W_MIN) and fenv[2, FM.W_PEAK] == fenv[2, FM.W_SUSTAIN] == B(M.W_MAX)   # 0.0005 up to the floor; 11.6 and 5.8 down to 3
    assert not fenv[4:].any() and cut[4:].tobytes() == before_c[4:].tobytes() and filt[4:].tobytes() == before_f[4:].tobytes()
    # without START the start level is neither computed nor clamped
    cut, fenv, filt, release = bank(1, 0.001)
    assert FM.apply(cut, fenv, filt, [0], FM.Rec(FM.REL, 4.0, 2.0, 1.5, 1.5, 0.9, 0.8)) == [1, 0, 0]
    # a record on a moving voice ends the movement; a new record restarts a contour
    cut, fenv, filt, release = bank(1, 0.1)
    cut[0, M.TARGET], cut[0, M.RATE_UP], cut[0, M.RATE_DOWN], cut[0, M.CARRY] = B(f32(2.0)), B(f32(1.1)), B(f32(0.9)), 33
    FM.apply(cut, fenv, filt, [0], FM.Rec(FM.ABS, 1.0, 0.5, 0.1, 1.5, 0.9, 0.8))
    assert cut[0, 1:5].tolist() == [int(B(f32(1.0))), int(B(f32(1.5))), int(B(f32(1.5))), 0]
    FM.advance(cut, fenv, release, filt, 0, 1, 100)
    assert cut[0, M.CARRY] == 36
    FM.apply(cut, fenv, filt, [0], FM.Rec(FM.ABS, 2.0, 0.5, 0.1, 1.25, 0.9, 0.8))
    assert cut[0, M.CARRY] == 0 and fenv[0, 0] == 1 and cut[0, M.TARGET] == B(f32(2.0))


def test_a_cutoff_call_ends_the_contour():
    cut, fenv, filt, release = bank(4, 0.1)
    owner = OM.new(4)
    owner[:] = 5
    inc = np.full(4, 0.01, f32)
    FM.apply(cut, fenv, filt, range(4), FM.Rec(FM.ABS, 1.0, 0.5, 0.1, 1.5, 0.9, 0.8))
    with FM.cutoff_ends(fenv):
        assert M.cutoff_match(owner, cut, None, inc, filt, 0, 1, 1, 1, (0, 0), M.Rec(M.ABS, 0.3)) == [1, 0, 0, 0]
        assert M.cutoff_match(owner, cut, None, inc, filt, 1, 1, 1, 1, (0, 0), M.Rec(M.ABS | M.GLIDE, 2.0, rate_up=1.2, rate_down=0.8)) == [1, 0, 0, 0]
        inc[2] = 0
        assert M.cutoff_match(owner, cut, None, inc, filt, 2, 1, 1, 1, (0, 0), M.Rec(M.TRACK, 3.0)) == [0, 1, 0, 0]   # withheld: the contour stays
    assert fenv[:, 0].tolist() == [0, 0, 1, 1] and not fenv[:2].any()
    assert cut[0, 1:5].tolist() == [0, 0, 0, 0] and cut[1, M.RATE_DOWN] == B(f32(0.8))
    FM.stop(cut, fenv, filt, 2, 2, True)
    assert not fenv.any() and (cut[2:, M.W] == B(f32(1.0))).all() and not cut[2:, 1:5].any()
    assert M.apply.__module__ == "cutoff_model"


# ---------------------------------------------------------------------------------------------- the pedal scene

def pedal_scene():
    """tests/owner_scenes.py's bank with its carriers filtered.  A key with a contour; its note-off is held back by the sustain pedal:
    the contour stays in sustain until pedal_up stamps the release clock, and releases in the pass behind that stamp."""
    from test_cutoff_cpu import filtered
    K, N = OS.K, OS.N
    bank_, tables, g = OS.bank()
    filtered(bank_, K, OS.MEMBERS)
    st = PM.Stage(bank_, tables, g, K, OS.MMASK)
    cut, fenv = M.new(N), FM.new(N)
    slot = int(OS.others()[5])
    vs = slot + np.array(OS.MEMBERS)
    tag = PM.tag_of(3, 60)
    assert st.strike([slot], [tag]) == [1, 0]
    FM.tag_clear(fenv, [slot], 1, None, K)
    filt, inc = st.truth["voice_filter"], st.truth["voice_phase_inc"]

    def rel():
        return st.truth["voice_amp_envelope"]["sample_release"]

    assert M.cutoff_tags_each(st.owner, cut, None, inc, filt, [M.Rec(M.TRACK | QM, M.track_value(4.0, 4096), 1.1, 1)], 0, N, K, OS.MMASK, [tag])[0][0] == 3
    assert FM.fenv_tags_each(st.owner, cut, fenv, filt, [FM.Rec(FM.REL, 6.0, 2.0, 1.0, 2.0, 0.7, 0.6)], 0, N, K, OS.MMASK, [tag])[0] == [3, 0, 0, 0]
    base = cut[vs, M.W].copy()
    log = []

    def block():
        log.append(FM.advance(cut, fenv, rel(), filt, 0, N, OS.F))
        st.block()

    for _ in range(10):
        block()
    assert (fenv[vs, 0] == 3).all() and log[-1] == [0, 0]
    assert st.off([tag], True) == [0, 0, 0, 1] and st.release_clock(slot) == 0       # the note-off is held back
    for _ in range(3):
        block()
    assert (fenv[vs, 0] == 3).all(), "the pedal holds the note: the contour rests in sustain"   # READ THE CLOCK: passes either way
    assert st.up(CHM.channel(3), PM.LIFT_SUSTAIN)[:2] == [1, 0] and st.release_clock(slot) == st.now()
    block()
    assert (fenv[vs, 0] == 4).all() and log[-1] == [3, 0], "the pass behind the pedal-up enters the release"   # READ THE CLOCK
    for _ in range(6):
        block()
    assert not fenv.any() and (cut[vs, M.W] == base).all()           # READ THE CLOCK
    return cut, fenv, filt.copy()


def test_a_note_off_held_by_the_sustain_pedal_keeps_stage_3_until_the_pedal_up_stamps():
    pedal_scene()


def test_the_pedal_scene_fails_on_a_model_that_does_not_read_the_release_clock():
    FM.READ_RELEASE_CLOCK = False
    try:
        with pytest.raises(AssertionError, match="enters the release"):
            pedal_scene()
    finally:
        FM.READ_RELEASE_CLOCK = True


# ---------------------------------------------------------------------------------------------- the clear rule

def test_a_thief_and_a_restruck_key_inherit_no_contour():
    """Two scenes on the model; each marked assertion fails with fenv_model.CLEAR_RULE = False."""
    K, n = 4, 32
    filt = np.zeros(n, [(c, f32) for c in M.COEFFS])
    inc = np.full(n, 0.02, f32)
    owner, cut, fenv, release = OM.new(n), M.new(n), FM.new(n), np.zeros(n, np.uint64)
    contour = FM.Rec(FM.ABS, 2.0, 0.5, 0.05, 1.2, 0.9, 0.8)
    for scene, new_tag in (("a re-struck key", 60), ("a thief", 99)):
        slot = 8 if scene == "a thief" else 16
        OM.tag_slots(owner, [slot], [60], None, K)
        M.tag_clear(cut, [slot], 1, None, K)
        FM.tag_clear(fenv, [slot], 1, None, K)
        assert M.cutoff_tags_each(owner, cut, None, inc, filt, [M.Rec(M.ABS | QM, 0.1, 0.9, 1)], 0, n, K, 0xF, [60])[0] == [K, 0, 0, 0]
        assert FM.fenv_tags_each(owner, cut, fenv, filt, [contour], 0, n, K, 0xF, [60])[0] == [K, 0, 0, 0]
        assert FM.advance(cut, fenv, release, filt, 0, n, 64) == [K, 0]
        held = filt[slot:slot + K].copy()
        OM.tag_slots(owner, [slot], [new_tag], None, K)              # the new note's tag launch
        M.tag_clear(cut, [slot], 1, None, K)
        FM.tag_clear(fenv, [slot], 1, None, K)
        assert not fenv[slot:slot + K].any(), scene                  # CLEAR RULE
        # the new note gets its own base cutoff; the old contour must not pick it up and run on with it
        assert M.cutoff_tags_each(owner, cut, None, inc, filt, [M.Rec(M.ABS | QM, 0.3, 0.9, 1)], 0, n, K, 0xF, [new_tag])[0] == [K, 0, 0, 0]
        held = filt[slot:slot + K].copy()
        assert FM.advance(cut, fenv, release, filt, 0, n, 64) == [0, 0], scene   # (the cutoff clear alone gives this)
        release[slot:slot + K] = 5
        assert FM.advance(cut, fenv, release, filt, 0, n, 64) == [0, 0], scene   # CLEAR RULE: the victim's release would start on the new note
        assert filt[slot:slot + K].tobytes() == held.tobytes() and (cut[slot:slot + K, M.W] == B(f32(0.3))).all(), scene   # CLEAR RULE
        release[:] = 0
        OM.clear(owner, slot, K)
        cut[slot:slot + K] = 0
        fenv[slot:slot + K] = 0


def test_the_scenes_fail_without_the_clear_rule():
    FM.CLEAR_RULE = False
    try:
        with pytest.raises(AssertionError):
            test_a_thief_and_a_restruck_key_inherit_no_contour()
    finally:
        FM.CLEAR_RULE = True


# ---------------------------------------------------------------------------------------------- the entry points' host checks

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    """tests/c_fenv_host.c with skred_bank_fenv.c, a program of its own, under ASan and UBSan (the command in the file's header)"""
    exe = str(tmp_path_factory.mktemp("fenv") / "c_fenv_host_san")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-g", "-Wall", "-Werror", "-std=gnu11", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"), os.path.join(HERE, "c_fenv_host.c"),
           os.path.join(CSRC, "skred_bank_fenv.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"), "-lskred_amd", "-L" + os.path.join(rocm, "lib"),
           "-lamdhip64", "-lm", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "skred_amd"), "-Wl,-rpath," + os.path.join(rocm, "lib")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-1500:]
    return out.stdout.strip().splitlines()


def test_host_program(host_lines):
    bad = [l for l in host_lines[:-1] if not l.endswith(" ok")]
    assert not bad, bad
    assert host_lines[-1] == "OK" and len(host_lines) >= 90
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "check", "pack", "perm", "match", "owned", "tags", "download", "untouched"}, groups


def test_check_through_ctypes_is_the_models():
    ok = dict(peak=2.0, sustain=0.5, end=0.1, rate_attack=1.5, rate_decay=0.9, rate_release=0.8)

    def r(set, **kw):
        return FM.Rec(set, **{**ok, **kw})

    nan, inf = float("nan"), float("inf")
    cases = [([r(FM.ABS)], 8, 0x77, 0x55), (None, 8, 0x77, 0x55), ([r(FM.ABS)], 12, 0x77, 0x55), ([r(FM.ABS)], 8, 0, 0x55), ([r(FM.ABS)], 8, 0x77, 0),
             ([r(FM.ABS)], 8, 0x77, 0x155), ([r(FM.ABS)], 8, 0x11, 0x55), ([r(FM.ABS | FM.REL)], 8, 0x77, 0x55), ([r(0)], 8, 0x77, 0x55),
             ([r(FM.ABS | 8)], 8, 0x77, 0x55), ([r(FM.ABS, start=0.3)], 8, 0x77, 0x55), ([r(FM.ABS | FM.START, start=0.3)], 8, 0x77, 0x55),
             ([r(FM.ABS | FM.START)], 8, 0x77, 0x55), ([r(FM.REL | FM.START)], 8, 0x77, 0x55), ([r(FM.ABS, peak=nan)], 8, 0x77, 0x55),
             ([r(FM.ABS, sustain=inf)], 8, 0x77, 0x55), ([r(FM.REL, end=nan)], 8, 0x77, 0x55), ([r(FM.ABS, rate_decay=nan)], 8, 0x77, 0x55),
             ([r(FM.ABS, peak=3.5)], 8, 0x77, 0x55), ([r(FM.ABS, end=2.0 ** -11)], 8, 0x77, 0x55), ([r(FM.REL, peak=3.5, sustain=1e-9)], 8, 0x77, 0x55),
             ([r(FM.REL, sustain=0.0)], 8, 0x77, 0x55), ([r(FM.REL, end=-1.0)], 8, 0x77, 0x55), ([r(FM.ABS, rate_attack=17.0)], 8, 0x77, 0x55),
             ([r(FM.ABS, rate_release=0.01)], 8, 0x77, 0x55), ([r(FM.ABS, rate_attack=1.0)], 8, 0x77, 0x55), ([r(FM.ABS, rate_decay=1.0)], 8, 0x77, 0x55),
             ([r(FM.ABS, rate_release=1.0)], 8, 0x77, 0x55), ([r(FM.ABS, rate_attack=0.5, rate_decay=2.0, rate_release=2.0)], 8, 0x77, 0x55),
             ([r(FM.ABS, peak=9.0)], 8, 0x11, 0x55), ([r(FM.ABS | FM.REL, peak=9.0)], 3, 0, 0), ([r(FM.ABS), r(FM.REL), r(0)], 8, 0x77, 0x55)]
    seen = set()
    for recs, K, vm, fm in cases:
        got = device.fenv_check([x.c() for x in recs] if recs is not None else None, K, vm, fm)
        assert got == FM.check(recs, K, vm, fm), (K, vm, fm, recs and vars(recs[0]))
        seen.add(got)
    assert seen == {0, BAD, RANGE}
