"""The filter envelope of the fixed-point bank, without a GPU: the state machine of include/skred_amd_fxpt.h, section "filter envelope".

tests/fx_fenv_model.py (numpy, block by block) against a plain per-voice Python-int loop that knows no blocks; every width the header
states; the stage chains (a peak equal to the start, a sustain equal to the peak, an end equal to the sustain, a release that lands in
the pass that enters it); REL clamping at both ends of the box; THE STATED PROPERTY over three cuttings of one performance compared
pairwise at every common multiple of 64; the two switches of the model, which must bite; skred_fx_fenv_check's refusal order through
the built library; every refusal of the entry points (tests/c_fx_fenv_host.c, a program of its own).
"""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import fx_cutoff_model as M
import fx_fenv_model as FM
from skred_amd import fxbank as fxb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
SYMBOLS = ("skred_fxbank_fenv_match", "skred_fxbank_fenv_owned_each", "skred_fxbank_fenv_tags_each", "skred_fxbank_download_fenv")
R = FM.Rec
TOTAL = 64 * 48                                                  # frames of the performance the cuttings share
RELEASES = (64 * 7, 777, 1601, 64 * 40 + 63)                     # where its note-offs fall: on the grid, off it, one frame before it


def odd_cutting(total, gen):
    """odd block sizes from 1 to 200 that add up to `total`"""
    out = []
    while sum(out) < total:
        left = total - sum(out)
        x = min(left, int(gen.integers(0, 100)) * 2 + 1)
        out += [x] if x % 2 else [x - 1, 1]                           # (what is left of an even span, as two odd blocks)
    return out


def cuttings(total, events, seed=0):
    """three cuttings of `total` frames with a cut at every event: all 64-frame blocks, odd sizes from 1 to 200, one large block"""
    gen = np.random.default_rng(seed)
    marks = sorted(set(events) | {total})
    out = []
    for how in ("64", "odd", "one"):
        blocks, at = [], 0
        for m in marks:
            span = m - at
            if span <= 0:
                continue
            if how == "64":
                pos = at
                while pos < m:                                        # up to the next line of the 64-frame grid, or to the call
                    blocks.append(min(m - pos, 64 - pos % 64))
                    pos += blocks[-1]
            elif how == "odd":
                blocks += odd_cutting(span, gen)
            else:
                blocks.append(span)
            at = m
        assert sum(blocks) == total
        out.append(blocks)
    return out


class Bare:
    """the model's arrays without a bank: n voices resting at w0 with q and mode, a release clock, the five coefficient arrays"""

    def __init__(self, w0, q=3 << 15, mode=1):
        n = len(w0)
        self.cut, self.fenv = M.new(n), FM.new(n)
        self.cut[:, M.W], self.cut[:, M.Q], self.cut[:, M.MODE] = w0, q, mode
        self.release = np.zeros(n, np.uint64)
        self.filt = {name: np.zeros(n, np.int32) for name in M.COEFFS}
        for v in range(n):
            if w0[v]:                                                 # (0: a voice without a cutoff word)
                M.store(self.filt, v, M.coeffs(mode, int(w0[v]), q))

    def record(self, v, rec, widths=None):
        return FM.apply(self.cut, self.fenv, self.filt, [v], rec, widths)

    def advance(self, frames, widths=None):
        return FM.advance(self.cut, self.fenv, self.release, self.filt, 0, len(self.cut), frames, widths)

    def coeffs_are_w(self, v):
        return [int(self.filt[name][v]) for name in M.COEFFS] == M.coeffs(int(self.cut[v, M.MODE]), int(self.cut[v, M.W]), int(self.cut[v, M.Q]))


def contours(gen, n):
    """n random (w0, record) pairs: ABS and REL, with and without START, rates from crawling to a landing in one step"""
    out = []
    for k in range(n):
        w0 = int(np.exp2(gen.uniform(20, 30)))
        rates = [int(np.exp2(gen.uniform(18, 31.9))) for _ in range(3)]
        if k % 2:
            lv = [int(np.exp2(gen.uniform(12, 20))) for _ in range(4)]
            out.append((w0, R(FM.REL | (FM.START if k % 4 == 1 else 0), lv[1], lv[2], lv[3], *rates, start=lv[0] if k % 4 == 1 else 0)))
        else:
            lv = [int(np.exp2(gen.uniform(19.1, 30.4))) for _ in range(4)]
            out.append((w0, R(FM.ABS | (FM.START if k % 4 == 0 else 0), lv[1], lv[2], lv[3], *rates, start=lv[0] if k % 4 == 0 else 0)))
    return out


def run_cutting(pairs, release_at, blocks):
    """the records at frame 0, voice v released (its clock stamped) at frame release_at[v]; w at every multiple of 64 a block ends on"""
    b = Bare([w for w, _ in pairs])
    for v, (_, rec) in enumerate(pairs):
        assert b.record(v, rec)[0] == 1
    seen, t = {0: b.cut[:, M.W].copy()}, 0
    for frames in blocks:
        for v, at in enumerate(release_at):
            if at == t:
                b.release[v] = 1000 + t
        b.advance(frames)
        t += frames
        if t % 64 == 0:
            seen[t] = b.cut[:, M.W].copy()
    return seen, b


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd_fxpt.h")).read()
    L = fxb._bind(fxb.load())
    for s in SYMBOLS + ("skred_fx_fenv_check",):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in fxb.FX_ABI_SYMBOLS + fxb.FX_HOST_ABI_SYMBOLS
    for phrase in ("ENTERING A STAGE", "A RECORD ON VOICE v (skred_fx_fenv_t", "THE STATED PROPERTY", "WHO ENDS AN ENVELOPE", "BELOW 2^63", "DECIDED HERE"):
        assert phrase in text, phrase
    assert (fxb.FX_FENV_ABS, fxb.FX_FENV_REL, fxb.FX_FENV_START) == (FM.ABS, FM.REL, FM.START)
    assert (fxb.FX_FENV_OFF, fxb.FX_FENV_ATTACK, fxb.FX_FENV_DECAY, fxb.FX_FENV_SUSTAIN, fxb.FX_FENV_RELEASE) == tuple(range(5))
    assert "Not built: the fixed-point bank" not in open(os.path.join(ROOT, "include", "skred_amd.h")).read()


# ---------------------------------------------------------------------------------------------- the model against a plain loop

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_a_plain_loop_over_three_cuttings(seed):
    """48 voices, random contours, a release at one of four frames (on and off the 64-frame grid) for two thirds of them.  The model under each of
    the three cuttings equals the plain loop at every multiple of 64 it stops at, and the cuttings equal each other PAIRWISE at every
    common multiple of 64: THE STATED PROPERTY."""
    gen = np.random.default_rng(seed)
    pairs = contours(gen, 48)
    release_at = [int(gen.choice(RELEASES)) if v % 3 else None for v in range(len(pairs))]
    events = [t for t in release_at if t is not None]
    cuts = cuttings(TOTAL, events, seed)
    assert all(x == 64 or x < 64 for x in cuts[0]) and all(x % 2 == 1 and x <= 200 for x in cuts[1]) and max(cuts[2]) > 200
    runs = [run_cutting(pairs, release_at, blocks)[0] for blocks in cuts]
    for v, (w0, rec) in enumerate(pairs):
        plain, _ = FM.plain_loop(w0, 3 << 15, 1, rec, {release_at[v]: "release"} if release_at[v] is not None else {}, TOTAL)
        for seen in runs:
            for t, ws in seen.items():
                assert int(ws[v]) == plain[t], (v, t, int(ws[v]), plain[t])
    assert set(runs[0]) >= set(range(0, TOTAL + 1, 64)) - {0} and len(runs[2]) >= 2
    compared = 0
    for a, b in itertools.combinations(range(3), 2):
        common = sorted(set(runs[a]) & set(runs[b]))
        assert TOTAL in common
        for t in common:
            assert np.array_equal(runs[a][t], runs[b][t]), (a, b, t)
            compared += 1
    assert compared > 6


def test_the_final_state_does_not_depend_on_the_cutting_either():
    gen = np.random.default_rng(9)
    pairs = contours(gen, 32)
    release_at = [64 * 5 + 17 if v % 2 else None for v in range(32)]
    ends = [run_cutting(pairs, release_at, blocks)[1] for blocks in cuttings(TOTAL, [64 * 5 + 17], 4)]
    for b in ends[1:]:
        assert np.array_equal(b.cut, ends[0].cut) and np.array_equal(b.fenv, ends[0].fenv)
        for name in M.COEFFS:
            assert np.array_equal(b.filt[name], ends[0].filt[name]), name
    assert all(ends[0].coeffs_are_w(v) for v in range(32))


def test_every_width_the_header_states():
    """Random and extreme records and advances: every intermediate the header bounds stays inside the stated width, evaluated in
    unbounded integers."""
    widths = {}
    gen = np.random.default_rng(11)
    extremes = [(M.W_MAX, R(FM.REL | FM.START, 0xFFFFFFFF, 0xFFFFFFFF, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, start=0xFFFFFFFF)),
                (M.W_MIN, R(FM.REL, 1, 0xFFFFFFFF, 1, 1, 1, 1)),
                (M.W_MAX, R(FM.ABS, M.W_MIN, M.W_MAX, M.W_MIN, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)),
                (M.W_MAX - 1, R(FM.ABS, M.W_MAX, M.W_MIN, M.W_MAX, 0xFFFFFFFF, 1, 0xFFFFFFFF))]
    pairs = extremes + contours(gen, 60)
    b = Bare([w for w, _ in pairs])
    for v, (_, rec) in enumerate(pairs):
        b.record(v, rec, widths)
    b.cut[:, M.CARRY] = 63                                           # the largest carry an advance can meet
    b.advance(65536, widths)
    b.release[:] = 5
    for frames in (1, 63, 64, 65536):
        b.advance(frames, widths)
    assert set(widths) == set(FM.STATED_BITS), sorted(widths)
    for name, bits in FM.STATED_BITS.items():
        assert widths[name] < 1 << bits, (name, widths[name].bit_length(), bits)
    assert widths["w_now * value_q16"] >= 1 << 62 and widths["carry + F"] == 63 + 65536     # the bounds are reached, not just kept


# ---------------------------------------------------------------------------------------------- stage chains

def test_stage_chains():
    w, fast = 1 << 26, 0xFFFFFFFF
    b = Bare([w] * 6)
    # a peak equal to the start: the attack lands at once, the decay is entered
    assert b.record(0, R(FM.ABS, w, 1 << 24, 1 << 22, 5, 1 << 28, 7)) == [1, 0, 0]
    assert b.fenv[0].tolist() == [FM.DECAY, w, 1 << 24, 1 << 22, 5, 1 << 28, 7, 0] and b.cut[0, :5].tolist() == [w, 1 << 24, 1 << 28, 1 << 28, 0]
    # ... under START too, and the coefficients are computed from the start level
    assert b.record(1, R(FM.ABS | FM.START, 1 << 27, 1 << 24, 1 << 22, 5, 6, 7, start=1 << 27)) == [1, 0, 0]
    assert b.fenv[1, FM.STAGE] == FM.DECAY and b.cut[1, :4].tolist() == [1 << 27, 1 << 24, 6, 6] and b.coeffs_are_w(1)
    # a sustain equal to the peak equal to the start: the voice rests in sustain at once, not moving
    assert b.record(2, R(FM.ABS, w, w, 1 << 22, 5, 6, 7)) == [1, 0, 0]
    assert b.fenv[2, FM.STAGE] == FM.SUSTAIN and b.cut[2, :5].tolist() == [w, 0, 0, 0, 0]
    # a sustain equal to the peak, reached by steps: the decay lands in the step that ends the attack
    assert b.record(3, R(FM.ABS, 1 << 27, 1 << 27, 1 << 22, fast, 6, 7)) == [1, 0, 0]
    assert b.fenv[3, FM.STAGE] == FM.ATTACK
    # an end equal to the sustain: the release lands in the pass that enters it, and the contour is gone
    assert b.record(4, R(FM.ABS, w, w, w, 5, 6, 7)) == [1, 0, 0]
    # a release that lands by a step in the pass that enters it
    assert b.record(5, R(FM.ABS, w, w, 1 << 25, 5, 6, fast)) == [1, 0, 0]
    held = {v: [int(b.filt[name][v]) for name in M.COEFFS] for v in range(6)}
    assert b.advance(128) == [2, 1]                                 # voices 0 and 1 decay on; voice 3 arrived (at two levels: once)
    assert b.fenv[3, FM.STAGE] == FM.SUSTAIN and b.cut[3, :5].tolist() == [1 << 27, 0, 0, 0, 0] and b.coeffs_are_w(3)
    assert [int(b.filt[name][2]) for name in M.COEFFS] == held[2], "a voice resting in sustain stores nothing"
    b.release[4] = b.release[5] = 77
    assert b.advance(64) == [2, 2]
    for v, end in ((4, w), (5, 1 << 25)):
        assert not b.fenv[v].any() and b.cut[v].tolist() == [end, 0, 0, 0, 0, 3 << 15, 1, 0] and b.coeffs_are_w(v)
    twin = Bare([1 << 25])                                           # a voice set with ABS at w_end: the same eight words, the same coefficients
    assert np.array_equal(twin.cut[0], b.cut[5]) and all(twin.filt[n][0] == b.filt[n][5] for n in M.COEFFS)
    assert b.advance(64) == [2, 0]                                  # the ended contours follow the plain rule: nothing moves, nothing arrives
    # carry survives a stage change and runs on through sustain; it ends with the contour
    c = Bare([w])
    c.record(0, R(FM.ABS, w + 5, w + 5, w, fast, 6, fast))
    assert c.advance(100) == [0, 1] and c.fenv[0, FM.STAGE] == FM.SUSTAIN and c.cut[0, M.CARRY] == 36
    assert c.advance(100) == [0, 0] and c.cut[0, M.CARRY] == (36 + 100) & 63
    c.release[0] = 1
    assert c.advance(27) == [1, 0] and c.fenv[0, FM.STAGE] == FM.RELEASE and c.cut[0, M.CARRY] == 35 and c.cut[0, M.TARGET] == w
    assert c.coeffs_are_w(0)
    assert c.advance(29) == [0, 1] and not c.fenv[0].any() and c.cut[0].tolist() == [w, 0, 0, 0, 0, 3 << 15, 1, 0]


def test_a_trigger_alone_does_not_restart_and_a_record_does():
    w = 1 << 26
    b = Bare([w])
    b.record(0, R(FM.ABS, 1 << 27, 1 << 25, 1 << 22, 1 << 24, 1 << 24, 1 << 24))
    b.release[0] = 9
    b.advance(64)
    assert b.fenv[0, FM.STAGE] == FM.RELEASE
    b.release[0] = 0                                                 # a trigger stamp clears the release clock: the contour goes on releasing
    b.advance(64)
    assert b.fenv[0, FM.STAGE] == FM.RELEASE and b.cut[0, M.TARGET] == 1 << 22
    b.record(0, R(FM.ABS, 1 << 27, 1 << 25, 1 << 22, 1 << 24, 1 << 24, 1 << 24))
    assert b.fenv[0, FM.STAGE] == FM.ATTACK and b.cut[0, M.CARRY] == 0


def test_rel_levels_clamp_at_both_ends_and_the_voice_counts_once():
    b = Bare([1 << 20, 1 << 30, 1 << 26, 0])
    # 2^20 * 2^-4 = 2^16 below the box; three levels clamped, one voice counted
    assert b.record(0, R(FM.REL | FM.START, 1 << 12, 1 << 12, 1 << 16, 5, 6, 7, start=1 << 12)) == [1, 0, 1]
    assert b.cut[0, M.W] == M.W_MIN and b.fenv[0].tolist() == [FM.SUSTAIN, M.W_MIN, M.W_MIN, 1 << 20, 5, 6, 7, 0] and b.coeffs_are_w(0)
    # 2^30 * 4 above the box
    assert b.record(1, R(FM.REL, 4 << 16, 1 << 16, 1 << 15, 5, 6, 7)) == [1, 0, 1]
    assert b.fenv[1].tolist() == [FM.ATTACK, M.W_MAX, 1 << 30, 1 << 29, 5, 6, 7, 0]
    # the ends themselves are inside: (2^26 * 24 * 2^16) >> 16 = 3 * 2^29 and 2^26 >> 7 = 2^19 do not count
    assert b.record(2, R(FM.REL, 24 << 16, 1 << 9, 1 << 16, 5, 6, 7)) == [1, 0, 0]
    assert b.fenv[2, 1:4].tolist() == [M.W_MAX, M.W_MIN, 1 << 26]
    # one past either end counts
    b2 = Bare([(1 << 26) + 1, (1 << 26) - 1])
    assert b2.record(0, R(FM.REL, 24 << 16, 1 << 16, 1 << 16, 5, 6, 7)) == [1, 0, 1] and b2.fenv[0, FM.W_PEAK] == M.W_MAX
    assert b2.record(1, R(FM.REL, 1 << 16, 1 << 9, 1 << 16, 5, 6, 7)) == [1, 0, 1] and b2.fenv[1, FM.W_SUSTAIN] == M.W_MIN
    # without START the start value is neither computed nor clamped; a voice without a cutoff word is withheld and untouched
    assert b.record(3, R(FM.REL, 1 << 16, 1 << 16, 1 << 16, 5, 6, 7)) == [0, 1, 0] and not b.cut[3, :5].any() and not b.fenv[3].any()


# ---------------------------------------------------------------------------------------------- the switches bite

def release_scene():
    """READ THE CLOCK: a contour rests in sustain; the clock is stamped; the first advance after it enters the release"""
    b = Bare([1 << 26])
    b.record(0, R(FM.ABS, 1 << 26, 1 << 26, 1 << 22, 5, 6, 1 << 24))
    assert b.advance(64) == [0, 0] and b.fenv[0, FM.STAGE] == FM.SUSTAIN
    b.release[0] = 4242
    assert b.advance(64) == [1, 0] and b.fenv[0, FM.STAGE] == FM.RELEASE and b.cut[0, M.W] < 1 << 26


def clear_scene():
    """CLEAR RULE: a tag launch, a cutoff record and a stop each end a contour, one resting in sustain included"""
    b = Bare([1 << 26] * 3)
    for v in range(3):
        b.record(v, R(FM.ABS, 1 << 26, 1 << 26, 1 << 22, 5, 6, 7))
    FM.tag_clear(b.fenv, [0], 1)
    with FM._ends(b.fenv):
        assert M.apply(b.cut, None, np.zeros(3, np.uint32), b.filt, [1], M.Rec(M.ABS, 1 << 25)) == [1, 0, 0]
    FM.stop(b.cut, b.fenv, b.filt, 2, 1, False)
    assert not b.fenv.any()


def test_the_scenes_pass_and_fail_without_their_rule(monkeypatch):
    release_scene()
    clear_scene()
    monkeypatch.setattr(FM, "READ_RELEASE_CLOCK", False)
    with pytest.raises(AssertionError):
        release_scene()
    clear_scene()
    monkeypatch.setattr(FM, "READ_RELEASE_CLOCK", True)
    monkeypatch.setattr(FM, "CLEAR_RULE", False)
    release_scene()
    with pytest.raises(AssertionError):
        clear_scene()


# ---------------------------------------------------------------------------------------------- refusals

def test_check_through_ctypes_is_the_models_in_the_headers_order():
    g = dict(peak=1 << 27, sustain=1 << 25, end=1 << 22, rate_attack=5, rate_decay=6, rate_release=7)
    mk = lambda set, **kw: R(set, **{**g, **kw})
    cases = [mk(FM.ABS), mk(FM.REL), mk(FM.ABS | FM.START, start=1 << 20), mk(FM.REL | FM.START, start=3),
             mk(8 | FM.ABS), mk(FM.ABS | FM.REL), mk(0), mk(FM.START, start=1 << 20), mk(FM.ABS, start=1 << 20), mk(FM.REL, start=1),
             mk(FM.ABS | FM.START, start=M.W_MIN - 1), mk(FM.ABS | FM.START, start=0), mk(FM.ABS, peak=M.W_MAX + 1), mk(FM.ABS, sustain=0),
             mk(FM.ABS, end=M.W_MIN - 1), mk(FM.ABS, peak=M.W_MAX, sustain=M.W_MIN, end=M.W_MIN),
             mk(FM.REL, peak=0), mk(FM.REL, sustain=0), mk(FM.REL, end=0), mk(FM.REL | FM.START, start=0), mk(FM.REL, peak=0xFFFFFFFF, end=1),
             mk(FM.ABS, rate_attack=0), mk(FM.ABS, rate_decay=0), mk(FM.REL, rate_release=0), mk(FM.ABS, rate_attack=0xFFFFFFFF),
             # two faults at once: the earlier one of the header's order decides
             mk(8 | FM.ABS, peak=0), mk(FM.ABS | FM.REL, peak=0), mk(FM.ABS, start=5, peak=0), mk(FM.ABS, peak=0, rate_attack=0),
             mk(FM.REL, end=0, rate_decay=0), mk(FM.ABS, start=5, rate_attack=0)]
    want = [0, 0, 0, 0, BAD, BAD, BAD, BAD, BAD, BAD, RANGE, RANGE, RANGE, RANGE, RANGE, 0, RANGE, RANGE, RANGE, RANGE, 0, BAD, BAD, BAD, 0,
            BAD, BAD, BAD, RANGE, RANGE, BAD]
    for r, w in zip(cases, want):
        assert FM.check([r]) == w, vars(r)
        assert fxb.fx_fenv_check([r.c()]) == w, vars(r)
    assert fxb.fx_fenv_check(None) == BAD and fxb.fx_fenv_check(None, n=-1) == BAD and fxb.fx_fenv_check([cases[0].c()], n=-1) == BAD
    assert fxb.fx_fenv_check([], n=0) == 0
    # record by record: a RANGE fault in record 0 is reported ahead of a BAD_ARG fault in record 1
    assert fxb.fx_fenv_check([cases[12].c(), cases[4].c()]) == RANGE and fxb.fx_fenv_check([cases[0].c(), cases[12].c()], n=1) == 0
    assert FM.check([cases[12], cases[4]]) == RANGE


@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fxfenv") / "c_fx_fenv_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_fx_fenv_host.c"), os.path.join(CSRC, "skred_fx_fenv.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"),
           "-lskred_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-lm", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "skred_amd"),
           "-Wl,-rpath," + os.path.join(rocm, "lib")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return out.stdout.strip().splitlines()


def test_host_program(host_lines):
    bad = [l for l in host_lines[:-1] if not l.endswith(" ok")]
    assert not bad, bad
    assert host_lines[-1] == "OK" and len(host_lines) > 80
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "check", "pack", "match", "owned", "tags", "download", "untouched"}, groups
