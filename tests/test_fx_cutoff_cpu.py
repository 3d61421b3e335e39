"""Filter cutoff on the fixed-point bank, without a GPU: the integer arithmetic and the state machine of include/skred_amd_fxpt.h, section
"filter cutoff".

THE ARITHMETIC: tests/fx_cutoff_model.py (Python integers of unbounded width) against skred_fx_filter_coeffs_w word for word on THE
GRID -- 201 values of w_q29 (both ends of the box, 72 spread geometrically, the pi / 2 seam and its 64 neighbours on either side) x 17
values of q_q16 x 5 modes -- and on 120 000 random (w_q29, q_q16, mode) of the box; every intermediate held to the width the header
states, on the grid, a random set and all corners; the largest absolute error of each word against fp64 on the exact rationals, held to
4 x the error of the route the bank had before (the same inputs in fp32 through skred_filter_coeffs, rounded to Q2.30 as
fxbank.q30_coeffs rounds); stability.  Figures of the accuracy test as measured (units of 2^-30; the yardstick's are 89 .. 244):
    mode 1: 0.80 1.31 0.80 2.12 1.45   mode 2: 1.02 1.67 1.02 2.12 1.45   mode 3: 0.98 0 0.98 2.12 1.45
    mode 4: 0.98 2.12 0.98 2.12 1.45   mode 5: 1.45 2.12 0 2.12 1.45

THE STATE MACHINE: the model against a plain per-voice, per-64-frame loop; landing on the target's bits, equal to an ABS twin; a
1 024-frame glide cut three ways; TRACK on a bent and on a gliding voice; clamps, k == 0, a first cutoff without Q and MODE; the clear
rule's scenes, which must FAIL without the rule; every refusal and the packing (tests/c_fx_cutoff_host.c, a program of its own); a mono
line with a tracked low-pass on oracle.cpuref.fx_render alone.
"""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import fx_bend_model as BM
import fx_cutoff_model as M
import fx_glide_model as GM
from oracle import cpuref
from skred_amd import device, fxbank as fxb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
SYMBOLS = ("skred_fxbank_cutoff_match", "skred_fxbank_cutoff_owned_each", "skred_fxbank_cutoff_tags_each", "skred_fxbank_cutoff_advance",
           "skred_fxbank_cutoff_stop", "skred_fxbank_download_cutoff")
R = M.Rec
BOTH = M.BOTH
CUTS = ([1024], [64] * 16, [100, 28, 512, 1, 383])              # 1 024 frames, three ways
f32 = np.float32


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd_fxpt.h")).read()
    L = fxb._bind(fxb.load())
    for s in SYMBOLS + ("skred_fx_cutoff_check", "skred_fx_filter_coeffs_w"):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in fxb.FX_ABI_SYMBOLS + fxb.FX_HOST_ABI_SYMBOLS
    assert "THE ARITHMETIC" in text and "ADVANCE BY F FRAMES" in text and "A NEW NOTE CLEARS THE WORDS" in text
    lits = dict(re.findall(r"#define SKRED_FX_CUTOFF_(\w+) (\(?-?[0-9][0-9ul< ]*\)?)", text))
    val = lambda s: eval(s.replace("u", "").replace("ll", ""))
    for name, want in [("W_MIN", M.W_MIN), ("W_MAX", M.W_MAX), ("Q_MIN", M.Q_MIN), ("Q_MAX", M.Q_MAX), ("PI_Q29", M.PI_Q29),
                       ("HALF_PI_Q29", M.HALF_PI_Q29)] + [("S%d" % (k + 1), v) for k, v in enumerate(M.S)] + \
                      [("C%d" % (k + 2), v) for k, v in enumerate(M.C)]:
        assert val(lits[name]) == want, (name, lits[name])
    assert M.PI_Q29 == round(np.pi * 2 ** 29) and M.HALF_PI_Q29 == round(np.pi / 2 * 2 ** 29)
    assert (fxb.FX_CUTOFF_W_MIN, fxb.FX_CUTOFF_W_MAX, fxb.FX_CUTOFF_Q_MIN, fxb.FX_CUTOFF_Q_MAX) == (M.W_MIN, M.W_MAX, M.Q_MIN, M.Q_MAX)
    assert (fxb.FX_CUTOFF_ABS, fxb.FX_CUTOFF_TRACK, fxb.FX_CUTOFF_GLIDE, fxb.FX_CUTOFF_Q, fxb.FX_CUTOFF_MODE) == (M.ABS, M.TRACK, M.GLIDE, M.SET_Q, M.SET_MODE)


# ---------------------------------------------------------------------------------------------- the arithmetic

def grid():
    ws = [M.W_MIN, M.W_MAX] + [int(round(x)) for x in np.geomspace(M.W_MIN, M.W_MAX, 72)] + [M.HALF_PI_Q29 + d for d in range(-64, 65)]
    ws = sorted(set(min(M.W_MAX, max(M.W_MIN, w)) for w in ws))
    qs = sorted(set([M.Q_MIN, M.Q_MAX] + [int(round(x)) for x in np.geomspace(M.Q_MIN, M.Q_MAX, 17)]))
    assert len(ws) == 201 and len(qs) == 17 and ws[0] == M.W_MIN and ws[-1] == M.W_MAX and qs[0] == M.Q_MIN and qs[-1] == M.Q_MAX
    return [(w, q) for w in ws for q in qs]


def lib_w(mode, w, q):
    rc, out = fxb.fx_filter_coeffs_w(mode, w, q)
    assert rc == 0
    return out.tolist()


@pytest.fixture(scope="module")
def on_grid():
    """the grid, {mode: int64 array (points, 5)} of the MODEL on it, the widths its intermediates reached, and the same arrays of
    skred_fx_filter_coeffs_w: accuracy and stability are asserted on the words the library gives"""
    g, widths = grid(), {}
    model = {m: np.array([M.coeffs(m, w, q, widths) for w, q in g], np.int64) for m in range(1, 6)}
    return g, model, widths, {m: np.array([lib_w(m, w, q) for w, q in g], np.int64) for m in range(1, 6)}


def test_model_is_the_host_function_on_the_grid(on_grid):
    _, model, _, lib = on_grid
    for mode in range(1, 6):
        assert np.array_equal(lib[mode], model[mode]), mode


def random_box(n, seed):
    rng = np.random.default_rng(seed)
    w = np.where(rng.integers(0, 2, n) == 0, rng.integers(M.W_MIN, M.W_MAX + 1, n),       # uniform, and uniform in the logarithm
                 np.exp2(rng.uniform(19.0, np.log2(M.W_MAX), n)).astype(np.int64))
    q = np.exp2(rng.uniform(10.0, 26.0, n)).astype(np.int64)
    return np.clip(w, M.W_MIN, M.W_MAX), np.clip(q, M.Q_MIN, M.Q_MAX), rng.integers(1, 6, n)


def test_model_is_the_host_function_on_random_inputs():
    w, q, mode = random_box(120000, 74)
    L, out = fxb._bind(fxb.load()), np.zeros(5, np.int32)
    for i in range(len(w)):
        assert L.skred_fx_filter_coeffs_w(int(mode[i]), int(w[i]), int(q[i]), out.ctypes.data) == 0
        assert out.tolist() == M.coeffs(mode[i], w[i], q[i]), (mode[i], w[i], q[i])


def test_every_intermediate_keeps_the_width_the_header_states(on_grid):
    widths = dict(on_grid[2])
    w, q, mode = random_box(20000, 75)
    for i in range(len(w)):
        M.coeffs(mode[i], w[i], q[i], widths)
    for w, q, mode in itertools.product((M.W_MIN, M.W_MIN + 1, M.HALF_PI_Q29, M.HALF_PI_Q29 + 1, M.W_MAX - 1, M.W_MAX),
                                        (M.Q_MIN, M.Q_MIN + 1, M.Q_MAX - 1, M.Q_MAX), range(1, 6)):
        M.coeffs(mode, w, q, widths)
    assert set(widths) == set(M.STATED_BITS)
    for name, top in sorted(widths.items()):
        print("%-16s reached %2d bits, stated %2d" % (name, top.bit_length(), M.STATED_BITS[name]))
        assert top.bit_length() <= M.STATED_BITS[name] <= 64, name
    # signed words fit int64 with their sign, the shifted numerator is unsigned, alpha reaches 32 and a few units (the sine's
    # polynomial overshoots 1 by 5e-10 at most) and no further
    for name in ("sine product", "cosine product", "t * z", "rs + half"):
        assert M.STATED_BITS[name] <= 63
    assert 1 << 35 <= widths["alpha"] < (1 << 35) + 64
    assert widths["numerator << s"] < 1 << 64


def yardstick(mode, w, q):
    """the parent's only route: the same inputs in fp32 through skred_filter_coeffs, rounded to Q2.30 as fxbank.q30_coeffs rounds"""
    L, out = device.load(), (C.c_float * 5)()
    two_pi = float(f32(2.0) * f32(np.pi))                            # freq / rate = w / (2 pi)
    assert L.skred_filter_coeffs(int(mode), float(f32(w / 2.0 ** 29)), float(f32(q / 2.0 ** 16)), two_pi, out) == 0
    return np.clip(np.round(np.array(out[:], f32).astype(np.float64) * (1 << 30)), -(1 << 31), (1 << 31) - 1)


def test_error_tables_and_the_factor_of_four(on_grid):
    g, _, _, lib = on_grid
    print("mode | skred_fx_filter_coeffs_w: b0 b1 b2 a1 a2 | fp32 skred_filter_coeffs, rounded: b0 b1 b2 a1 a2   (units of 2^-30)")
    worst = 0.0
    for mode in range(1, 6):
        ref = np.clip(np.array([M.coeffs_fp64(mode, w, q) for w, q in g]), -(1 << 31), (1 << 31) - 1)
        ea = np.abs(lib[mode] - ref).max(axis=0)
        eo = np.abs(np.array([yardstick(mode, w, q) for w, q in g]) - ref).max(axis=0)
        print(mode, "|", " ".join("%6.2f" % x for x in ea), "|", " ".join("%7.1f" % x for x in eo))
        for k in range(5):
            assert ea[k] <= 4.0 * eo[k], (mode, M.COEFFS[k], ea[k], eo[k])
            worst = max(worst, ea[k] / eo[k] if eo[k] else 0.0)
    print("largest ratio %.3f" % worst)


def test_int32_and_stable_on_the_grid(on_grid):
    lib = on_grid[3]
    for mode in range(1, 6):
        c = lib[mode]
        assert (c >= M.I32_MIN).all() and (c <= M.I32_MAX).all(), mode
        a1, a2 = c[:, 3], c[:, 4]
        assert (np.abs(a2) < 1 << 30).all() and (np.abs(a1) < (1 << 30) + a2).all(), mode
    assert fxb.fx_filter_coeffs_w(0, 1 << 26, 1 << 16)[0] == 1
    for args in ((1, M.W_MIN - 1, 1 << 16), (1, M.W_MAX + 1, 1 << 16), (1, 1 << 26, M.Q_MIN - 1), (1, 1 << 26, M.Q_MAX + 1)):
        assert fxb.fx_filter_coeffs_w(*args)[0] == RANGE, args
    assert fxb.fx_filter_coeffs_w(6, 1 << 26, 1 << 16)[0] == BAD and fxb.fx_filter_coeffs_w(-1, 1 << 26, 1 << 16)[0] == BAD


# ---------------------------------------------------------------------------------------------- the state machine

def fresh(n):
    cut, inc = M.new(n), np.zeros(n, np.uint32)
    filt = {name: np.full(n, 12345, np.int32) for name in M.COEFFS}
    return cut, inc, filt


def plain_loop(w, target, up, down, carry, frames):
    """one voice, 64 frames at a time: (w, target, carry) after `frames` more frames"""
    if target == 0:
        return w, 0, 0
    c = carry + frames
    for _ in range(c >> 6):
        if w == target:
            return target, 0, 0
        if w < target:
            w = w + max(1, (w * up) >> 32)
            if w >= target:
                return target, 0, 0
        else:
            w = w - max(1, (w * down) >> 32)
            if w <= target:
                return target, 0, 0
    if w == target:
        return target, 0, 0
    return w, target, c & 63


def advance_scene(seed, n=96):
    """n voices: a third sweep up, a third down, the rest rest; rates from crawling to jumping; every voice owned and set"""
    rng = np.random.default_rng(seed)
    cut, inc, filt = fresh(n)
    owner = np.arange(1, n + 1, dtype=np.uint32)
    for v in range(n):
        w0 = int(np.exp2(rng.uniform(20.0, 30.0)))
        assert M.cutoff_owned_each(owner, cut, None, inc, filt, [R(M.ABS | BOTH, w0, int(np.exp2(rng.uniform(12, 20))), 1 + v % 5)], [v], [v + 1]) == [1, 0, 0, 0]
        if v % 3 == 2:
            continue
        octaves = float(rng.uniform(0.2, 3.0))
        t = int(min(M.W_MAX, w0 * 2.0 ** octaves)) if v % 3 == 0 else int(max(M.W_MIN, w0 / 2.0 ** octaves))
        up, down = M.rate_q32(float(rng.choice([20.0, 200.0, 700.0])))
        assert M.cutoff_owned_each(owner, cut, None, inc, filt, [R(M.ABS | M.GLIDE, t, up_q32=up, down_q32=down)], [v], [v + 1]) == [1, 0, 0, 0]
    return cut, filt


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_a_plain_loop(seed):
    cut, filt = advance_scene(seed)
    want = [[int(x) for x in row] for row in cut]
    ups = int(((cut[:, M.TARGET] != 0) & (cut[:, M.W] < cut[:, M.TARGET])).sum())
    downs = int(((cut[:, M.TARGET] != 0) & (cut[:, M.W] > cut[:, M.TARGET])).sum())
    assert ups >= 1 and downs >= 1
    landed = 0
    for frames in (1, 63, 64, 65, 130, 700, 1):
        res = M.advance(cut, filt, 0, len(cut), frames)
        still = arrived = 0
        for v, row in enumerate(want):
            if row[M.TARGET] == 0:
                continue
            w, t, c = plain_loop(row[M.W], row[M.TARGET], row[M.UP], row[M.DOWN], row[M.CARRY], frames)
            row[M.W], row[M.TARGET], row[M.CARRY] = w, t, c
            if t == 0:
                row[M.UP] = row[M.DOWN] = 0
                arrived += 1
            else:
                still += 1
            assert [int(filt[name][v]) for name in M.COEFFS] == M.coeffs(row[M.MODE], w, row[M.Q]), v
        assert res == [still, arrived] and cut.tolist() == want, frames
        landed += arrived
    assert landed >= 1 and still >= 1, "every advance scene has a voice that lands and one still moving"


@pytest.mark.parametrize("start, target", [(1 << 22, 1 << 27), (1 << 27, 1 << 22), (M.W_MIN, M.W_MAX), (M.W_MAX, M.W_MIN), (5000001, 5000002)])
def test_a_sweep_lands_on_the_targets_bits(start, target):
    cut, inc, filt = fresh(2)
    owner = np.array([7, 8], np.uint32)
    up, down = M.rate_q32(900.0)
    assert M.cutoff_owned_each(owner, cut, None, inc, filt, [R(M.ABS | BOTH, start, 5 << 15, 2), R(M.ABS | BOTH, target, 5 << 15, 2)], [0, 1], [7, 8]) == [2, 0, 0, 0]
    assert M.cutoff_owned_each(owner, cut, None, inc, filt, [R(M.ABS | M.GLIDE, target, up_q32=up, down_q32=down)], [0], [7]) == [1, 0, 0, 0]
    assert cut[0].tolist() == [start, target, up, down, 0, 5 << 15, 2, 0]
    for _ in range(400):
        if M.advance(cut, filt, 0, 2, 64) == [0, 1]:
            break
    else:
        raise AssertionError("never arrived")
    assert cut[0].tolist() == cut[1].tolist() == [target, 0, 0, 0, 0, 5 << 15, 2, 0]
    assert all(filt[name][0] == filt[name][1] for name in M.COEFFS), "arrival equals a twin set with ABS at the target"


def test_three_block_cuttings_agree_at_every_multiple_of_64():
    """Every pair of cuttings is compared at every multiple of 64 frames they both stop at (1 024 for all three; 128, 640 and 1 024
    for 16 x 64 against the uneven one), and the 16 x 64 cutting -- the one that stops at EVERY multiple -- is compared at each of its
    sixteen stops with the plain per-voice loop run over that many frames in one go from the start: so the words at every multiple
    of 64 are those of the definition, whatever the cutting."""
    at64 = []
    start = advance_scene(9)[0]
    for cutting in CUTS:
        cut, filt = advance_scene(9)
        seen, t, moving0 = {}, 0, int((cut[:, M.TARGET] != 0).sum())
        for frames in cutting:
            M.advance(cut, filt, 0, len(cut), frames)
            t += frames
            if t % 64 == 0:
                seen[t] = (cut[:, [M.W, M.TARGET]].copy(), {k: v.copy() for k, v in filt.items()})
        assert t == 1024
        at64.append(seen)
        left = int((cut[:, M.TARGET] != 0).sum())
        assert 0 < left < moving0, "some voice landed and some voice still moves"
    assert set(at64[0]) == {1024} and set(at64[1]) == set(range(64, 1025, 64)) and set(at64[2]) == {128, 640, 1024}
    compared = []
    for a, b in itertools.combinations(range(3), 2):
        for t in sorted(set(at64[a]) & set(at64[b])):
            assert np.array_equal(at64[a][t][0], at64[b][t][0]), (a, b, t)
            assert all(np.array_equal(at64[a][t][1][k], at64[b][t][1][k]) for k in M.COEFFS), (a, b, t)
            compared.append((a, b, t))
    assert compared == [(0, 1, 1024), (0, 2, 1024), (1, 2, 128), (1, 2, 640), (1, 2, 1024)]
    for t in range(64, 1025, 64):
        for v, row in enumerate(start.tolist()):
            w, target, _ = plain_loop(row[M.W], row[M.TARGET], row[M.UP], row[M.DOWN], 0, t)
            assert at64[1][t][0][v].tolist() == [w, target], (t, v)
            assert [int(at64[1][t][1][k][v]) for k in M.COEFFS] == M.coeffs(row[M.MODE], w, row[M.Q]), (t, v)


def test_track_reads_the_key_of_a_bent_and_of_a_gliding_voice():
    n = 4
    cut, inc, filt = fresh(n)
    owner = np.array([1, 2, 3, 4], np.uint32)
    inc[:] = [40000003, 40000003, 40000003, 0]
    bend, glide = BM.new(n), GM.new(n)
    assert BM.apply(bend, inc, [1], BM.ratio_of(7.0)) == [1, 0] and inc[1] != 40000003 and bend[1, 0] == 40000003
    up, down = GM.per_64(700.0)
    assert GM.start_owned(owner, glide, inc, [GM.Glide(GM.TO_INC, up, down, target_inc=80000001)], [2], [3]) == [1, 0, 0]
    GM.advance(glide, inc, 0, n, 256)
    assert 40000003 < inc[2] < 80000001
    rec = R(M.TRACK | BOTH, M.track_q24(4), 1 << 16, 1)
    assert M.cutoff_owned_each(owner, cut, bend, inc, filt, [rec] * 4, [0, 1, 2, 3], [1, 2, 3, 4]) == [3, 1, 0, 0]
    assert cut[0, M.W] == cut[1, M.W] == (40000003 * M.track_q24(4)) >> 27, "a bent voice tracks its key, not its sounding increment"
    assert cut[2, M.W] == (int(inc[2]) * M.track_q24(4)) >> 27, "a gliding voice tracks where the glide is"
    assert not cut[3].any() and filt["b0_q30"][3] == 12345, "k == 0 is withheld and leaves everything"
    # without the bend array the sounding increment is all there is
    cut2, _, filt2 = fresh(n)
    assert M.cutoff_owned_each(owner, cut2, None, inc, filt2, [rec], [1], [2]) == [1, 0, 0, 0] and cut2[1, M.W] == (int(inc[1]) * M.track_q24(4)) >> 27


def test_clamps_and_withheld_records_are_counted():
    n = 6
    cut, inc, filt = fresh(n)
    owner = np.arange(1, n + 1, dtype=np.uint32)
    inc[:] = [1, 0xFFFFFFFF, 40000003, 0, 40000003, 40000003]
    recs = [R(M.TRACK | BOTH, 1, 1 << 16, 1),                        # 1 * 1 >> 27 = 0: clamped to the lower end
            R(M.TRACK | BOTH, 0xFFFFFFFF, 1 << 16, 2),               # far above 3: clamped to the upper end
            R(M.TRACK | BOTH, M.track_q24(3), 1 << 16, 3),           # inside
            R(M.TRACK | BOTH, M.track_q24(3), 1 << 16, 3),           # k == 0: withheld
            R(M.TRACK | M.SET_Q, M.track_q24(3), 1 << 16),           # a first cutoff without MODE: withheld
            R(M.ABS | M.SET_MODE, 1 << 25, 0, 4)]                    # a first cutoff without Q: withheld
    before = cut.copy()
    assert M.cutoff_owned_each(owner, cut, None, inc, filt, recs, list(range(n)), owner.tolist()) == [3, 3, 0, 2]
    assert cut[0, M.W] == M.W_MIN and cut[1, M.W] == M.W_MAX and M.W_MIN < cut[2, M.W] < M.W_MAX
    assert np.array_equal(cut[3:], before[3:]) and all((filt[k][3:] == 12345).all() for k in M.COEFFS)
    assert [int(filt[k][0]) for k in M.COEFFS] == M.coeffs(1, M.W_MIN, 1 << 16)
    # once set, a record may leave q and mode alone; a stolen voice counts as not owned
    assert M.cutoff_owned_each(owner, cut, None, inc, filt, [R(M.ABS, 1 << 26), R(M.ABS, 1 << 26)], [2, 1], [3, 99]) == [1, 0, 1, 0]
    assert cut[2].tolist() == [1 << 26, 0, 0, 0, 0, 1 << 16, 3, 0]
    assert M.cutoff_match(owner, cut, None, inc, filt, 0, n, (0, 0), R(M.ABS, 1 << 24)) == [3, 3, 0, 0]


def test_randomised_scenes_are_not_vacuous():
    """the generator of the GPU tests: at most a quarter of its records are withheld or clamped"""
    import fx_cutoff_scenes as S
    for n in (65, 255, 1500):
        bank, pool, c0 = fxb.bank_fx(n)
        st = M.FxCutoffStage(S.silent_voice(bank), pool, c0)
        tally = S.random_performance(st, np.random.default_rng(n), blocks=False)
        print(n, tally)
        assert tally["records"] >= n and 4 * (tally["withheld"] + tally["clamped"]) <= tally["records"], tally
        assert tally["landed"] >= 1 and tally["still"] >= 1 and tally["up"] >= 1 and tally["down"] >= 1, tally


@pytest.mark.parametrize("name", M.SCENES)
def test_scene_on_the_oracle(name):
    bank, pool, c0 = fxb.bank_fx(600)
    M.run_scene(name, M.FxCutoffStage(bank, pool, c0))


@pytest.mark.parametrize("name", M.SCENES)
def test_the_scenes_fail_without_the_clear_rule(name, monkeypatch):
    monkeypatch.setattr(M, "CLEAR_RULE", False)
    bank, pool, c0 = fxb.bank_fx(600)
    with pytest.raises(AssertionError):
        M.run_scene(name, M.FxCutoffStage(bank, pool, c0))


# ---------------------------------------------------------------------------------------------- refusals

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fxcutoff") / "c_fx_cutoff_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_fx_cutoff_host.c"), os.path.join(CSRC, "skred_fx_cutoff.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"),
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
    assert host_lines[-1] == "OK" and len(host_lines) > 70
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "coeffs", "check", "pack", "match", "owned", "tags", "advance", "stop", "download", "untouched"}, groups


def test_check_through_ctypes_is_the_models():
    up, down = M.rate_q32(60.0)
    cases = [R(M.ABS | BOTH, 1 << 24, 1 << 16, 1), R(M.TRACK, 5), R(M.ABS | M.TRACK, 1 << 24), R(0, 1 << 24), R(32 | M.ABS, 1 << 24),
             R(M.ABS, M.W_MIN - 1), R(M.ABS, M.W_MAX + 1), R(M.ABS, M.W_MIN), R(M.ABS, M.W_MAX), R(M.TRACK, 0), R(M.TRACK, 0xFFFFFFFF),
             R(M.ABS | M.SET_Q, 1 << 24, M.Q_MIN - 1), R(M.ABS | M.SET_Q, 1 << 24, M.Q_MAX + 1), R(M.ABS | M.SET_Q, 1 << 24, M.Q_MAX),
             R(M.ABS, 1 << 24, 5), R(M.ABS | M.SET_MODE, 1 << 24, 0, 0), R(M.ABS | M.SET_MODE, 1 << 24, 0, 6), R(M.ABS, 1 << 24, 0, 9),
             R(M.ABS | M.GLIDE, 1 << 24, up_q32=up, down_q32=down), R(M.ABS | M.GLIDE, 1 << 24, up_q32=0, down_q32=down),
             R(M.ABS | M.GLIDE, 1 << 24, up_q32=up, down_q32=0), R(M.ABS, 1 << 24, up_q32=0, down_q32=0),
             R(M.ABS, 1 << 24, reserved=(0, 1)), R(M.ABS, 1 << 24, reserved=(1, 0))]
    seen = set()
    for first_time in (False, True):
        for r in cases:
            want = M.check([r], first_time=first_time)
            assert fxb.fx_cutoff_check([r.c()], first_time=first_time) == want, (vars(r), first_time)
            seen.add(want)
    assert seen == {0, BAD, RANGE}
    assert fxb.fx_cutoff_check(None) == BAD and fxb.fx_cutoff_check([cases[0].c()], n=-1) == BAD and fxb.fx_cutoff_check([], n=0) == 0
    assert fxb.fx_cutoff_check([cases[0].c(), cases[9].c()]) == RANGE and fxb.fx_cutoff_check([cases[0].c(), cases[9].c()], n=1) == 0


# ---------------------------------------------------------------------------------------------- end to end

def test_a_mono_line_with_a_tracked_low_pass_on_the_oracle():
    """Three keys on one voice, each with a low-pass at 4 x its own frequency that opens from 1 x: the model's coefficients go into the
    oracle's bank block by block; the filter is heard (the blocks differ from an unfiltered twin) and every block's words are the model's."""
    n, v, tag = 8, 3, [0x0300003C]
    bank, pool, c0 = fxb.bank_fx(n)
    bank["filter_mode"][:] = 0
    bank["filter_mode"][v] = 1
    st = M.FxCutoffStage(bank, pool, c0)
    dry = M.FxCutoffStage(bank, pool, c0)
    dry.truth["filter_mode"][v] = 0
    up, down = M.rate_q32(40.0)
    differs = 0
    for key in (20000003, 30000001, 25000007):
        for s in (st, dry):
            s.strike([v], tag, [key])
        assert st.cut_tags([R(M.TRACK | BOTH, M.track_q24(1), 3 << 16, 1)], tag) == [1, 0, 0, 0]
        assert st.cut_tags([R(M.TRACK | M.GLIDE, M.track_q24(4), up_q32=up, down_q32=down)], tag) == [1, 0, 0, 0]
        w = [int(st.cut[v, M.W])]
        for _ in range(12):
            res = st.cut_advance(64)
            assert [int(st.filt[k][v]) for k in M.COEFFS] == M.coeffs(1, int(st.cut[v, M.W]), 3 << 16)
            w.append(int(st.cut[v, M.W]))
            mix, _ = st.block()
            dmix, _ = dry.block()
            differs += int((mix != dmix).any())
        assert w == sorted(w) and w[0] == (key * M.track_q24(1)) >> 27 and w[-1] > w[0]
        assert res == [1, 0], "two octaves at 40 octaves per second take 56 blocks of 64 frames: after 12 the sweep still moves"
    assert differs >= 30
