"""Filter cutoff on the device, without a GPU: the symbols against the header; the defined coefficient arithmetic -- the numpy model
(tests/cutoff_model.py) bit for bit against skred_filter_coeffs_w on the grid and on 120 000 random bit patterns of the box, both
error tables against fp64 and the factor of 4 between them, finiteness and stability; the model of the calls against a plain loop over
every voice and every 64-frame step; landing, the block cuttings, TRACK under a bend and a glide, clamps and withheld records, the two
clear-rule scenes, every refusal with its return code, the packing and the permutation (through tests/c_cutoff_host.c, a program of
its own on a bank that is nothing but its size), and a mono line with a tracked low-pass on the oracle alone.

THE GRID: 201 values of w -- both ends of the box, 72 values spread geometrically over it, SKRED_CUTOFF_HALF_PI (the one seam of the
range reduction) and the 64 fp32 values on either side of it -- times 17 values of q (both ends, geometric) times the five modes.
THE FACTOR: the issue fixes it -- per mode and coefficient, the new function's largest absolute error against fp64 is at most 4 x
skred_filter_coeffs' (two polynomial results, each a few ulp off, feed the same divisions).
"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bend_model as BM
import cutoff_model as M
import glide_model as GM
import owner_model as OM
import owner_scenes as OS
from oracle import cpuref
from skred_amd import device

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
f32 = np.float32
SYMBOLS = ("skred_bank_cutoff_match", "skred_bank_cutoff_owned_each", "skred_bank_cutoff_tags_each", "skred_bank_cutoff_advance",
           "skred_bank_cutoff_stop", "skred_bank_download_cutoff")
QM = M.SET_Q | M.SET_MODE


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    L = device.load()
    for s in SYMBOLS + ("skred_cutoff_check", "skred_filter_coeffs_w"):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in device.ABI_SYMBOLS + device.HOST_ABI_SYMBOLS
    assert "filter cutoff on the device" in text and "THE ARITHMETIC" in text and "ADVANCE BY F FRAMES" in text
    # the header's literals are the model's
    for name, want in [("W_MIN", M.W_MIN), ("W_MAX", M.W_MAX), ("Q_MIN", M.Q_MIN), ("Q_MAX", M.Q_MAX), ("HALF_PI", M.HALF_PI), ("PI_HI", M.PI_HI),
                       ("PI_LO", M.PI_LO), ("RATE_MIN", M.RATE_MIN), ("RATE_MAX", M.RATE_MAX)] + \
                      [("S%d" % (k + 1), v) for k, v in enumerate(M.S)] + [("C%d" % (k + 1), v) for k, v in enumerate(M.C)]:
        lit = re.search(r"#define SKRED_CUTOFF_%s (\S+)f\b" % name, text).group(1)
        assert f32(float.fromhex(lit) if "x" in lit else float(lit)) == want, name


# ---------------------------------------------------------------------------------------------- the arithmetic

def grid():
    ws = [M.W_MIN, M.W_MAX, M.HALF_PI] + list(np.geomspace(2.0 ** -10, 3.0, 72).astype(f32))
    lo = hi = M.HALF_PI
    for _ in range(64):
        lo, hi = np.nextafter(lo, f32(0), dtype=f32), np.nextafter(hi, f32(4), dtype=f32)
        ws += [lo, hi]
    ws = np.unique(np.clip(np.array(ws, f32), M.W_MIN, M.W_MAX))
    qs = np.unique(np.r_[np.geomspace(2.0 ** -6, 2.0 ** 10, 17).astype(f32), M.Q_MIN, M.Q_MAX])
    w, q = (a.reshape(-1) for a in np.meshgrid(ws, qs, indexing="ij"))
    assert len(ws) == 201 and len(qs) == 17 and ws[0] == M.W_MIN and ws[-1] == M.W_MAX and qs[0] == M.Q_MIN and qs[-1] == M.Q_MAX
    return w, q


def lib_w(mode, w, q):
    L, out, r = device.load(), (C.c_float * 5)(), np.zeros((5, len(w)), f32)
    for i in range(len(w)):
        assert L.skred_filter_coeffs_w(int(mode if np.isscalar(mode) else mode[i]), float(w[i]), float(q[i]), out) == 0
        r[:, i] = out[:]
    return r


def lib_libm(mode, w, q):
    L, out, r = device.load(), (C.c_float * 5)(), np.zeros((5, len(w)), f32)
    two_pi = float(f32(2.0) * f32(np.pi))                            # freq / rate = w / (2 pi): skred_filter_coeffs forms 2 pi * w / (2 pi)
    for i in range(len(w)):
        assert L.skred_filter_coeffs(int(mode), float(w[i]), float(q[i]), two_pi, out) == 0
        r[:, i] = out[:]
    return r


def fp64(mode, w, q):
    w, q = w.astype(np.float64), q.astype(np.float64)
    sn, cs = np.sin(w), np.cos(w)
    al = sn / (2 * q)
    a0 = 1 + al
    b = {1: ((1 - cs) / 2, 1 - cs, (1 - cs) / 2), 2: ((1 + cs) / 2, -(1 + cs), (1 + cs) / 2), 3: (al, 0 * al, -al),
         4: (1 + 0 * al, -2 * cs, 1 + 0 * al), 5: (1 - al, -2 * cs, 1 + al)}[mode]
    return np.stack([b[0] / a0, b[1] / a0, b[2] / a0, -2 * cs / a0, (1 - al) / a0])


@pytest.fixture(scope="module")
def on_grid():
    w, q = grid()
    return w, q, {m: lib_w(m, w, q) for m in range(1, 6)}


def test_model_is_the_host_function_on_the_grid(on_grid):
    w, q, got = on_grid
    for mode in range(1, 6):
        assert M.coeffs(mode, w, q).tobytes() == got[mode].tobytes(), mode


def test_model_is_the_host_function_on_random_bit_patterns():
    rng = np.random.default_rng(74)
    n = 120000
    w = rng.integers(int(M.bits(M.W_MIN)), int(M.bits(M.W_MAX)) + 1, n).astype(np.uint32).view(f32)
    q = rng.integers(int(M.bits(M.Q_MIN)), int(M.bits(M.Q_MAX)) + 1, n).astype(np.uint32).view(f32)
    mode = rng.integers(1, 6, n)
    assert w.min() >= M.W_MIN and w.max() <= M.W_MAX and q.min() >= M.Q_MIN and q.max() <= M.Q_MAX
    got, want = lib_w(mode, w, q), M.coeffs(mode, w, q)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=0))
    assert not len(bad), (len(bad), w[bad[:4]], q[bad[:4]], mode[bad[:4]])
    assert np.isfinite(want).all()


def test_error_tables_and_the_factor_of_four(on_grid):
    w, q, got = on_grid
    print("mode | skred_filter_coeffs_w: b0 b1 b2 a1 a2 | skred_filter_coeffs: b0 b1 b2 a1 a2")
    worst = 0.0
    for mode in range(1, 6):
        ref = fp64(mode, w, q)
        ea, eo = np.abs(got[mode] - ref).max(axis=1), np.abs(lib_libm(mode, w, q) - ref).max(axis=1)
        print(mode, "|", " ".join("%.1e" % x for x in ea), "|", " ".join("%.1e" % x for x in eo))
        for k in range(5):
            assert ea[k] <= 4.0 * eo[k], (mode, M.COEFFS[k], ea[k], eo[k])
            worst = max(worst, ea[k] / eo[k] if eo[k] else 0.0)
    print("largest ratio %.2f" % worst)


def test_finite_and_stable_on_the_grid(on_grid):
    w, q, got = on_grid
    for mode in range(1, 6):
        c = got[mode]
        assert np.isfinite(c).all(), mode
        a1, a2 = c[3].astype(np.float64), c[4].astype(np.float64)
        assert (np.abs(a2) < 1).all() and (np.abs(a1) < 1 + a2).all(), mode
    assert device.filter_coeffs_w(0, 0.3, 0.9) is None
    for args in ((1, 2.0 ** -11, 0.9), (1, 3.0000002, 0.9), (1, 0.3, 2.0 ** -7), (1, 0.3, 1025.0), (1, float("nan"), 0.9)):
        assert device.load().skred_filter_coeffs_w(args[0], args[1], args[2], (C.c_float * 5)()) == RANGE, args
    assert device.load().skred_filter_coeffs_w(6, 0.3, 0.9, (C.c_float * 5)()) == BAD


# ---------------------------------------------------------------------------------------------- the model against a plain loop

def r32(x):
    """one rounding to fp32: the double result of one + - * / on fp32 operands rounds to the correctly rounded fp32 result"""
    return struct.unpack("f", struct.pack("f", x))[0]


def brute_coeffs(mode, w, q):
    """THE ARITHMETIC by another road: Python doubles, one r32 per operation"""
    w, q = float(f32(w)), float(f32(q))
    up = w > float(M.HALF_PI)
    r = r32(r32(float(M.PI_HI) - w) + float(M.PI_LO)) if up else w
    z = r32(r * r)
    p = float(M.S[3])
    for k in (2, 1, 0):
        p = r32(r32(p * z) + float(M.S[k]))
    sn = r32(r + r32(r32(r * z) * p))
    c = float(M.C[4])
    for k in (3, 2, 1, 0):
        c = r32(r32(c * z) + float(M.C[k]))
    c = r32(1.0 + r32(z * c))
    cs = -c if up else c
    al = r32(sn / r32(2.0 * q))
    a0 = r32(1.0 + al)
    m2 = r32(-2.0 * cs)
    if mode == 2:
        s = r32(1.0 + cs)
        b = (r32(s / 2.0), -s, r32(s / 2.0))
    elif mode == 3:
        b = (al, 0.0, -al)
    elif mode == 4:
        b = (1.0, m2, 1.0)
    elif mode == 5:
        b = (r32(1.0 - al), m2, r32(1.0 + al))
    else:
        d = r32(1.0 - cs)
        b = (r32(d / 2.0), d, r32(d / 2.0))
    return [r32(b[0] / a0), r32(b[1] / a0), r32(b[2] / a0), r32(m2 / a0), r32(r32(1.0 - al) / a0)]


def fbits(x):
    return struct.unpack("I", struct.pack("f", x))[0]


def bfloat(b):
    return struct.unpack("f", struct.pack("I", int(b)))[0]


def brute_store(filt, v, mode, wbits, qbits):
    for name, x in zip(M.COEFFS, brute_coeffs(mode, bfloat(wbits), bfloat(qbits))):
        filt[name][v] = f32(x)


def brute_voice(cut, bend, inc, filt, v, rec):
    """A RECORD ON VOICE v.  Returns (1: set or started, 2: withheld; clamped)."""
    row = [int(x) for x in cut[v]]
    has = row[M.W] != 0
    if not has and (rec.set & QM) != QM:
        return 2, False
    q = fbits(float(rec.q)) if rec.set & M.SET_Q else row[M.Q]
    mode = rec.mode if rec.set & M.SET_MODE else row[M.MODE]
    wn, clamped = fbits(float(rec.value)), False
    if rec.set & M.TRACK:
        k = int(inc.view(np.uint32)[v])
        if bend is not None and int(bend[v, 0]):
            k = int(bend[v, 0])
        k &= 0x7FFFFFFF
        if k == 0 or k >= 0x7F800000:
            return 2, False
        prod = bfloat(k) * float(rec.value)
        f = float("inf") if abs(prod) > 3.5e38 else r32(prod)
        clamped = not (float(M.W_MIN) <= f <= float(M.W_MAX))
        f = min(max(f, float(M.W_MIN)), float(M.W_MAX))
        wn = fbits(f)
    if rec.set & M.GLIDE and has:
        cut[v] = (row[M.W], wn, fbits(float(rec.rate_up)), fbits(float(rec.rate_down)), 0, q, mode, 0)
        return 1, clamped
    cut[v] = (wn, 0, 0, 0, 0, q, mode, 0)
    brute_store(filt, v, mode, wn, q)
    return 1, clamped


def brute_match(owner, cut, bend, inc, filt, first, count, K, fmask, match, rec):
    res = [0, 0, 0, 0]
    for s in range(first, first + count, K):
        o = int(owner[s])
        if o == 0 or (o & match[1]) != match[0]:
            res[2] += 1
            continue
        for l in range(K):
            if (fmask >> l) & 1:
                d, cl = brute_voice(cut, bend, inc, filt, s + l, rec)
                res[d - 1] += 1
                res[3] += int(cl and d == 1)
    return res


def brute_advance(cut, filt, first, count, frames):
    res = [0, 0]
    for v in range(first, first + count):
        w, t, up, down, carry, q, mode, _ = (int(x) for x in cut[v])
        if not t:
            continue
        c = carry + frames
        there = False
        for _ in range(c >> 6):                                      # every 64-frame step
            if there:
                break
            if w < t:
                w = fbits(r32(bfloat(w) * bfloat(up)))
                there = w >= t
            elif w > t:
                w = fbits(r32(bfloat(w) * bfloat(down)))
                there = w <= t
            else:
                there = True
        if there:
            cut[v] = (t, 0, 0, 0, 0, q, mode, 0)
            w = t
        else:
            cut[v] = (w, t, up, down, c & 63, q, mode, 0)
        res[1 if there else 0] += 1
        brute_store(filt, v, mode, w, q)
    return res


def small_bank(rng, n, K):
    inc = (rng.uniform(1e-3, 0.5, n) * rng.choice([1, 1, 1, -1], n)).astype(f32)
    inc[rng.integers(0, n, 4)] = 0.0
    inc[rng.integers(0, n, 3)] = f32(np.inf)
    inc[rng.integers(0, n, 2)] = f32(np.nan)
    inc[rng.integers(0, n, 3)] = f32(3e38)
    filt = np.zeros(n, [(c, f32) for c in M.COEFFS])
    for c in M.COEFFS:
        filt[c] = rng.uniform(-1, 1, n).astype(f32)
    owner = OM.new(n)
    heads = np.arange(0, n, K)
    owner[heads] = (rng.integers(1, 4, len(heads)).astype(np.uint32) << np.uint32(24)) | (heads // K + 1).astype(np.uint32)
    owner[heads[rng.integers(0, len(heads), 5)]] = 0
    bend = BM.new(n)
    bent = rng.integers(0, n, n // 8)
    bend[bent, 0] = M.bits(rng.uniform(1e-3, 0.5, len(bent)).astype(f32))
    bend[bent, 1] = M.bits(f32(1.25))
    return owner, M.new(n), bend, inc, filt


def records():
    up, down = M.per_64(40.0)
    return [M.Rec(M.ABS | QM, 0.25, 0.9, 1), M.Rec(M.TRACK | QM, 3.0, 2.0, 2), M.Rec(M.ABS | M.GLIDE, 2.5, rate_up=up, rate_down=down),
            M.Rec(M.TRACK | M.GLIDE | M.SET_Q, 0.5, 8.0, rate_up=1.5, rate_down=0.5), M.Rec(M.ABS, 0.01), M.Rec(M.TRACK | M.SET_MODE, 1e-4, mode=4),
            M.Rec(M.ABS | M.GLIDE | QM, float(M.W_MIN), 0.05, 5, rate_up=1.0 + 2.0 ** -23, rate_down=0.7), M.Rec(M.TRACK, 40.0),
            M.Rec(M.ABS | M.GLIDE, 1.5707964, rate_up=1.01, rate_down=0.99), M.Rec(M.ABS | QM, 3.0, 1024.0, 3)]


@pytest.mark.parametrize("K", [1, 4, 64])
def test_model_against_a_plain_loop(K):
    rng = np.random.default_rng(700 + K)
    n = 768
    owner, cut, bend, inc, filt = small_bank(rng, n, K)
    full = (1 << K) - 1
    part = full if K == 1 else (1 << (K - 1)) | 1
    seen, moved = [0, 0, 0, 0], [0, 0]
    for step, rec in enumerate(records() * 2):
        first = (int(rng.integers(0, n // K // 2)) * K) if step % 2 else 0
        count = (int(rng.integers(1, n // K // 2)) * K) if step % 2 else n
        match = ((int(rng.integers(1, 4)) << 24), 0xFF000000) if step % 3 else (0, 0)
        fmask = part if step % 4 == 3 else full
        b = bend if step % 2 else None
        ca, cb, fa, fb = cut.copy(), cut.copy(), filt.copy(), filt.copy()
        got = M.cutoff_match(owner, ca, b, inc, fa, first, count, K, fmask, match, rec)
        want = brute_match(owner, cb, b, inc, fb, first, count, K, fmask, match, rec)
        assert got == want and ca.tobytes() == cb.tobytes() and fa.tobytes() == fb.tobytes(), (K, step, got, want)
        cut, filt = ca, fa
        seen = [a + b for a, b in zip(seen, got)]
        for frames in (64, 37, 200):
            ca, cb, fa, fb = cut.copy(), cut.copy(), filt.copy(), filt.copy()
            got = M.advance(ca, fa, 0, n, frames)
            want = brute_advance(cb, fb, 0, n, frames)
            assert got == want and ca.tobytes() == cb.tobytes() and fa.tobytes() == fb.tobytes(), (K, step, frames, got, want)
            cut, filt = ca, fa
            moved = [a + b for a, b in zip(moved, got)]
    assert all(seen) and all(moved), (seen, moved)
    assert (cut[:, M.RESERVED] == 0).all() and (cut[:, M.CARRY] < 64).all()
    w = cut[cut[:, M.W] != 0, M.W].view(f32)
    assert (w >= M.W_MIN).all() and (w <= M.W_MAX).all()


# ---------------------------------------------------------------------------------------------- landing, cuttings, tracking

def one_voice_bank(n=8):
    filt = np.zeros(n, [(c, f32) for c in M.COEFFS])
    inc = np.full(n, 0.0123, f32)
    return M.new(n), inc, filt, OM.new(n)


@pytest.mark.parametrize("start,target", [(0.05, 1.9), (2.7, 0.004)])
def test_a_sweep_lands_on_the_targets_bits(start, target):
    cut, inc, filt, owner = one_voice_bank()
    owner[:] = 5
    up, down = M.per_64(60.0)
    M.cutoff_match(owner, cut, None, inc, filt, 0, 8, 1, 1, (0, 0), M.Rec(M.ABS | QM, start, 1.3, 1))
    M.cutoff_match(owner, cut, None, inc, filt, 0, 4, 1, 1, (0, 0), M.Rec(M.ABS | M.GLIDE, target, rate_up=up, rate_down=down))
    before = filt.copy()
    assert (cut[:4, M.TARGET] == M.bits(f32(target))).all() and (cut[:4, M.W] == M.bits(f32(start))).all()
    steps, res = 0, [4, 0]
    while res[0]:
        res = M.advance(cut, filt, 0, 8, 64)
        steps += 1
        assert steps < 2000
    assert steps > 20 and res == [0, 4]
    assert (cut[:4, M.W] == M.bits(f32(target))).all() and not cut[:4, M.TARGET:M.CARRY + 1].any()
    # a twin set with ABS at the target holds the same coefficient bits
    M.cutoff_match(owner, cut, None, inc, filt, 4, 4, 1, 1, (0, 0), M.Rec(M.ABS, target))
    assert filt[:4].tobytes() == filt[4:].tobytes() and filt[:4].tobytes() != before[:4].tobytes()
    assert cut[:4].tobytes() == cut[4:].tobytes()
    assert M.advance(cut, filt, 0, 8, 64) == [0, 0]


def test_three_block_cuttings_agree_at_every_multiple_of_64():
    cuttings = [(64,) * 8, (512,), (100, 412)]
    states = []
    for cutting in cuttings:
        cut, inc, filt, owner = one_voice_bank()
        owner[:] = 5
        inc[:] = np.linspace(0.01, 0.3, 8).astype(f32)
        M.cutoff_match(owner, cut, None, inc, filt, 0, 8, 1, 1, (0, 0), M.Rec(M.TRACK | QM, 2.0, 0.8, 1))
        M.cutoff_match(owner, cut, None, inc, filt, 0, 8, 1, 1, (0, 0), M.Rec(M.ABS | M.GLIDE, 1.0, rate_up=1.07, rate_down=0.93))
        at, seen = 0, {}
        for f in cutting:
            M.advance(cut, filt, 0, 8, f)
            at += f
            if at % 64 == 0:
                seen[at] = (cut.copy(), filt.copy())
        states.append(seen)
    for at, (c, f) in states[1].items():
        assert c.tobytes() == states[0][at][0].tobytes() and f.tobytes() == states[0][at][1].tobytes(), at
    for at, (c, f) in states[2].items():
        assert c.tobytes() == states[0][at][0].tobytes() and f.tobytes() == states[0][at][1].tobytes(), at
    assert set(states[1]) == set(states[2]) == {512} and len(states[0]) == 8
    assert states[0][512][0][:, M.TARGET].any() and not (states[0][512][0][:, M.CARRY]).any()


def test_track_reads_the_key_of_a_bent_and_of_a_gliding_voice():
    cut, inc, filt, owner = one_voice_bank()
    owner[:] = 5
    bend, glide = BM.new(8), GM.new(8)
    key = inc.copy()
    BM.apply(bend, inc, [0, 1], M.bits(f32(1.5)))                    # voices 0, 1 bent: the sounding increment is key * 1.5
    assert (inc[:2] != key[:2]).all()
    OM.tag_slots(owner, [2], [9], None, 1)
    GM.start_owned(owner, glide, inc, [GM.Glide(GM.FROM_SCALE, 2.0, 0.5, 0.25)], 1, 1, [2], [9])   # voice 2 glides up from a quarter
    assert inc[2] == key[2] * f32(0.25)
    value = f32(7.0)
    assert M.cutoff_match(owner, cut, bend, inc, filt, 0, 8, 1, 1, (0, 0), M.Rec(M.TRACK | QM, value, 0.9, 1)) == [8, 0, 0, 0]
    assert (cut[:2, M.W] == M.bits(key[:2] * value)).all(), "a bent voice tracks its key, not the wheel"
    assert cut[2, M.W] == M.bits(inc[2] * value) != M.bits(key[2] * value), "a gliding voice tracks where the glide is now"
    # without the bend array the sounding increment is all there is
    cut2 = M.new(8)
    M.cutoff_match(owner, cut2, None, inc, filt, 0, 8, 1, 1, (0, 0), M.Rec(M.TRACK | QM, value, 0.9, 1))
    assert (cut2[:2, M.W] == M.bits(inc[:2] * value)).all() and (cut2[:2, M.W] != cut[:2, M.W]).all()
    # a glide under the bend moves the key; the tracked cutoff follows when it is sent again
    GM.advance(glide, inc, 0, 8, 64)
    M.cutoff_match(owner, cut, bend, inc, filt, 0, 8, 1, 1, (0, 0), M.Rec(M.TRACK, value))
    assert cut[2, M.W] == M.bits(inc[2] * value) and inc[2] == key[2] * f32(0.5)


def test_clamps_and_withheld_records_are_counted():
    cut, inc, filt, owner = one_voice_bank()
    owner[:] = 5
    inc[:] = np.array([0.0, np.inf, np.nan, 3e38, 1e-30, 0.01, -0.01, 0.2], f32)
    before = filt.copy()
    res = M.cutoff_match(owner, cut, None, inc, filt, 0, 8, 1, 1, (0, 0), M.Rec(M.TRACK | QM, 10.0, 0.9, 1))
    assert res == [5, 3, 0, 2]                                       # zero, inf, nan withheld; 3e38 and 1e-30 clamped
    assert not cut[:3].any() and filt[:3].tobytes() == before[:3].tobytes()
    assert cut[3, M.W] == M.bits(M.W_MAX) and cut[4, M.W] == M.bits(M.W_MIN)
    assert cut[5, M.W] == cut[6, M.W] == M.bits(f32(0.01) * f32(10.0)), "|k|: a negative increment tracks like its positive twin"
    # an overflowing product is clamped, not withheld
    assert M.cutoff_match(owner, cut, None, inc, filt, 3, 1, 1, 1, (0, 0), M.Rec(M.TRACK, 1e30)) == [1, 0, 0, 1]
    # a first record without q and mode is withheld; a later one is not
    cut2 = M.new(8)
    assert M.cutoff_match(owner, cut2, None, inc, filt, 5, 3, 1, 1, (0, 0), M.Rec(M.ABS | M.SET_Q, 0.5, 0.9)) == [0, 3, 0, 0]
    assert not cut2.any()
    assert M.cutoff_match(owner, cut, None, inc, filt, 5, 3, 1, 1, (0, 0), M.Rec(M.ABS, 0.5)) == [3, 0, 0, 0]
    # GLIDE on a voice without a cutoff word sets it at once
    assert M.cutoff_match(owner, cut2, None, inc, filt, 5, 1, 1, 1, (0, 0), M.Rec(M.ABS | M.GLIDE | QM, 0.5, 0.9, 2, 1.5, 0.5)) == [1, 0, 0, 0]
    assert cut2[5].tolist() == [int(M.bits(f32(0.5))), 0, 0, 0, 0, int(M.bits(f32(0.9))), 2, 0]
    assert filt[5].tobytes() == M.coeffs(2, [f32(0.5)], [f32(0.9)])[:, 0].tobytes()


# ---------------------------------------------------------------------------------------------- the clear rule

def test_a_thief_and_a_restruck_key_do_not_inherit_a_moving_cutoff():
    """Two scenes on the model; each marked assertion fails with cutoff_model.CLEAR_RULE = False."""
    K, n = 4, 32
    filt = np.zeros(n, [(c, f32) for c in M.COEFFS])
    inc = np.full(n, 0.02, f32)
    owner, cut = OM.new(n), M.new(n)
    sweep = M.Rec(M.ABS | M.GLIDE, 2.0, rate_up=1.2, rate_down=0.8)
    for scene, new_tag in (("a re-struck key", 60), ("a thief", 99)):
        slot = 8 if scene == "a thief" else 16
        OM.tag_slots(owner, [slot], [60], None, K)
        M.tag_clear(cut, [slot], 1, None, K)
        assert M.cutoff_tags_each(owner, cut, None, inc, filt, [M.Rec(M.ABS | QM, 0.1, 0.9, 1)], 0, n, K, 0xF, [60])[0] == [K, 0, 0, 0]
        assert M.cutoff_tags_each(owner, cut, None, inc, filt, [sweep], 0, n, K, 0xF, [60])[0] == [K, 0, 0, 0]
        assert M.advance(cut, filt, 0, n, 64) == [K, 0]
        held = filt[slot:slot + K].copy()
        OM.tag_slots(owner, [slot], [new_tag], None, K)              # the new note's tag launch
        M.tag_clear(cut, [slot], 1, None, K)
        assert not cut[slot:slot + K].any(), scene                   # CLEAR RULE
        assert M.advance(cut, filt, 0, n, 64) == [0, 0], scene       # CLEAR RULE: the old sweep would move the new note's filter
        assert filt[slot:slot + K].tobytes() == held.tobytes(), scene   # CLEAR RULE; the coefficients stay what they were
        # the new note's first record needs q and mode again
        assert M.cutoff_tags_each(owner, cut, None, inc, filt, [M.Rec(M.ABS, 0.3)], 0, n, K, 0xF, [new_tag])[0] == [0, K, 0, 0]   # CLEAR RULE
        OM.clear(owner, slot, K)
        cut[slot:slot + K] = 0


def test_the_scenes_fail_without_the_clear_rule():
    M.CLEAR_RULE = False
    try:
        with pytest.raises(AssertionError):
            test_a_thief_and_a_restruck_key_do_not_inherit_a_moving_cutoff()
    finally:
        M.CLEAR_RULE = True


# ---------------------------------------------------------------------------------------------- the entry points' host checks

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cutoff") / "c_cutoff_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-I" + os.path.join(rocm, "include"), os.path.join(HERE, "c_cutoff_host.c"), os.path.join(CSRC, "skred_bank_cutoff.c"), "-o", exe,
           "-L" + os.path.join(ROOT, "skred_amd"), "-lskred_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-lm", "-lpthread",
           "-Wl,-rpath," + os.path.join(ROOT, "skred_amd"), "-Wl,-rpath," + os.path.join(rocm, "lib")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return out.stdout.strip().splitlines()


def test_host_program(host_lines):
    bad = [l for l in host_lines[:-1] if not l.endswith(" ok")]
    assert not bad, bad
    assert host_lines[-1] == "OK" and len(host_lines) >= 120
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "coeffs", "check", "pack", "perm", "match", "owned", "tags", "advance", "stop", "download", "untouched"}, groups


def test_check_through_ctypes_is_the_models():
    up, down = M.per_64(30.0)
    cases = [([M.Rec(M.ABS | QM, 0.3, 0.9, 1)], 8, 0x77, 0x55, False), (None, 8, 0x77, 0x55, False), ([M.Rec(M.ABS, 0.3)], 12, 0x77, 0x55, False),
             ([M.Rec(M.ABS, 0.3)], 8, 0, 0x55, False), ([M.Rec(M.ABS, 0.3)], 8, 0x77, 0, False), ([M.Rec(M.ABS, 0.3)], 8, 0x77, 0x155, False),
             ([M.Rec(M.ABS, 0.3)], 8, 0x11, 0x55, False), ([M.Rec(M.ABS | M.TRACK, 0.3)], 8, 0x77, 0x55, False), ([M.Rec(QM, 0.3, 0.9, 1)], 8, 0x77, 0x55, False),
             ([M.Rec(M.ABS | 32, 0.3)], 8, 0x77, 0x55, False), ([M.Rec(M.ABS, 0.3, reserved=(0, 3))], 8, 0x77, 0x55, False),
             ([M.Rec(M.ABS, 0.3)], 8, 0x77, 0x55, True), ([M.Rec(M.ABS | QM, 0.3, 0.9, 1)], 8, 0x77, 0x55, True),
             ([M.Rec(M.ABS, float("nan"))], 8, 0x77, 0x55, False), ([M.Rec(M.ABS | M.SET_Q, 0.3, float("inf"))], 8, 0x77, 0x55, False),
             ([M.Rec(M.ABS, 3.5)], 8, 0x77, 0x55, False), ([M.Rec(M.ABS, 2.0 ** -11)], 8, 0x77, 0x55, False), ([M.Rec(M.TRACK, 0.0)], 8, 0x77, 0x55, False),
             ([M.Rec(M.TRACK, 1e30)], 8, 0x77, 0x55, False), ([M.Rec(M.ABS | M.SET_Q, 0.3, 2.0 ** -7)], 8, 0x77, 0x55, False),
             ([M.Rec(M.ABS | M.SET_MODE, 0.3, mode=6)], 8, 0x77, 0x55, False), ([M.Rec(M.ABS | M.GLIDE, 0.3, rate_up=up, rate_down=down)], 8, 0x77, 0x55, False),
             ([M.Rec(M.ABS | M.GLIDE, 0.3, rate_up=1.0, rate_down=down)], 8, 0x77, 0x55, False), ([M.Rec(M.ABS | M.GLIDE, 0.3, rate_up=up, rate_down=1.0)], 8, 0x77, 0x55, False),
             ([M.Rec(M.ABS | M.GLIDE, 0.3, rate_up=17.0, rate_down=down)], 8, 0x77, 0x55, False), ([M.Rec(M.ABS | M.GLIDE, 0.3, rate_up=up, rate_down=0.01)], 8, 0x77, 0x55, False),
             ([M.Rec(M.ABS, 9.0)], 8, 0x11, 0x55, False), ([M.Rec(M.ABS | M.TRACK, 9.0)], 3, 0, 0, False)]
    seen = set()
    for recs, K, vm, fm, first in cases:
        got = device.cutoff_check([r.c() for r in recs] if recs is not None else None, K, vm, fm, first)
        assert got == M.check(recs, K, vm, fm, first), (K, vm, fm, first, recs and vars(recs[0]))
        seen.add(got)
    assert seen == {0, BAD, RANGE}


# ---------------------------------------------------------------------------------------------- a mono line on the oracle

def filtered(bank, K, members, mode=1):
    """the bank with the filter of voices `members` of every copy switched on (coefficients of a 2 kHz low-pass until a call says otherwise)"""
    sel = np.isin(np.arange(bank.n) % K, members)
    bank["voice_filter_mode"][sel] = mode
    for c, v in zip(M.COEFFS, device.filter_coeffs(mode, 2000.0, 0.707, 44100.0)):
        bank["voice_filter"][c][sel] = v
    return sel


def test_a_mono_line_with_a_tracked_low_pass_on_the_oracle():
    """tests/owner_scenes.py's bank (3.sk tiled over 256 voices, K = 4) with its carriers filtered, one slot, three keys.  Both lines
    play the same keys; ahead of every key each line sends its tracked low-pass (harmonic 3 on one line, harmonic 12 on the other)
    through the model, whose coefficient stores go into the oracle's bank.  The stems of the slot's carriers differ between the lines
    in every key, nothing outside the slot ever changes, and with the same harmonic on both lines the stems are equal bit for bit."""
    K, N, F = OS.K, OS.N, OS.F
    slot = int(OS.others()[5])
    vs = np.arange(slot, slot + K)
    rest = np.setdiff1d(np.arange(N), vs)

    def line(harmonic):
        bank, tables, g = OS.bank()
        filtered(bank, K, OS.MEMBERS)
        owner, cut = OM.new(N), M.new(N)
        OM.tag_slots(owner, [slot], [0x03000030], None, K)
        base = bank["voice_phase_inc"][vs].copy()
        size = int(bank["voice_table_size"][slot])
        out, ws = [], []
        for semis in (0, 5, -3):
            bank["voice_phase_inc"][vs] = (base * f32(2.0 ** (semis / 12.0))).astype(f32)
            res, _ = M.cutoff_tags_each(owner, cut, None, bank["voice_phase_inc"], bank["voice_filter"],
                                        [M.Rec(M.TRACK | QM, M.track_value(harmonic, size), 2.0, 1)], 0, N, K, OS.MMASK, [0x03000030])
            assert res[0] == len(OS.MEMBERS) and res[1] == 0
            ws.append(cut[vs[0], M.W].view(f32))
            for _ in range(3):
                out.append(cpuref.render(bank, g, tables, F, 0, want_stems=True)["stems"].copy())
        return out, ws

    a, wa = line(3.0)
    b, wb = line(12.0)
    c, wc = line(3.0)
    assert wa[1] > wa[0] > wa[2] and all(y > x for x, y in zip(wa, wb)), "the cutoff follows the key and the harmonic"
    for k, (x, y, z) in enumerate(zip(a, b, c)):
        assert x[:, rest].tobytes() == y[:, rest].tobytes(), f"block {k}: a voice outside the slot changed"
        assert x[:, vs[:3]].tobytes() != y[:, vs[:3]].tobytes(), f"block {k}: the tracking value left the stems alone"
        assert x.tobytes() == z.tobytes(), f"block {k}: the same line twice differs"
        assert np.abs(x[:, vs[:3]]).sum() > 0
