"""Filter cutoff on the device, stated in numpy: the coefficient arithmetic operation by operation, and the cutoff words and the five
coefficient words as pure functions of the call sequence.  Written from the definition in include/skred_amd.h (section "filter cutoff
on the device"), not from the kernels.

`cut` is a uint32 array of shape (n_voices, 8): w, target, rate_up, rate_down (fp32 bit patterns), carry, q (bits), mode, 0 per voice;
w == 0 is "no device cutoff", target == 0 "not moving".  `inc` is the bank's voice_phase_inc (float32, read only), `filt` its
voice_filter (a structured array with b0 b1 b2 a1 a2, stored in place), `bend` bend_model's array or None.  Every operation is one
np.float32 operation: the IEEE round-to-nearest result the device's __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn give.  Inside the box
no operand or result is denormal.

The guard and the find pass are owner_model's.  `CLEAR_RULE` switched off gives the model of a bank whose tag launches leave the
cutoff words alone: the tests name the assertions that fail on it.
"""
import numpy as np

import ctl_model as CM
import owner_model as OM
import slot_model as SM

f32 = np.float32
W, TARGET, RATE_UP, RATE_DOWN, CARRY, Q, MODE, RESERVED = range(8)
ABS, TRACK, GLIDE, SET_Q, SET_MODE = 1, 2, 4, 8, 16
ALL = 31
BAD, RANGE = -2, -4
CLEAR_RULE = True
COEFFS = ("b0", "b1", "b2", "a1", "a2")

W_MIN, W_MAX = f32(2.0 ** -10), f32(3.0)
Q_MIN, Q_MAX = f32(2.0 ** -6), f32(2.0 ** 10)
RATE_MIN, RATE_MAX = f32(2.0 ** -4), f32(2.0 ** 4)
HALF_PI = f32(float.fromhex("0x1.921fb6p+0"))
PI_HI = f32(float.fromhex("0x1.921fb6p+1"))
PI_LO = f32(float.fromhex("-0x1.777a5cp-24"))
S = [f32(float.fromhex(x)) for x in ("-0x1.555548p-3", "0x1.110e6ap-7", "-0x1.9f5ff4p-13", "0x1.5cf92cp-19")]            # S1 .. S4
C = [f32(float.fromhex(x)) for x in ("-0x1p-1", "0x1.555548p-5", "-0x1.6c138p-10", "0x1.9f6f7ep-16", "-0x1.18003p-22")]   # C1 .. C5
ONE, TWO, MINUS_TWO = f32(1.0), f32(2.0), f32(-2.0)


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


def flt(b):
    return np.asarray(b, np.uint32).view(f32)


def new(n_voices):
    return np.zeros((n_voices, 8), np.uint32)


def sincos(w):
    """steps 1 .. 4 of THE ARITHMETIC on a float32 array"""
    w = np.asarray(w, f32)
    upper = w > HALF_PI
    r = np.where(upper, (PI_HI - w) + PI_LO, w).astype(f32)
    z = r * r
    p = np.full_like(z, S[3])
    for k in (S[2], S[1], S[0]):
        p = p * z
        p = p + k
    t = r * z
    t = t * p
    sn = r + t
    c = np.full_like(z, C[4])
    for k in (C[3], C[2], C[1], C[0]):
        c = c * z
        c = c + k
    c = z * c
    c = ONE + c
    cs = np.where(upper, -c, c).astype(f32)
    assert sn.dtype == f32 and cs.dtype == f32
    return sn, cs


def coeffs(mode, w, q):
    """THE ARITHMETIC: (5, n) float32 -- b0 b1 b2 a1 a2 -- for arrays of mode (1 .. 5), w and q inside the box"""
    mode, w, q = np.broadcast_arrays(np.asarray(mode, np.int64), np.asarray(w, f32), np.asarray(q, f32))
    sn, cs = sincos(w)
    alpha = sn / (TWO * q)
    a0 = ONE + alpha
    d, s = ONE - cs, ONE + cs
    m2cs = MINUS_TWO * cs
    one = np.ones_like(cs)
    zero = np.zeros_like(cs)
    b0 = np.select([mode == 2, mode == 3, mode == 4, mode == 5], [s / TWO, alpha, one, ONE - alpha], d / TWO)
    b1 = np.select([mode == 2, mode == 3, mode == 4, mode == 5], [-s, zero, m2cs, m2cs], d)
    b2 = np.select([mode == 2, mode == 3, mode == 4, mode == 5], [s / TWO, -alpha, one, ONE + alpha], d / TWO)
    out = np.stack([b0 / a0, b1 / a0, b2 / a0, m2cs / a0, (ONE - alpha) / a0])
    assert out.dtype == f32
    return out


class Rec:
    """one skred_cutoff_t"""

    def __init__(self, set, value, q=0.0, mode=0, rate_up=0.0, rate_down=0.0, reserved=(0, 0)):
        self.set, self.value, self.q, self.mode = int(set), f32(value), f32(q), int(mode)
        self.rate_up, self.rate_down, self.reserved = f32(rate_up), f32(rate_down), tuple(reserved)

    def c(self):
        from skred_amd import device
        r = device.cutoff(self.set, float(self.value), float(self.q), self.mode, float(self.rate_up), float(self.rate_down))
        r.reserved[0], r.reserved[1] = self.reserved
        return r


def _in_box(x, lo, hi):
    return bool(np.isfinite(x) and lo <= x <= hi)


def check(recs, K, voice_mask, filter_mask, first_time=False):
    """skred_cutoff_check: 0, SKRED_E_BAD_ARG or SKRED_E_RANGE, in the header's order (None: a NULL array)."""
    if recs is None:
        return BAD
    if K < 1 or K > 64 or K & (K - 1):
        return RANGE
    for m in (voice_mask, filter_mask):
        if not m or (K < 64 and m >> K):
            return BAD
    for r in recs:
        how = r.set & (ABS | TRACK)
        if r.set & ~ALL or how not in (ABS, TRACK):
            return BAD
        if first_time and (r.set & (SET_Q | SET_MODE)) != (SET_Q | SET_MODE):
            return BAD
        if any(r.reserved):
            return BAD
        glide = bool(r.set & GLIDE)
        if not np.isfinite(r.value) or (r.set & SET_Q and not np.isfinite(r.q)) or (glide and not (np.isfinite(r.rate_up) and np.isfinite(r.rate_down))):
            return BAD
        if r.set & SET_Q and not _in_box(r.q, Q_MIN, Q_MAX):
            return RANGE
        if how == ABS and not _in_box(r.value, W_MIN, W_MAX):
            return RANGE
        if how == TRACK and not r.value > 0:
            return RANGE
        if r.set & SET_MODE and not 1 <= r.mode <= 5:
            return RANGE
        if glide:
            if not _in_box(r.rate_up, RATE_MIN, RATE_MAX) or not _in_box(r.rate_down, RATE_MIN, RATE_MAX):
                return RANGE
            if not r.rate_up > 1 or not r.rate_down < 1:
                return BAD
    if filter_mask & ~voice_mask:
        return BAD
    return 0


def store(filt, vs, c5):
    for k, name in enumerate(COEFFS):
        filt[name][vs] = c5[k]


def apply(cut, bend, inc, filt, voices, rec):
    """A RECORD ON VOICE v for `voices` (distinct indices).  Returns [set or started, withheld, clamped]."""
    vs = np.asarray(voices, np.int64).reshape(-1)
    if not len(vs):
        return [0, 0, 0]
    a = cut[vs]
    has = a[:, W] != 0
    both = (rec.set & (SET_Q | SET_MODE)) == (SET_Q | SET_MODE)
    withheld = ~has & (not both)
    q = np.where(rec.set & SET_Q, bits(rec.q), a[:, Q]).astype(np.uint32)
    mode = np.where(rec.set & SET_MODE, np.uint32(rec.mode), a[:, MODE]).astype(np.uint32)
    wn = np.full(len(vs), bits(rec.value), np.uint32)
    clamped = np.zeros(len(vs), bool)
    if rec.set & TRACK:
        k = inc.view(np.uint32)[vs].copy()
        if bend is not None:
            key = bend[vs, 0]
            k = np.where(key != 0, key, k)
        k &= np.uint32(0x7FFFFFFF)
        withheld |= (k == 0) | (k >= 0x7F800000)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            f = (flt(k) * rec.value).astype(f32)
            clamped = ~((f >= W_MIN) & (f <= W_MAX))
            f = np.where(f < W_MIN, W_MIN, np.where(f > W_MAX, W_MAX, f)).astype(f32)
        wn = bits(f)
    ok = ~withheld
    start = ok & has & bool(rec.set & GLIDE)
    now = ok & ~start
    a[start, TARGET] = wn[start]
    a[start, RATE_UP], a[start, RATE_DOWN] = bits(rec.rate_up), bits(rec.rate_down)
    a[now, W] = wn[now]
    a[now, TARGET] = a[now, RATE_UP] = a[now, RATE_DOWN] = 0
    a[ok, CARRY] = 0
    a[ok, Q], a[ok, MODE] = q[ok], mode[ok]
    cut[vs] = a
    if now.any():
        store(filt, vs[now], coeffs(mode[now], flt(wn[now]), flt(q[now])))
    return [int(ok.sum()), int(withheld.sum()), int((clamped & ok).sum())]


def matches(owner, heads, match):
    value, mask = (np.uint32(x) for x in match)
    words = owner[heads]
    return (words != 0) & ((words & mask) == value)


def cutoff_match(owner, cut, bend, inc, filt, first, count, K, filter_mask, match, rec):
    """The channel sweep.  Returns [set or started, withheld, slots of the range that did not match, clamped]."""
    full = (1 << K) - 1
    assert check([rec], K, full, filter_mask) == 0 and first % K == 0 and count % K == 0 and count > 0
    heads = np.arange(first, first + count, K)
    hit = matches(owner, heads, match)
    lanes = np.array(SM.lanes(filter_mask, K), np.int64)
    vs = (heads[hit][:, None] + lanes[None, :]).reshape(-1)
    a = apply(cut, bend, inc, filt, vs, rec)
    return [a[0], a[1], int((~hit).sum()), a[2]]


def cutoff_owned_each(owner, cut, bend, inc, filt, recs, K, filter_mask, entries, tags, count=None):
    """Returns [set or started, withheld, slots whose owner differs, clamped]."""
    assert OM.tags_check(tags) == 0 and check(recs, K, (1 << K) - 1, filter_mask) == 0 and len(recs) == len(tags)
    res = [0, 0, 0, 0]
    seen = set()
    lanes = np.array(SM.lanes(filter_mask, K), np.int64)
    for k, e in enumerate(OM.looked(entries, len(tags), count)):
        if not CM.slot_valid(e, K, len(owner)):
            continue
        if int(owner[e]) != int(tags[k]):
            res[2] += 1
            continue
        assert e not in seen, "a slot named twice: unspecified"
        seen.add(e)
        a = apply(cut, bend, inc, filt, e + lanes, recs[k])
        res = [res[0] + a[0], res[1] + a[1], res[2], res[3] + a[2]]
    return res


def cutoff_tags_each(owner, cut, bend, inc, filt, recs, first, count, K, filter_mask, tags):
    """find_owned, then cutoff_owned_each on its list.  Returns (d_result, the list)."""
    lst = OM.find_owned(owner, first, count, K, tags)
    res = cutoff_owned_each(owner, cut, bend, inc, filt, recs, K, filter_mask, lst, tags)
    assert res[2] == 0
    return res, lst


def advance(cut, filt, first, count, frames):
    """ADVANCE BY F FRAMES over [first, first + count).  Returns [still moving, arrived]."""
    assert 1 <= frames <= 65536
    g = cut[first:first + count]
    on = g[:, TARGET] != 0
    t = g[:, TARGET]
    cur = g[:, W].copy()
    there = np.zeros(len(g), bool)
    c = g[:, CARRY] + np.uint32(frames)
    m = c >> np.uint32(6)
    for step in range(int(m[on].max()) if on.any() else 0):
        act = on & ~there & (m > step)
        if not act.any():
            break
        up, down, level = act & (cur < t), act & (cur > t), act & (cur == t)
        cur = np.where(up, bits(flt(cur) * flt(g[:, RATE_UP])), np.where(down, bits(flt(cur) * flt(g[:, RATE_DOWN])), cur)).astype(np.uint32)
        there |= level | (up & (cur >= t)) | (down & (cur <= t))
    still = on & ~there
    g[there, W] = t[there]
    g[still, W] = cur[still]
    g[still, CARRY] = c[still] & np.uint32(63)
    g[there, TARGET] = g[there, RATE_UP] = g[there, RATE_DOWN] = g[there, CARRY] = 0
    if on.any():
        vs = first + np.flatnonzero(on)
        store(filt, vs, coeffs(g[on, MODE], flt(g[on, W]), flt(g[on, Q])))
    return [int(still.sum()), int(there.sum())]


def stop(cut, filt, first, count, snap):
    g = cut[first:first + count]
    on = g[:, TARGET] != 0
    if snap and on.any():
        g[on, W] = g[on, TARGET]
        store(filt, first + np.flatnonzero(on), coeffs(g[on, MODE], flt(g[on, W]), flt(g[on, Q])))
    g[on, TARGET] = g[on, RATE_UP] = g[on, RATE_DOWN] = g[on, CARRY] = 0


def tag_clear(cut, entries, n_tags, count, K):
    """what follows every tag launch once the array exists: all eight words of all K voices of the tagged slots"""
    if not CLEAR_RULE:
        return
    for e in OM.looked(entries, n_tags, count):
        if CM.slot_valid(e, K, len(cut)):
            cut[e:e + K] = 0


def per_64(octaves_per_second, rate=44100.0):
    """(rate_up, rate_down) of a sweep of that speed: the factor per 64 frames"""
    r = 2.0 ** (octaves_per_second * 64.0 / rate)
    return f32(r), f32(1.0 / r)


def track_value(harmonic, table_size):
    """what the host supplies with TRACK: harmonic * 2 pi / table_size"""
    return f32(harmonic * 2.0 * np.pi / table_size)
