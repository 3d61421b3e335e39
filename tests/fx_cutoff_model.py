"""Filter cutoff on the fixed-point bank, stated in Python integers of unbounded width: THE ARITHMETIC (the five Q2.30 words as a pure
function of mode, w_q29 and q_q16) and the cutoff words and coefficient words as pure functions of the call sequence.  Written from the
definition in include/skred_amd_fxpt.h (section "filter cutoff"), not from the kernels.

`cut` is a uint32 array of shape (n_voices, 8): w_q29, target_q29, up_q32, down_q32, carry, q_q16, mode, 0.  `inc` is the bank's
phase_inc (uint32), `bend` fx_bend_model's array or None, `filt` a dict of the five int32 coefficient arrays (the bank's b0_q30 ..
a2_q30, changed in place).  Nothing here rounds in floating point: the model, skred_fx_filter_coeffs_w and the device must agree bit for
bit.  coeffs(..., widths=dict) also records the largest magnitude every named intermediate reached, for the header's bounds.

CLEAR_RULE = False gives the model of a bank whose tag launches leave the cutoff words alone: the scenes of tests/test_fx_cutoff_cpu.py
fail on it.
"""
import numpy as np

import fx_owner_model as om

W, TARGET, UP, DOWN, CARRY, Q, MODE, RESERVED = range(8)
ABS, TRACK, GLIDE, SET_Q, SET_MODE = 1, 2, 4, 8, 16
ALL = 31
BAD, RANGE = -2, -4
COEFFS = ("b0_q30", "b1_q30", "b2_q30", "a1_q30", "a2_q30")
CLEAR_RULE = True

W_MIN, W_MAX = 1 << 19, 3 << 29            # [2^-10, 3] in Q29
Q_MIN, Q_MAX = 1 << 10, 1 << 26            # [2^-6, 2^10] in Q16
PI_Q29, HALF_PI_Q29 = 1686629713, 843314857
ONE_Q30, ONE_Q31 = 1 << 30, 1 << 31
S = (-1431655761, 286331072, -27269072, 1513217, -52533)          # S1 .. S5, Q31
C = (1431655759, -190887371, 13634516, -605274, 17511)            # C2 .. C6, Q31
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

# the widths the header states: name -> bits of the magnitude (the signed ones need one bit more and fit int64 with it)
STATED_BITS = {"r": 30, "rr": 60, "z": 32, "sine product": 63, "sinc": 32, "r * sinc": 61, "cosine product": 63, "t": 30,
               "t * z": 62, "cos": 32, "q << 15": 42, "rs + half": 62, "alpha": 36, "a0": 36, "numerator": 36, "numerator << s": 64,
               "quotient": 29, "remainder << 2": 39, "result": 32}


def _note(widths, name, value):
    if widths is not None:
        widths[name] = max(widths.get(name, 0), abs(int(value)))


def rshift_round(x, s):
    """(x + 2^(s-1)) >> s, the shift arithmetic (a floor): to nearest, ties towards plus infinity"""
    return (x + (1 << (s - 1))) >> s


def sincos(w, widths=None):
    """rs = sin(w) in Q60, cs = cos(w) in Q31 for w_q29 in the box"""
    upper = w > HALF_PI_Q29
    r = PI_Q29 - w if upper else w
    rr = r * r
    z = rshift_round(rr, 28)                 # (r / 2)^2 in Q32
    _note(widths, "r", r), _note(widths, "rr", rr), _note(widths, "z", z)
    p = S[4]
    for k in (3, 2, 1, 0):
        _note(widths, "sine product", p * z)
        p = rshift_round(p * z, 32) + S[k]
    _note(widths, "sine product", p * z)
    sinc = ONE_Q31 + rshift_round(p * z, 32)
    _note(widths, "sinc", sinc), _note(widths, "r * sinc", r * sinc)
    rs = r * sinc                            # sin(w) in Q60
    c = C[4]
    for k in (3, 2, 1, 0):
        _note(widths, "cosine product", c * z)
        c = rshift_round(c * z, 32) + C[k]
    _note(widths, "cosine product", c * z)
    t = rshift_round(c * z, 32)
    _note(widths, "t", t), _note(widths, "t * z", t * z)
    cos = ONE_Q31 - z + rshift_round(t * z, 32)
    _note(widths, "cos", cos)
    return rs, (-cos if upper else cos)


def quotient(num, a0, s, widths=None):
    """round(num * 2^(s + 2) / a0) on the magnitude, ties away from zero, the sign put back: two divides, nothing above 64 bits"""
    n = abs(num)
    _note(widths, "numerator", n), _note(widths, "numerator << s", n << s)
    qa, ra = divmod(n << s, a0)
    _note(widths, "quotient", qa), _note(widths, "remainder << 2", (ra << 2) + (a0 >> 1))
    res = (qa << 2) + ((ra << 2) + (a0 >> 1)) // a0
    _note(widths, "result", res)
    res = -res if num < 0 else res
    return max(I32_MIN, min(I32_MAX, res))


def coeffs(mode, w, q, widths=None):
    """THE ARITHMETIC: the five Q2.30 words b0 b1 b2 a1 a2 of (mode 1 .. 5, w_q29, q_q16), all in the box"""
    mode, w, q = int(mode), int(w), int(q)
    assert 1 <= mode <= 5 and W_MIN <= w <= W_MAX and Q_MIN <= q <= Q_MAX
    rs, cs = sincos(w, widths)
    den = q << 15
    _note(widths, "q << 15", den), _note(widths, "rs + half", rs + (den >> 1))
    alpha = (rs + (den >> 1)) // den         # sn / (2 q) in Q30, to nearest
    a0 = ONE_Q30 + alpha
    _note(widths, "alpha", alpha), _note(widths, "a0", a0)
    quo = lambda num, s=28: quotient(num, a0, s, widths)
    # cs is Q31: 1 -+ cs as Q31 numerators take a shift one shorter, their halves one shorter again; -2 cs in Q30 is -cs as it stands
    if mode == 1:
        d = ONE_Q31 - cs
        b0 = quo(d, 26); b1 = quo(d, 27); b2 = b0
    elif mode == 2:
        s = ONE_Q31 + cs
        b0 = quo(s, 26); b1 = quo(-s, 27); b2 = b0
    elif mode == 3:
        b0 = quo(alpha); b1 = 0; b2 = quo(-alpha)
    elif mode == 4:
        b0 = quo(ONE_Q30); b1 = quo(-cs); b2 = b0
    else:
        b0 = quo(ONE_Q30 - alpha); b1 = quo(-cs); b2 = quo(a0)
    return [b0, b1, b2, quo(-cs), quo(ONE_Q30 - alpha)]


def coeffs_fp64(mode, w, q):
    """the RBJ formulas in fp64 on the exact rationals w_q29 / 2^29 and q_q16 / 2^16, in units of 2^-30"""
    wf, qf = w / float(1 << 29), q / float(1 << 16)
    sn, cs = np.sin(wf), np.cos(wf)
    alpha = sn / (2.0 * qf)
    a0 = 1.0 + alpha
    b = {1: ((1 - cs) / 2, 1 - cs, (1 - cs) / 2), 2: ((1 + cs) / 2, -(1 + cs), (1 + cs) / 2), 3: (alpha, 0.0, -alpha),
         4: (1.0, -2 * cs, 1.0), 5: (1 - alpha, -2 * cs, 1 + alpha)}[mode]
    return [x / a0 * (1 << 30) for x in (*b, -2 * cs, 1 - alpha)]


class Rec:
    """skred_fx_cutoff_t"""

    def __init__(self, set, value, q_q16=0, mode=0, up_q32=0, down_q32=0, reserved=(0, 0)):
        self.set, self.value, self.q_q16, self.mode = int(set), int(value), int(q_q16), int(mode)
        self.up_q32, self.down_q32, self.reserved = int(up_q32), int(down_q32), tuple(reserved)

    def c(self):
        from skred_amd import fxbank as fxb
        r = fxb.fx_cutoff(self.set, self.value, self.q_q16, self.mode, self.up_q32, self.down_q32)
        r.reserved[0], r.reserved[1] = self.reserved
        return r


def new(n_voices):
    return np.zeros((n_voices, 8), np.uint32)


def check(recs, n=None, first_time=False):
    """skred_fx_cutoff_check: 0, SKRED_E_BAD_ARG or SKRED_E_RANGE, in the header's order (None: a NULL array)"""
    if recs is None or (n is not None and n < 0):
        return BAD
    for r in list(recs)[:n]:
        how = r.set & (ABS | TRACK)
        if r.set & ~ALL or how not in (ABS, TRACK):
            return BAD
        if first_time and (r.set & (SET_Q | SET_MODE)) != (SET_Q | SET_MODE):
            return BAD
        if any(r.reserved):
            return BAD
        if r.set & SET_Q and not Q_MIN <= r.q_q16 <= Q_MAX:
            return RANGE
        if how == ABS and not W_MIN <= r.value <= W_MAX:
            return RANGE
        if how == TRACK and r.value == 0:
            return RANGE
        if r.set & SET_MODE and not 1 <= r.mode <= 5:
            return RANGE
        if r.set & GLIDE and (r.up_q32 == 0 or r.down_q32 == 0):
            return BAD
    return 0


def store(filt, v, c5):
    for k, name in enumerate(COEFFS):
        filt[name][v] = c5[k]


def track(k, value):
    """(wn, clamped) of a key word k != 0 and a tracking value"""
    wn = (int(k) * int(value)) >> 27
    return max(W_MIN, min(W_MAX, wn)), not W_MIN <= wn <= W_MAX


def apply(cut, bend, inc, filt, voices, rec):
    """A RECORD ON VOICE v for `voices` (distinct indices).  Returns [set or started, withheld, clamped]."""
    res = [0, 0, 0]
    for v in np.asarray(voices, np.int64).reshape(-1).tolist():
        a = [int(x) for x in cut[v]]
        has = a[W] != 0
        if not has and (rec.set & (SET_Q | SET_MODE)) != (SET_Q | SET_MODE):
            res[1] += 1
            continue
        q = rec.q_q16 if rec.set & SET_Q else a[Q]
        mode = rec.mode if rec.set & SET_MODE else a[MODE]
        wn, clamped = rec.value, False
        if rec.set & TRACK:
            k = int(inc[v])
            if bend is not None and int(bend[v, 0]):
                k = int(bend[v, 0])
            if k == 0:
                res[1] += 1
                continue
            wn, clamped = track(k, rec.value)
        if rec.set & GLIDE and has:
            cut[v] = [a[W], wn, rec.up_q32, rec.down_q32, 0, q, mode, 0]
        else:
            cut[v] = [wn, 0, 0, 0, 0, q, mode, 0]
            store(filt, v, coeffs(mode, wn, q))
        res[0] += 1
        res[2] += int(clamped)
    return res


def cutoff_match(owner, cut, bend, inc, filt, first, count, match, rec):
    """The channel sweep.  Returns [set or started, withheld, voices of the range that did not match, clamped]."""
    assert check([rec]) == 0 and count > 0 and 0 <= first and first + count <= len(owner)
    value, mask = (np.uint32(x) for x in match)
    v = np.arange(first, first + count)
    words = owner[v]
    hit = (words != 0) & ((words & mask) == value)
    a = apply(cut, bend, inc, filt, v[hit], rec)
    return [a[0], a[1], int((~hit).sum()), a[2]]


def cutoff_owned_each(owner, cut, bend, inc, filt, recs, entries, tags, count=None):
    """Returns [set or started, withheld, voices whose owner differs, clamped]."""
    assert om.tags_check(tags, 0) == 0 and check(recs) == 0 and len(recs) == len(tags)
    res, seen = [0, 0, 0, 0], set()
    for k, v in enumerate(om.looked(entries, len(tags), count).tolist()):
        if v < 0 or v >= len(owner):
            continue
        if int(owner[v]) != int(tags[k]):
            res[2] += 1
            continue
        assert v not in seen, "a voice named twice: unspecified"
        seen.add(v)
        a = apply(cut, bend, inc, filt, [v], recs[k])
        res = [res[0] + a[0], res[1] + a[1], res[2], res[3] + a[2]]
    return res


def cutoff_tags_each(owner, cut, bend, inc, filt, recs, first, count, tags):
    """find_owned, then cutoff_owned_each on its list.  Returns (d_result, the list)."""
    lst = om.find_owned(owner, first, count, tags)
    res = cutoff_owned_each(owner, cut, bend, inc, filt, recs, lst, tags)
    assert res[2] == 0
    return res, lst


def step(w, target, up, down):
    """one 64-frame step of a moving w != target: (next, arrived) -- the fixed-point portamento's step"""
    if w < target:
        nxt = w + max(1, (w * up) >> 32)
        return nxt, nxt >= target
    nxt = w - max(1, (w * down) >> 32)
    return nxt, nxt <= target


def advance(cut, filt, first, count, frames):
    """ADVANCE BY F FRAMES over [first, first + count).  Returns [still moving, arrived]."""
    assert 1 <= frames <= 65536
    res = [0, 0]
    for v in range(first, first + count):
        w, target, up, down, carry, q, mode, _ = (int(x) for x in cut[v])
        if target == 0:
            continue
        c = carry + frames
        there = w == target
        for _ in range(c >> 6):
            if there:
                break
            w, there = step(w, target, up, down)
        if there:
            cut[v] = [target, 0, 0, 0, 0, q, mode, 0]
            w = target
        else:
            cut[v, W], cut[v, CARRY] = w, c & 63
        res[1 if there else 0] += 1
        store(filt, v, coeffs(mode, w, q))
    return res


def stop(cut, filt, first, count, snap):
    for v in range(first, first + count):
        w, target, _, _, _, q, mode, _ = (int(x) for x in cut[v])
        if target == 0:
            continue
        if snap:
            w = target
            store(filt, v, coeffs(mode, w, q))
        cut[v] = [w, 0, 0, 0, 0, q, mode, 0]


def tag_clear(cut, entries, n_tags, count=None):
    """what follows every tag launch once the array exists: all eight words of the tagged voices"""
    if not CLEAR_RULE:
        return
    e = om.looked(entries, n_tags, count)
    cut[e[(e >= 0) & (e < len(cut))]] = 0


def rate_q32(octaves_per_second, rate=48000.0):
    """(up_q32, down_q32) of a sweep of that speed: the fractions added and taken away per 64 frames"""
    r = 2.0 ** (octaves_per_second * 64.0 / rate)
    top = 0xFFFFFFFF
    return min(top, max(1, int(round((r - 1.0) * 4294967296.0)))), min(top, max(1, int(round((1.0 - 1.0 / r) * 4294967296.0))))


def track_q24(harmonic):
    """what the host supplies with TRACK: harmonic * 2 pi in Q24"""
    return int(round(harmonic * 2.0 * np.pi * (1 << 24)))


# ---------------------------------------------------------------------------------------------- the stage

import fx_bend_model as BM  # noqa: E402  (the stage stands on the bend stage; the arithmetic above needs none of it)


class FxCutoffStage(BM.FxBendStage):
    """fx_bend_model.FxBendStage with the cutoff array: the oracle's bank, the owner, glide, bend and cutoff arrays and the clock.  The
    coefficient words the calls store are the oracle bank's own b0_q30 .. a2_q30, so the next rendered block runs on them."""

    def __init__(self, bank, pool, c0, **kw):
        super().__init__(bank, pool, c0, **kw)
        self.cut = new(bank.n)

    @property
    def filt(self):
        return {name: self.truth[name] for name in COEFFS}

    def tag(self, entries, tags, count=None):
        res = super().tag(entries, tags, count)
        tag_clear(self.cut, entries, len(tags), count)
        return res

    def cut_match(self, match, rec, rng=None):
        first, count = rng or self.whole
        return cutoff_match(self.owner, self.cut, self.bend, self.inc, self.filt, first, count, match, rec)

    def cut_tags(self, recs, tags, rng=None):
        first, count = rng or self.whole
        return cutoff_tags_each(self.owner, self.cut, self.bend, self.inc, self.filt, recs, first, count, tags)[0]

    def cut_list(self, recs, entries, tags, count=None):
        return cutoff_owned_each(self.owner, self.cut, self.bend, self.inc, self.filt, recs, entries, tags, count)

    def cut_advance(self, frames, rng=None):
        first, count = rng or self.whole
        return advance(self.cut, self.filt, first, count, frames)

    def cut_stop(self, snap, rng=None):
        first, count = rng or self.whole
        stop(self.cut, self.filt, first, count, snap)


# ---------------------------------------------------------------------------------------------- the clear rule's scenes

SCENES = ("thief", "restrike")
TAG_A, TAG_B = 0x0300003C, 0x03000040
CHAN = (0x03000000, 0xFF000000)
BOTH = SET_Q | SET_MODE


def run_scene(name, st):
    """Two scenes on a stage, each of which FAILS on a bank whose tag launches leave the cutoff words alone (CLEAR_RULE = False).
    thief:    a note's cutoff sweeps up; another note takes its voice.  The thief must not inherit the sweep: the advances that follow
              find nobody moving and its coefficients stay what the note-on left; a record without Q and MODE is withheld on it.
    restrike: a key is struck again in the same voice under the same tag while its cutoff glides down; the new note's first record is
              a first cutoff again, and a GLIDE on it sets the cutoff at once."""
    up, down = rate_q32(60.0)
    if name == "thief":
        v = 300
        st.strike([v], [TAG_A], [30000001])
        assert st.cut_tags([Rec(ABS | BOTH, 1 << 24, 2 << 16, 1)], [TAG_A]) == [1, 0, 0, 0]
        assert st.cut_tags([Rec(ABS | GLIDE, 1 << 28, up_q32=up, down_q32=down)], [TAG_A]) == [1, 0, 0, 0]
        assert st.cut_advance(64) == [1, 0] and 1 << 24 < st.cut[v, W] < 1 << 28
        st.block()
        st.strike([v], [TAG_B], [52000003])
        assert not st.cut[v].any(), "the thief inherited its victim's cutoff words"
        held = [int(st.filt[name][v]) for name in COEFFS]
        for _ in range(3):
            assert st.cut_advance(64) == [0, 0], "the thief's cutoff goes on sweeping"
            st.block()
        assert [int(st.filt[name][v]) for name in COEFFS] == held
        assert st.cut_tags([Rec(ABS, 1 << 25)], [TAG_B]) == [0, 1, 0, 0], "a record without Q and MODE found the victim's q and mode"
        assert st.cut_tags([Rec(ABS | BOTH, 1 << 25, 1 << 16, 2)], [TAG_A]) == [0, 0, 0, 0]      # nobody carries the victim's tag
    elif name == "restrike":
        v = 64
        st.strike([v], [TAG_A], [40000003])
        assert st.cut_tags([Rec(TRACK | BOTH, track_q24(8), 3 << 16, 1)], [TAG_A]) == [1, 0, 0, 0]
        assert st.cut_tags([Rec(TRACK | GLIDE, track_q24(2), up_q32=up, down_q32=down)], [TAG_A]) == [1, 0, 0, 0]
        assert st.cut_advance(64) == [1, 0]
        st.block()
        st.strike([v], [TAG_A], [53393781])
        assert st.cut_advance(64) == [0, 0], "the key struck again goes on gliding towards the old note's cutoff"
        st.block()
        want = track(53393781, track_q24(4))[0]
        assert st.cut_tags([Rec(TRACK | GLIDE | BOTH, track_q24(4), 3 << 16, 1, up, down)], [TAG_A]) == [1, 0, 0, 0]
        assert st.cut[v].tolist() == [want, 0, 0, 0, 0, 3 << 16, 1, 0], "a first cutoff under GLIDE is set at once"
        assert [int(st.filt[name][v]) for name in COEFFS] == coeffs(1, want, 3 << 16)
        st.block()
    else:
        raise KeyError(name)
