"""The filter envelope, stated in numpy on top of tests/cutoff_model.py: the fenv words, the cutoff words and the five coefficient words
as pure functions of the call sequence.  Written from the definition in include/skred_amd.h (section "filter envelope"), not from the
kernels.

`fenv` is a uint32 array of shape (n_voices, 8): stage, w_peak, w_sustain, w_end (fp32 bit patterns), rate_attack, rate_decay,
rate_release (bits), 0 per voice; stage 0 is "no envelope" and then the row is zero.  `cut` is cutoff_model's array, `filt` the bank's
voice_filter (stored in place), `release` the bank's sample_release per voice (read only: the advance pass looks at "is it 0").  The
envelope has no arithmetic of its own: a step is one np.float32 multiply, a coefficient store is cutoff_model.coeffs.

Two switches give the models of a library that lacks a rule, and the tests name the assertions that fail on them: `CLEAR_RULE` off
is a bank whose tag launches leave the fenv words alone; `READ_RELEASE_CLOCK` off is an advance pass that never looks at
sample_release.
"""
from contextlib import contextmanager

import numpy as np

import ctl_model as CM
import cutoff_model as M
import owner_model as OM
import slot_model as SM

f32 = np.float32
STAGE, W_PEAK, W_SUSTAIN, W_END, RATE_ATTACK, RATE_DECAY, RATE_RELEASE, RESERVED = range(8)
OFF, ATTACK, DECAY, SUSTAIN, RELEASE = range(5)
ABS, REL, START = 1, 2, 4
ALL = 7
BAD, RANGE = -2, -4
CLEAR_RULE = True
READ_RELEASE_CLOCK = True
LEVEL = {ATTACK: W_PEAK, DECAY: W_SUSTAIN, RELEASE: W_END}
RATE = {ATTACK: RATE_ATTACK, DECAY: RATE_DECAY, RELEASE: RATE_RELEASE}
NEXT = {ATTACK: DECAY, DECAY: SUSTAIN, SUSTAIN: SUSTAIN, RELEASE: OFF, OFF: OFF}

bits, flt = M.bits, M.flt


def new(n_voices):
    return np.zeros((n_voices, 8), np.uint32)


class Rec:
    """one skred_fenv_t"""

    def __init__(self, set, peak, sustain, end, rate_attack, rate_decay, rate_release, start=0.0):
        self.set, self.start, self.peak, self.sustain, self.end = int(set), f32(start), f32(peak), f32(sustain), f32(end)
        self.rate_attack, self.rate_decay, self.rate_release = f32(rate_attack), f32(rate_decay), f32(rate_release)

    def c(self):
        from skred_amd import device
        return device.fenv(self.set, float(self.peak), float(self.sustain), float(self.end), float(self.rate_attack), float(self.rate_decay),
                           float(self.rate_release), float(self.start))


def check(recs, K, voice_mask, filter_mask):
    """skred_fenv_check: 0, SKRED_E_BAD_ARG or SKRED_E_RANGE, in the header's order (None: a NULL array)."""
    if recs is None:
        return BAD
    if K < 1 or K > 64 or K & (K - 1):
        return RANGE
    for m in (voice_mask, filter_mask):
        if not m or (K < 64 and m >> K):
            return BAD
    for r in recs:
        how = r.set & (ABS | REL)
        if r.set & ~ALL or how not in (ABS, REL):
            return BAD
        start = bool(r.set & START)
        if not start and not r.start == 0:
            return BAD
        levels = ([r.start] if start else []) + [r.peak, r.sustain, r.end]
        rates = [r.rate_attack, r.rate_decay, r.rate_release]
        if not all(np.isfinite(x) for x in levels + rates):
            return BAD
        if how == ABS and not all(M.W_MIN <= x <= M.W_MAX for x in levels):
            return RANGE
        if how == REL and not all(x > 0 for x in levels):
            return RANGE
        if not all(M.RATE_MIN <= x <= M.RATE_MAX for x in rates):
            return RANGE
        if any(x == 1 for x in rates):
            return BAD
    if filter_mask & ~voice_mask:
        return BAD
    return 0


def enter(stage, f, w):
    """ENTERING A STAGE from w on a voice whose fenv words are f.  Returns (the stage the voice is in, w, target, rate, landed)."""
    landed = False
    while stage in LEVEL:
        T, r = int(f[LEVEL[stage]]), int(f[RATE[stage]])
        up = flt(r) > 1
        if w != T and (w < T if up else w > T):
            return stage, w, T, r, landed
        w, landed, stage = T, True, NEXT[stage]
    return stage, w, 0, 0, landed


def apply(cut, fenv, filt, voices, rec):
    """A RECORD ON VOICE v for `voices` (distinct indices).  Returns [started, withheld, clamped]."""
    res = [0, 0, 0]
    for v in np.asarray(voices, np.int64).reshape(-1):
        w_now = int(cut[v, M.W])
        if w_now == 0:
            res[1] += 1
            continue
        clamped = [False]

        def level(x):
            if rec.set & ABS:
                return int(bits(x))
            f = flt(w_now) * f32(x)
            assert f.dtype == f32
            if not M.W_MIN <= f <= M.W_MAX:
                clamped[0] = True
            return int(bits(min(max(f, M.W_MIN), M.W_MAX)))

        w = level(rec.start) if rec.set & START else w_now
        f = np.array([ATTACK, level(rec.peak), level(rec.sustain), level(rec.end), bits(rec.rate_attack), bits(rec.rate_decay),
                      bits(rec.rate_release), 0], np.uint32)
        stage, w, target, rate, _ = enter(ATTACK, f, w)
        assert stage in (ATTACK, DECAY, SUSTAIN)
        f[STAGE] = stage
        cut[v, M.W], cut[v, M.TARGET], cut[v, M.RATE_UP], cut[v, M.RATE_DOWN], cut[v, M.CARRY] = w, target, rate, rate, 0
        fenv[v] = f
        if w != w_now:
            M.store(filt, [v], M.coeffs(cut[v, M.MODE], flt(w), flt(cut[v, M.Q])).reshape(5, 1))
        res[0] += 1
        res[2] += clamped[0]
    return res


def fenv_match(owner, cut, fenv, filt, first, count, K, filter_mask, match, rec):
    """The channel sweep.  Returns [started, withheld, slots of the range that did not match, clamped]."""
    assert check([rec], K, (1 << K) - 1, filter_mask) == 0 and first % K == 0 and count % K == 0 and count > 0
    heads = np.arange(first, first + count, K)
    hit = M.matches(owner, heads, match)
    lanes = np.array(SM.lanes(filter_mask, K), np.int64)
    a = apply(cut, fenv, filt, (heads[hit][:, None] + lanes[None, :]).reshape(-1), rec)
    return [a[0], a[1], int((~hit).sum()), a[2]]


def fenv_owned_each(owner, cut, fenv, filt, recs, K, filter_mask, entries, tags, count=None):
    """Returns [started, withheld, slots whose owner differs, clamped]."""
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
        a = apply(cut, fenv, filt, e + lanes, recs[k])
        res = [res[0] + a[0], res[1] + a[1], res[2], res[3] + a[2]]
    return res


def fenv_tags_each(owner, cut, fenv, filt, recs, first, count, K, filter_mask, tags):
    """find_owned, then fenv_owned_each on its list.  Returns (d_result, the list)."""
    lst = OM.find_owned(owner, first, count, K, tags)
    res = fenv_owned_each(owner, cut, fenv, filt, recs, K, filter_mask, lst, tags)
    assert res[2] == 0
    return res, lst


def advance(cut, fenv, release, filt, first, count, frames):
    """skred_bank_cutoff_advance on a bank with the array.  Returns [moving after the pass, arrived in it]."""
    assert 1 <= frames <= 65536
    env = first + np.flatnonzero(fenv[first:first + count, STAGE] != 0)
    rows = cut[env].copy()
    cut[env, M.TARGET] = 0                                            # (the cutoff section's rule sees the voices without a contour)
    res = M.advance(cut, filt, first, count, frames)
    cut[env] = rows
    for v in env:
        a, f = cut[v].copy(), fenv[v].copy()
        stage, w, target, rate = int(f[STAGE]), int(a[M.W]), int(a[M.TARGET]), int(a[M.RATE_UP])
        assert a[M.RATE_UP] == a[M.RATE_DOWN] and (target != 0) == (stage != SUSTAIN)
        arrived = False
        entered = READ_RELEASE_CLOCK and int(release[v]) != 0 and stage != RELEASE
        if entered:
            stage, w, target, rate, arrived = enter(RELEASE, f, w)
        compute = a[M.TARGET] != 0 or entered
        c = int(a[M.CARRY]) + frames
        m = c >> 6
        while m and target:
            up = w < target
            w = int(bits(flt(w) * flt(rate)))
            if (w >= target) if up else (w <= target):
                stage, w, target, rate, _ = enter(NEXT[stage], f, target)
                arrived = True
            m -= 1
        cut[v, M.W], cut[v, M.TARGET], cut[v, M.RATE_UP], cut[v, M.RATE_DOWN] = w, target, rate, rate
        cut[v, M.CARRY] = c & 63 if stage else 0
        if stage:
            fenv[v, STAGE] = stage
        else:
            fenv[v] = 0
        if compute:
            M.store(filt, [v], M.coeffs(a[M.MODE], flt(w), flt(a[M.Q])).reshape(5, 1))
        res[0] += target != 0
        res[1] += arrived
    return [int(res[0]), int(res[1])]


@contextmanager
def cutoff_ends(fenv):
    """cutoff_model's record calls on a bank with the array: a voice they set or start loses its contour.  (Voices are independent, so
    the record is applied voice by voice to see which ones were withheld.)"""
    plain = M.apply

    def ending(cut, bend, inc, filt, voices, rec):
        res = [0, 0, 0]
        for v in np.asarray(voices, np.int64).reshape(-1):
            a = plain(cut, bend, inc, filt, [v], rec)
            if a[0]:
                fenv[v] = 0
            res = [x + y for x, y in zip(res, a)]
        return res

    M.apply = ending
    try:
        yield
    finally:
        M.apply = plain


def stop(cut, fenv, filt, first, count, snap):
    """skred_bank_cutoff_stop on a bank with the array: every contour of the range ends"""
    M.stop(cut, filt, first, count, snap)
    fenv[first:first + count] = 0


def tag_clear(fenv, entries, n_tags, count, K):
    """what follows every tag launch once the array exists: all eight words of all K voices of the tagged slots"""
    if not CLEAR_RULE:
        return
    for e in OM.looked(entries, n_tags, count):
        if CM.slot_valid(e, K, len(fenv)):
            fenv[e:e + K] = 0
