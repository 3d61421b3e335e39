"""The filter envelope of the fixed-point bank, stated in numpy integers on top of tests/fx_cutoff_model.py: the fenv words, the cutoff
words and the five coefficient words as pure functions of the call sequence.  Written from the definition in
include/skred_amd_fxpt.h (section "filter envelope"), not from the kernels.

`fenv` is a uint32 array of shape (n_voices, 8): stage, w_peak, w_sustain, w_end (w_q29), rate_attack_q32, rate_decay_q32,
rate_release_q32, 0 per voice; stage 0 is "no envelope" and then the row is zero.  `cut` is fx_cutoff_model's array, `filt` its dict of
coefficient arrays, `release` the bank's sample_release per voice (read only: the advance pass looks at "is it 0").  The envelope has
no arithmetic of its own: a step is fx_cutoff_model.step with both rates the stage's, a coefficient store is fx_cutoff_model.coeffs.

Two switches give the models of a library that lacks a rule, and the tests name the assertions that fail on them: `CLEAR_RULE` off
is a bank whose tag launches, cutoff records and cutoff_stop leave the fenv words alone; `READ_RELEASE_CLOCK` off is an advance pass
that never looks at sample_release.
"""
import numpy as np

import fx_cutoff_model as M
import fx_expr_model as em
import fx_live_model as live
import fx_owner_model as om
import fx_pedal_model as PM

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
# the widths the header states: name -> bits of the magnitude
STATED_BITS = {"w_now * value_q16": 63, "level before the clamp": 47, "carry + F": 17, "w * rate": 63, "next": 32}


def new(n_voices):
    return np.zeros((n_voices, 8), np.uint32)


class Rec:
    """one skred_fx_fenv_t"""

    def __init__(self, set, peak, sustain, end, rate_attack, rate_decay, rate_release, start=0):
        self.set, self.start, self.peak, self.sustain, self.end = int(set), int(start), int(peak), int(sustain), int(end)
        self.rate_attack, self.rate_decay, self.rate_release = int(rate_attack), int(rate_decay), int(rate_release)

    def c(self):
        from skred_amd import fxbank as fxb
        return fxb.fx_fenv(self.set, self.peak, self.sustain, self.end, self.rate_attack, self.rate_decay, self.rate_release, self.start)


def check(recs, n=None):
    """skred_fx_fenv_check: 0, SKRED_E_BAD_ARG or SKRED_E_RANGE, in the header's order (None: a NULL array)"""
    if recs is None or (n is not None and n < 0):
        return BAD
    for r in list(recs)[:n]:
        how = r.set & (ABS | REL)
        if r.set & ~ALL:
            return BAD
        if how not in (ABS, REL):
            return BAD
        start = bool(r.set & START)
        if not start and r.start != 0:
            return BAD
        levels = ([r.start] if start else []) + [r.peak, r.sustain, r.end]
        if how == ABS and not all(M.W_MIN <= x <= M.W_MAX for x in levels):
            return RANGE
        if how == REL and not all(x != 0 for x in levels):
            return RANGE
        if not (r.rate_attack and r.rate_decay and r.rate_release):
            return BAD
    return 0


def _note(widths, name, value):
    if widths is not None:
        widths[name] = max(widths.get(name, 0), int(value))


def level(rec, w_now, x, widths=None):
    """(the level, clamped) of one value of a record on a voice whose cutoff is w_now"""
    if rec.set & ABS:
        return int(x), False
    _note(widths, "w_now * value_q16", int(w_now) * int(x))
    f = (int(w_now) * int(x)) >> 16
    _note(widths, "level before the clamp", f)
    return max(M.W_MIN, min(M.W_MAX, f)), not M.W_MIN <= f <= M.W_MAX


def enter(stage, f, w):
    """ENTERING A STAGE from w on a voice whose fenv words are f.  Returns (the stage the voice is in, target, rate, landed)."""
    landed = False
    while stage in LEVEL:
        T, r = int(f[LEVEL[stage]]), int(f[RATE[stage]])
        if w != T:
            return stage, T, r, landed
        landed, stage = True, NEXT[stage]
    return stage, 0, 0, landed


def apply(cut, fenv, filt, voices, rec, widths=None):
    """A RECORD ON VOICE v for `voices` (distinct indices).  Returns [started, withheld, clamped]."""
    res = [0, 0, 0]
    for v in np.asarray(voices, np.int64).reshape(-1).tolist():
        w_now = int(cut[v, M.W])
        if w_now == 0:
            res[1] += 1
            continue
        named = ([rec.start] if rec.set & START else []) + [rec.peak, rec.sustain, rec.end]
        lv = [level(rec, w_now, x, widths) for x in named]
        clamped = any(c for _, c in lv)
        w = lv[0][0] if rec.set & START else w_now
        peak, sustain, end = (x for x, _ in lv[-3:])
        f = np.array([ATTACK, peak, sustain, end, rec.rate_attack, rec.rate_decay, rec.rate_release, 0], np.uint32)
        stage, target, rate, _ = enter(ATTACK, f, w)
        assert stage in (ATTACK, DECAY, SUSTAIN)
        f[STAGE] = stage
        cut[v, M.W], cut[v, M.TARGET], cut[v, M.UP], cut[v, M.DOWN], cut[v, M.CARRY] = w, target, rate, rate, 0
        fenv[v] = f
        if w != w_now:
            M.store(filt, v, M.coeffs(cut[v, M.MODE], w, cut[v, M.Q]))
        res[0] += 1
        res[2] += int(clamped)
    return res


def fenv_match(owner, cut, fenv, filt, first, count, match, rec):
    """The channel sweep.  Returns [started, withheld, voices of the range that did not match, clamped]."""
    assert check([rec]) == 0 and count > 0 and 0 <= first and first + count <= len(owner)
    value, mask = (np.uint32(x) for x in match)
    v = np.arange(first, first + count)
    words = owner[v]
    hit = (words != 0) & ((words & mask) == value)
    a = apply(cut, fenv, filt, v[hit], rec)
    return [a[0], a[1], int((~hit).sum()), a[2]]


def fenv_owned_each(owner, cut, fenv, filt, recs, entries, tags, count=None):
    """Returns [started, withheld, voices whose owner differs, clamped]."""
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
        a = apply(cut, fenv, filt, [v], recs[k])
        res = [res[0] + a[0], res[1] + a[1], res[2], res[3] + a[2]]
    return res


def fenv_tags_each(owner, cut, fenv, filt, recs, first, count, tags):
    """find_owned, then fenv_owned_each on its list.  Returns (d_result, the list)."""
    lst = om.find_owned(owner, first, count, tags)
    res = fenv_owned_each(owner, cut, fenv, filt, recs, lst, tags)
    assert res[2] == 0
    return res, lst


def advance(cut, fenv, release, filt, first, count, frames, widths=None):
    """skred_fxbank_cutoff_advance on a bank with the array.  Returns [with a target after the pass, arrived in it]."""
    assert 1 <= frames <= 65536
    env = first + np.flatnonzero(fenv[first:first + count, STAGE] != 0)
    rows = cut[env].copy()
    cut[env, M.TARGET] = 0                                            # (the cutoff section's rule sees the voices without a contour)
    res = M.advance(cut, filt, first, count, frames)
    cut[env] = rows
    for v in env.tolist():
        a, f = [int(x) for x in cut[v]], fenv[v].copy()
        stage, w, target, rate = int(f[STAGE]), a[M.W], a[M.TARGET], a[M.UP]
        assert a[M.UP] == a[M.DOWN] and (target != 0) == (stage != SUSTAIN)
        arrived = False
        entered = READ_RELEASE_CLOCK and int(release[v]) != 0 and stage != RELEASE
        if entered:
            stage, target, rate, arrived = enter(RELEASE, f, w)
        compute = a[M.TARGET] != 0 or entered
        c = a[M.CARRY] + frames
        _note(widths, "carry + F", c)
        m = c >> 6
        while m and target:
            _note(widths, "w * rate", w * rate)
            w, there = M.step(w, target, rate, rate)
            _note(widths, "next", w)
            if there:
                w = target
                stage, target, rate, _ = enter(NEXT[stage], f, w)
                arrived = True
            m -= 1
        cut[v, M.W], cut[v, M.TARGET], cut[v, M.UP], cut[v, M.DOWN] = w, target, rate, rate
        cut[v, M.CARRY] = c & 63 if stage else 0
        if stage:
            fenv[v, STAGE] = stage
        else:
            fenv[v] = 0
        if compute:
            M.store(filt, v, M.coeffs(a[M.MODE], w, a[M.Q]))
        res[0] += int(target != 0)
        res[1] += int(arrived)
    return [int(res[0]), int(res[1])]


class _ends:
    """fx_cutoff_model's record calls on a bank with the array: a voice they set or start loses its contour (a withheld record leaves
    it).  Voices are independent, so the record is applied voice by voice to see which ones were withheld"""

    def __init__(self, fenv):
        self.fenv = fenv

    def __enter__(self):
        self.plain = M.apply
        plain, fenv = self.plain, self.fenv

        def ending(cut, bend, inc, filt, voices, rec):
            res = [0, 0, 0]
            for v in np.asarray(voices, np.int64).reshape(-1).tolist():
                a = plain(cut, bend, inc, filt, [v], rec)
                if a[0] and CLEAR_RULE:
                    fenv[v] = 0
                res = [x + y for x, y in zip(res, a)]
            return res

        M.apply = ending

    def __exit__(self, *exc):
        M.apply = self.plain


def stop(cut, fenv, filt, first, count, snap):
    """skred_fxbank_cutoff_stop on a bank with the array: every contour of the range ends, a resting one too"""
    M.stop(cut, filt, first, count, snap)
    if CLEAR_RULE:
        fenv[first:first + count] = 0


def tag_clear(fenv, entries, n_tags, count=None):
    """what follows every tag launch once the array exists: all eight words of the tagged voices"""
    if not CLEAR_RULE:
        return
    e = om.looked(entries, n_tags, count)
    fenv[e[(e >= 0) & (e < len(fenv))]] = 0


def plain_loop(w, q, mode, rec, events, total):
    """ONE voice, frame by frame in Python ints of unbounded width, no blocks at all: the record at frame 0 on a voice resting at w,
    `events` a dict frame -> "release".  The contour moves on the note's 64-frame grid: at every frame that is a multiple of 64 after
    the record one step is taken -- a release that was stamped at frame t is seen by the first step at or after t (a block is cut at
    every call).  Returns {frame: w} at every multiple of 64 from 0 to total, and the final (stage, w, target)."""
    named = ([rec.start] if rec.set & START else []) + [rec.peak, rec.sustain, rec.end]
    lv = [level(rec, w, x)[0] for x in named]
    if rec.set & START:
        w = lv[0]
    levels = {ATTACK: lv[-3], DECAY: lv[-2], RELEASE: lv[-1]}
    rates = {ATTACK: rec.rate_attack, DECAY: rec.rate_decay, RELEASE: rec.rate_release}

    def go(stage):
        while stage in levels:
            if w != levels[stage]:
                return stage, levels[stage], rates[stage]
            stage = NEXT[stage]
        return stage, 0, 0

    stage, target, rate = go(ATTACK)
    released, out = False, {0: w}
    for t in range(1, total + 1):
        if events.get(t - 1) == "release":                            # stamped before the block that holds frame t - 1 .. began
            released = True
        if t % 64:
            continue
        if stage and released and stage != RELEASE:
            stage, target, rate = go(RELEASE)
        if target:
            if w < target:
                w = w + max(1, (w * rate) >> 32)
                there = w >= target
            else:
                w = w - max(1, (w * rate) >> 32)
                there = w <= target
            if there:
                w = target
                stage, target, rate = go(NEXT[stage])
        out[t] = w
    return out, (stage, w, target)


# ---------------------------------------------------------------------------------------------- the stage

class FxFenvStage(M.FxCutoffStage):
    """fx_cutoff_model.FxCutoffStage with the fenv array and a pedal array: the oracle's bank, the owner, glide, bend, cutoff, fenv and
    pedal arrays and the clock.  The release clock the advance reads is the oracle bank's sample_release, which every note-off path
    below stamps."""

    def __init__(self, bank, pool, c0, **kw):
        super().__init__(bank, pool, c0, **kw)
        self.fenv, self.pedal = new(bank.n), PM.new(bank.n)

    @property
    def release(self):
        return self.truth["sample_release"]

    def tag(self, entries, tags, count=None):
        res = super().tag(entries, tags, count)
        tag_clear(self.fenv, entries, len(tags), count)
        e = om.looked(entries, len(tags), count)
        self.pedal[e[(e >= 0) & (e < self.n)]] = 0
        return res

    # the cutoff calls on a bank with the array
    def cut_match(self, match, rec, rng=None):
        with _ends(self.fenv):
            return super().cut_match(match, rec, rng)

    def cut_tags(self, recs, tags, rng=None):
        with _ends(self.fenv):
            return super().cut_tags(recs, tags, rng)

    def cut_list(self, recs, entries, tags, count=None):
        with _ends(self.fenv):
            return super().cut_list(recs, entries, tags, count)

    def cut_advance(self, frames, rng=None):
        first, count = rng or self.whole
        return advance(self.cut, self.fenv, self.release, self.filt, first, count, frames)

    def cut_stop(self, snap, rng=None):
        first, count = rng or self.whole
        stop(self.cut, self.fenv, self.filt, first, count, snap)

    # the record calls
    def fenv_match(self, match, rec, rng=None):
        first, count = rng or self.whole
        return fenv_match(self.owner, self.cut, self.fenv, self.filt, first, count, match, rec)

    def fenv_tags(self, recs, tags, rng=None):
        first, count = rng or self.whole
        return fenv_tags_each(self.owner, self.cut, self.fenv, self.filt, recs, first, count, tags)[0]

    def fenv_list(self, recs, entries, tags, count=None):
        return fenv_owned_each(self.owner, self.cut, self.fenv, self.filt, recs, entries, tags, count)

    # the note-off paths a release can come through
    def off(self, tags, hold_all, rng=None):
        first, count = rng or self.whole
        return PM.release_tags_pedal(self.owner, self.pedal, self.truth, first, count, tags, hold_all, self.now())[0]

    def plain_off(self, tags, rng=None):
        first, count = rng or self.whole
        return om.release_tags(self.owner, self.truth, first, count, tags, PM.REL, self.now())[0]

    def off_match(self, match, rng=None):
        first, count = rng or self.whole
        return em.stamp_match(self.owner, self.truth, first, count, match[0], match[1], PM.REL, self.now())[0]

    def latch(self, match, rng=None):
        first, count = rng or self.whole
        return PM.latch(self.owner, self.pedal, self.truth, first, count, match)

    def up(self, match, flags, rng=None):
        first, count = rng or self.whole
        return PM.up(self.owner, self.pedal, self.truth, first, count, match, flags, self.now())[0]

    def retrigger(self, voices):
        live.stamp(self.truth, np.asarray(voices, np.int32), PM.TRIG, self.now())
