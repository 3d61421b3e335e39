"""Portamento, stated in numpy: the glide words and voice_phase_inc as pure functions of the call sequence.  Written from the definition
in include/skred_amd.h (section "portamento"), not from the kernels.

`glide` is a uint32 array of shape (n_voices, 4): target, rate_up, rate_down (fp32 bit patterns) and carry per voice; target == 0 is
"not gliding".  `inc` is the bank's voice_phase_inc (a float32 array, changed in place).  Every multiply is numpy's float32 multiply:
the IEEE round-to-nearest product of two fp32 values, which is what __fmul_rn gives.  The one place the two could part is a denormal
operand or product (a host that flushes them, a device that does not): the tests keep increments, targets and products in the normal
range, |x| >= 2 ** -126, and say so where they choose them.

The guard and the find pass are owner_model's.  `CLEAR_RULE` switched off gives the model of a bank whose tag launches leave the
glide words alone: tests/test_glide.py names the assertions that fail on it.
"""
import numpy as np

import ctl_model as CM
import owner_model as OM
import slot_model as SM

FROM_SCALE, TO_SCALE = 1, 2
TARGET, RATE_UP, RATE_DOWN, CARRY = 0, 1, 2, 3
ABS = np.uint32(0x7FFFFFFF)
EXP = np.uint32(0x7F800000)
BAD, RANGE = -2, -4
CLEAR_RULE = True


def new(n_voices):
    return np.zeros((n_voices, 4), np.uint32)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def mul(a, b):
    """the fp32 product of two bit patterns (arrays or scalars), as bits"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (np.asarray(a, np.uint32).view(np.float32) * np.asarray(b, np.uint32).view(np.float32)).astype(np.float32).view(np.uint32)


def finite(w):
    return (np.asarray(w, np.uint32) & EXP) != EXP


def usable(w):
    """finite and not zero: what a glide can start from or aim at"""
    w = np.asarray(w, np.uint32)
    return finite(w) & ((w & ABS) != 0)


class Glide:
    """one entry of the two starting calls"""

    def __init__(self, set, rate_up, rate_down, scale):
        self.set, self.rate_up, self.rate_down, self.scale = int(set), np.float32(rate_up), np.float32(rate_down), np.float32(scale)

    def c(self):
        from skred_amd import device
        return device.glide(self.set, float(self.rate_up), float(self.rate_down), float(self.scale))


def check(glides, K, voice_mask):
    """skred_glide_check: 0, SKRED_E_BAD_ARG or SKRED_E_RANGE, in the header's order (None: a NULL array)."""
    if glides is None:
        return BAD
    if K < 1 or K > 64 or K & (K - 1):
        return RANGE
    if not voice_mask or (K < 64 and voice_mask >> K):
        return BAD
    for g in glides:
        if g.set not in (FROM_SCALE, TO_SCALE):
            return BAD
        if not (np.isfinite(g.rate_up) and np.isfinite(g.rate_down) and np.isfinite(g.scale)):
            return BAD
        if not g.rate_up > 1 or not 0 < g.rate_down < 1 or not g.scale > 0:
            return BAD
    return 0


def tag_clear(glide, entries, n_tags, count, K):
    """what follows every tag launch once the array exists: the words of all K voices of the tagged slots"""
    if not CLEAR_RULE:
        return
    for e in OM.looked(entries, n_tags, count):
        if CM.slot_valid(e, K, len(glide)):
            glide[e:e + K] = 0


def start_owned(owner, glide, inc, glides, K, voice_mask, entries, tags, count=None):
    """Returns [voices set gliding, starts withheld, slots whose owner differs]."""
    assert OM.tags_check(tags) == 0 and check(glides, K, voice_mask) == 0 and len(glides) == len(tags)
    w = inc.view(np.uint32)
    res = [0, 0, 0]
    seen = set()
    for k, e in enumerate(OM.looked(entries, len(tags), count)):
        if not CM.slot_valid(e, K, len(owner)):
            continue
        if int(owner[e]) != int(tags[k]):
            res[2] += 1
            continue
        assert e not in seen, "a slot named twice: unspecified"
        seen.add(e)
        g = glides[k]
        for l in SM.lanes(voice_mask, K):
            v = e + l
            cur = np.uint32(w[v])
            if g.set == FROM_SCALE:
                target, nxt = cur, mul(cur, bits(g.scale))
            else:
                old = np.uint32(glide[v, TARGET])
                target, nxt = mul(old if old else cur, bits(g.scale)), cur
            if usable(cur) and usable(target) and usable(nxt):
                w[v] = nxt
                glide[v] = (target, bits(g.rate_up), bits(g.rate_down), 0)
                res[0] += 1
            else:
                res[1] += 1
    return res


def start_tags(owner, glide, inc, glides, first, count, K, voice_mask, tags):
    """find_owned, then start_owned on its list.  Returns (d_result, the list)."""
    lst = OM.find_owned(owner, first, count, K, tags)
    res = start_owned(owner, glide, inc, glides, K, voice_mask, lst, tags)
    assert res[2] == 0
    return res, lst


def advance(glide, inc, first, count, frames):
    """The advance pass by `frames` frames over [first, first + count).  Returns [still gliding, arrived]."""
    assert 1 <= frames <= 65536
    g = glide[first:first + count]
    w = inc[first:first + count].view(np.uint32)
    on = g[:, TARGET] != 0
    t = g[:, TARGET] & ABS
    cur = w.copy()
    there = on & (~usable(cur) | (((cur ^ g[:, TARGET]) >> np.uint32(31)) != 0))
    c = g[:, CARRY] + np.uint32(frames)
    m = c >> np.uint32(6)
    for step in range(int(m[on].max()) if on.any() else 0):
        act = on & ~there & (m > step)
        if not act.any():
            break
        a = cur & ABS
        up, down, level = act & (a < t), act & (a > t), act & (a == t)
        cur = np.where(up, mul(cur, g[:, RATE_UP]), np.where(down, mul(cur, g[:, RATE_DOWN]), cur))
        a = cur & ABS
        there |= level | (up & (~finite(cur) | (a >= t))) | (down & (~finite(cur) | (a <= t)))
    still = on & ~there
    w[there] = g[there, TARGET]
    w[still] = cur[still]
    g[still, CARRY] = c[still] & np.uint32(63)
    g[there] = 0
    return [int(still.sum()), int(there.sum())]


def stop(glide, inc, first, count, snap):
    g = glide[first:first + count]
    w = inc[first:first + count].view(np.uint32)
    on = g[:, TARGET] != 0
    if snap:
        w[on] = g[on, TARGET]
    g[:] = 0


def per_64(semitones_per_second, rate=44100.0):
    """(rate_up, rate_down) of a glide of that speed: the factor per 64 frames"""
    r = 2.0 ** (semitones_per_second / 12.0 * 64.0 / rate)
    return np.float32(r), np.float32(1.0 / r)
