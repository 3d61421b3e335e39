"""The pitch wheel, stated in numpy: the bend words and voice_phase_inc as pure functions of the call sequence, and the glide calls on
a bank that has a bend array.  Written from the definition in include/skred_amd.h (section "pitch wheel"), not from the kernels.

`bend` is a uint32 array of shape (n_voices, 2): key and ratio (fp32 bit patterns) per voice; key == 0 is "not bent".  `inc` is the
bank's voice_phase_inc (a float32 array, changed in place); `glide` is glide_model's array.  Every multiply is glide_model.mul: numpy's
float32 product, the IEEE round-to-nearest product __fmul_rn gives.  Host and device both keep denormals, and the one denormal case
the tests choose (the smallest denormal times 0.25) rounds to zero on either.

The guard and the find pass are owner_model's, the glide definition glide_model's.  `CLEAR_RULE` switched off gives the model of a
bank whose tag launches leave the bend words alone: the tests name the assertions that fail on it.
"""
import numpy as np

import ctl_model as CM
import glide_model as GM
import owner_model as OM
import slot_model as SM

KEY, RATIO = 0, 1
ONE = np.uint32(0x3F800000)
BAD, RANGE = -2, -4
CLEAR_RULE = True

bits, mul, usable = GM.bits, GM.mul, GM.usable


def new(n_voices):
    return np.zeros((n_voices, 2), np.uint32)


def check(ratios, K, voice_mask):
    """skred_bend_check: 0, SKRED_E_BAD_ARG or SKRED_E_RANGE, in the header's order (None: a NULL array)."""
    if ratios is None:
        return BAD
    if K < 1 or K > 64 or K & (K - 1):
        return RANGE
    if not voice_mask or (K < 64 and voice_mask >> K):
        return BAD
    for r in np.asarray(ratios, np.float32).reshape(-1):
        if not np.isfinite(r) or not r > 0:
            return BAD
    return 0


def apply(bend, inc, voices, ratio):
    """THE RULE on `voices` (distinct indices), to `ratio` (fp32 bits: one for all, or one per voice).  Returns [stored or restored,
    withheld]."""
    vs = np.asarray(voices, np.int64).reshape(-1)
    w = inc.view(np.uint32)
    r = np.broadcast_to(np.asarray(ratio, np.uint32), vs.shape)
    key, old_r, cur = bend[vs, KEY], bend[vs, RATIO], w[vs]
    k = np.where(key != 0, key, cur)
    centre = r == ONE
    p = mul(k, r)
    ok = ~centre & usable(k) & usable(p)
    withheld = ~centre & ~ok
    restored = centre & (key != 0)
    w[vs] = np.where(restored, key, np.where(ok, p, cur))
    bend[vs, KEY] = np.where(centre, 0, np.where(ok, k, key))
    bend[vs, RATIO] = np.where(centre, 0, np.where(ok, r, old_r))
    return [int(ok.sum() + restored.sum()), int(withheld.sum())]


def matches(owner, heads, match):
    value, mask = (np.uint32(x) for x in match)
    words = owner[heads]
    return (words != 0) & ((words & mask) == value)


def bend_match(owner, bend, inc, first, count, K, voice_mask, match, ratio):
    """The channel wheel.  Returns [stored or restored, withheld, slots of the range that did not match]."""
    assert check([ratio], K, voice_mask) == 0 and first % K == 0 and count % K == 0 and count > 0
    heads = np.arange(first, first + count, K)
    hit = matches(owner, heads, match)
    lanes = np.array(SM.lanes(voice_mask, K), np.int64)
    vs = (heads[hit][:, None] + lanes[None, :]).reshape(-1)
    return apply(bend, inc, vs, bits(np.float32(ratio))) + [int((~hit).sum())]


def bend_owned_each(owner, bend, inc, ratios, K, voice_mask, entries, tags, count=None):
    """Returns [stored or restored, withheld, slots whose owner differs]."""
    assert OM.tags_check(tags) == 0 and check(ratios, K, voice_mask) == 0 and len(ratios) == len(tags)
    res = [0, 0, 0]
    seen = set()
    lanes = np.array(SM.lanes(voice_mask, K), np.int64)
    for k, e in enumerate(OM.looked(entries, len(tags), count)):
        if not CM.slot_valid(e, K, len(owner)):
            continue
        if int(owner[e]) != int(tags[k]):
            res[2] += 1
            continue
        assert e not in seen, "a slot named twice: unspecified"
        seen.add(e)
        a = apply(bend, inc, e + lanes, bits(np.float32(ratios[k])))
        res = [res[0] + a[0], res[1] + a[1], res[2]]
    return res


def bend_tags_each(owner, bend, inc, ratios, first, count, K, voice_mask, tags):
    """find_owned, then bend_owned_each on its list.  Returns (d_result, the list)."""
    lst = OM.find_owned(owner, first, count, K, tags)
    res = bend_owned_each(owner, bend, inc, ratios, K, voice_mask, lst, tags)
    assert res[2] == 0
    return res, lst


def clear(bend, inc, first, count, snap):
    b = bend[first:first + count]
    w = inc[first:first + count].view(np.uint32)
    on = b[:, KEY] != 0
    if snap:
        w[on] = b[on, KEY]
    b[:] = 0


def tag_clear(bend, entries, n_tags, count, K):
    """what follows every tag launch once the array exists: the words of all K voices of the tagged slots"""
    if not CLEAR_RULE:
        return
    for e in OM.looked(entries, n_tags, count):
        if CM.slot_valid(e, K, len(bend)):
            bend[e:e + K] = 0


# ---- the glide calls on a bank that has a bend array: on a voice with a key the glide runs on the key

def sound(bend, inc, voices):
    """the sounding increment of bent voices stored again as key * ratio; that store is withheld where the product is not usable"""
    vs = np.asarray(voices, np.int64).reshape(-1)
    vs = vs[bend[vs, KEY] != 0]
    p = mul(bend[vs, KEY], bend[vs, RATIO])
    ok = usable(p)
    inc.view(np.uint32)[vs[ok]] = p[ok]


def _keys_in(bend, inc):
    """the increments the glide definition reads: the key of a bent voice, else voice_phase_inc"""
    bent = bend[:, KEY] != 0
    return np.where(bent, bend[:, KEY], inc.view(np.uint32)).view(np.float32).copy(), bent


def _keys_out(bend, inc, eff, bent):
    bend[bent, KEY] = eff.view(np.uint32)[bent]
    inc.view(np.uint32)[~bent] = eff.view(np.uint32)[~bent]


def glide_start_owned(owner, glide, bend, inc, glides, K, voice_mask, entries, tags, count=None):
    """glide_model.start_owned under a bend array.  Returns its d_result."""
    eff, bent = _keys_in(bend, inc)
    # which starts were not withheld: glide_model's own condition, read off a run on carry words no start can store (a start stores 0)
    probe = glide.copy()
    probe[:, GM.CARRY] = 99
    GM.start_owned(owner, probe, eff.copy(), glides, K, voice_mask, entries, tags, count)
    started = probe[:, GM.CARRY] != 99
    res = GM.start_owned(owner, glide, eff, glides, K, voice_mask, entries, tags, count)
    _keys_out(bend, inc, eff, bent)
    sound(bend, inc, np.flatnonzero(started & bent))
    return res


def glide_start_tags(owner, glide, bend, inc, glides, first, count, K, voice_mask, tags):
    lst = OM.find_owned(owner, first, count, K, tags)
    res = glide_start_owned(owner, glide, bend, inc, glides, K, voice_mask, lst, tags)
    assert res[2] == 0
    return res, lst


def glide_advance(glide, bend, inc, first, count, frames):
    """glide_model.advance under a bend array.  Returns its d_result."""
    eff, bent = _keys_in(bend, inc)
    gliding = np.zeros(len(inc), bool)
    gliding[first:first + count] = glide[first:first + count, GM.TARGET] != 0
    res = GM.advance(glide, eff, first, count, frames)
    _keys_out(bend, inc, eff, bent)
    sound(bend, inc, np.flatnonzero(gliding & bent))
    return res


def glide_stop(glide, bend, inc, first, count, snap):
    eff, bent = _keys_in(bend, inc)
    gliding = np.zeros(len(inc), bool)
    gliding[first:first + count] = glide[first:first + count, GM.TARGET] != 0
    GM.stop(glide, eff, first, count, snap)
    _keys_out(bend, inc, eff, bent)
    if snap:
        sound(bend, inc, np.flatnonzero(gliding & bent))


def ratio_of(semitones):
    """the wheel at `semitones` (0: exactly 1.0f, the centre); an array gives an array"""
    return (2.0 ** (np.asarray(semitones, np.float64) / 12.0)).astype(np.float32)[()]
