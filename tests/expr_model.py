"""Channels and per-note expression, stated in numpy: the masked owner match, the ordered list and count of skred_bank_find_match,
the one-pass stamps and controllers under the match guard, and the per-entry controller values with their two products.  Written
from the definition in include/skred_amd.h (section "channels and per-note expression"), not from the kernels.  `owner` is
owner_model's array; the stamps are slot_model.stamp's, the controller stores ctl_model.store_voice's.

The arithmetic: np.float32 * np.float32 is one IEEE fp32 multiply, round to nearest even, subnormals kept -- what the device computes
with -ffp-contract=off and without a denormal flush (skred_amd/csrc/Makefile).
"""
import numpy as np

import ctl_model as CM
import owner_model as OM
import slot_model as SM

EACH_INC_SCALE, EACH_AMP_SCALE, EACH_VELOCITY, EACH_PAN = 1, 2, 4, 8
EACH_ALL = 15
EACH_LISTS = EACH_AMP_SCALE | EACH_VELOCITY               # the entry bits that put a voice on the motion list
BAD, RANGE = -2, -4
U32 = 0xFFFFFFFF


def match_check(value, mask):
    """skred_owner_match_check: 0 or SKRED_E_BAD_ARG."""
    return BAD if (int(value) & ~int(mask) & U32) else 0


def matches(words, value, mask):
    """Elementwise: owner != 0 and (owner & mask) == value."""
    w = np.asarray(words, np.uint32)
    return (w != 0) & ((w & np.uint32(mask)) == np.uint32(value))


def heads(first, count, K):
    return np.arange(first, first + count, K, dtype=np.int64)


def find_match(owner, first, count, K, value, mask, max_out):
    """(the list: the first voices of the matching slots, ascending, cut at max_out; d_count[0] = the TOTAL)."""
    assert match_check(value, mask) == 0
    h = heads(first, count, K)
    hit = h[matches(owner[h], value, mask)].astype(np.int32)
    return hit[:max_out], len(hit)


def stamp_match(owner, truth, first, count, K, voice_mask, value, mask, stamps, now):
    """Returns (d_result = [slots stamped, slots that did not match], the voices stamped).  `truth` receives slot_model.stamp."""
    lst, total = find_match(owner, first, count, K, value, mask, count)
    voices = np.array([e + l for e in lst for l in SM.lanes(voice_mask, K)], np.int32)
    SM.stamp(truth, voices, stamps, now)
    return [total, count // K - total], voices


def ctl_match(owner, views, ctls, first, count, voice_mask, value, mask):
    """ctl_model's stores on the matching slots.  Returns ([written, withheld, slots that did not match], voices written)."""
    K = len(ctls)
    lst, total = find_match(owner, first, count, K, value, mask, count)
    voices = [(int(e) + l, l) for e in lst for l in CM.lanes(voice_mask, K)]
    (written, withheld), touched = CM.apply(views, ctls, voices)
    return [written, withheld, count // K - total], touched


def lists_range(ctls, voice_mask, first, count):
    """What ctl_match adds to the motion-list bound: as ctl_range on the same range (0: the planner's reports are left alone)."""
    return (count // len(ctls)) * bin(CM.listed(ctls, voice_mask)).count("1")


# ---- per-entry values

class Rec:
    """A controller record as plain attributes (what store_voice reads), made from a CtlC or from nothing."""
    FIELDS = ("phase_inc", "inc_scale", "amp", "pan_left", "pan_right", "b0", "b1", "b2", "a1", "a2", "attack_time", "decay_time",
              "sustain_level", "release_time", "velocity", "smoothing", "fm_depth", "freq_scale", "am_depth", "pan_depth", "cz_depth",
              "cz_dist")

    def __init__(self, c=None):
        self.set = int(c.set) if c is not None else 0
        for f in self.FIELDS:
            setattr(self, f, np.float32(getattr(c, f)) if c is not None else np.float32(0))


def each_check(each, ctls, K, voice_mask):
    """skred_ctl_each_check without the checks skred_ctl_check makes on `ctls` itself: 0, BAD or RANGE."""
    if K < 1 or K > 64 or K & (K - 1):
        return RANGE
    if not voice_mask or (K < 64 and voice_mask >> K):
        return BAD
    ls = CM.lanes(voice_mask, K)
    sets = [int(ctls[l].set) for l in ls] if ctls is not None else []
    for e in each:
        s = int(e.set)
        if s & ~EACH_ALL or not s or e.reserved[0] or e.reserved[1]:
            return BAD
        named = [(EACH_INC_SCALE, (e.inc_scale,)), (EACH_AMP_SCALE, (e.amp_scale,)), (EACH_VELOCITY, (e.velocity,)),
                 (EACH_PAN, (e.pan_left, e.pan_right))]
        if any(s & bit and not np.isfinite(v) for bit, vals in named for v in vals):
            return BAD
        if s & EACH_AMP_SCALE and (e.amp_scale == 0 or ctls is None or not all(x & CM.AMP for x in sets)):
            return BAD
        if s & EACH_INC_SCALE and any(x & (CM.PHASE_INC | CM.INC_SCALE) for x in sets):
            return BAD
    return 0


def lay_over(rec, e):
    """Entry e laid over record rec: (the record the voice receives, stores withheld by the amp product)."""
    r = Rec(rec)
    withheld = 0
    s = int(e.set)
    if s & EACH_INC_SCALE:
        r.set |= CM.INC_SCALE
        r.inc_scale = np.float32(e.inc_scale)
    if s & EACH_AMP_SCALE:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            prod = np.float32(r.amp) * np.float32(e.amp_scale)
        if np.isfinite(prod) and prod != 0:
            r.amp = prod
        else:
            r.set &= ~CM.AMP
            withheld = 1
    if s & EACH_VELOCITY:
        r.set |= CM.VELOCITY
        r.velocity = np.float32(e.velocity)
    if s & EACH_PAN:
        r.set |= CM.PAN
        r.pan_left, r.pan_right = np.float32(e.pan_left), np.float32(e.pan_right)
    return r, withheld


def ctl_owned_each(owner, views, ctls, each, K, voice_mask, entries, tags, count):
    """Entry k on d_slots[k] when that is a slot whose owner is tags[k].  Returns ([written, withheld, owner differs], the distinct
    voices written, ascending).  A slot named twice is the caller's business (unspecified with INC_SCALE): refused here."""
    assert OM.tags_check(tags) == 0 and each_check(each, ctls, K, voice_mask) == 0 and len(each) == len(tags)
    n_voices = len(owner)
    res = [0, 0, 0]
    seen, touched = set(), []
    m = len(tags) if count is None else min(len(tags), count)
    for k in range(m):
        e = int(entries[k])
        if not CM.slot_valid(e, K, n_voices):
            continue
        if int(owner[e]) != int(tags[k]):
            res[2] += 1
            continue
        assert e not in seen, "a slot named twice: unspecified"
        seen.add(e)
        for l in CM.lanes(voice_mask, K):
            r, w = lay_over(ctls[l] if ctls is not None else None, each[k])
            got = None
            for view in views:
                h = w + CM.store_voice(view, e + l, r)
                assert got in (None, h), "the views disagree about the guards: one of them is stale"
                got = h
            res[0] += 1
            res[1] += got
            touched.append(e + l)
    return res, np.array(sorted(touched), np.int32)


def pack(tags, each):
    """What skred_bank_ctl_tags_each ships: the tags sorted as unsigned numbers, and each entry still beside its tag."""
    srt, perm = OM.pack(tags)
    return srt, [each[int(j)] for j in perm], perm


def ctl_tags_each(owner, views, ctls, each, first, count, K, voice_mask, tags):
    """find_owned, then ctl_owned_each on its list.  Returns (d_result, voices written, the list in the CALLER's tag order)."""
    lst = OM.find_owned(owner, first, count, K, tags)
    res, touched = ctl_owned_each(owner, views, ctls, each, K, voice_mask, lst, tags, None)
    assert res[2] == 0
    return res, touched, lst


def lists_each(ctls, each, K, voice_mask, n):
    """What the per-entry calls add to the motion-list bound."""
    named = any(int(e.set) & EACH_LISTS for e in each) or (ctls is not None and CM.listed(ctls, voice_mask))
    return n * bin(voice_mask).count("1") if named else 0
