"""Per-note timbre, stated in numpy: the per-entry filter coefficients of skred_bank_ctl_owned_each_filter / _ctl_tags_each_filter
and skred_filter_each_check, written from the definition in include/skred_amd.h (section "channels and per-note expression", C),
not from the kernels.  It extends tests/expr_model.py: entry k's record on voice l is that model's lay_over with SKRED_CTL_FILTER
and the entry's five words laid over it where bit l of filter_mask is set, and the stores are ctl_model.store_voice's.  A set of
coefficients is a skred_amd.device.FilterEachC."""
import numpy as np

import ctl_model as CM
import expr_model as EM
import owner_model as OM

BAD, RANGE = EM.BAD, EM.RANGE
COEFFS = ("b0", "b1", "b2", "a1", "a2")


def filter_check(filt, ctls, K, voice_mask, filter_mask):
    """skred_filter_each_check without the checks skred_ctl_check makes on `ctls` itself: 0, BAD or RANGE."""
    if filt is None:
        return BAD
    if K < 1 or K > 64 or K & (K - 1):
        return RANGE
    if not voice_mask or (K < 64 and voice_mask >> K):
        return BAD
    if not filter_mask or filter_mask & ~voice_mask:
        return BAD
    if ctls is not None and any(int(ctls[l].set) & CM.FILTER for l in CM.lanes(filter_mask, K)):
        return BAD
    for f in filt:
        if any(f.reserved) or not all(np.isfinite(getattr(f, k)) for k in COEFFS):
            return BAD
    return 0


def lay_over(rec, e, f):
    """Entry e (or nothing) and coefficients f (or nothing: a voice outside filter_mask) laid over record rec."""
    r, withheld = EM.lay_over(rec, e) if e is not None else (EM.Rec(rec), 0)
    if f is not None:
        r.set |= CM.FILTER
        for k in COEFFS:
            setattr(r, k, np.float32(getattr(f, k)))
    return r, withheld


def ctl_owned_each_filter(owner, views, ctls, each, filt, K, voice_mask, filter_mask, entries, tags, count):
    """Entry k on d_slots[k] when that is a slot whose owner is tags[k].  Returns ([written, withheld, owner differs], the distinct
    voices written, ascending)."""
    assert OM.tags_check(tags) == 0 and filter_check(filt, ctls, K, voice_mask, filter_mask) == 0 and len(filt) == len(tags)
    assert each is None or (EM.each_check(each, ctls, K, voice_mask) == 0 and len(each) == len(tags))
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
            r, w = lay_over(ctls[l] if ctls is not None else None, each[k] if each is not None else None,
                            filt[k] if (filter_mask >> l) & 1 else None)
            got = None
            for view in views:
                h = w + CM.store_voice(view, e + l, r)
                assert got in (None, h), "the views disagree about the guards: one of them is stale"
                got = h
            res[0] += 1
            res[1] += got
            touched.append(e + l)
    return res, np.array(sorted(touched), np.int32)


def ctl_tags_each_filter(owner, views, ctls, each, filt, first, count, K, voice_mask, filter_mask, tags):
    """find_owned, then the call above on its list.  Returns (d_result, voices written, the list in the CALLER's tag order)."""
    lst = OM.find_owned(owner, first, count, K, tags)
    res, touched = ctl_owned_each_filter(owner, views, ctls, each, filt, K, voice_mask, filter_mask, lst, tags, None)
    assert res[2] == 0
    return res, touched, lst


def lists(ctls, each, K, voice_mask, n):
    """What the calls add to the motion-list bound: FILTER is not a listing word, so what expr_model.lists_each says of the rest."""
    return EM.lists_each(ctls, each if each is not None else [], K, voice_mask, n)
