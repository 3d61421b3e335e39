"""Numpy statement of channels and per-note expression on the fixed-point bank (include/skred_amd_fxpt.h: skred_fx_ctl_each_check,
skred_fxbank_find_match / _stamp_match / _ctl_match / _ctl_owned_each / _ctl_tags_each), on the arrays oracle.cpuref.fx_render
works on.  The owner array is tests/fx_owner_model.py's, the stamps tests/fx_live_model.py's, a record's stores
tests/fx_ctl_model.py's; an entry is a skred_amd.fxbank.FxCtlEachC.  Every step is exact: plain Python integers."""
import numpy as np

import fx_ctl_model as cm
import fx_live_model as live
import fx_owner_model as om
from skred_amd import fxbank as fxb
from skred_amd.fxbank import fx_ctl

BAD = -2
M32 = 0xFFFFFFFF


def match_check(value, mask):
    """skred_owner_match_check's verdict: a value with bits outside the mask is a value no owner word can give."""
    return BAD if value & ~mask & M32 else 0


def matches(owner, value, mask):
    """bool per voice: owner != 0 and (owner & mask) == value"""
    assert match_check(value, mask) == 0
    o = np.asarray(owner, np.uint32)
    return (o != 0) & ((o & np.uint32(mask)) == np.uint32(value))


def find_match(owner, first, count, value, mask, max_out=None):
    """(the listed voices int32, ascending, cut at max_out; the total)"""
    assert count > 0 and 0 <= first and first + count <= len(owner)
    hit = (first + np.flatnonzero(matches(owner, value, mask)[first:first + count])).astype(np.int32)
    return hit[:len(hit) if max_out is None else max_out], int(hit.size)


def stamp_match(owner, bank, first, count, value, mask, stamps, now):
    """The stamps on every matching voice of the range.  Returns ([stamped, did not match], the voices stamped)."""
    voices, total = find_match(owner, first, count, value, mask)
    live.stamp(bank, voices, stamps, now)
    return [total, count - total], voices


def ctl_match(owner, bank, c, first, count, value, mask):
    """ctl_range on the matching voices.  Returns [written, withheld, did not match]."""
    assert cm.check(c) == 0
    voices, total = find_match(owner, first, count, value, mask)
    return [total, sum(cm.store(bank, c, int(v)) for v in voices), count - total]


# ---------------------------------------------------------------------------------------------- per-entry values

EACH_RANGES = {fxb.EACH_VELOCITY: ("velocity_q15",), fxb.EACH_PAN: ("pan_left_q15", "pan_right_q15")}


def each_check(entries, c, n=None):
    """skred_fx_ctl_each_check's verdict: 0 or SKRED_E_BAD_ARG."""
    if entries is None or (n is not None and n < 0):
        return BAD
    if c is not None and cm.check(c) != 0:
        return BAD
    which = c.which if c is not None else 0
    for e in list(entries)[:n]:
        if e.set == 0 or e.set & ~fxb.EACH_ALL or any(e.reserved):
            return BAD
        for bit, names in EACH_RANGES.items():
            if e.set & bit and not all(0 <= getattr(e, k) <= 65535 for k in names):
                return BAD
        if e.set & fxb.EACH_AMP_SCALE and (e.amp_scale_q16 == 0 or not which & fxb.CTL_AMP):
            return BAD
        if e.set & fxb.EACH_INC_SCALE and which & (fxb.CTL_PHASE_INC | fxb.CTL_INC_SCALE):
            return BAD
    return 0


def overlay(c, e):
    """(the record voice k stores: `c` (or nothing) with entry `e` laid over it, or None when nothing is left to store; the amp
    products withheld, 0 or 1)"""
    r = fx_ctl(0)
    if c is not None:
        for name, _ in fxb.FxCtlC._fields_:
            if name != "reserved":
                setattr(r, name, getattr(c, name))
    withheld = 0
    if e.set & fxb.EACH_INC_SCALE:
        r.which |= fxb.CTL_INC_SCALE
        r.inc_scale_q16 = e.inc_scale_q16
    if e.set & fxb.EACH_AMP_SCALE:
        prod = (int(r.amp_q15) * int(e.amp_scale_q16)) >> 16
        if 1 <= prod <= 65535:
            r.amp_q15 = prod
        else:
            r.which &= ~fxb.CTL_AMP                       # the amp is left alone: its guard cannot count the voice again
            withheld = 1
    if e.set & fxb.EACH_VELOCITY:
        r.which |= fxb.CTL_VELOCITY
        r.velocity_q15 = e.velocity_q15
    if e.set & fxb.EACH_PAN:
        r.which |= fxb.CTL_PAN
        r.pan_left_q15, r.pan_right_q15 = e.pan_left_q15, e.pan_right_q15
    return (r if r.which else None), withheld


def ctl_owned_each(owner, bank, c, entries, voices, tags, d_count=None):
    """Entry k on voices[k] where that is a voice whose owner word is tags[k], in list order.  Returns [written, withheld, owner
    differs].  A scaled increment on a voice listed twice is unspecified on the device, so such lists are refused here."""
    n = len(tags)
    assert om.tags_check(tags, 0) == 0 and each_check(entries, c, n) == 0 and len(entries) >= n
    res, seen = [0, 0, 0], set()
    for k, v in enumerate(om.looked(voices, n, d_count).tolist()):
        if v < 0 or v >= bank.n:
            continue
        if owner[v] != np.uint32(tags[k]):
            res[2] += 1
            continue
        r, withheld = overlay(c, entries[k])
        scaled = r is not None and r.which & fxb.CTL_INC_SCALE
        assert not (scaled and v in seen), "a scaled increment on a voice listed twice is unspecified"
        seen.add(v)
        res[0] += 1
        res[1] += withheld + (cm.store(bank, r, v) if r is not None else 0)
    return res


def ctl_tags_each(owner, bank, c, entries, first, count, tags):
    """find_owned, then ctl_owned_each on that list: entries[k] reaches the lowest voice that carries tags[k].  Returns (the result
    words, the list in the caller's order)."""
    assert om.tags_check(tags, om.UNIQUE) == 0
    lst = om.find_owned(owner, first, count, tags)
    res = ctl_owned_each(owner, bank, c, entries, lst, tags)
    assert res[2] == 0
    return res, lst


def single_record(c, e):
    """The record n single skred_fxbank_ctl_owned calls would take in place of entry e over c (None: the call is left out), for the
    twin bank.  The amp product is the host's here; where it is withheld the twin's record drops SKRED_CTL_AMP."""
    return overlay(c, e)[0]
