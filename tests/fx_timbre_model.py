"""Numpy statement of per-note timbre on the fixed-point bank (include/skred_amd_fxpt.h: skred_fx_filter_each_check,
skred_fxbank_ctl_owned_each_filter / _ctl_tags_each_filter), on the arrays oracle.cpuref.fx_render works on.  It extends
tests/fx_expr_model.py: entry k's record is that model's overlay with SKRED_CTL_FILTER and the entry's five Q2.30 words laid over
it, and the stores are tests/fx_ctl_model.py's.  A set of coefficients is a skred_amd.fxbank.FxFilterEachC.  Every step is exact."""
import numpy as np

import fx_ctl_model as cm
import fx_expr_model as em
import fx_owner_model as om
from skred_amd import fxbank as fxb
from skred_amd.fxbank import fx_ctl

BAD = -2
COEFFS = ("b0_q30", "b1_q30", "b2_q30", "a1_q30", "a2_q30")


def filter_check(filt, c, n=None):
    """skred_fx_filter_each_check's verdict: 0 or SKRED_E_BAD_ARG."""
    if filt is None or (n is not None and n < 0):
        return BAD
    if c is not None and (cm.check(c) != 0 or c.which & fxb.CTL_FILTER):
        return BAD
    return BAD if any(any(f.reserved) for f in list(filt)[:n]) else 0


def overlay(c, e, f):
    """(the record the voice stores: `c` (or nothing) with entry `e` (or nothing) and the coefficients `f` laid over it; the amp
    products withheld, 0 or 1)"""
    r, withheld = em.overlay(c, e) if e is not None else (None, 0)
    if r is None:
        r = fx_ctl(0)
        if c is not None and e is None:
            for name, _ in fxb.FxCtlC._fields_:
                if name != "reserved":
                    setattr(r, name, getattr(c, name))
    r.which |= fxb.CTL_FILTER
    for k in COEFFS:
        setattr(r, k, getattr(f, k))
    return r, withheld


def ctl_owned_each_filter(owner, bank, c, entries, filt, voices, tags, d_count=None):
    """Entry k and filt[k] on voices[k] where that is a voice whose owner word is tags[k], in list order.  Returns [written,
    withheld, owner differs]."""
    n = len(tags)
    assert om.tags_check(tags, 0) == 0 and filter_check(filt, c, n) == 0 and len(filt) >= n
    assert entries is None or (em.each_check(entries, c, n) == 0 and len(entries) >= n)
    res, seen = [0, 0, 0], set()
    for k, v in enumerate(om.looked(voices, n, d_count).tolist()):
        if v < 0 or v >= bank.n:
            continue
        if owner[v] != np.uint32(tags[k]):
            res[2] += 1
            continue
        r, withheld = overlay(c, entries[k] if entries is not None else None, filt[k])
        assert not (r.which & fxb.CTL_INC_SCALE and v in seen), "a scaled increment on a voice listed twice is unspecified"
        seen.add(v)
        res[0] += 1
        res[1] += withheld + cm.store(bank, r, v)
    return res


def ctl_tags_each_filter(owner, bank, c, entries, filt, first, count, tags):
    """find_owned, then the call above on that list: filt[k] reaches the lowest voice that carries tags[k].  Returns (the result
    words, the list in the caller's order)."""
    assert om.tags_check(tags, om.UNIQUE) == 0
    lst = om.find_owned(owner, first, count, tags)
    res = ctl_owned_each_filter(owner, bank, c, entries, filt, lst, tags)
    assert res[2] == 0
    return res, lst


def single_record(c, e, f):
    """The record a single skred_fxbank_ctl_owned call takes in place of entry e and coefficients f over c, for a twin bank."""
    return overlay(c, e, f)[0]


def q30(x):
    """An fp32 coefficient as Q2.30, round to nearest, saturated to int32 -- the host's conversion, as for an upload."""
    return int(max(-(1 << 31), min((1 << 31) - 1, round(float(x) * (1 << 30)))))
