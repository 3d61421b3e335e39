"""Channel polyphony on the fixed-point bank, stated in numpy on an FxVoiceBank, `now` and an owner array (include/skred_amd_fxpt.h,
section "channel polyphony"): the owner guard and the sounding count on top of tests/fx_steal_model.py, and the a / b rule of
skred_fxbank_note_on_channel on top of tests/fx_live_model.py and tests/fx_owner_model.py.  Written from the definition, not from the
kernel.  `owner` is a uint32 array of one word per voice; a match is (value, mask).  The a / b rule and the names of a burst's
outcomes are the float bank's (tests/chan_model.py: split, kind), by import.
"""
import numpy as np

import fx_live_model as live
import fx_owner_model as OM
import fx_steal_model as sm
from chan_model import NO_CAP, channel, kind, matches, split      # noqa: F401  (re-exported: the tests name them through this module)
from fx_steal_model import STEAL_MAX


def terms(bank, now, q, owner, match):
    """Per voice of the range: (voices, sounding, candidate, key)."""
    v, cand, cls, primary, _ = sm.fields(bank, now, q)
    ok = matches(np.asarray(owner, np.uint32)[v], match)
    sounding = ok & (bank["use_envelope"][v] != 0) & (bank["is_active"][v] != 0)
    if q.exclude_idle:
        sounding &= ~live.idle_mask(bank, q.exclude_idle, q.settle_q15)[v]
    return v, sounding, cand & ok, (cls << np.uint64(62)) | primary


def victim_order(bank, now, q, owner, match):
    """(every candidate of the match: ascending key, ties by ascending voice; the sounding count)."""
    v, sounding, cand, key = terms(bank, now, q, owner, match)
    v, key = v[cand], key[cand]
    return v[np.lexsort((v, key))].astype(np.int32), int(sounding.sum())


def query(bank, now, q, owner, match):
    """What skred_fxbank_find_steal_match leaves: (the list as written, [written, total, sounding])."""
    order, sounding = victim_order(bank, now, q, owner, match)
    written = min(len(order), q.max_out)
    return order[:written], [written, len(order), sounding]


def burst(bank, now, owner, iq, sq, match, cap, n):
    """skred_fxbank_note_on_channel's decisions for n notes: (d_assigned, [placed, dropped, stolen, S], idle voices listed).  `iq`: an
    FxIdleQueryC (first, count, which, settle_q15, start); `sq`: a fx_steal_model.Query."""
    idle, _ = live.idle_list(bank, iq.first, iq.count, iq.which, iq.settle_q15, iq.start, n)
    q = sq.but(exclude_idle=iq.which, settle_q15=iq.settle_q15, max_out=min(n, STEAL_MAX))
    victims, (written, total, sounding) = query(bank, now, q, owner, match)
    assert not set(idle.tolist()) & set(victims.tolist())
    a, b = split(n, len(idle), sounding, written, cap)
    out = np.full(n, -1, np.int32)
    out[:a] = idle[:a]
    out[a:a + b] = victims[:b]
    return out, [a + b, n - a - b, b, sounding], len(idle)


def tag(owner, assigned, tags):
    """The tags of the placed notes, as skred_fxbank_tag_list on d_assigned writes them (-1 entries are skipped)."""
    return OM.tag_list(owner, assigned, tags)
