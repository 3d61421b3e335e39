"""Channel polyphony, stated in numpy on a VoiceBank, `now` and an owner array (include/skred_amd.h, section "channel polyphony"):
the owner guard and the sounding count on top of tests/slot_steal_model.py, and the a / b rule of skred_bank_note_on_channel on top
of tests/slot_model.py and tests/owner_model.py.  Written from the definition, not from the kernels.  `owner` is a uint32 array of
one word per voice; a slot's owner is the word at its first voice; a match is (value, mask).
"""
import numpy as np

import owner_model as OM
import slot_model as SM
import slot_steal_model as M
from slot_steal_model import STEAL_MAX

NO_CAP = 0xFFFFFFFF


def matches(words, match):
    """skred_owner_match_t's rule on an array of owner words."""
    value, mask = match
    words = np.asarray(words, np.uint32)
    return (words != 0) & ((words & np.uint32(mask)) == np.uint32(value))


def channel(c):
    """The match of channel c under tag = channel << 24 | note id."""
    return (c << 24, 0xFF000000)


def terms(host, now, q, owner, match):
    """Per slot of the range: (first voices, sounding, candidate, key)."""
    heads, cand, cls, primary, t = M.terms(host, now, q)
    ok = matches(owner[heads], match)
    sounding = ok & t["live"].any(1)
    if q.exclude_idle:
        sounding &= ~t["idle"].all(1)
    return heads, sounding, cand & ok, (cls << np.uint64(62)) | primary


def victim_slots(host, now, q, owner, match):
    """(every candidate slot of the match: ascending key, ties by ascending first voice; the sounding count)."""
    heads, sounding, cand, key = terms(host, now, q, owner, match)
    heads, key = heads[cand], key[cand]
    return heads[np.lexsort((heads, key))].astype(np.int32), int(sounding.sum())


def query(host, now, q, owner, match):
    """What skred_bank_find_steal_slots_match leaves: (the list as written, [written, total, sounding])."""
    order, sounding = victim_slots(host, now, q, owner, match)
    written = min(len(order), q.max_out)
    return order[:written], [written, len(order), sounding]


def split(n, idle, sounding, victims, cap):
    """The a / b rule: notes on idle slots, notes on victims."""
    a = min(n, idle, cap - sounding if cap > sounding else 0)
    b = min(n - a, victims)
    return a, b


def burst(host, now, owner, iq, sq, match, cap, n):
    """skred_bank_note_on_channel's decisions for n notes: (d_assigned, [placed, dropped, stolen, S], idle slots listed).  `iq`: a
    SlotQueryC (first, count, slot_voices, member_mask, which, settle_level, start); `sq`: a slot_steal_model.SlotQuery."""
    idle = SM.idle_slots(host, iq.first, iq.count, iq.slot_voices, iq.member_mask, iq.which, iq.settle_level, iq.start)[:n]
    q = sq.but(exclude_idle=iq.which, settle_level=float(iq.settle_level), max_out=min(n, STEAL_MAX))
    victims, (written, total, sounding) = query(host, now, q, owner, match)
    assert not set(idle.tolist()) & set(victims.tolist())
    a, b = split(n, len(idle), sounding, written, cap)
    out = np.full(n, -1, np.int32)
    out[:a] = idle[:a]
    out[a:a + b] = victims[:b]
    return out, [a + b, n - a - b, b, sounding], len(idle)


def tag(owner, assigned, tags, K):
    """The tags of the placed notes, as skred_bank_tag_slots on d_assigned writes them (-1 entries are skipped)."""
    return OM.tag_slots(owner, assigned, tags, None, K)


def kind(n, n_idle, res, cap):
    """The name of what a burst showed (tests/test_chan_cpu.py and tests/test_chan.py assert the set of names seen)."""
    placed, dropped, stolen, sounding = res
    if cap == 1:
        return "mono"
    if n_idle == 0:
        return "no idle"
    if dropped:
        return "dropped"
    if sounding > cap:
        return "above"
    if stolen == n:
        return "at"
    if stolen == 0 and sounding + n <= cap:
        return "under"
    return "mixed"
