"""The victim order of skred_bank_find_steal_slots, stated in numpy on a VoiceBank plus `now` (include/skred_amd.h, section "slot
stealing", gives the definition field by field; every comparison is exact).  Written from that definition, not from the kernel: a
slot is K consecutive voices from a multiple of K, named by its first voice; only voices with a bit in member_mask are looked at,
and of those only the live ones decide age, class and key.  The idle exclusion is steal_model.idle_pred.
"""
from dataclasses import dataclass, replace

import numpy as np

import steal_model as sm
from steal_model import CAP, OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, STEAL_MAX  # noqa: F401


@dataclass(frozen=True)
class SlotQuery:
    first: int
    count: int
    K: int
    mask: int
    policy: int = OLDEST
    flags: int = 0
    min_age: int = 0
    exclude_idle: int = 0
    settle_level: float = 0.0
    max_out: int = 16

    def c(self):
        from skred_amd.bank import slot_steal_query
        return slot_steal_query(self.first, self.count, self.K, self.mask, self.policy, self.flags, self.min_age, self.exclude_idle,
                                self.settle_level, self.max_out)

    def but(self, **kw):
        return replace(self, **kw)

    def voice(self):
        """The per-voice query of a K = 1 slot query."""
        assert self.K == 1 and self.mask == 1
        return sm.Query(self.first, self.count, self.policy, self.flags, self.min_age, self.exclude_idle, self.settle_level, self.max_out)


def lanes(mask, K):
    return [l for l in range(K) if (mask >> l) & 1]


def terms(host, now, q):
    """Per slot of the range: (first voices, candidate, class, primary as uint64) and, per slot and member lane, the per-voice terms
    (member lanes, live, released, age, idle, the value a live member offers for the primary in class 0 and in class 1)."""
    a = host.a
    e = a["voice_amp_envelope"]
    heads = np.arange(q.first, q.first + q.count, q.K)
    mem = np.array(lanes(q.mask, q.K), np.int64)
    v = heads[:, None] + mem[None, :]                                     # [slots, members]: the only voices ever read
    start, release = e["sample_start"][v].astype(np.uint64), e["sample_release"][v].astype(np.uint64)
    live = (a["voice_use_amp_envelope"][v] != 0) & (e["is_active"][v] != 0)
    released = release != 0
    age = np.where(start > np.uint64(now), np.uint64(0), np.uint64(now) - start)
    some = live.any(1)
    cand = some & ~(live & (age < np.uint64(q.min_age))).any(1)
    all_released = ~(live & ~released).any(1)
    if q.flags & RELEASED_ONLY:
        cand &= all_released
    idle = np.zeros(v.shape, bool)
    if q.exclude_idle:
        idle = sm.idle_pred(host, v.reshape(-1), q.exclude_idle, q.settle_level).reshape(v.shape)
        cand &= ~idle.all(1)
    cls = np.where(all_released, 0, 1) if q.flags & RELEASED_FIRST else np.ones(len(heads), np.int64)
    if q.policy == OLDEST:
        offer0, offer1 = release, start
    else:
        bits = np.abs(a["voice_smoother_gain"][v].astype(np.float32)).view(np.uint32).astype(np.uint64)
        offer0 = offer1 = np.where(a["voice_smoother_enable"][v] != 0, bits, np.uint64(0x7fffffff))
    offer = np.where((cls == 0)[:, None], offer0, offer1)
    primary = np.where(live, offer, np.uint64(0)).max(1) if len(mem) else np.zeros(len(heads), np.uint64)
    primary = np.minimum(primary.astype(np.uint64), np.uint64(CAP))
    return heads, cand, cls.astype(np.uint64), primary, dict(v=v, live=live, released=released, age=age, idle=idle, offer=offer)


def keys(host, now, q):
    heads, cand, cls, primary, _ = terms(host, now, q)
    return heads, cand, (cls << np.uint64(62)) | primary


def victim_slots(host, now, q):
    """Every candidate slot of the range: ascending key, ties by ascending first voice (int32)."""
    heads, cand, key = keys(host, now, q)
    heads, key = heads[cand], key[cand]
    return heads[np.lexsort((heads, key))].astype(np.int32)


def brute_force(host, now, q):
    """The same, slot by slot and voice by voice with Python integers and sorted(): no numpy in the rules or the ordering."""
    a = host.a
    e = a["voice_amp_envelope"]
    rows = []
    for h in range(q.first, q.first + q.count, q.K):
        live = []
        members = [h + l for l in lanes(q.mask, q.K)]
        for v in members:
            if a["voice_use_amp_envelope"][v] != 0 and e["is_active"][v] != 0:
                live.append(v)
        if not live:
            continue
        ages = [0 if int(e["sample_start"][v]) > now else now - int(e["sample_start"][v]) for v in live]
        if min(ages) < q.min_age:
            continue
        all_released = all(int(e["sample_release"][v]) != 0 for v in live)
        if (q.flags & RELEASED_ONLY) and not all_released:
            continue
        if q.exclude_idle and sm.idle_pred(host, np.array(members), q.exclude_idle, q.settle_level).all():
            continue
        cls = 0 if (q.flags & RELEASED_FIRST) and all_released else 1
        if q.policy == OLDEST:
            primary = max(int(e["sample_release"][v]) if cls == 0 else int(e["sample_start"][v]) for v in live)
        else:
            primary = max(int(np.abs(np.float32(a["voice_smoother_gain"][v])).view(np.uint32)) if a["voice_smoother_enable"][v] != 0
                          else 0x7fffffff for v in live)
        rows.append(((cls << 62) | min(primary, CAP), h))
    return np.array([h for _, h in sorted(rows)], np.int32)
