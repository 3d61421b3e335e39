"""The victim order of skred_fxbank_find_steal, stated in numpy on an FxVoiceBank plus `now` (include/skred_amd_fxpt.h gives the
definition field by field; every comparison is exact).  The idle predicate is tests/fx_live_model.py's."""
from dataclasses import dataclass, replace

import numpy as np

import fx_live_model as live
from skred_amd import fxbank as fxb

FIN, ENV, AMP = fxb.IDLE_FINISHED, fxb.IDLE_ENV_DONE, fxb.IDLE_AMP_ZERO
OLDEST, QUIETEST = fxb.STEAL_OLDEST, fxb.STEAL_QUIETEST
RELEASED_FIRST, RELEASED_ONLY = fxb.STEAL_RELEASED_FIRST, fxb.STEAL_RELEASED_ONLY
STEAL_MAX = fxb.STEAL_MAX
CAP = (1 << 62) - 1
NO_GAIN = 0x7FFFFFFF


@dataclass(frozen=True)
class Query:
    first: int
    count: int
    policy: int = OLDEST
    flags: int = 0
    min_age: int = 0
    exclude_idle: int = 0
    settle_q15: int = 0
    max_out: int = 16

    def c(self):
        return fxb.fx_steal_query(self.first, self.count, self.policy, self.flags, self.min_age, self.exclude_idle, self.settle_q15,
                                  self.max_out)

    def but(self, **kw):
        return replace(self, **kw)


def fields(bank, now, q):
    """(voices of the range, candidate mask, class, primary as uint64, released)"""
    v = np.arange(q.first, q.first + q.count)
    start, release = bank["sample_start"][v].astype(np.uint64), bank["sample_release"][v].astype(np.uint64)
    released = release != 0
    age = np.where(start > np.uint64(now), np.uint64(0), np.uint64(now) - start)
    cand = (bank["use_envelope"][v] != 0) & (bank["is_active"][v] != 0) & (age >= np.uint64(q.min_age))
    if q.flags & RELEASED_ONLY:
        cand &= released
    if q.exclude_idle:
        cand &= ~live.idle_mask(bank, q.exclude_idle, q.settle_q15)[v]
    cls = np.where(released, 0, 1) if q.flags & RELEASED_FIRST else np.ones(len(v), np.int64)
    if q.policy == OLDEST:
        primary = np.where(cls == 0, release, start)
    else:
        mag = np.minimum(np.abs(bank["smoother_gain_q15"][v].astype(np.int64)), NO_GAIN).astype(np.uint64)
        primary = np.where(bank["smoother_enable"][v] != 0, mag, np.uint64(NO_GAIN))
    return v, cand, cls.astype(np.uint64), np.minimum(primary.astype(np.uint64), np.uint64(CAP)), released


def keys(bank, now, q):
    v, cand, cls, primary, _ = fields(bank, now, q)
    return v, cand, (cls << np.uint64(62)) | primary


def victim_order(bank, now, q):
    """Every candidate of the range: ascending key, ties by ascending voice index (int32)."""
    v, cand, key = keys(bank, now, q)
    v, key = v[cand], key[cand]
    return v[np.lexsort((v, key))].astype(np.int32)


def victims(bank, now, q):
    """(the list the query writes: the first max_out of the order, total candidates)"""
    order = victim_order(bank, now, q)
    return order[:q.max_out], int(order.size)


def brute_force(bank, now, q):
    """The definition once more with Python integers and sorted(): no numpy in the predicate, the key or the ordering."""
    rows = []
    for v in range(q.first, q.first + q.count):
        start, release = int(bank["sample_start"][v]), int(bank["sample_release"][v])
        released = release != 0
        age = 0 if start > now else now - start
        gain = abs(int(bank["smoother_gain_q15"][v]))
        smooth = int(bank["smoother_enable"][v]) != 0
        active = int(bank["is_active"][v]) != 0
        if not (int(bank["use_envelope"][v]) != 0 and active and age >= q.min_age):
            continue
        if (q.flags & RELEASED_ONLY) and not released:
            continue
        idle = False
        if q.exclude_idle & FIN:
            idle |= int(bank["finished"][v]) != 0
        if q.exclude_idle & ENV:
            idle |= (not active) and (not smooth or gain <= q.settle_q15)      # (use_envelope != 0 holds here)
        if q.exclude_idle & AMP:
            idle |= int(bank["amp_q15"][v]) == 0
        if idle:
            continue
        cls = 0 if (q.flags & RELEASED_FIRST) and released else 1
        if q.policy == OLDEST:
            primary = release if cls == 0 else start
        else:
            primary = min(gain, NO_GAIN) if smooth else NO_GAIN
        rows.append(((cls << 62) | min(primary, CAP), v))
    return np.array([v for _, v in sorted(rows)], np.int32)


def assert_not_vacuous(bank, now, q, threshold=False):
    """Candidates and non-candidates both occur; every active restriction that CAN exclude a candidate does (an ENV_DONE exclusion
    cannot: it asks for is_active == 0, a candidate has is_active != 0); both classes occur under RELEASED_FIRST; with `threshold`
    the candidates reach past max_out and at least two voices are tied at the threshold key, one on each side of max_out."""
    order = victim_order(bank, now, q)
    n_with = len(order)
    assert 0 < n_with < q.count, f"{q}: {n_with} candidates of {q.count}"
    for name, without in (("min_age", q.but(min_age=0) if q.min_age else None),
                          ("RELEASED_ONLY", q.but(flags=q.flags & ~RELEASED_ONLY) if q.flags & RELEASED_ONLY else None),
                          ("exclude_idle", q.but(exclude_idle=0) if q.exclude_idle & (FIN | AMP) else None)):
        if without is not None:
            assert len(victim_order(bank, now, without)) > n_with, f"{q}: {name} excludes no candidate"
    if q.flags & RELEASED_FIRST and not q.flags & RELEASED_ONLY:
        _, cand, cls, _, _ = fields(bank, now, q)
        assert (cls[cand] == 0).any() and (cls[cand] == 1).any(), f"{q}: one class only"
    if threshold:
        assert n_with > q.max_out > 0, f"{q}: {n_with} candidates do not reach past max_out"
        v, _, key = keys(bank, now, q)
        key_of = dict(zip(v.tolist(), key.tolist()))
        assert key_of[int(order[q.max_out - 1])] == key_of[int(order[q.max_out])], f"{q}: no tie straddles max_out"
    return n_with
