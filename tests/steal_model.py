"""The victim order of skred_bank_find_steal, stated in numpy on a VoiceBank plus `now` (include/skred_amd.h gives the definition
field by field; every comparison is exact).  The idle predicate and the named set are tests/test_idle.py's."""
from dataclasses import dataclass, replace

import numpy as np

from test_idle import FIN, ENV, AMP, UNNAMED, criteria, named_set

OLDEST, QUIETEST = 0, 1
RELEASED_FIRST, RELEASED_ONLY, STEAL_UNNAMED = 1, 2, 256
STEAL_MAX = 1024
CAP = (1 << 62) - 1


@dataclass(frozen=True)
class Query:
    first: int
    count: int
    policy: int = OLDEST
    flags: int = 0
    min_age: int = 0
    exclude_idle: int = 0
    settle_level: float = 0.0
    max_out: int = 16

    def c(self):
        from skred_amd import device
        return device.steal_query(self.first, self.count, self.policy, self.flags, self.min_age, self.exclude_idle,
                                  self.settle_level, self.max_out)

    def but(self, **kw):
        return replace(self, **kw)


def idle_pred(host, v, which, settle):
    """skred_bank_find_idle's predicate for the voices v: any selected criterion, and with UNNAMED not in the named set."""
    idle = np.zeros(len(v), bool)
    for bit, holds in criteria(host, v, settle).items():
        if which & bit:
            idle |= holds
    if which & UNNAMED:
        idle &= ~named_set(host)[v]
    return idle


def fields(host, now, q):
    """(voices of the range, candidate mask, class, primary as uint64, released)"""
    a = host.a
    e = a["voice_amp_envelope"]
    v = np.arange(q.first, q.first + q.count)
    start, release = e["sample_start"][v].astype(np.uint64), e["sample_release"][v].astype(np.uint64)
    released = release != 0
    age = np.where(start > np.uint64(now), np.uint64(0), np.uint64(now) - start)
    cand = (a["voice_use_amp_envelope"][v] != 0) & (e["is_active"][v] != 0) & (age >= np.uint64(q.min_age))
    if q.flags & RELEASED_ONLY:
        cand &= released
    if q.flags & STEAL_UNNAMED:
        cand &= ~named_set(host)[v]
    if q.exclude_idle:
        cand &= ~idle_pred(host, v, q.exclude_idle, q.settle_level)
    cls = np.where(released, 0, 1) if q.flags & RELEASED_FIRST else np.ones(len(v), np.int64)
    if q.policy == OLDEST:
        primary = np.where(cls == 0, release, start)
    else:
        bits = np.abs(a["voice_smoother_gain"][v].astype(np.float32)).view(np.uint32).astype(np.uint64)
        primary = np.where(a["voice_smoother_enable"][v] != 0, bits, np.uint64(0x7fffffff))
    return v, cand, cls.astype(np.uint64), np.minimum(primary.astype(np.uint64), np.uint64(CAP)), released


def keys(host, now, q):
    v, cand, cls, primary, _ = fields(host, now, q)
    return v, cand, (cls << np.uint64(62)) | primary


def victim_order(host, now, q):
    """Every candidate of the range: ascending key, ties by ascending voice index (int32)."""
    v, cand, key = keys(host, now, q)
    v, key = v[cand], key[cand]
    return v[np.lexsort((v, key))].astype(np.int32)


def brute_force(host, now, q):
    """The same with Python integers and sorted(): no numpy in the ordering."""
    v, cand, cls, primary, _ = fields(host, now, q)
    rows = [((int(c) << 62) | min(int(p), CAP), int(i)) for i, ok, c, p in zip(v, cand, cls, primary) if ok]
    return np.array([i for _, i in sorted(rows)], np.int32)


def assert_not_vacuous(host, now, q, threshold=False):
    """Every active restriction excludes some voice that would otherwise be a candidate; both classes are present under
    RELEASED_FIRST; with `threshold` more candidates than max_out."""
    n_with = len(victim_order(host, now, q))
    a = host.a
    v = np.arange(q.first, q.first + q.count)
    base = (a["voice_use_amp_envelope"][v] != 0) & (a["voice_amp_envelope"]["is_active"][v] != 0)
    assert base.any() and not base.all(), f"{q}: the envelope rule is vacuous ({int(base.sum())} of {q.count})"
    for name, without in (("min_age", q.but(min_age=0) if q.min_age else None),
                          ("RELEASED_ONLY", q.but(flags=q.flags & ~RELEASED_ONLY) if q.flags & RELEASED_ONLY else None),
                          ("UNNAMED", q.but(flags=q.flags & ~STEAL_UNNAMED) if q.flags & STEAL_UNNAMED else None),
                          ("exclude_idle", q.but(exclude_idle=0) if q.exclude_idle else None)):
        if without is not None:
            assert len(victim_order(host, now, without)) > n_with, f"{q}: {name} excludes no candidate"
    assert n_with > 0, f"{q}: no candidate"
    if q.flags & RELEASED_FIRST:
        _, cand, cls, _, _ = fields(host, now, q)
        assert (cls[cand] == 0).any() and (cls[cand] == 1).any(), f"{q}: one class only"
    if threshold:
        assert n_with > q.max_out, f"{q}: {n_with} candidates do not reach past max_out"
    return n_with


__all__ = ["Query", "victim_order", "brute_force", "assert_not_vacuous", "keys", "fields", "idle_pred", "FIN", "ENV", "AMP", "UNNAMED"]
