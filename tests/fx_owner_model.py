"""Numpy statement of the fixed-point bank's note owners (include/skred_amd_fxpt.h: skred_fxbank_tag_list / _find_owned /
_stamp_owned / _release_tags / _owner_clear), on the arrays oracle.cpuref.fx_render works on.  The owner array is a plain uint32
array beside the bank; the stamps are tests/fx_live_model.py's."""
import numpy as np

import fx_live_model as live
from skred_amd import fxbank as fxb

MAX_TAGS, ALLOW_ZERO, UNIQUE = fxb.OWNER_MAX_TAGS, fxb.OWNER_ALLOW_ZERO, fxb.OWNER_UNIQUE
BAD = -2


def new(n):
    return np.zeros(n, np.uint32)


def tags_check(tags, flags):
    """skred_owner_tags_check's verdict: 0 or SKRED_E_BAD_ARG."""
    tags = [int(t) for t in tags]
    if flags & ~(ALLOW_ZERO | UNIQUE):
        return BAD
    if flags & UNIQUE and len(tags) > MAX_TAGS:
        return BAD
    if not flags & ALLOW_ZERO and any(t == 0 for t in tags):
        return BAD
    if flags & UNIQUE and len(set(tags)) != len(tags):
        return BAD
    return 0


def pack(tags):
    """(sorted ascending as unsigned numbers, where each stood): the find pass's view of the tags"""
    tags = np.asarray(tags, np.uint32)
    perm = np.argsort(tags, kind="stable").astype(np.uint32)
    return tags[perm], perm


def looked(entries, n, d_count):
    m = n if d_count is None else min(n, int(d_count))
    return np.asarray(entries, np.int64)[:m]


def tag_list(owner, entries, tags, d_count=None):
    """owner[entry] = tag for the looked-at entries that are voices.  Returns [tagged, no voice].  (The entries that are voices must be
    distinct, or carry equal tags: the device's result is otherwise unspecified.)"""
    e = looked(entries, len(tags), d_count)
    valid = (e >= 0) & (e < len(owner))
    t = np.asarray(tags, np.uint32)[:len(e)]
    seen = {}
    for v, tag in zip(e[valid].tolist(), t[valid].tolist()):
        assert seen.setdefault(v, tag) == tag, "a voice named twice with different tags"
    owner[e[valid]] = t[valid]
    return [int(valid.sum()), int((~valid).sum())]


def find_owned(owner, first, count, tags):
    """int32[n]: the lowest voice of [first, first + count) whose owner equals tags[k], or -1"""
    assert tags_check(tags, UNIQUE) == 0 and count > 0 and 0 <= first and first + count <= len(owner)
    out = np.full(len(tags), -1, np.int32)
    rng = owner[first:first + count]
    for k, t in enumerate(tags):
        hit = np.flatnonzero(rng == np.uint32(t))
        if hit.size:
            out[k] = first + int(hit[0])
    return out


def stamp_owned(owner, bank, entries, tags, d_count, stamps, now):
    """The guarded stamps on `bank`.  Returns ([stamped, owner differs, no voice], the voices stamped in list order)."""
    assert tags_check(tags, 0) == 0
    e = looked(entries, len(tags), d_count)
    res, voices = [0, 0, 0], []
    for k, v in enumerate(e.tolist()):
        if v < 0 or v >= len(owner):
            res[2] += 1
        elif owner[v] != np.uint32(tags[k]):
            res[1] += 1
        else:
            res[0] += 1
            voices.append(v)
    live.stamp(bank, voices, stamps, now)
    return res, np.array(voices, np.int32)


def release_tags(owner, bank, first, count, tags, stamps, now):
    """find_owned, then stamp_owned on that list with the same tags.  Returns (result, voices stamped, the list)."""
    lst = find_owned(owner, first, count, tags)
    res, voices = stamp_owned(owner, bank, lst, tags, None, stamps, now)
    assert res[1] == 0
    return res, voices, lst


def clear(owner, first, count):
    owner[first:first + count] = 0
