"""Note owners, stated in numpy: the owner array as a pure function of the call sequence, the lowest-match rule of the find pass, the
guard of the stamps and controllers, and the counts.  Written from the definition in include/skred_amd.h (section "note owners"), not
from the kernels.  `owner` is a uint32 array of one word per voice; a slot's owner is the word at its first voice, 0 is nobody.
The stamps themselves are slot_model.stamp's, the controller stores ctl_model.apply's.
"""
import numpy as np

import ctl_model as CM
import slot_model as SM

MAX_TAGS = 1024
ALLOW_ZERO, UNIQUE = 1, 2
BAD = -2


def new(n_voices):
    return np.zeros(n_voices, np.uint32)


def tags_check(tags, flags=0):
    """skred_owner_tags_check: 0 or SKRED_E_BAD_ARG."""
    tags = [int(t) for t in tags]
    if flags & ~(ALLOW_ZERO | UNIQUE):
        return BAD
    if (flags & UNIQUE) and len(tags) > MAX_TAGS:
        return BAD
    if not (flags & ALLOW_ZERO) and any(t == 0 for t in tags):
        return BAD
    if (flags & UNIQUE) and len(set(tags)) != len(tags):
        return BAD
    return 0


def pack(tags):
    """(sorted tags as unsigned numbers, perm: where each stood) -- what the find pass stages."""
    tags = np.asarray(tags, np.uint32)
    perm = np.argsort(tags, kind="stable").astype(np.uint32)
    return tags[perm], perm


def looked(entries, n, count):
    m = n if count is None else min(n, count)
    return [int(e) for e in entries[:m]]


def tag_slots(owner, entries, tags, count, K):
    """owner[entry] = tag on the first min(len(tags), count) entries that are slots.  Returns [tagged, skipped]."""
    tagged = skipped = 0
    seen = {}
    for k, e in enumerate(looked(entries, len(tags), count)):
        if CM.slot_valid(e, K, len(owner)):
            assert seen.setdefault(e, int(tags[k])) == int(tags[k]), "a slot named twice with different tags: unspecified"
            owner[e] = np.uint32(tags[k])
            tagged += 1
        else:
            skipped += 1
    return [tagged, skipped]


def find_owned(owner, first, count, K, tags):
    """The lowest first voice of a slot of the range whose owner word is the tag, or -1."""
    assert tags_check(tags, UNIQUE) == 0
    heads = np.arange(first, first + count, K)
    words = owner[heads]
    out = np.full(len(tags), -1, np.int32)
    for k, t in enumerate(tags):
        hit = heads[words == np.uint32(t)]
        if len(hit):
            out[k] = hit.min()
    return out


def guard(owner, entries, tags, count, K):
    """(entries that pass, [passed, owner differs, no slot]) over the first min(len(tags), count) entries, in list order."""
    assert tags_check(tags) == 0
    passed, res = [], [0, 0, 0]
    for k, e in enumerate(looked(entries, len(tags), count)):
        if not CM.slot_valid(e, K, len(owner)):
            res[2] += 1
        elif int(owner[e]) != int(tags[k]):
            res[1] += 1
        else:
            res[0] += 1
            passed.append(e)
    return passed, res


def stamp_owned(owner, truth, entries, tags, count, K, voice_mask, stamps, now):
    """Returns (d_result, the voices stamped).  `truth` (the oracle's bank) receives slot_model.stamp."""
    passed, res = guard(owner, entries, tags, count, K)
    voices = np.array([e + l for e in passed for l in SM.lanes(voice_mask, K)], np.int32)
    SM.stamp(truth, voices, stamps, now)
    return res, voices


def release_tags(owner, truth, first, count, K, voice_mask, tags, stamps, now):
    """find_owned, then stamp_owned on its list: every tag stamps at most one slot, the lowest.  Returns (d_result, voices, the list)."""
    lst = find_owned(owner, first, count, K, tags)
    res, voices = stamp_owned(owner, truth, lst, tags, None, K, voice_mask, stamps, now)
    assert res[1] == 0
    return res, voices, lst


def ctl_owned(owner, views, ctls, voice_mask, entries, tags, count):
    """ctl_model's stores on the entries that pass the guard.  Returns ([written, withheld, owner differs], voices written)."""
    K = len(ctls)
    passed, res = guard(owner, entries, tags, count, K)
    voices = [(e + l, l) for e in passed for l in CM.lanes(voice_mask, K)]
    (written, withheld), touched = CM.apply(views, ctls, voices)
    return [written, withheld, res[1]], touched


def clear(owner, first, count):
    owner[first:first + count] = 0
