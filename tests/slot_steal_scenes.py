"""The scenes of the slot-stealing tests (tests/test_slot_steal_cpu.py asserts on the oracle's state that none of them is vacuous,
tests/test_slot_steal.py runs them on the device): banks of the C2 recipe cut into slots of K voices, every slot of a KIND --

  0 held         every member (a bit in member_mask) sustains;
  1 released     every member is in a release that does not end;
  2 one held     every member released but ONE, which is held: that member alone keeps the slot out of RELEASED_ONLY and moves it
                 from class 0 to class 1;
  3 one young    every member old but ONE, started a few frames ago: that member alone keeps the slot off a min_age query;
  4 shadowed     the members old and released, every voice outside the mask young, held and loud: a kernel that read them would
                 rank the slot elsewhere;
  5 partly idle  some members at rest, the others sounding: a candidate all the same;
  6 dead         no live member: never a candidate;
  7 finished     every member a finished voice whose envelope is still active (held, or in release): live, a candidate -- unless
                 the exclusion lists it.

Within kinds 0 .. 2 the DECIDING member -- the one with the latest clocks -- sits at the lowest member lane, at the highest, or at
a drawn one; its clocks are drawn from few values, so that many slots share a key and the threshold of a short list falls among
ties.  The first and the last eight slots hold every kind once.
"""
import functools

import numpy as np

import slot_steal_model as M
from oracle import cpuref
from skred_amd import banks
from slot_scenes import masks
from steal_model import OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, FIN, ENV

FRAMES = (65, 130)
SETTLE = np.float32(1e-3)
EXCLUDE = FIN | ENV
KINDS = 8
YOUNG_START = 5            # frames before the scene's clock a young voice starts: its age when queried is 5 + sum(FRAMES) = 200
MIN_AGE = 1000             # between a young voice's age and every old one's


def build(n, K, mask, seed=0):
    bank, tables, g = banks.bank_c2(n)
    now = int(g.synth_sample_count)
    e = bank["voice_amp_envelope"]
    rng = np.random.default_rng(9000 + 17 * n + K + 1000 * seed + (mask % 9973))
    slots = n // K
    kind = rng.integers(0, KINDS, slots)
    kind[:min(KINDS, slots)] = np.arange(min(KINDS, slots))
    if slots >= 2 * KINDS:
        kind[slots - KINDS:] = np.arange(KINDS)
    mem = M.lanes(mask, K)
    e["attack_time"], e["decay_time"] = np.float32(20.0), np.float32(50.0)
    e["release_time"] = np.float32(1e6)                                        # a release that does not end inside the scene
    e["is_active"] = 1
    bank["voice_use_amp_envelope"][:] = 1
    e["velocity"] = rng.uniform(0.2, 0.6, n).astype(np.float32)

    def held(v, r):
        e["sample_start"][v], e["sample_release"][v] = np.uint64(now - 40000 + r), np.uint64(0)

    def released(v, r):
        e["sample_start"][v], e["sample_release"][v] = np.uint64(now - 40000 + r), np.uint64(now - 3000 + r)

    def young(v):
        held(v, 0)
        e["sample_start"][v] = np.uint64(now - YOUNG_START)
        e["velocity"][v] = np.float32(1.0)

    def rest(v):
        e["is_active"][v] = 0
        bank["voice_smoother_gain"][v] = np.float32(0.0)

    for s in range(slots):
        k, h = int(kind[s]), s * K
        fin_released = bool(rng.integers(0, 2))
        decide = mem[0] if s % 3 == 0 else mem[-1] if s % 3 == 1 else int(rng.choice(mem))
        for l in range(K):
            v = h + l
            r = 1500 + 3 * int(rng.integers(0, 6)) if l == decide else int(rng.integers(0, 1000))
            if l not in mem:                                                     # outside the mask: anything, never looked at
                [lambda: held(v, r), lambda: released(v, r), lambda: young(v), lambda: rest(v)][int(rng.integers(0, 4))]()
                if k == 4:
                    young(v)
                continue
            if k == 0:
                held(v, r)
            elif k in (1, 2, 4):
                released(v, r)
            elif k == 3:
                (held if rng.integers(0, 2) else released)(v, r)
            elif k == 5:
                (held if rng.integers(0, 2) else released)(v, r)
                if l != decide:
                    rest(v) if rng.integers(0, 2) else None
            elif k == 6:
                rest(v)
                if rng.integers(0, 2):
                    bank["voice_use_amp_envelope"][v] = 0
            else:
                (released if s == 7 or fin_released else held)(v, r)
                bank["voice_finished"][v] = 1
        if k == 2:
            held(h + int(rng.choice(mem)), int(rng.integers(0, 1000)))
        if k == 3:
            young(h + int(rng.choice(mem)))
        if k == 5 and len(mem) > 1:
            rest(h + (mem[0] if decide != mem[0] else mem[1]))
    return bank, tables, g, kind


@functools.lru_cache(maxsize=64)
def scene(n, K, mask, seed=0):
    """(bank, tables, globals, the oracle's bank after FRAMES, `now` there, kind per slot)"""
    bank, tables, g, kind = build(n, K, mask, seed)
    truth, gl = bank.copy(), g.copy()
    for f in FRAMES:
        cpuref.render(truth, gl, tables, f, 0)
    return bank, tables, g, truth, int(gl.synth_sample_count), kind


def queries(n, K, mask, first=0, count=None):
    """What every scene runs: both policies x every flag combination x exclude_idle off / on, a list longer than the candidates;
    then min_age, short lists (the threshold) and a count."""
    count = n - first if count is None else count
    room = min(count // K, M.STEAL_MAX)
    base = M.SlotQuery(first, count, K, mask, max_out=room)
    out = []
    for policy in (OLDEST, QUIETEST):
        for flags in (0, RELEASED_FIRST, RELEASED_ONLY, RELEASED_FIRST | RELEASED_ONLY):
            for ex in (0, EXCLUDE):
                out.append(base.but(policy=policy, flags=flags, exclude_idle=ex, settle_level=float(SETTLE)))
    out.append(base.but(min_age=MIN_AGE))
    out.append(base.but(min_age=MIN_AGE, flags=RELEASED_FIRST, policy=QUIETEST, exclude_idle=EXCLUDE, settle_level=float(SETTLE)))
    out.append(base.but(max_out=0))
    return out


def threshold_queries(host, now, n, K, mask, first=0, count=None):
    """Short lists whose last entry ties with the first entry left out (found on the model; empty when the scene has no such tie)."""
    count = n - first if count is None else count
    out = []
    for flags in (0, RELEASED_FIRST):
        q = M.SlotQuery(first, count, K, mask, flags=flags)
        heads, cand, key = M.keys(host, now, q)
        order = np.lexsort((heads[cand], key[cand]))
        ks = key[cand][order]
        ties = np.flatnonzero(ks[1:] == ks[:-1]) + 1                             # list lengths that cut a run of equal keys
        ties = ties[ties <= M.STEAL_MAX]
        if len(ties):
            out.append(q.but(max_out=int(ties[len(ties) // 2])))
            out.append(q.but(max_out=int(ties[0])))
    return out


# (n, K, mask name): 64 voices = one wavefront, 320 = two workgroups, the last ragged, 1088 = five, 4160 = seventeen.  A FULL case has
# at least sixteen slots, room for every kind twice; the small ones run against the model all the same
FULL_CASES = [(n, K, name) for n in (64, 320, 1088) for K in (1, 2, 8, 64) if n // K >= 16 for name in masks(K)] + \
             [(4160, 64, name) for name in masks(64)] + [(4160, 8, "alt")]    # seventeen workgroups, several slots per wavefront
SMALL_CASES = [(64, 8, "all"), (64, 8, "alt"), (64, 64, "all"), (64, 64, "high"), (320, 64, "alt")]
UNALIGNED = (320, 8, 0x55, 24, 296)                                              # K-aligned, not 64-aligned
