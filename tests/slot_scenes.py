"""The scenes of the patch-note tests (tests/test_slots_cpu.py asserts on the oracle's state that they are not vacuous,
tests/test_slots.py runs them on the device): small banks of the C2 recipe, cut into slots of K voices, every slot of a KIND --

  0 free        every voice at rest;
  1 one short   every member voice (a bit in member_mask) at rest but ONE, which sounds: only that voice keeps the slot off the list;
  2 shadowed    every member at rest, every voice outside the mask sounding: listed all the same;
  3 busy        several members sounding.

A voice at rest is one of: released so that the release ends inside the blocks the scene renders, with a fast smoother (gain far
below SETTLE afterwards) or without a smoother; a finished voice; an envelope that was never started (gain exactly 0); and, for
queries with AMP_ZERO, a voice without an envelope whose voice_amp is 0.  A sounding voice is one of: sustaining; still in its
release; released with a slow smoother (gain above SETTLE when the query runs); no envelope at all (ENV_DONE must not list it).
"""
import functools

import numpy as np

from oracle import cpuref
from skred_amd import banks
from slot_model import AMP, ENV, FIN, lanes, slot_idle, voice_idle

FRAMES = (65, 130)          # the blocks every scene renders before it is queried
SETTLE = np.float32(1e-3)
WHICH_ALL, WHICH_NOTES = FIN | ENV | AMP, FIN | ENV

REST = (0, 1, 2, 4, 3)      # the last one only with AMP_ZERO
SOUND = (10, 11, 12, 13)


def masks(K):
    """name -> mask: all K bits, the lowest bit, the highest bit, every other bit (duplicates dropped)."""
    full = (1 << K) - 1
    out, seen = {}, set()
    for name, m in (("all", full), ("low", 1), ("high", 1 << (K - 1)), ("alt", 0x5555555555555555 & full)):
        if m not in seen:
            seen.add(m)
            out[name] = m
    return out


def build(n, K, member_mask, with_amp=True, seed=0):
    """(bank, tables, globals, kind per slot) before any block."""
    bank, tables, g = banks.bank_c2(n)
    now = int(g.synth_sample_count)
    e = bank["voice_amp_envelope"]
    e["attack_time"], e["decay_time"] = np.float32(20.0), np.float32(50.0)     # (a release only counts once attack and decay are over)
    e["release_time"] = np.float32(200.0)
    e["sample_start"] = np.uint64(now - 40000)                                  # every sounding voice is in its sustain stage
    rng = np.random.default_rng(7000 + 13 * n + K + 1000 * seed + (member_mask % 9973))
    slots = n // K
    kind = rng.choice(4, slots, p=[0.3, 0.25, 0.2, 0.25])
    kind[:min(4, slots)] = np.arange(min(4, slots))
    if slots >= 8:
        kind[slots - 4:] = np.arange(4)
    mem = lanes(member_mask, K)
    rest = REST if with_amp else REST[:4]
    role = np.zeros(n, np.int64)
    for s in range(slots):
        r = rng.choice(rest, K) if kind[s] in (0, 1, 2) else rng.choice(rest + SOUND, K)
        if kind[s] == 1:
            r[rng.choice(mem)] = rng.choice(SOUND)
        elif kind[s] == 2:
            for l in range(K):
                if l not in mem:
                    r[l] = rng.choice(SOUND)
        elif kind[s] == 3:
            for l in rng.choice(mem, min(2, len(mem)), replace=False):
                r[l] = rng.choice(SOUND)
        role[s * K:(s + 1) * K] = r
    role[slots * K:] = 10
    v = np.arange(n)
    rel = (role == 0) | (role == 4) | (role == 12)
    e["sample_release"][rel] = np.uint64(now - 10)
    e["release_time"][rel] = (10 + 20 + (v[rel] % 150)).astype(np.float32)
    bank["voice_smoother_gain"][rel] = np.float32(0.7)
    bank["voice_smoother_smoothing"][role == 0] = np.float32(0.5)
    bank["voice_smoother_smoothing"][role == 12] = np.float32(0.002)
    bank["voice_smoother_enable"][role == 4] = 0
    bank["voice_finished"][role == 1] = 1
    e["is_active"][role == 2] = 0
    bank["voice_use_amp_envelope"][role == 3] = 0
    bank["voice_amp"][role == 3] = 0.0
    e["sample_release"][role == 11] = np.uint64(now - 10)
    e["release_time"][role == 11] = np.float32(1e6)
    bank["voice_use_amp_envelope"][role == 13] = 0
    e["is_active"][role == 13] = 0
    return bank, tables, g, kind


@functools.lru_cache(maxsize=64)
def scene(n, K, member_mask, with_amp=True, seed=0):
    """(bank, tables, globals, the oracle's bank after FRAMES, the oracle's globals there)."""
    bank, tables, g, _ = build(n, K, member_mask, with_amp, seed)
    truth, gl = bank.copy(), g.copy()
    for f in FRAMES:
        cpuref.render(truth, gl, tables, f, 0)
    return bank, tables, g, truth, gl


def conditions(truth, first, count, K, member_mask, which, settle=SETTLE):
    """(a slot is listed, a slot is kept off the list by exactly one member, a listed slot's voices outside the mask all sound --
    with all K bits in the mask there are none, and any listed slot qualifies)."""
    heads, ok = slot_idle(truth, first, count, K, member_mask, which, settle)
    idle = voice_idle(truth, which, settle)
    mem = np.array(lanes(member_mask, K))
    non = np.array([l for l in range(K) if not (member_mask >> l) & 1], np.int64)
    busy_members = np.array([int((~idle[h + mem]).sum()) for h in heads])
    shadowed = np.array([bool(ok[i]) and bool((~idle[h + non]).all()) for i, h in enumerate(heads)])
    return bool(ok.any()), bool((busy_members == 1).any()), bool(shadowed.any())


# (n voices, K, which mask): 64 voices = one wave, 320 = a ragged last workgroup, 1088 = five workgroups (offsets and the rank of
# `from` cross workgroup edges); a bank needs at least five slots to hold every kind
QUERY_CASES = [(n, K, name) for n in (64, 320, 1088) for K in (1, 2, 8, 64) if n // K >= 5 for name in masks(K)]
# 17 workgroups, one case (the last arriver's scan gives every workgroup's count a thread of its own up to 256 workgroups --
# 65 536 voices --, a boundary tests/test_idle.py crosses on the code both lists share)
BIG_CASE = (4160, 8, "alt")
