"""Random banks, control actions and block lists for the fuzz tiers (test_oracle_fuzz.py, test_mod_fuzz.py, the fuzz_mod_*
fixtures of golden/gen_golden.py).  numpy only: nothing here renders, predicts or checks anything.

Everything is drawn from the numpy Generator that is passed in, so a seed names one bank, one action list and one block list.
"""
import numpy as np

from skred_amd import banks
from skred_amd.bank import VoiceBank

# SKRED_DIRTY_* / SKRED_STAMP_* of include/skred_amd.h (skred_amd.device loads the HIP library, which this module must not need)
DIRTY_PARAMS, DIRTY_PHASE, STAMP_TRIGGER, STAMP_RELEASE = 1, 2, 256, 512

COUNT0 = 50000                      # synth_sample_count the banks are drawn for (envelope clocks lie just before it)
MOD_FIELDS = (("voice_freq_mod_osc", "voice_freq_mod_depth", 0.2), ("voice_amp_mod_osc", "voice_amp_mod_depth", 0.2),
              ("voice_pan_mod_osc", "voice_pan_mod_depth", 0.15), ("voice_cz_mod_osc", "voice_cz_mod_depth", 0.3))
MAX_TIERS = 8                       # cross-group chains: at most this many groups deep (the library allows 16 pre-pass levels)
SPARSE_LIVE = 8                     # sparse banks: at most this many voices of a 64-voice group can sound ...
SPARSE_PALETTE = 4                  # ... and at most this many of its voices serve other groups as modulators


def catalogue(bank):
    """The (offset, size) pairs of the tables a fixture's voices sit on, sorted."""
    return sorted({(int(o), int(s)) for o, s in zip(bank["voice_table_offset"], bank["voice_table_size"]) if s > 0})


class Tiers:
    """Cross-group routing plan.  `tier`: a random order of the 64-voice groups cut into at most MAX_TIERS bands; a group reads only
    groups of a lower band, so the graph of groups has no cycle and no chain longer than the number of bands.  `palette` (sparse
    banks, else None): the SPARSE_PALETTE lanes of each group that other groups may name."""

    def __init__(self, tier, palette=None):
        self.tier, self.palette = tier, palette


def group_tiers(rng, n):
    G = (n + 63) // 64
    T = int(min(G, rng.integers(4, MAX_TIERS + 1)))
    tier = np.zeros(G, np.int64)
    tier[rng.permutation(G)] = (np.arange(G) * T) // G
    return Tiers(tier)


def cross_sources(rng, voices, tiers, n):
    """For each of `voices` (all in groups of tier > 0) one voice of a group of a lower tier."""
    tier = tiers.tier
    order = np.argsort(tier, kind="stable")                    # groups by tier
    below = np.searchsorted(tier[order], tier[voices >> 6])    # how many groups lie in lower tiers
    g = order[(rng.random(len(voices)) * below).astype(np.int64)]
    u = rng.random(len(voices))
    if tiers.palette is not None:
        return (g * 64 + tiers.palette[g, (u * SPARSE_PALETTE).astype(np.int64)]).astype(np.int32)
    width = np.minimum(64, n - g * 64)                         # the last group may be ragged
    return (g * 64 + (u * width).astype(np.int64)).astype(np.int32)


def wild_bank(rng, n, tables_catalogue, routing, cross_share=0.35, sparse=False):
    """The feature mix of test_gpu_parity.py::test_random_feature_mix_vs_oracle on n voices.  Returns (bank, tiers); tiers is the
    plan of group_tiers() for routing "cross_group", else None.  `sparse`: the same bank with most amps set to 0 -- 1 to SPARSE_LIVE
    voices of every 64-voice group can sound, and the modulators that come from other groups sit on SPARSE_PALETTE lanes of their
    group -- so that every group needs well under 32 lanes of a packed wavefront (SKRED_OPT_PACK), the dead modulators that voices
    that can sound name included.  The dense bank's draws are not touched."""
    assert routing in ("own_group", "cross_group", "any64")
    assert routing != "any64" or n == 64
    cat = tables_catalogue
    b = VoiceBank(n)
    pick = rng.integers(0, len(cat), n)
    off = np.array([cat[i][0] for i in pick]); size = np.array([cat[i][1] for i in pick])
    b["voice_table_offset"], b["voice_table_size"] = off, size.astype(np.int32)
    b["voice_one_shot"] = (rng.random(n) < 0.3).astype(np.int32)
    b["voice_loop_enabled"] = (rng.random(n) < 0.4).astype(np.int32)
    ls = (rng.random(n) * 0.4 * size).astype(np.int32)
    le = (ls + 2 + rng.random(n) * 0.5 * size).astype(np.int32)
    b["voice_loop_start_f"], b["voice_loop_end_f"] = ls.astype(np.float32), np.minimum(le, size).astype(np.float32)
    b["voice_loop_valid"] = (b["voice_loop_end_f"] > b["voice_loop_start_f"]).astype(np.int32)
    b["voice_direction"] = (rng.random(n) < 0.2).astype(np.int32)
    b["voice_phase"] = (rng.random(n) * (size - 1)).astype(np.float32)
    b["voice_phase_inc"] = (rng.random(n) ** 3 * 40.0).astype(np.float32)
    b["voice_amp"] = np.where(rng.random(n) < 0.15, 0.0, rng.random(n) * 2).astype(np.float32)
    pan = (rng.random(n) * 2 - 1).astype(np.float32)
    b["voice_pan_left"], b["voice_pan_right"] = banks.pan_gains(pan)
    b["voice_disconnect"] = (rng.random(n) < 0.15).astype(np.int32)
    b["voice_wave_table_index"] = np.where(rng.random(n) < 0.08, 6, 200).astype(np.int32)
    b["voice_sample_hold_max"] = np.where(rng.random(n) < 0.15, rng.integers(1, 9, n), 0).astype(np.int32)
    b["voice_quantize"] = np.where(rng.random(n) < 0.15, rng.integers(1, 12, n), 0).astype(np.int32)
    b["voice_smoother_enable"] = (rng.random(n) < 0.8).astype(np.int32)
    b["voice_smoother_smoothing"] = (0.001 + rng.random(n) * 0.5).astype(np.float32)
    mode = np.where(rng.random(n) < 0.5, rng.integers(1, 6, n), 0).astype(np.int32)
    co = banks.biquad_coeffs(np.maximum(mode, 1), 100 + rng.random(n) * 8000, 0.5 + rng.random(n) * 3, 44100)
    for k, v in co.items():
        b["voice_filter"][k] = v
    b["voice_filter_mode"] = mode
    e = b["voice_amp_envelope"]
    for name, top in (("attack_time", 300), ("decay_time", 300), ("release_time", 400)):
        e[name] = np.where(rng.random(n) < 0.12, 0.0, rng.random(n) * top).astype(np.float32)     # zero times too
    e["sustain_level"] = rng.random(n).astype(np.float32)
    e["sample_start"] = (COUNT0 - rng.integers(0, 500, n)).astype(np.uint64)
    e["sample_release"] = np.where(rng.random(n) < 0.4, COUNT0 - rng.integers(0, 200, n), 0).astype(np.uint64)
    e["is_active"] = (rng.random(n) < 0.9).astype(np.int32)
    e["velocity"] = (0.2 + rng.random(n)).astype(np.float32)
    b["voice_use_amp_envelope"] = (rng.random(n) < 0.6).astype(np.int32)

    # modulators: the probabilities of that test, thinned per 64-voice group by a random factor -- dense groups need the level
    # loop, thin ones have a single dependency level (the frame-lag form) or none
    v = np.arange(n)
    base = (v >> 6) << 6
    width = np.minimum(64, n - base)
    density = rng.choice([1.0, 0.25, 0.04], (n + 63) // 64)[v >> 6]
    tiers = group_tiers(rng, n) if routing == "cross_group" else None
    for key, depth, p in MOD_FIELDS:
        src = np.where(rng.random(n) < p * density, base + (rng.random(n) * width).astype(np.int64), -1).astype(np.int32)
        if tiers is not None:
            far = np.where((rng.random(n) < p * cross_share) & (tiers.tier[v >> 6] > 0))[0]
            src[far] = cross_sources(rng, far, tiers, n)
        b[key] = src
        b[depth] = (rng.random(n) * 2).astype(np.float32)
    b["voice_freq_scale"] = (0.5 + rng.random(n)).astype(np.float32)
    b["voice_cz_mode"] = np.where(rng.random(n) < 0.3, rng.integers(1, 8, n), 0).astype(np.int32)
    b["voice_cz_distortion"] = rng.random(n).astype(np.float32)
    if sparse:
        G = (n + 63) // 64
        key = rng.random(n) + (v >> 6)                             # a random order of the voices inside every group
        rank = np.empty(n, np.int64)
        rank[np.argsort(key)] = v
        keep = rng.integers(1, SPARSE_LIVE + 1, G)
        b["voice_amp"] = np.where(rank - base < keep[v >> 6], b["voice_amp"], 0.0).astype(np.float32)
        if tiers is not None:
            gw = np.minimum(64, n - np.arange(G) * 64)
            tiers.palette = (rng.random((G, SPARSE_PALETTE)) * gw[:, None]).astype(np.int64)
            for key_, _, _ in MOD_FIELDS:
                m = np.asarray(b[key_]).astype(np.int64)
                far = (m >= 0) & ((m >> 6) != (v >> 6))
                m[far] = (m[far] >> 6) * 64 + tiers.palette[m[far] >> 6, (m[far] & 63) % SPARSE_PALETTE]
                b[key_] = m.astype(np.int32)
    return b, tiers


class Action:
    """One control action.  apply(host, now) changes the host bank as the control path would at synth_sample_count `now` and
    returns (voices, dirty): what skred_bank_update / skred_bank_defer has to be told (the STAMP actions are written out on the
    host here; the library stamps them itself)."""

    def __init__(self, kind, voices, fn):
        self.kind, self.voices, self.fn = kind, np.asarray(voices, np.int32), fn

    def apply(self, host, now):
        return self.fn(host, self.voices, np.uint64(now))

    def __repr__(self):
        return f"Action({self.kind}, {len(self.voices)} voices)"


def _some(rng, n, share, most=4096):
    k = int(max(1, min(most, round(n * share))))
    return np.sort(rng.choice(n, k, replace=False)).astype(np.int32)


def events(rng, host, count, tiers=None):
    """`count` control actions for a bank shaped like `host` (its size and, with `tiers`, its cross-group plan): amp to 0 and back,
    note-off, re-trigger of finished one-shots, a modulator re-pointed (inside the group, to a lower tier's group, to -1), depth and
    phase_inc changes, CZ mode on / off.  Every kind appears once before any repeats; the order is random."""
    n = host.n

    def mute_pair():
        vs, saved = _some(rng, n, 0.1), {}

        def mute(h, vs, now):
            saved["amp"] = h["voice_amp"][vs].copy()
            h["voice_amp"][vs] = 0.0
            return vs, DIRTY_PARAMS

        def unmute(h, vs, now):
            h["voice_amp"][vs] = saved["amp"]
            return vs, DIRTY_PARAMS

        return Action("mute", vs, mute), Action("unmute", vs, unmute)

    def note_off(h, vs, now):                                   # amp_envelope_release, synth.c:391-395
        e = h["voice_amp_envelope"]
        act = e["is_active"][vs] != 0
        e["sample_release"][vs[act]] = now
        return vs, STAMP_RELEASE

    def retrigger(h, vs, now):                                  # osc_trigger + amp_envelope_trigger on what has finished
        vs = vs[h["voice_finished"][vs] != 0]
        h["voice_finished"][vs] = 0
        h["voice_phase"][vs] = np.where(h["voice_loop_enabled"][vs] != 0, h["voice_loop_start_f"][vs], np.float32(0.0))
        e = h["voice_amp_envelope"]
        e["sample_start"][vs] = now
        e["sample_release"][vs] = 0
        e["is_active"][vs] = 1
        return vs, DIRTY_PHASE | STAMP_TRIGGER

    def repoint(field, new):
        def fn(h, vs, now):
            h[field][vs] = new
            return vs, DIRTY_PARAMS
        return fn

    def retune(field, new):
        def fn(h, vs, now):
            h[field][vs] = new
            return vs, DIRTY_PARAMS
        return fn

    def make(kind):
        field = MOD_FIELDS[int(rng.integers(0, 4))]
        if kind == "note_off":
            return Action(kind, _some(rng, n, 0.3), note_off)
        if kind == "retrigger":
            return Action(kind, _some(rng, n, 0.5, most=n), retrigger)
        if kind == "repoint_own":
            vs = _some(rng, n, 0.08)
            base = (vs >> 6) << 6
            new = base + (rng.random(len(vs)) * np.minimum(64, n - base)).astype(np.int64)
            return Action(kind, vs, repoint(field[0], new.astype(np.int32)))
        if kind == "repoint_far":
            if tiers is None:
                return make("repoint_own")
            vs = _some(rng, n, 0.08)
            vs = vs[tiers.tier[vs >> 6] > 0]
            return Action(kind, vs, repoint(field[0], cross_sources(rng, vs, tiers, n)))
        if kind == "unplug":
            return Action(kind, _some(rng, n, 0.08), repoint(field[0], np.int32(-1)))
        if kind == "depth":
            vs = _some(rng, n, 0.1)
            return Action(kind, vs, retune(field[1], (rng.random(len(vs)) * 2).astype(np.float32)))
        if kind == "phase_inc":
            vs = _some(rng, n, 0.1)
            return Action(kind, vs, retune("voice_phase_inc", (rng.random(len(vs)) ** 3 * 40.0).astype(np.float32)))
        if kind == "cz_on":
            vs = _some(rng, n, 0.1)
            return Action(kind, vs, retune("voice_cz_mode", rng.integers(1, 8, len(vs)).astype(np.int32)))
        if kind == "cz_off":
            return Action(kind, _some(rng, n, 0.1), retune("voice_cz_mode", np.int32(0)))
        raise ValueError(kind)

    kinds = ["mute", "note_off", "retrigger", "repoint_own", "repoint_far", "unplug", "depth", "phase_inc", "cz_on", "cz_off"]
    out, undo = [], []
    while len(out) < count:
        for kind in rng.permutation(kinds):
            if kind == "mute":
                m, u = mute_pair()
                out.append(m)
                undo.append((m, u))
            else:
                out.append(make(str(kind)))
    for m, u in undo:                                           # the amp comes back at a random later place
        i = [k for k, a in enumerate(out) if a is m][0]
        out.insert(int(rng.integers(i + 1, len(out) + 1)), u)
    return out[:count]


def block_lengths(rng):
    """Block lengths around the 64-frame edge, the shortest two, and one above 512, in random order."""
    return [int(x) for x in rng.permutation([1, 2, 63, 64, 65, int(rng.integers(513, 700))])]


def spread(rng, actions, n_blocks):
    """Deal `actions`, in order, to the gaps before blocks 1 .. n_blocks-1: a list of n_blocks lists (block 0 gets none)."""
    slots = np.sort(rng.integers(1, n_blocks, len(actions)))
    out = [[] for _ in range(n_blocks)]
    for s, a in zip(slots, actions):
        out[int(s)].append(a)
    return out
