"""Which form each wavefront of the modulated kernel (skred_render_generic.hip: sk_render_mod_kernel) takes, predicted from the bank:
the host's dependency levels (skred_bank_plan.c: sk_plan_levels) and the kernel's lag vote, for the unpacked layout (one 64-voice group per
wavefront).  The tests compare this with what the kernel counted (skred_bank_set_form_counter)."""
import numpy as np


def group_lanes(bank):
    """The four modulator fields as lanes inside the voice's own 64-voice group, -1 = none (skred_bank_update.c: FM ignores a self
    reference, the CZ source counts only with CZ on)."""
    n = bank.n
    v = np.arange(n)
    fm = np.asarray(bank["voice_freq_mod_osc"]).copy()
    fm[fm == v] = -1
    cz = np.where(np.asarray(bank["voice_cz_mode"]) != 0, np.asarray(bank["voice_cz_mod_osc"]), -1)
    out = []
    for m in (fm, np.asarray(bank["voice_amp_mod_osc"]), np.asarray(bank["voice_pan_mod_osc"]), cz):
        ok = (m >= 0) & ((m >> 6) == (v >> 6))
        out.append(np.where(ok, m & 63, -1))
    return np.stack(out, 1)


def levels(bank):
    """Dependency level of every voice: 0 needs no same-frame value, else 1 + the highest level of its modulators below it."""
    mods = group_lanes(bank)
    lv = np.zeros(bank.n, np.int64)
    for g0 in range(0, bank.n, 64):
        for l in range(min(64, bank.n - g0)):
            for s in mods[g0 + l]:
                if 0 <= s < l:
                    lv[g0 + l] = max(lv[g0 + l], lv[g0 + s] + 1)
    return lv


def lag_groups(bank):
    """Per 64-voice group: True when its wavefront passes the lag vote (one level of same-frame dependencies, every edge a source
    below its reader one level lower or a source above it on the reader's own level, some lane on level 1)."""
    mods, lv = group_lanes(bank), levels(bank)
    res = []
    for g0 in range(0, bank.n, 64):
        ok, any1 = True, False
        for l in range(min(64, bank.n - g0)):                 # (the lanes past a ragged last group are empty: level 0, no edges)
            me = lv[g0 + l]
            any1 |= me == 1
            ok &= me <= 1
            for s in mods[g0 + l]:
                if s >= 0 and s != l:
                    ok &= lv[g0 + s] == (me - 1 if s < l else me)
        res.append(bool(ok and any1))
    return np.array(res)


def expected_counts(bank, frames, skew):
    """[lag waves, level-loop waves] of one unpacked launch of `frames` frames without stems.  The launch covers the bank padded to
    whole passes of 1024 voices (skred_bank.c: n_groups); a wavefront without voices has no lane on level 1, fails the lag vote and
    counts, like every other, as a level-loop wave of a bank that has same-frame dependencies somewhere.  That the second figure
    takes in the voiceless padding waves is how the counter is defined (skred_device_layout.h: form_counts, "+= 1 per wave and
    pass ... the level loop with max_level >= 1", max_level being the launch's), not a property of the bank."""
    if levels(bank).max() < 1:
        return [0, 0]
    waves = -(-bank.n // 1024) * 16
    lag = lag_groups(bank) if (skew and frames >= 2) else np.zeros(1, bool)
    return [int(lag.sum()), waves - int(lag.sum())]


# ---- packed lanes (SKRED_OPT_PACK; skred_bank.c: sk_pack_refresh, skred_device_layout.h: pack_mask) ----

def far_sources(bank):
    """The distinct modulators that sit outside their reader's 64-voice group: the sources of the tape (SKRED_OPT_CROSS_GROUP)."""
    v = np.arange(bank.n)
    fm = np.asarray(bank["voice_freq_mod_osc"]).copy()
    fm[fm == v] = -1
    cz = np.where(np.asarray(bank["voice_cz_mode"]) != 0, np.asarray(bank["voice_cz_mod_osc"]), -1)
    out = set()
    for m in (fm, np.asarray(bank["voice_amp_mod_osc"]), np.asarray(bank["voice_pan_mod_osc"]), cz):
        out |= set(int(x) for x in m[(m >= 0) & ((m >> 6) != (v >> 6))])
    return out


def usable(bank):
    return (np.asarray(bank["voice_table_size"]) > 0) | (np.asarray(bank["voice_wave_table_index"]) == 6)


def pack_words(bank, sources=()):
    """[groups of the padded bank][64] bool: the voices that keep a lane in a packed launch -- those that can sound by their
    parameters (a table and voice_amp != 0), the voices of their group those name as modulators, and the tape's `sources`."""
    n = bank.n
    v = np.arange(n)
    has = np.zeros(-(-n // 1024) * 1024, bool)
    live = usable(bank) & (np.asarray(bank["voice_amp"]) != 0)
    has[:n] = live
    mods = group_lanes(bank)
    for k in range(4):
        sel = live & (mods[:, k] >= 0)
        has[((v[sel] >> 6) << 6) + mods[sel, k]] = True
    has[sorted(sources)] = True
    return has.reshape(-1, 64)


def pack_lanes(bank, sources=()):
    """Lanes per 64-voice group of a launch with SKRED_OPT_PACK 2 and no stems (skred_bank_last_pack): the most lanes any group
    needs, rounded up to a power of two; 0 (not packed) when that is 64.  (A bank below 3 x 256 voices per CU is meant: above, the
    library also packs on its own.)"""
    most = int(pack_words(bank, sources).sum(1).max())
    s = 1
    while s < most:
        s *= 2
    return 0 if s >= 64 else s


def expected_packed_counts(bank, frames, skew, sources=()):
    """[lag waves, level-loop waves] of one PACKED launch without stems.  A wavefront holds 64 / pack_lanes() groups; a workgroup
    pass is four of them, and the last pass may hold wavefronts without voices.  The vote is the unpacked one over the lanes that
    are there, but a lane that is dead as the launch starts (no table, voice_amp == 0, voice_finished) keeps its level and has no
    edges (sk_render_mod_kernel: dead0)."""
    S = pack_lanes(bank, sources)
    assert S, "the launch is not packed"
    lv = levels(bank)
    if lv.max() < 1:
        return [0, 0]
    words = pack_words(bank, sources)
    per_wave = 64 // S
    waves = -(-len(words) // (4 * per_wave)) * 4
    if not (skew and frames >= 2):
        return [0, waves]
    mods = group_lanes(bank)
    dead = ~usable(bank) | (np.asarray(bank["voice_amp"]) == 0) | (np.asarray(bank["voice_finished"]) != 0)
    lag = 0
    for w in range(waves):
        ok, any1 = True, False
        for g in range(w * per_wave, min((w + 1) * per_wave, len(words))):
            for l in np.flatnonzero(words[g]):
                me = lv[g * 64 + l]
                any1 |= me == 1
                ok &= me <= 1
                if not dead[g * 64 + l]:
                    for s in mods[g * 64 + l]:
                        if s >= 0 and s != l:
                            ok &= lv[g * 64 + s] == (me - 1 if s < l else me)
        lag += bool(ok and any1)
    return [lag, waves - lag]
