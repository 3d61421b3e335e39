"""Which form each wavefront of the modulated kernel (skred_render_generic.hip: sk_render_mod_kernel) takes, predicted from the bank:
the host's dependency levels (skred_bank.c: classify) and the kernel's lag vote, for the unpacked layout (one 64-voice group per
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
        for l in range(64):
            me = lv[g0 + l]
            any1 |= me == 1
            ok &= me <= 1
            for s in mods[g0 + l]:
                if s >= 0 and s != l:
                    ok &= lv[g0 + s] == (me - 1 if s < l else me)
        res.append(bool(ok and any1))
    return np.array(res)


def expected_counts(bank, frames, skew):
    """[lag waves, level-loop waves] of one unpacked launch of `frames` frames without stems."""
    if levels(bank).max() < 1:
        return [0, 0]
    lag = lag_groups(bank) if (skew and frames >= 2) else np.zeros(bank.n // 64, bool)
    return [int(lag.sum()), int((~lag).sum())]
