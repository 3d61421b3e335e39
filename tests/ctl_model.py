"""Patch controllers, stated in numpy on a host view (VoiceBank): the words skred_bank_ctl_range / skred_bank_ctl_slots store, the two
device-side guards, the skip rules of the list and the two result counts.  Written from the definition in include/skred_amd.h
(section "patch controllers"), not from the kernels.  The view must hold voice_phase_inc and voice_amp AS THE DEVICE HOLDS THEM (the
two guards read them): the uploaded view with every later store mirrored, or a DeviceBank.download_ctl.

The one piece of arithmetic is INC_SCALE: np.float32 * np.float32 is one IEEE fp32 multiply, round to nearest even, subnormals kept --
what the device computes with -ffp-contract=off and without a denormal flush (skred_amd/csrc/Makefile).
"""
import numpy as np

PHASE_INC, INC_SCALE, AMP, PAN, FILTER, ENV_TIMES, VELOCITY, SMOOTHING = (1 << i for i in range(8))
FM_DEPTH, FREQ_SCALE, AM_DEPTH, PAN_DEPTH, CZ_DEPTH, CZ_DIST = (1 << i for i in range(8, 14))
ALL = (1 << 14) - 1
BITS = [1 << i for i in range(14)]
LISTS = AMP | ENV_TIMES | VELOCITY | SMOOTHING            # the voice goes on the motion list

# bit -> ((field of the view, sub-field or None, attribute of the record), ...): absolute stores
STORES = {
    PHASE_INC: (("voice_phase_inc", None, "phase_inc"),),
    PAN: (("voice_pan_left", None, "pan_left"), ("voice_pan_right", None, "pan_right")),
    FILTER: tuple(("voice_filter", k, k) for k in ("b0", "b1", "b2", "a1", "a2")),
    ENV_TIMES: tuple(("voice_amp_envelope", k, k) for k in ("attack_time", "decay_time", "sustain_level", "release_time")),
    VELOCITY: (("voice_amp_envelope", "velocity", "velocity"),),
    SMOOTHING: (("voice_smoother_smoothing", None, "smoothing"),),
    FM_DEPTH: (("voice_freq_mod_depth", None, "fm_depth"),),
    FREQ_SCALE: (("voice_freq_scale", None, "freq_scale"),),
    AM_DEPTH: (("voice_amp_mod_depth", None, "am_depth"),),
    PAN_DEPTH: (("voice_pan_mod_depth", None, "pan_depth"),),
    CZ_DEPTH: (("voice_cz_mod_depth", None, "cz_depth"),),
    CZ_DIST: (("voice_cz_distortion", None, "cz_dist"),),
}
# every word a controller can store: (field, sub-field) -- what DeviceBank.download_ctl returns
CTL_WORDS = sorted({(f, s) for st in STORES.values() for f, s, _ in st} | {("voice_phase_inc", None), ("voice_amp", None)},
                   key=lambda t: (t[0], t[1] or ""))


def lanes(mask, K):
    return [l for l in range(K) if (mask >> l) & 1]


def word(view, field, sub):
    a = view[field]
    return a if sub is None else a[sub]


def store_voice(view, v, rec):
    """Record `rec` on voice v of `view`.  Returns the stores the guards withheld (0, 1 or 2)."""
    withheld = 0
    s = rec.set
    for bit, stores in STORES.items():
        if s & bit:
            for field, sub, attr in stores:
                word(view, field, sub)[v] = np.float32(getattr(rec, attr))
    if s & INC_SCALE:
        with np.errstate(over="ignore", invalid="ignore"):
            prod = np.float32(view["voice_phase_inc"][v]) * np.float32(rec.inc_scale)
        if np.isfinite(prod):
            view["voice_phase_inc"][v] = prod
        else:
            withheld += 1
    if s & AMP:
        if view["voice_amp"][v] != 0:                       # (-0.0 is 0: the voice cannot sound and stays so)
            view["voice_amp"][v] = np.float32(rec.amp)
        else:
            withheld += 1
    return withheld


def slot_valid(e, K, n_voices):
    return e >= 0 and e % K == 0 and e + K <= n_voices


def range_voices(first, count, K, voice_mask):
    """The voices skred_bank_ctl_range writes, with the record each receives: (voice, l), ascending."""
    ls = lanes(voice_mask, K)
    return [(s + l, l) for s in range(first, first + count, K) for l in ls]


def slots_voices(entries, n, count, K, voice_mask, n_voices):
    """The same for skred_bank_ctl_slots: the masked voices of the first min(n, count) entries (count None: n) that are slots of the
    bank, in list order -- a slot named twice appears twice."""
    m = n if count is None else min(n, count)
    ls = lanes(voice_mask, K)
    out = []
    for e in entries[:m]:
        e = int(e)
        if slot_valid(e, K, n_voices):
            out.extend((e + l, l) for l in ls)
    return out


def apply(views, ctls, voices):
    """The stores on every view of `views` (each with the device's increments and amps).  Returns (d_result = [voices written, stores
    withheld], the distinct voices written in ascending order)."""
    written = withheld = 0
    for i, view in enumerate(views):
        w = h = 0
        for v, l in voices:
            h += store_voice(view, v, ctls[l])
            w += 1
        if i == 0:
            written, withheld = w, h
        else:
            assert (w, h) == (written, withheld), "the views disagree about the guards: one of them is stale"
    return [written, withheld], np.unique(np.array([v for v, _ in voices], np.int64)).astype(np.int32)


def ctl_range(views, ctls, first, count, voice_mask):
    return apply(views, ctls, range_voices(first, count, len(ctls), voice_mask))


def ctl_slots(views, ctls, voice_mask, entries, n, count, n_voices):
    return apply(views, ctls, slots_voices(entries, n, count, len(ctls), voice_mask, n_voices))


def listed(ctls, voice_mask):
    """Bit l: voice l of a slot goes on the motion list."""
    return sum(1 << l for l in lanes(voice_mask, len(ctls)) if ctls[l].set & LISTS)


def words_differ(a, b):
    """{field[.sub]: voices whose bits differ} over every word a controller can store."""
    bad = {}
    for field, sub in CTL_WORDS:
        x, y = word(a, field, sub), word(b, field, sub)
        m = int((x.view("<u4") != y.view("<u4")).sum())
        if m:
            bad[field + ("." + sub if sub else "")] = m
    return bad
