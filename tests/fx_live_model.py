"""Numpy statement of the fixed-point bank's live control (include/skred_amd_fxpt.h), for tests/test_fx_live*.py:

  apply_update   what skred_fxbank_update stores, per dirty bit, on an FxVoiceBank
  idle_mask / idle_list   the idle predicate and the rotated listing of skred_fxbank_find_idle
  place_notes    which voice note k lands on (entry first_entry + k, the drop rules) and what a placed note stores
"""
import numpy as np

from skred_amd import fxbank as fxb

PARAM_FIELDS = ["phase_inc", "table_offset", "log2_size", "amp_q15", "disconnect", "use_envelope", "smoother_enable", "one_shot",
                "filter_mode", "attack_frames", "decay_frames", "release_frames", "sustain_q15", "b0_q30", "b1_q30", "b2_q30",
                "a1_q30", "a2_q30", "smoother_k_q15", "velocity_q15"]
FIELDS_OF = {
    fxb.DIRTY_PARAMS: PARAM_FIELDS,
    fxb.DIRTY_PAN: ["pan_left_q15", "pan_right_q15"],
    fxb.DIRTY_PHASE: ["phase", "finished"],
    fxb.DIRTY_ENV_STATE: ["is_active"],
    fxb.DIRTY_FILTER_STATE: ["x1", "x2", "y1", "y2"],
    fxb.DIRTY_SMOOTHER: ["smoother_gain_q15"],
    fxb.DIRTY_SAMPLE: ["voice_sample"],
    fxb.DIRTY_ENV_CLOCK: ["sample_start", "sample_release"],
}
BOOLS = ("finished", "is_active")                      # one bit on the device: any non-zero host value reads back as 1
ALL_VALUE_BITS = sum(FIELDS_OF)


def stamp(bank, voices, stamps, now):
    """sk_fx_stamp_kernel's stores: the trigger first, then the release if the envelope is (now) active."""
    for v in np.asarray(voices).reshape(-1):
        if stamps & fxb.STAMP_TRIGGER:
            bank["sample_start"][v] = now
            bank["sample_release"][v] = 0
            bank["is_active"][v] = 1
        if (stamps & fxb.STAMP_RELEASE) and bank["is_active"][v]:
            bank["sample_release"][v] = now


def apply_update(bank, host, voices, dirty, now):
    """`bank` (the device's state, as the oracle holds it) after skred_fxbank_update(host, voices, dirty) at clock `now`.
    The listed voices are taken in order; everything not named is left alone."""
    assert dirty and not dirty & ~0x7FF and not dirty & fxb.DIRTY_HOLD
    for v in np.asarray(voices).reshape(-1):
        for bit, names in FIELDS_OF.items():
            if dirty & bit:
                for name in names:
                    x = host[name][v]
                    bank[name][v] = (1 if x else 0) if name in BOOLS else x
        stamp(bank, [v], dirty, now)


def idle_mask(bank, which, settle_q15=0):
    """The predicate of every voice (bool array); every comparison exact."""
    idle = np.zeros(bank.n, bool)
    if which & fxb.IDLE_FINISHED:
        idle |= bank["finished"] != 0
    if which & fxb.IDLE_ENV_DONE:
        settled = (bank["smoother_enable"] == 0) | (np.abs(bank["smoother_gain_q15"].astype(np.int64)) <= settle_q15)
        idle |= (bank["use_envelope"] != 0) & (bank["is_active"] == 0) & settled
    if which & fxb.IDLE_AMP_ZERO:
        idle |= bank["amp_q15"] == 0
    return idle


def idle_list(bank, first, count, which, settle_q15=0, start=None, max_out=None):
    """(listed voices int32, total): ascending from `start`, wrapping to `first`; written = min(total, max_out)."""
    start = first if start is None else start
    assert first <= start < first + count
    m = idle_mask(bank, which, settle_q15)
    order = np.concatenate([np.arange(start, first + count), np.arange(first, start)])
    hit = order[m[order]].astype(np.int32)
    max_out = count if max_out is None else max_out
    return hit[:max_out], int(hit.size)


def place_notes(bank, notes, listed, count0, first_entry, now):
    """Note k takes entry first_entry + k of `listed` when that entry lies below count0 and names a voice of the bank; the stores of a
    placed note go into `bank`.  Returns (assigned int32[n] with -1 holes, (placed, dropped))."""
    assigned = np.full(len(notes), -1, np.int32)
    for k, t in enumerate(notes):
        at = first_entry + k
        if at >= count0:
            continue
        v = int(listed[at])
        if v < 0 or v >= bank.n:
            continue
        assigned[k] = v
        bank["phase_inc"][v] = t.phase_inc
        bank["velocity_q15"][v] = t.velocity_q15
        if t.flags & fxb.NOTE_SET_PHASE:
            bank["phase"][v] = t.phase
            bank["finished"][v] = 0
        if t.flags & fxb.NOTE_SET_PAN:
            bank["pan_left_q15"][v] = t.pan_left_q15
            bank["pan_right_q15"][v] = t.pan_right_q15
        stamp(bank, [v], fxb.STAMP_TRIGGER, now)
    placed = int((assigned >= 0).sum())
    return assigned, (placed, len(notes) - placed)
