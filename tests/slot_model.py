"""Patch notes, stated in numpy on a host view (VoiceBank) as oracle.cpuref leaves it: which slots are idle, which slot a patch note
takes, and the fields a note or a stamp stores.  Written from the definition in include/skred_amd.h (section "patch notes"), not from
the kernels: a slot is K consecutive voices from a multiple of K, named by its first voice; it is idle when every voice with a bit
in member_mask satisfies the per-voice predicate; voices without a bit never decide anything.
"""
import numpy as np

FIN, ENV, AMP, UNNAMED = 1, 2, 4, 256
STAMP_TRIGGER, STAMP_RELEASE = 256, 512
SET_PHASE, SET_PAN = 1, 2


def voice_idle(host, which, settle=0.0):
    """The per-voice predicate of skred_bank_find_idle for every voice of the bank (any selected criterion holds)."""
    a = host.a
    e = a["voice_amp_envelope"]
    idle = np.zeros(host.n, bool)
    if which & FIN:
        idle |= a["voice_finished"] != 0
    if which & ENV:
        settled = (a["voice_smoother_enable"] == 0) | (np.abs(a["voice_smoother_gain"]) <= np.float32(settle))
        idle |= (a["voice_use_amp_envelope"] != 0) & (e["is_active"] == 0) & settled
    if which & AMP:
        idle |= a["voice_amp"] == 0
    return idle


def lanes(mask, K):
    return [l for l in range(K) if (mask >> l) & 1]


def slot_idle(host, first, count, K, member_mask, which, settle=0.0):
    """(first voices of the range's slots, idle flag per slot)."""
    idle = voice_idle(host, which, settle)
    heads = np.arange(first, first + count, K)
    ok = np.ones(len(heads), bool)
    for l in lanes(member_mask, K):
        ok &= idle[heads + l]
    return heads, ok


def idle_slots(host, first, count, K, member_mask, which, settle=0.0, start=None):
    """The listing: first voices of the idle slots, ascending from `start` (default `first`), wrapping to `first`."""
    heads, ok = slot_idle(host, first, count, K, member_mask, which, settle)
    lst = heads[ok]
    k = int(np.searchsorted(lst, first if start is None else start))
    return np.concatenate([lst[k:], lst[:k]]).astype(np.int32)


def place(n, K, entries, listed, first_entry, n_voices):
    """d_assigned of n patch notes on a list: entry first_entry + k when it exists and is a slot of the bank, else -1."""
    out = np.full(n, -1, np.int32)
    for k in range(n):
        at = first_entry + k
        if at < listed:
            e = int(entries[at])
            if e >= 0 and e % K == 0 and e + K <= n_voices:
                out[k] = e
    return out


def store_notes(hosts, truth, notes, K, voice_mask, assigned, now):
    """What the placement stores: record k * K + l onto voice assigned[k] + l for every masked l.  `hosts` get the values (a twin's
    skred_bank_update carries them), `truth` the trigger stamp too.  Returns the voices stored to, in order."""
    touched = []
    for k, e in enumerate(assigned):
        if e < 0:
            continue
        for l in lanes(voice_mask, K):
            t, v = notes[k * K + l], int(e) + l
            touched.append(v)
            for h in hosts:
                h["voice_phase_inc"][v] = t.phase_inc
                h["voice_amp_envelope"]["velocity"][v] = t.velocity
                if t.flags & SET_PHASE:
                    h["voice_phase"][v] = t.phase
                    h["voice_finished"][v] = 0
                if t.flags & SET_PAN:
                    h["voice_pan_left"][v] = t.pan_left
                    h["voice_pan_right"][v] = t.pan_right
            env = truth["voice_amp_envelope"]
            env["sample_start"][v] = now
            env["sample_release"][v] = 0
            env["is_active"][v] = 1
    return np.array(touched, np.int32)


def stamp_voices(entries, n, count, K, voice_mask, n_voices):
    """The voices skred_bank_stamp_slots stamps: the masked voices of the first min(n, count) entries that are slots of the bank."""
    m = n if count is None else min(n, count)
    out = []
    for e in entries[:m]:
        e = int(e)
        if e >= 0 and e % K == 0 and e + K <= n_voices:
            out.extend(e + l for l in lanes(voice_mask, K))
    return np.array(out, np.int32)


def stamp(truth, voices, stamps, now):
    """SKRED_STAMP_TRIGGER and / or SKRED_STAMP_RELEASE on the listed voices of the oracle's bank: a release only counts on an
    envelope that is active (after the trigger, when both are asked for)."""
    e = truth["voice_amp_envelope"]
    for v in voices:
        if stamps & STAMP_TRIGGER:
            e["sample_start"][v], e["sample_release"][v], e["is_active"][v] = now, 0, 1
        if (stamps & STAMP_RELEASE) and e["is_active"][v] != 0:
            e["sample_release"][v] = now
