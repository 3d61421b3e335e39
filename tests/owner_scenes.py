"""The theft scene of the note-owner tests (tests/test_owner.py runs it on the device, tests/test_owner_cpu.py asserts on the oracle's
state that it really steals): 3.sk tiled over 256 voices, 64 slots of K = 4, envelopes on voices 0 .. 2 of every copy.

  t0   eight slots are at rest, the other 56 sound.  Chord A (8 notes) goes to the idle slots and is tagged: the bank is full.
  t1   one block later the 56 other slots are played again (a trigger stamp) and tagged: A's slots are now the oldest.
  t2   one block later chord B (6 notes) arrives through note_on_steal_slots, OLDEST: no slot is idle, so it steals the six oldest
       of A's slots, and is tagged from its own d_assigned -- which overwrites A's tags there.
  then A's key is lifted: its note-off names all eight of its slots, six of which hold B's notes by now.

Everything here is the CPU model's; the device is held to it step by step.
"""
import numpy as np

import owner_model as OM
import slot_model as SM
import slot_steal_model as M
from oracle import cpuref
from skred_amd import banks
from skred_amd.bank import slot_query
from steal_model import OLDEST, FIN, ENV

N, K, F = 256, 4, 64
MEMBERS, VOICES = (0, 1, 2), (0, 1, 2, 3)
MMASK, VMASK = 0b0111, 0b1111
WHICH, SETTLE = FIN | ENV, 1e-3
A_SLOTS = np.array([3, 10, 17, 24, 38, 45, 59, 63], np.int32) * K          # at rest at t0 (the last slot of the bank among them)
A_TAGS = np.array([0x80000001 + 7 * k for k in range(8)], np.uint32)        # every one at or above 2^31
B_COUNT = 6
B_TAGS = np.array([0x1000 + k for k in range(B_COUNT)], np.uint32)
C_TAGS_BASE = 0x70000000


def bank(n=N, rest=A_SLOTS):
    """bank_patch("3sk") with every copy sounding since long ago, except the slots `rest`, whose members are at rest."""
    b, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    v = np.arange(n)
    sel = np.isin(v % K, MEMBERS)
    e = b["voice_amp_envelope"]
    b["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel] = np.float32(20.0), np.float32(50.0)
    e["sustain_level"][sel], e["release_time"][sel] = np.float32(0.6), np.float32(200.0)
    e["velocity"][sel] = np.float32(1.0)
    e["is_active"][sel] = 1
    e["sample_start"][sel] = (now - 40000 - ((v[sel] // K) * 37) % 1000).astype(np.uint64)
    e["sample_release"][sel] = np.uint64(0)
    b["voice_smoother_smoothing"][sel] = np.float32(0.5)
    rest = sel & np.isin(v - v % K, rest)
    e["is_active"][rest] = 0
    b["voice_smoother_gain"][rest] = np.float32(0.0)
    return b, tables, g


def notes(count, seed):
    from test_slots import slot_notes
    return slot_notes(count, K, VMASK, seed, [SM.SET_PHASE, SM.SET_PHASE | SM.SET_PAN])


def idle_q():
    return slot_query(0, N, K, MMASK, WHICH, SETTLE, 0, 0)


def steal_q():
    return M.SlotQuery(0, N, K, MMASK, OLDEST, 0, max_out=B_COUNT)


def others():
    return np.setdiff1d(np.arange(0, N, K, dtype=np.int32), A_SLOTS).astype(np.int32)


def c_tags():
    return (C_TAGS_BASE + np.arange(len(others()))).astype(np.uint32)


class Story:
    """The scene on the oracle, one step per method, in the order the device test takes them.  `truth` is the oracle's bank, `owner`
    the model's owner array; every step returns what the device must report."""

    def __init__(self):
        self.bank, self.tables, self.g = bank()
        self.truth, self.gl = self.bank.copy(), self.g.copy()
        self.owner = OM.new(N)

    def now(self):
        return int(self.gl.synth_sample_count)

    def block(self, stems=False):
        return cpuref.render(self.truth, self.gl, self.tables, F, 0, want_stems=stems)

    def chord_a(self):
        idle = SM.idle_slots(self.truth, 0, N, K, MMASK, WHICH, SETTLE)
        self.a_notes = notes(len(A_SLOTS), 1)
        self.a_assigned = SM.place(len(A_SLOTS), K, idle, len(idle), 0, N)
        SM.store_notes((self.truth,), self.truth, self.a_notes, K, VMASK, self.a_assigned, self.now())
        return self.a_assigned, OM.tag_slots(self.owner, self.a_assigned, A_TAGS, None, K)

    def fill_up(self):
        SM.stamp(self.truth, SM.stamp_voices(others(), len(others()), None, K, MMASK, N), SM.STAMP_TRIGGER, self.now())
        return OM.tag_slots(self.owner, others(), c_tags(), None, K)

    def chord_b(self):
        """(d_assigned, (placed, dropped, stolen)) of the burst, as the two placement models give it."""
        now, iq, sq = self.now(), idle_q(), steal_q()
        idle = SM.idle_slots(self.truth, 0, N, K, MMASK, WHICH, SETTLE)[:B_COUNT]
        victims = M.victim_slots(self.truth, now, sq.but(exclude_idle=WHICH, settle_level=SETTLE, max_out=B_COUNT))[:B_COUNT]
        joined = np.concatenate([idle, victims]).astype(np.int32)[:B_COUNT]
        self.b_assigned = np.full(B_COUNT, -1, np.int32)
        self.b_assigned[:len(joined)] = joined
        counts = (len(joined), B_COUNT - len(joined), len(joined) - len(idle))
        self.b_notes = notes(B_COUNT, 2)
        SM.store_notes((self.truth,), self.truth, self.b_notes, K, VMASK, self.b_assigned, now)
        return self.b_assigned, counts, OM.tag_slots(self.owner, self.b_assigned, B_TAGS, None, K)

    def a_off(self):
        return OM.stamp_owned(self.owner, self.truth, self.a_assigned, A_TAGS, None, K, VMASK, SM.STAMP_RELEASE, self.now())

    def b_off(self):
        return OM.release_tags(self.owner, self.truth, 0, N, K, VMASK, B_TAGS, SM.STAMP_RELEASE, self.now())
