"""The channel scene of the expression tests (tests/test_expr.py runs it on the device, tests/test_expr_cpu.py on the oracle's state
alone): tests/owner_scenes.py's theft on 3.sk over 256 voices -- 64 slots of K = 4, the smallest bank that fills -- with tags that
carry a CHANNEL in their top byte, tag = channel << 24 | note id.

  chord A (8 notes, channel 0x0A) takes the idle slots; the 56 other slots are played again on channel 0x0C; chord B (6 notes, channel
  0x0B) finds the bank full and steals the six oldest of A's slots.  Then, all by channel or by note id and never by slot index:
  stamp_match(A) releases A's two survivors and none of B; ctl_match(B) moves B's filter and pan; ctl_tags_each on B's tags bends every
  note of B by its own amount and gives it its own velocity.

Everything here is the CPU model's; the device is held to it step by step.
"""
import numpy as np

import ctl_model as CM
import expr_model as EM
import owner_model as OM
import owner_scenes as S
import slot_model as SM
from skred_amd import banks, device
from skred_amd.device import ctl, ctl_each

N, K, F = S.N, S.K, S.F
CH_A, CH_B, CH_C = 0x0A, 0x0B, 0x0C
CH_MASK = 0xFF000000
A_TAGS = np.array([CH_A << 24 | (k + 1) for k in range(len(S.A_SLOTS))], np.uint32)
B_TAGS = np.array([CH_B << 24 | (0x100 - 37 * k) for k in range(S.B_COUNT)], np.uint32)      # descending: the sort has work to do
C_TAGS = (np.uint32(CH_C << 24) + np.arange(len(S.others()), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)


def channel(ch):
    return device.owner_match(ch << 24, CH_MASK)


def sweep():
    """B's mod wheel: a cutoff and a pan on voices 0 .. 2 of a copy (FILTER and PAN list nobody)."""
    co = banks.biquad_coeffs(np.array([1]), np.array([900.0], np.float32), np.array([1.2], np.float32), 48000)
    return [ctl(CM.FILTER | CM.PAN, pan_left=0.3 + 0.1 * l, pan_right=0.6, b0=float(co["b0"][0]), b1=float(co["b1"][0]),
                b2=float(co["b2"][0]), a1=float(co["a1"][0]), a2=float(co["a2"][0])) for l in range(K)]


def bends():
    """one entry per note of B: its own bend and its own velocity"""
    return [ctl_each(EM.EACH_INC_SCALE | EM.EACH_VELOCITY, inc_scale=float(np.float32(2.0 ** ((k - 2) / 24.0))), velocity=0.4 + 0.1 * k)
            for k in range(S.B_COUNT)]


class Story(S.Story):
    """owner_scenes.Story with channel tags, and the three channel calls on the oracle."""

    def chord_a(self):
        idle = SM.idle_slots(self.truth, 0, N, K, S.MMASK, S.WHICH, S.SETTLE)
        self.a_notes = S.notes(len(S.A_SLOTS), 1)
        self.a_assigned = SM.place(len(S.A_SLOTS), K, idle, len(idle), 0, N)
        SM.store_notes((self.truth,), self.truth, self.a_notes, K, S.VMASK, self.a_assigned, self.now())
        return self.a_assigned, OM.tag_slots(self.owner, self.a_assigned, A_TAGS, None, K)

    def fill_up(self):
        SM.stamp(self.truth, SM.stamp_voices(S.others(), len(S.others()), None, K, S.MMASK, N), SM.STAMP_TRIGGER, self.now())
        return OM.tag_slots(self.owner, S.others(), C_TAGS, None, K)

    def chord_b(self):
        owner, self.owner = self.owner, OM.new(N)          # (the parent tags with its own ids: into a scratch array)
        assigned, counts, _ = S.Story.chord_b(self)
        self.owner = owner
        return assigned, counts, OM.tag_slots(self.owner, assigned, B_TAGS, None, K)

    def count(self, ch):
        return EM.find_match(self.owner, 0, N, K, ch << 24, CH_MASK, N)

    def a_all_notes_off(self):
        return EM.stamp_match(self.owner, self.truth, 0, N, K, S.VMASK, CH_A << 24, CH_MASK, SM.STAMP_RELEASE, self.now())

    def b_sweep(self):
        return EM.ctl_match(self.owner, (self.truth,), sweep(), 0, N, S.MMASK, CH_B << 24, CH_MASK)

    def b_bends(self):
        return EM.ctl_tags_each(self.owner, (self.truth,), None, bends(), 0, N, K, S.MMASK, B_TAGS)
