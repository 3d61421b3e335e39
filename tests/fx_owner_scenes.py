"""The theft scene of the fixed-point note-owner tests, on the model and the oracle alone (tests/test_fx_owner_cpu.py shows that it
really steals; tests/test_fx_owner.py runs the same calls on the GPU and compares after every step).

64 voices of the bank_fx recipe.  Eight of them are idle, the rest sounds.  Chord A (eight tagged notes) takes the idle voices; a
block later the bank is full and chord B (eight tagged notes, QUIETEST) steals A's voices -- they have only just begun their
attack -- and overwrites their tags.  Then A's keys are lifted."""
import numpy as np

import fx_live_model as live
import fx_owner_model as om
import fx_steal_model as sm
from oracle import cpuref
from skred_amd import fxbank as fxb

N, CHORD = 64, 8
WHICH, SETTLE = fxb.IDLE_ENV_DONE, 0
IDLE = np.arange(5, N, 7)[:CHORD]                       # the voices at rest when the scene opens
WARM = 512                                              # frames rendered first: the sounding voices' smoothers come up
A_TAGS = [0x80000001 + 17 * k for k in range(CHORD)]
B_TAGS = [0x00010000 + 3 * k for k in range(CHORD)]
B_TAGS[3] = 0xFFFFFFFF
REL = fxb.STAMP_RELEASE


def notes(k, seed):
    return [fxb.FxNoteC(3000017 + 40009 * i + seed, 20000 + 23 * i, (0x01234567 * (i + 1)) & 0xFFFFFFFF, 700 + 31 * i, 32000 - 29 * i,
                        fxb.NOTE_SET_PHASE | fxb.NOTE_SET_PAN) for i in range(k)]


def theft_bank():
    b, pool, c0 = fxb.bank_fx(N)
    b["is_active"][IDLE] = 0
    return b, pool, c0


def steal_query():
    return sm.Query(0, N, sm.QUIETEST, 0, 0, WHICH, SETTLE, CHORD)


class Story:
    """The scene's state as the device should hold it: the oracle's bank, the owner words, the clock."""

    def __init__(self):
        self.start, self.pool, self.c0 = theft_bank()
        self.truth, self.cnt = self.start.copy(), self.c0
        self.owner = om.new(N)
        self.mixes = []

    def block(self, frames=64, interp=1):
        mix, _, self.cnt = cpuref.fx_render(self.truth, self.pool, self.cnt, frames, interp)
        self.mixes.append(mix)
        return mix

    def chord_a(self):
        """note_on_idle + tag_list: (d_assigned, (placed, dropped), [tagged, no voice])"""
        listed, _ = live.idle_list(self.truth, 0, N, WHICH, SETTLE, 0, CHORD)
        assigned, counts = live.place_notes(self.truth, notes(CHORD, 1), listed, len(listed), 0, self.cnt)
        return assigned, counts, om.tag_list(self.owner, assigned, A_TAGS)

    def chord_b(self, k=CHORD):
        """note_on_steal + tag_list: (d_assigned, (placed, dropped, stolen), [tagged, no voice])"""
        listed, _ = live.idle_list(self.truth, 0, N, WHICH, SETTLE, 0, k)
        victims, _ = sm.victims(self.truth, self.cnt, steal_query().but(max_out=min(k, sm.STEAL_MAX)))
        joined = np.concatenate([listed, victims])[:k].astype(np.int32)
        assigned, counts = live.place_notes(self.truth, notes(k, 2), joined, len(joined), 0, self.cnt)
        stolen = max(0, min(k, len(joined)) - len(listed))
        return assigned, counts + (stolen,), om.tag_list(self.owner, assigned, B_TAGS[:k])

    def a_off_by_tag(self):
        return om.release_tags(self.owner, self.truth, 0, N, A_TAGS, REL, self.cnt)

    def a_off_guarded(self, a_assigned):
        return om.stamp_owned(self.owner, self.truth, a_assigned, A_TAGS, None, REL, self.cnt)

    def a_off_unguarded(self, a_assigned):
        """the hole: skred_fxbank_stamp_list on the old d_assigned"""
        v = a_assigned[(a_assigned >= 0) & (a_assigned < N)]
        live.stamp(self.truth, v, REL, self.cnt)
        return v
