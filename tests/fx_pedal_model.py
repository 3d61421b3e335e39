"""Pedals on the fixed-point bank, stated in numpy: the pedal array as a pure function of the call sequence -- the held-back note-off,
sostenuto's latch, the pedal-up, and the rule that a new note clears the word.  Written from the definition in
include/skred_amd_fxpt.h (section "pedals"), not from the kernels, on the arrays oracle.cpuref.fx_render works on plus the owner array
of tests/fx_owner_model.py and a pedal array: one uint32 word per voice.  The matches are tests/fx_expr_model.py's, the stamps
tests/fx_live_model.py's -- so a voice whose envelope is not active gets no release clock and is counted as stamped or released all
the same, which is what the header says of this bank.

FxStage moves the oracle's bank, the two arrays and the clock together and has the method set of pedal_model.Stage, so
pedal_model.run_scene runs the float bank's scenes (a) .. (f) on it unchanged, at one voice per slot: tests/test_fx_pedal_cpu.py on
the oracle alone, tests/test_fx_pedal.py on an FxStage that drives a device bank beside it.
"""
import numpy as np

import fx_expr_model as em
import fx_live_model as live
import fx_owner_model as om
from oracle import cpuref
from skred_amd import fxbank as fxb

PENDING, LATCHED = fxb.PEDAL_PENDING, fxb.PEDAL_LATCHED
LIFT_SUSTAIN, LIFT_SOSTENUTO, SUSTAIN_DOWN = fxb.PEDAL_LIFT_SUSTAIN, fxb.PEDAL_LIFT_SOSTENUTO, fxb.PEDAL_SUSTAIN_DOWN
REL, TRIG = fxb.STAMP_RELEASE, fxb.STAMP_TRIGGER
BAD, RANGE = -2, -4
NOT = 0xFFFFFFFF


def new(n_voices):
    return np.zeros(n_voices, np.uint32)


def tag_list(owner, pedal, entries, tags, count=None, clear_rule=True):
    """fx_owner_model.tag_list, and -- a bank that has a pedal array -- the tagged voices' pedal words cleared."""
    res = om.tag_list(owner, entries, tags, count)
    if pedal is not None and clear_rule:
        e = om.looked(entries, len(tags), count)
        pedal[e[(e >= 0) & (e < len(owner))]] = 0
    return res


def stamp_owned_pedal(owner, pedal, bank, entries, tags, count, hold_all, now):
    """([stamped, owner differs, no voice, held back], the voices stamped in list order)."""
    assert om.tags_check(tags, 0) == 0
    res, voices = [0, 0, 0, 0], []
    for k, v in enumerate(om.looked(entries, len(tags), count).tolist()):
        if v < 0 or v >= len(owner):
            res[2] += 1
        elif int(owner[v]) != int(tags[k]):
            res[1] += 1
        elif hold_all or (int(pedal[v]) & LATCHED):
            pedal[v] |= np.uint32(PENDING)
            res[3] += 1
        else:
            res[0] += 1
            voices.append(v)
    live.stamp(bank, voices, REL, now)
    return res, np.array(voices, np.int32)


def release_tags_pedal(owner, pedal, bank, first, count, tags, hold_all, now):
    """find_owned, then stamp_owned_pedal on that list.  Returns (result, voices stamped, the list)."""
    lst = om.find_owned(owner, first, count, tags)
    res, voices = stamp_owned_pedal(owner, pedal, bank, lst, tags, None, hold_all, now)
    assert res[1] == 0
    return res, voices, lst


def held(bank):
    """Per voice: an envelope that runs and has no release clock -- candidate and released of skred_fxbank_find_steal."""
    return (bank["use_envelope"] != 0) & (bank["is_active"] != 0) & (bank["sample_release"] == 0)


def latch(owner, pedal, bank, first, count, match):
    """[voices that satisfy the latch rule, voices of the range that did not match]."""
    rng = slice(first, first + count)
    hit = em.matches(owner[rng], *match)
    take = hit & ((pedal[rng] & PENDING) == 0) & held(bank)[rng]
    pedal[rng][take] |= np.uint32(LATCHED)
    return [int(take.sum()), int((~hit).sum())]


def up(owner, pedal, bank, first, count, match, flags, now):
    """([released, still pending, did not match], the voices stamped)."""
    assert up_flags_check(flags) == 0
    rng = slice(first, first + count)
    hit = em.matches(owner[rng], *match)
    word = pedal[rng].copy()
    if flags & LIFT_SOSTENUTO:
        word[hit] &= np.uint32(~LATCHED & NOT)
    release = hit & ((word & PENDING) != 0) & ((word & LATCHED) == 0) & (not flags & SUSTAIN_DOWN)
    word[release] &= np.uint32(~PENDING & NOT)
    pedal[rng] = word
    voices = (first + np.flatnonzero(release)).astype(np.int32)
    live.stamp(bank, voices, REL, now)
    return [int(release.sum()), int((hit & ((word & PENDING) != 0)).sum()), int((~hit).sum())], voices


def clear(pedal, first, count):
    pedal[first:first + count] = 0


def up_flags_check(flags):
    if flags & ~(LIFT_SUSTAIN | LIFT_SOSTENUTO | SUSTAIN_DOWN) or not flags & (LIFT_SUSTAIN | LIFT_SOSTENUTO):
        return BAD
    return BAD if (flags & SUSTAIN_DOWN) and (flags & LIFT_SUSTAIN) else 0


# ---------------------------------------------------------------------------------------------- the stage

class FxStage:
    """The oracle's fixed-point bank, the owner and pedal arrays and the clock, under the method names of pedal_model.Stage (a slot is a
    voice).  Every method is one call of the interface; a subclass performs it on a device too and compares (tests/test_fx_pedal.py).
    clear_rule=False: a model WITHOUT the clear behind a tag launch."""
    F, INTERP = 64, 1

    def __init__(self, bank, pool, c0, clear_rule=True):
        self.bank, self.pool = bank, pool
        self.truth, self.cnt = bank.copy(), int(c0)
        self.n, self.K, self.vmask = bank.n, 1, 1
        self.owner, self.pedal = om.new(bank.n), new(bank.n)
        self.clear_rule = clear_rule
        self.whole = (0, bank.n)

    def now(self):
        return self.cnt

    def tag(self, entries, tags, count=None):
        return tag_list(self.owner, self.pedal, entries, tags, count, self.clear_rule)

    def strike(self, slots, tags):
        """A note-on the host places itself: the trigger stamp on the listed voices, then their tags."""
        live.stamp(self.truth, np.asarray(slots, np.int32), TRIG, self.now())
        return self.tag(slots, tags)

    def off(self, tags, hold_all, rng=None):
        first, count = rng or self.whole
        return release_tags_pedal(self.owner, self.pedal, self.truth, first, count, tags, hold_all, self.now())[0]

    def off_list(self, entries, tags, hold_all, count=None):
        return stamp_owned_pedal(self.owner, self.pedal, self.truth, entries, tags, count, hold_all, self.now())[0]

    def plain_off(self, tags, rng=None):
        """skred_fxbank_release_tags: no pedal decision, the bits stay."""
        first, count = rng or self.whole
        return om.release_tags(self.owner, self.truth, first, count, tags, REL, self.now())[0]

    def latch(self, match, rng=None):
        first, count = rng or self.whole
        return latch(self.owner, self.pedal, self.truth, first, count, match)

    def up(self, match, flags, rng=None):
        first, count = rng or self.whole
        return up(self.owner, self.pedal, self.truth, first, count, match, flags, self.now())[0]

    def pedal_clear(self, first, count):
        clear(self.pedal, first, count)

    def block(self):
        mix, stems, self.cnt = cpuref.fx_render(self.truth, self.pool, self.cnt, self.F, self.INTERP, want_stems=True)
        return mix, stems

    def release_clock(self, slot):
        return int(self.truth["sample_release"][slot])

    def word(self, slot):
        return int(self.pedal[slot])
