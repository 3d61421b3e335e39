"""Pedals, stated in numpy: the pedal array as a pure function of the call sequence -- the held-back note-off, sostenuto's latch, the
pedal-up, and the rule that a new note clears the word.  Written from the definition in include/skred_amd.h (section "pedals"), not
from the kernels, on the oracle's state plus an owner array (tests/owner_model.py) and a pedal array: one uint32 word per voice, a
slot's word at its first voice.  The stamps themselves are slot_model.stamp's.

Stage moves the oracle's bank, the two arrays and the clock together; the scenes (a) .. (f) below are written against its methods, so
tests/test_pedal_cpu.py runs them on the oracle alone and tests/test_pedal.py on a Stage that drives a device bank beside it.
"""
import numpy as np

import chan_model as CM
import ctl_model as CTL
import owner_model as OM
import slot_model as SM
from oracle import cpuref

PENDING, LATCHED = 1, 2
LIFT_SUSTAIN, LIFT_SOSTENUTO, SUSTAIN_DOWN = 1, 2, 4
REL, TRIG = SM.STAMP_RELEASE, SM.STAMP_TRIGGER
BAD, RANGE = -2, -4


def new(n_voices):
    return np.zeros(n_voices, np.uint32)


def tag_slots(owner, pedal, entries, tags, count, K, clear_rule=True):
    """owner_model.tag_slots, and -- a bank that has a pedal array -- the tagged slots' pedal words cleared."""
    res = OM.tag_slots(owner, entries, tags, count, K)
    if pedal is not None and clear_rule:
        for e in OM.looked(entries, len(tags), count):
            if CTL.slot_valid(e, K, len(owner)):
                pedal[e] = 0
    return res


def stamp_owned_pedal(owner, pedal, truth, entries, tags, count, K, voice_mask, hold_all, now):
    """([stamped, owner differs, no slot, held back], the voices stamped)."""
    assert OM.tags_check(tags) == 0
    res, voices = [0, 0, 0, 0], []
    for k, e in enumerate(OM.looked(entries, len(tags), count)):
        if not CTL.slot_valid(e, K, len(owner)):
            res[2] += 1
        elif int(owner[e]) != int(tags[k]):
            res[1] += 1
        elif hold_all or (int(pedal[e]) & LATCHED):
            pedal[e] |= np.uint32(PENDING)
            res[3] += 1
        else:
            res[0] += 1
            voices.extend(e + l for l in SM.lanes(voice_mask, K))
    voices = np.array(voices, np.int32)
    SM.stamp(truth, voices, REL, now)
    return res, voices


def release_tags_pedal(owner, pedal, truth, first, count, K, voice_mask, tags, hold_all, now):
    lst = OM.find_owned(owner, first, count, K, tags)
    res, voices = stamp_owned_pedal(owner, pedal, truth, lst, tags, None, K, voice_mask, hold_all, now)
    assert res[1] == 0
    return res, voices, lst


def held(truth):
    """Per voice: live and not released, as skred_slot_steal_query_t defines the two."""
    e = truth["voice_amp_envelope"]
    return (truth["voice_use_amp_envelope"] != 0) & (e["is_active"] != 0) & (e["sample_release"] == 0)


def latch(owner, pedal, truth, first, count, K, voice_mask, match):
    """[slots that satisfy the latch rule, slots of the range that did not match]."""
    heads = np.arange(first, first + count, K)
    hit = CM.matches(owner[heads], match)
    h = held(truth)
    some = np.zeros(len(heads), bool)
    for l in SM.lanes(voice_mask, K):
        some |= h[heads + l]
    take = hit & ((pedal[heads] & PENDING) == 0) & some
    pedal[heads[take]] |= np.uint32(LATCHED)
    return [int(take.sum()), int((~hit).sum())]


def up(owner, pedal, truth, first, count, K, voice_mask, match, flags, now):
    """([released, still pending, did not match], the voices stamped)."""
    heads = np.arange(first, first + count, K)
    hit = CM.matches(owner[heads], match)
    word = pedal[heads].copy()
    if flags & LIFT_SOSTENUTO:
        word[hit] &= np.uint32(~LATCHED & 0xFFFFFFFF)
    release = hit & ((word & PENDING) != 0) & ((word & LATCHED) == 0) & (not flags & SUSTAIN_DOWN)
    word[release] &= np.uint32(~PENDING & 0xFFFFFFFF)
    pedal[heads] = word
    voices = np.array([int(e) + l for e in heads[release] for l in SM.lanes(voice_mask, K)], np.int32)
    SM.stamp(truth, voices, REL, now)
    return [int(release.sum()), int((hit & ((word & PENDING) != 0)).sum()), int((~hit).sum())], voices


def clear(pedal, first, count):
    pedal[first:first + count] = 0


def up_flags_check(flags):
    if flags & ~(LIFT_SUSTAIN | LIFT_SOSTENUTO | SUSTAIN_DOWN) or not flags & (LIFT_SUSTAIN | LIFT_SOSTENUTO):
        return BAD
    return BAD if (flags & SUSTAIN_DOWN) and (flags & LIFT_SUSTAIN) else 0


# ---------------------------------------------------------------------------------------------- the stage

def tag_of(channel, key):
    return (channel << 24) | key


class Stage:
    """The oracle's bank, the owner and pedal arrays and the clock.  Every method is one call of the interface; a subclass performs it
    on a device too and compares (tests/test_pedal.py).  clear_rule=False: a model WITHOUT the clear behind a tag launch."""
    F = 64

    def __init__(self, bank, tables, g, K, vmask, clear_rule=True):
        self.bank, self.tables = bank, tables
        self.truth, self.gl = bank.copy(), g.copy()
        self.n, self.K, self.vmask = bank.n, K, vmask
        self.owner, self.pedal = OM.new(bank.n), new(bank.n)
        self.clear_rule = clear_rule
        self.whole = (0, bank.n - bank.n % K)

    def now(self):
        return int(self.gl.synth_sample_count)

    def tag(self, entries, tags, count=None):
        return tag_slots(self.owner, self.pedal, entries, tags, count, self.K, self.clear_rule)

    def strike(self, slots, tags):
        """A note-on the host places itself: the trigger stamp on the listed slots, then their tags."""
        slots = np.asarray(slots, np.int32)
        SM.stamp(self.truth, SM.stamp_voices(slots, len(slots), None, self.K, self.vmask, self.n), TRIG, self.now())
        return self.tag(slots, tags)

    def off(self, tags, hold_all, rng=None):
        first, count = rng or self.whole
        return release_tags_pedal(self.owner, self.pedal, self.truth, first, count, self.K, self.vmask, tags, hold_all, self.now())[0]

    def off_list(self, entries, tags, hold_all, count=None):
        return stamp_owned_pedal(self.owner, self.pedal, self.truth, entries, tags, count, self.K, self.vmask, hold_all, self.now())[0]

    def plain_off(self, tags, rng=None):
        """skred_bank_release_tags: no pedal decision, the bits stay."""
        first, count = rng or self.whole
        return OM.release_tags(self.owner, self.truth, first, count, self.K, self.vmask, tags, REL, self.now())[0]

    def latch(self, match, rng=None):
        first, count = rng or self.whole
        return latch(self.owner, self.pedal, self.truth, first, count, self.K, self.vmask, match)

    def up(self, match, flags, rng=None):
        first, count = rng or self.whole
        return up(self.owner, self.pedal, self.truth, first, count, self.K, self.vmask, match, flags, self.now())[0]

    def pedal_clear(self, first, count):
        clear(self.pedal, first, count)

    def block(self):
        return cpuref.render(self.truth, self.gl, self.tables, self.F, 0)

    def release_clock(self, slot):
        """sample_release of the slot's masked voices (one value: they are stamped together)."""
        r = self.truth["voice_amp_envelope"]["sample_release"][[slot + l for l in SM.lanes(self.vmask, self.K)]]
        assert len(set(r.tolist())) == 1, r
        return int(r[0])

    def word(self, slot):
        return int(self.pedal[slot])


# ---------------------------------------------------------------------------------------------- the scenes
# Each takes a Stage whose slots 0 .. 7 (first voices s[0] .. s[7]) hold sustaining notes that nobody has tagged yet, and asserts on
# the model's state; run on a device Stage, every call is also held to the device.  CH, OTHER: two channels.
CH, OTHER = 3, 5
SCENES = ("a", "b", "c", "d", "e", "f")


def scene_a(st, s):
    """Sustain: on, off under the pedal, two blocks, pedal up -- the release clock is the pedal-up block's, not the note-off's."""
    t = [tag_of(CH, 60), tag_of(CH, 64)]
    assert st.strike(s[:2], t) == [2, 0]
    st.block()
    t_off = st.now()
    assert st.off(t, True) == [0, 0, 0, 2]
    assert st.word(s[0]) == st.word(s[1]) == PENDING and st.release_clock(s[0]) == 0
    st.block(), st.block()
    t_up = st.now()
    assert t_up > t_off
    assert st.up(CM.channel(CH), LIFT_SUSTAIN)[:2] == [2, 0]
    assert st.release_clock(s[0]) == st.release_clock(s[1]) == t_up and st.word(s[0]) == 0
    st.block()
    assert st.up(CM.channel(CH), LIFT_SUSTAIN)[:2] == [0, 0]                       # nothing is held any more
    assert st.release_clock(s[0]) == t_up


def scene_b(st, s):
    """Re-strike: the same tag on the SAME slot in the same block, after its note-off was held.  The pedal-up must not release the
    new note."""
    t = [tag_of(CH, 60)]
    st.strike(s[:1], t)
    st.block()
    assert st.off(t, True) == [0, 0, 0, 1]
    st.strike(s[:1], t)                                                           # mono: the key again, the old note's slot
    st.block()
    st.up(CM.channel(CH), LIFT_SUSTAIN)
    st.block()
    assert st.release_clock(s[0]) == 0, "the pedal-up released a key that is still down"
    assert st.word(s[0]) == 0


def scene_c(st, s):
    """Theft of a pending note by another tag: the thief's tag call clears the victim's bits; the victim's later note-off misses."""
    a, b = [tag_of(CH, 60)], [tag_of(CH, 72)]
    st.strike(s[:1], a)
    st.block()
    assert st.off(a, True) == [0, 0, 0, 1]
    st.strike(s[:1], b)                                                           # b steals a's slot
    assert st.word(s[0]) == 0
    st.block()
    assert st.up(CM.channel(CH), LIFT_SUSTAIN)[:2] == [0, 0]
    assert st.release_clock(s[0]) == 0
    assert st.off(a, False) == [0, 0, 1, 0]                                       # a's tag is carried by nobody
    assert st.off(b, False) == [1, 0, 0, 0] and st.release_clock(s[0]) == st.now()
    st.block()


def scene_d(st, s):
    """Sostenuto catches held notes only: neither later ones nor ones already pending."""
    t = [tag_of(CH, 60 + k) for k in range(4)]
    st.strike(s[:3], t[:3])
    st.block()
    assert st.off(t[2:3], True) == [0, 0, 0, 1]                                   # note 2: pending under sustain
    assert st.off(t[1:2], False) == [1, 0, 0, 0]                                  # note 1: released, no longer held
    assert st.latch(CM.channel(CH))[0] == 1                                        # note 0 alone
    assert [st.word(x) for x in s[:3]] == [LATCHED, 0, PENDING]
    st.strike(s[3:4], t[3:4])                                                     # struck after the pedal went down
    st.block()
    assert st.off([t[0], t[3]], False) == [1, 0, 0, 1]                             # 3 is released at once, 0 is held by sostenuto
    assert st.word(s[0]) == LATCHED | PENDING and st.release_clock(s[0]) == 0 and st.release_clock(s[3]) == st.now()
    st.block()
    assert st.up(CM.channel(CH), LIFT_SOSTENUTO)[:2] == [2, 0]                     # 0, and 2 (the host says sustain is up by now)
    assert st.release_clock(s[0]) == st.release_clock(s[2]) == st.now() and st.word(s[0]) == st.word(s[2]) == 0
    st.block()


def scene_e(st, s):
    """Both pedals, lifted in either order; sostenuto lifted while sustain stays down."""
    t = [tag_of(CH, 60 + k) for k in range(6)]
    st.strike(s[:6], t)
    st.block()
    assert st.latch(CM.channel(CH))[0] == 6
    # sustain first: the latched notes stay
    assert st.off(t[:2], True) == [0, 0, 0, 2]
    assert st.up(CM.channel(CH), LIFT_SUSTAIN)[:2] == [0, 2]
    assert st.release_clock(s[0]) == 0 and st.word(s[0]) == LATCHED | PENDING
    st.block()
    # sostenuto lifts, sustain is down (again): everything pending stays pending, the latch is gone
    assert st.off(t[2:4], True) == [0, 0, 0, 2]
    assert st.up(CM.channel(CH), LIFT_SOSTENUTO | SUSTAIN_DOWN)[:2] == [0, 4]
    assert [st.word(x) for x in s[:6]] == [PENDING] * 4 + [0, 0] and st.release_clock(s[2]) == 0
    st.block()
    t_up = st.now()
    assert st.up(CM.channel(CH), LIFT_SUSTAIN)[:2] == [4, 0]
    assert all(st.release_clock(x) == t_up for x in s[:4]) and st.release_clock(s[4]) == 0
    # both at once
    assert st.latch(CM.channel(CH))[0] == 2
    assert st.off(t[4:6], False) == [0, 0, 0, 2]
    assert st.up(CM.channel(CH), LIFT_SUSTAIN | LIFT_SOSTENUTO)[:2] == [2, 0]
    assert st.release_clock(s[5]) == st.now() and not st.pedal.any()
    st.block()


def scene_f(st, s):
    """Two channels in one range: a pedal on one never touches the other."""
    a = [tag_of(CH, 60), tag_of(CH, 61)]
    b = [tag_of(OTHER, 60), tag_of(OTHER, 61)]
    st.strike([s[0], s[2]], a)
    st.strike([s[1], s[3]], b)
    st.block()
    assert st.off(a[:1], True) == [0, 0, 0, 1] and st.off(b[:1], True) == [0, 0, 0, 1]
    assert st.latch(CM.channel(OTHER))[0] == 1 and st.word(s[3]) == LATCHED and st.word(s[2]) == 0
    st.block()
    assert st.up(CM.channel(CH), LIFT_SUSTAIN | LIFT_SOSTENUTO)[:2] == [1, 0]
    assert st.release_clock(s[0]) == st.now() and st.release_clock(s[1]) == 0
    assert [st.word(x) for x in s[:4]] == [0, PENDING, 0, LATCHED]
    st.block()
    assert st.up(CM.channel(OTHER), LIFT_SUSTAIN)[:2] == [1, 0]
    assert st.release_clock(s[1]) == st.now() and st.word(s[3]) == LATCHED
    st.pedal_clear(0, st.n)
    assert not st.pedal.any()
    st.block()


def run_scene(name, st, slots):
    {"a": scene_a, "b": scene_b, "c": scene_c, "d": scene_d, "e": scene_e, "f": scene_f}[name](st, list(slots))
