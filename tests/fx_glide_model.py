"""Portamento on the fixed-point bank, stated in numpy on uint64: the glide words and phase_inc as pure functions of the call
sequence.  Written from the definition in include/skred_amd_fxpt.h (section "portamento"), not from the kernels.

`glide` is a uint32 array of shape (n_voices, 4): target, up_q32, down_q32 and carry per voice; target == 0 is "not gliding".  `inc`
is the bank's phase_inc (a uint32 array, changed in place).  Every product is formed in uint64, where (2^32 - 1)^2 fits: no step
rounds, so the model, the plain Python-integer loop of tests/test_fx_glide_cpu.py and the device must agree bit for bit.

The guard and the find pass are fx_owner_model's.  FxStage moves the oracle's bank, the owner and glide arrays and the clock together;
clear_rule=False gives the model of a bank whose tag launches leave the glide words alone: the scenes of tests/test_fx_glide_cpu.py
fail on it.
"""
import numpy as np

import fx_live_model as live
import fx_owner_model as om
from oracle import cpuref
from skred_amd import fxbank as fxb

FROM_SCALE, TO_SCALE, TO_INC = fxb.FX_GLIDE_FROM_SCALE, fxb.FX_GLIDE_TO_SCALE, fxb.FX_GLIDE_TO_INC
TARGET, UP, DOWN, CARRY = 0, 1, 2, 3
BAD, RANGE = -2, -4
TOP = 0xFFFFFFFF
U64 = np.uint64


def new(n_voices):
    return np.zeros((n_voices, 4), np.uint32)


class Glide:
    """one entry of the two starting calls"""

    def __init__(self, set, up_q32, down_q32, scale_q16=0, target_inc=0, reserved=(0, 0, 0)):
        self.set, self.up, self.down, self.scale, self.target_inc = int(set), int(up_q32), int(down_q32), int(scale_q16), int(target_inc)
        self.reserved = tuple(reserved)

    def c(self):
        g = fxb.glide(self.set, self.up, self.down, self.scale, self.target_inc)
        g.reserved[:] = self.reserved
        return g


def check(glides, n=None):
    """skred_fx_glide_check: 0 or SKRED_E_BAD_ARG (None: a NULL array)."""
    if glides is None or (n is not None and n < 0):
        return BAD
    for g in glides[:n]:
        if g.set not in (FROM_SCALE, TO_SCALE, TO_INC) or any(g.reserved) or not g.up or not g.down:
            return BAD
        if (g.set == TO_INC and not g.target_inc) or (g.set != TO_INC and not g.scale):
            return BAD
    return 0


def tag_list(owner, glide, entries, tags, count=None, clear_rule=True):
    """fx_owner_model.tag_list, and -- a bank that has a glide array -- the tagged voices' four words cleared."""
    res = om.tag_list(owner, entries, tags, count)
    if glide is not None and clear_rule:
        e = om.looked(entries, len(tags), count)
        glide[e[(e >= 0) & (e < len(owner))]] = 0
    return res


def start_one(inc, words, g):
    """The start of entry g on a voice that holds `inc` and the glide words `words` (Python integers): (the new inc, the new words),
    or None where the start is withheld."""
    if g.set == FROM_SCALE:
        target, nxt = inc, (inc * g.scale) >> 16
    elif g.set == TO_SCALE:
        target, nxt = ((words[TARGET] or inc) * g.scale) >> 16, inc
    else:
        target, nxt = g.target_inc, inc
    if not (1 <= inc <= TOP and 1 <= nxt <= TOP and 1 <= target <= TOP):
        return None
    return nxt, (target, g.up, g.down, 0)


def start_owned(owner, glide, inc, glides, entries, tags, count=None):
    """Returns [voices set gliding, starts withheld, voices whose owner differs]."""
    assert om.tags_check(tags, 0) == 0 and check(glides) == 0 and len(glides) == len(tags)
    res, seen = [0, 0, 0], set()
    for k, v in enumerate(om.looked(entries, len(tags), count).tolist()):
        if v < 0 or v >= len(owner):
            continue
        if int(owner[v]) != int(tags[k]):
            res[2] += 1
            continue
        assert v not in seen, "a voice named twice: unspecified"
        seen.add(v)
        out = start_one(int(inc[v]), [int(w) for w in glide[v]], glides[k])
        if out is None:
            res[1] += 1
        else:
            inc[v], glide[v] = out
            res[0] += 1
    return res


def start_tags(owner, glide, inc, glides, first, count, tags):
    """find_owned, then start_owned on its list.  Returns (d_result, the list)."""
    lst = om.find_owned(owner, first, count, tags)
    res = start_owned(owner, glide, inc, glides, lst, tags)
    assert res[2] == 0
    return res, lst


def advance(glide, inc, first, count, frames):
    """The advance pass by `frames` frames over [first, first + count).  Returns [still gliding, arrived]."""
    assert 1 <= frames <= 65536
    g = glide[first:first + count]
    w = inc[first:first + count]
    on = g[:, TARGET] != 0
    target = g[:, TARGET].astype(U64)
    cur = w.astype(U64)
    there = on & ((cur == 0) | (cur == target))
    c = g[:, CARRY].astype(U64) + U64(frames)
    m = c >> U64(6)
    one = U64(1)
    for step in range(int(m[on].max()) if on.any() else 0):
        act = on & ~there & (m > U64(step))
        if not act.any():
            break
        up, down = act & (cur < target), act & (cur > target)
        d_up = np.maximum(one, (cur * g[:, UP].astype(U64)) >> U64(32))
        d_down = np.maximum(one, (cur * g[:, DOWN].astype(U64)) >> U64(32))
        assert (d_down[down] <= cur[down]).all()
        cur = np.where(up, cur + d_up, np.where(down, cur - np.minimum(d_down, cur), cur))
        there |= (up & (cur >= target)) | (down & (cur <= target))
    still = on & ~there
    assert (cur[still] <= U64(TOP)).all()
    w[there] = g[there, TARGET]
    w[still] = cur[still].astype(np.uint32)
    g[still, CARRY] = (c[still] & U64(63)).astype(np.uint32)
    g[there] = 0
    return [int(still.sum()), int(there.sum())]


def stop(glide, inc, first, count, snap):
    g = glide[first:first + count]
    w = inc[first:first + count]
    on = g[:, TARGET] != 0
    if snap:
        w[on] = g[on, TARGET]
    g[:] = 0


def q16_route(inc, scale_q16):
    """What the bank offered before: one SKRED_EACH_INC_SCALE per block -- (inc * scale) >> 16, withheld above 32 bits."""
    prod = (int(inc) * int(scale_q16)) >> 16
    return prod if prod <= TOP else int(inc)


def per_64(semitones_per_second, rate=44100.0):
    """(up_q32, down_q32) of a glide of that speed: the factor per 64 frames, as the two Q32 fractions"""
    r = 2.0 ** (semitones_per_second / 12.0 * 64.0 / rate)
    return max(1, min(TOP, int(round((r - 1.0) * 2.0 ** 32)))), max(1, min(TOP, int(round((1.0 - 1.0 / r) * 2.0 ** 32))))


def scale_q16(semitones):
    return int(round(2.0 ** (semitones / 12.0) * 65536.0))


# ---------------------------------------------------------------------------------------------- the stage

class FxStage:
    """The oracle's fixed-point bank, the owner and glide arrays and the clock.  Every method is one call of the interface; a subclass
    performs it on a device too and compares (tests/test_fx_glide.py).  clear_rule=False: a model WITHOUT the clear behind a tag
    launch.  The glide array exists from the first start, as on the device: before it, a tag launch clears nothing."""
    F, INTERP = 64, 1

    def __init__(self, bank, pool, c0, clear_rule=True):
        self.bank, self.pool = bank, pool
        self.truth, self.cnt = bank.copy(), int(c0)
        self.n = bank.n
        self.owner, self.glide = om.new(bank.n), new(bank.n)
        self.clear_rule = clear_rule
        self.whole = (0, bank.n)

    def now(self):
        return self.cnt

    @property
    def inc(self):
        return self.truth["phase_inc"]

    def tag(self, entries, tags, count=None):
        return tag_list(self.owner, self.glide, entries, tags, count, self.clear_rule)

    def strike(self, voices, tags, incs=None):
        """A note-on the host places itself: the trigger stamp on the listed voices, then their tags (incs: the keys' increments)."""
        voices = np.asarray(voices, np.int32)
        if incs is not None:
            self.truth["phase_inc"][voices] = np.asarray(incs, np.uint32)
        live.stamp(self.truth, voices, fxb.STAMP_TRIGGER, self.now())
        return self.tag(voices, tags)

    def start(self, glides, tags, rng=None):
        first, count = rng or self.whole
        return start_tags(self.owner, self.glide, self.inc, glides, first, count, tags)[0]

    def start_list(self, glides, entries, tags, count=None):
        return start_owned(self.owner, self.glide, self.inc, glides, entries, tags, count)

    def advance(self, frames, rng=None):
        first, count = rng or self.whole
        return advance(self.glide, self.inc, first, count, frames)

    def stop(self, snap, rng=None):
        first, count = rng or self.whole
        stop(self.glide, self.inc, first, count, snap)

    def block(self, frames=None):
        mix, stems, self.cnt = cpuref.fx_render(self.truth, self.pool, self.cnt, frames or self.F, self.INTERP, want_stems=True)
        return mix, stems


# ---------------------------------------------------------------------------------------------- the clear rule's scenes

SCENES = ("thief", "restrike")
TAG_A, TAG_B = 0x0300003C, 0x03000040


def run_scene(name, st):
    """Two scenes on a stage, each of which FAILS on a bank whose tag launches leave the glide words alone.
    thief:    a note glides towards a far key; another note takes its voice (a thief's tag launch).  The thief must not inherit
              the glide, and the victim's later glide call finds nobody.
    restrike: mono mode -- a note slides into its key; the key is struck again on the same voice under the same tag at another
              pitch.  The new note must stay where it was struck; the legato the host wants is note-on, then glide_tags(FROM_SCALE)."""
    up, down = per_64(700.0)
    if name == "thief":
        v, key_a, key_b, far = 300, 30000001, 52000003, 90000001
        st.strike([v], [TAG_A], [key_a])
        st.block()
        assert st.start([Glide(TO_INC, up, down, target_inc=far)], [TAG_A]) == [1, 0, 0]
        assert st.advance(64) == [1, 0] and key_a < st.inc[v] < far
        st.block()
        st.strike([v], [TAG_B], [key_b])
        assert not st.glide[v].any(), "the thief inherited its victim's glide"
        for _ in range(3):
            assert st.advance(64) == [0, 0]
            st.block()
        assert st.inc[v] == key_b
        assert st.start([Glide(TO_INC, up, down, target_inc=far)], [TAG_A]) == [0, 0, 0]      # nobody carries the victim's tag
        assert not st.glide.any()
    elif name == "restrike":
        v, key_1, key_2 = 64, 40000003, 53393781
        st.strike([v], [TAG_A], [key_1])
        assert st.start([Glide(FROM_SCALE, up, down, scale_q16(-5))], [TAG_A]) == [1, 0, 0]
        assert st.glide[v, TARGET] == key_1 and st.inc[v] == (key_1 * scale_q16(-5)) >> 16
        assert st.advance(64) == [1, 0]
        st.block()
        st.strike([v], [TAG_A], [key_2])
        assert st.advance(64) == [0, 0] and st.inc[v] == key_2, "the key struck again slides towards the old note's key"
        st.block()
        # mono legato as the header orders it: the note-on (above), then the slide into it from the previous key
        assert st.start([Glide(FROM_SCALE, up, down, (key_1 << 16) // key_2)], [TAG_A]) == [1, 0, 0]
        assert abs(int(st.inc[v]) - key_1) <= key_1 >> 15 and st.glide[v, TARGET] == key_2
        for _ in range(40):
            res = st.advance(64)
            st.block()
            if res == [0, 1]:
                break
        assert st.inc[v] == key_2 and not st.glide.any(), "the slide lands on the struck key's bits"
    else:
        raise KeyError(name)
