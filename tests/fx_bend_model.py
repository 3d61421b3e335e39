"""The pitch wheel of the fixed-point bank, stated in numpy on uint64: the bend words and phase_inc as pure functions of the call
sequence, and the glide calls on a bank that has a bend array.  Written from the definition in include/skred_amd_fxpt.h (section
"pitch wheel"), not from the kernels.

`bend` is a uint32 array of shape (n_voices, 2): key and ratio_q24 per voice; key == 0 is "not bent".  `inc` is the bank's phase_inc
(a uint32 array, changed in place); `glide` is fx_glide_model's array.  Every product is formed in uint64, where (2^32 - 1)^2 fits: no
step rounds, so the model, the plain Python-integer loop of tests/test_fx_bend_cpu.py and the device must agree bit for bit.

The guard and the find pass are fx_owner_model's, the glide definition fx_glide_model's.  FxBendStage moves the oracle's bank, the
owner, glide and bend arrays and the clock together; bend_clear_rule=False gives the model of a bank whose tag launches leave the bend
words alone: the scenes of tests/test_fx_bend_cpu.py fail on it.  A zeroed bend array and no bend array are the same bank to every
call here (a clear of zeros, a glide on voices without a key), so the stage holds the array from the start.
"""
import numpy as np

import fx_glide_model as GM
import fx_owner_model as om
from skred_amd import fxbank as fxb

KEY, RATIO = 0, 1
ONE = fxb.FX_BEND_ONE
BAD, RANGE = -2, -4
TOP = 0xFFFFFFFF
U64 = np.uint64


def new(n_voices):
    return np.zeros((n_voices, 2), np.uint32)


def check(ratios, n=None):
    """skred_fx_bend_check: 0 or SKRED_E_BAD_ARG (None: a NULL array)."""
    if ratios is None or (n is not None and n < 0):
        return BAD
    return BAD if any(int(r) == 0 for r in list(ratios)[:n]) else 0


def product(key, ratio):
    """(key * ratio_q24) >> 24 on uint64 arrays"""
    return (np.asarray(key).astype(U64) * np.asarray(ratio).astype(U64)) >> U64(24)


def apply(bend, inc, voices, ratio):
    """THE RULE on `voices` (distinct indices), to `ratio` (one for all, or one per voice).  Returns [stored or restored, withheld]."""
    vs = np.asarray(voices, np.int64).reshape(-1)
    r = np.broadcast_to(np.asarray(ratio, np.uint32), vs.shape)
    key, old_r, cur = bend[vs, KEY], bend[vs, RATIO], inc[vs]
    k = np.where(key != 0, key, cur)
    centre = r == np.uint32(ONE)
    p = product(k, r)
    ok = ~centre & (k != 0) & (p >= U64(1)) & (p <= U64(TOP))
    withheld = ~centre & ~ok
    restored = centre & (key != 0)
    inc[vs] = np.where(restored, key, np.where(ok, p.astype(np.uint32), cur))
    bend[vs, KEY] = np.where(centre, 0, np.where(ok, k, key))
    bend[vs, RATIO] = np.where(centre, 0, np.where(ok, r, old_r))
    return [int(ok.sum() + restored.sum()), int(withheld.sum())]


def bend_match(owner, bend, inc, first, count, match, ratio):
    """The channel wheel.  Returns [stored or restored, withheld, voices of the range that did not match]."""
    assert check([ratio]) == 0 and count > 0 and 0 <= first and first + count <= len(owner)
    value, mask = (np.uint32(x) for x in match)
    v = np.arange(first, first + count)
    words = owner[v]
    hit = (words != 0) & ((words & mask) == value)
    return apply(bend, inc, v[hit], ratio) + [int((~hit).sum())]


def bend_owned_each(owner, bend, inc, ratios, entries, tags, count=None):
    """Returns [stored or restored, withheld, voices whose owner differs]."""
    assert om.tags_check(tags, 0) == 0 and check(ratios) == 0 and len(ratios) == len(tags)
    res, seen = [0, 0, 0], set()
    for k, v in enumerate(om.looked(entries, len(tags), count).tolist()):
        if v < 0 or v >= len(owner):
            continue
        if int(owner[v]) != int(tags[k]):
            res[2] += 1
            continue
        assert v not in seen, "a voice named twice: unspecified"
        seen.add(v)
        a = apply(bend, inc, [v], int(ratios[k]))
        res = [res[0] + a[0], res[1] + a[1], res[2]]
    return res


def bend_tags_each(owner, bend, inc, ratios, first, count, tags):
    """find_owned, then bend_owned_each on its list.  Returns (d_result, the list)."""
    lst = om.find_owned(owner, first, count, tags)
    res = bend_owned_each(owner, bend, inc, ratios, lst, tags)
    assert res[2] == 0
    return res, lst


def clear(bend, inc, first, count, snap):
    b = bend[first:first + count]
    w = inc[first:first + count]
    on = b[:, KEY] != 0
    if snap:
        w[on] = b[on, KEY]
    b[:] = 0


def tag_clear(bend, entries, n_tags, count=None):
    """what follows every tag launch once the array exists: the words of the tagged voices"""
    e = om.looked(entries, n_tags, count)
    bend[e[(e >= 0) & (e < len(bend))]] = 0


# ---- the glide calls on a bank that has a bend array: on a voice with a key the glide runs on the key

def sound(bend, inc, voices):
    """the sounding increment of bent voices stored again as (key * ratio) >> 24; that store alone is withheld where the product is 0
    or above 32 bits"""
    vs = np.asarray(voices, np.int64).reshape(-1)
    vs = vs[bend[vs, KEY] != 0]
    p = product(bend[vs, KEY], bend[vs, RATIO])
    ok = (p >= U64(1)) & (p <= U64(TOP))
    inc[vs[ok]] = p[ok].astype(np.uint32)


def _keys_in(bend, inc):
    """the increments the glide definition reads: the key of a bent voice, else phase_inc"""
    bent = bend[:, KEY] != 0
    return np.where(bent, bend[:, KEY], inc).astype(np.uint32), bent


def _keys_out(bend, inc, eff, bent):
    bend[bent, KEY] = eff[bent]
    inc[~bent] = eff[~bent]


def glide_start_owned(owner, glide, bend, inc, glides, entries, tags, count=None):
    """fx_glide_model.start_owned under a bend array.  Returns its d_result."""
    eff, bent = _keys_in(bend, inc)
    # which starts were not withheld: fx_glide_model's own condition, read off a run on carry words no start can store (a start stores 0)
    probe = glide.copy()
    probe[:, GM.CARRY] = 99
    GM.start_owned(owner, probe, eff.copy(), glides, entries, tags, count)
    started = probe[:, GM.CARRY] != 99
    res = GM.start_owned(owner, glide, eff, glides, entries, tags, count)
    _keys_out(bend, inc, eff, bent)
    sound(bend, inc, np.flatnonzero(started & bent))
    return res


def glide_start_tags(owner, glide, bend, inc, glides, first, count, tags):
    lst = om.find_owned(owner, first, count, tags)
    res = glide_start_owned(owner, glide, bend, inc, glides, lst, tags)
    assert res[2] == 0
    return res, lst


def glide_advance(glide, bend, inc, first, count, frames):
    """fx_glide_model.advance under a bend array.  Returns its d_result."""
    eff, bent = _keys_in(bend, inc)
    gliding = np.zeros(len(inc), bool)
    gliding[first:first + count] = glide[first:first + count, GM.TARGET] != 0
    res = GM.advance(glide, eff, first, count, frames)
    _keys_out(bend, inc, eff, bent)
    sound(bend, inc, np.flatnonzero(gliding & bent))
    return res


def glide_stop(glide, bend, inc, first, count, snap):
    eff, bent = _keys_in(bend, inc)
    gliding = np.zeros(len(inc), bool)
    gliding[first:first + count] = glide[first:first + count, GM.TARGET] != 0
    GM.stop(glide, eff, first, count, snap)
    _keys_out(bend, inc, eff, bent)
    if snap:
        sound(bend, inc, np.flatnonzero(gliding & bent))


def ratio_of(semitones):
    """the wheel at `semitones` as a Q24 ratio (0: exactly ONE, the centre)"""
    return fxb.bend_ratio_q24(semitones)


def q16_of(ratio_q24):
    """the nearest Q16 scale of a Q24 ratio: what the INC_SCALE route can send for that wheel position"""
    return (int(ratio_q24) + 128) >> 8


def q16_sweep(inc, ratios_q24):
    """The route the bank offered before, driven by the same sweep and back to the centre: the host remembers the last position and
    sends the ratio of the ratios as a Q16 scale, (inc * scale) >> 16 per message.  Returns the increment it ends on."""
    inc, last = int(inc), ONE
    for r in list(ratios_q24) + [ONE]:
        scale = (int(r) * 65536 + last // 2) // last
        inc = GM.q16_route(inc, scale)
        last = int(r)
    return inc


# ---------------------------------------------------------------------------------------------- the stage

class FxBendStage(GM.FxStage):
    """fx_glide_model.FxStage with the bend array: every glide call of the stage runs under it.  bend_clear_rule=False: a model WITHOUT
    the clear of the bend words behind a tag launch (the glide words' clear stays)."""

    def __init__(self, bank, pool, c0, clear_rule=True, bend_clear_rule=True):
        super().__init__(bank, pool, c0, clear_rule)
        self.bend = new(bank.n)
        self.bend_clear_rule = bend_clear_rule

    def tag(self, entries, tags, count=None):
        res = super().tag(entries, tags, count)
        if self.bend_clear_rule:
            tag_clear(self.bend, entries, len(tags), count)
        return res

    def start(self, glides, tags, rng=None):
        first, count = rng or self.whole
        return glide_start_tags(self.owner, self.glide, self.bend, self.inc, glides, first, count, tags)[0]

    def start_list(self, glides, entries, tags, count=None):
        return glide_start_owned(self.owner, self.glide, self.bend, self.inc, glides, entries, tags, count)

    def advance(self, frames, rng=None):
        first, count = rng or self.whole
        return glide_advance(self.glide, self.bend, self.inc, first, count, frames)

    def stop(self, snap, rng=None):
        first, count = rng or self.whole
        glide_stop(self.glide, self.bend, self.inc, first, count, snap)

    def wheel(self, match, ratio, rng=None):
        first, count = rng or self.whole
        return bend_match(self.owner, self.bend, self.inc, first, count, match, ratio)

    def bend_tags(self, ratios, tags, rng=None):
        first, count = rng or self.whole
        return bend_tags_each(self.owner, self.bend, self.inc, ratios, first, count, tags)[0]

    def bend_list(self, ratios, entries, tags, count=None):
        return bend_owned_each(self.owner, self.bend, self.inc, ratios, entries, tags, count)

    def bend_clear(self, snap, rng=None):
        first, count = rng or self.whole
        clear(self.bend, self.inc, first, count, snap)


# ---------------------------------------------------------------------------------------------- the clear rule's scenes

SCENES = ("thief", "restrike")
TAG_A, TAG_B = 0x0300003C, 0x03000040
CHAN = (0x03000000, 0xFF000000)


def run_scene(name, st):
    """Two scenes on a stage, each of which FAILS on a bank whose tag launches leave the bend words alone.
    thief:    a note sounds under a deflected wheel; another note takes its voice (a thief's tag launch).  The thief's first bend must
              capture the THIEF's key, and the centre must give the thief's bits, not restore the victim's.
    restrike: a key is struck again in the same voice under the same tag at another pitch while the wheel is up; the bend that follows
              the note-on (the header's order) must rest on the new key, and the centre must give the new key's bits."""
    up = ratio_of(1.5)
    if name == "thief":
        v, key_a, key_b = 300, 30000001, 52000003
        st.strike([v], [TAG_A], [key_a])
        assert st.wheel(CHAN, up) == [1, 0, st.n - 1]
        assert st.inc[v] == (key_a * up) >> 24 and st.bend[v].tolist() == [key_a, up]
        st.block()
        st.strike([v], [TAG_B], [key_b])
        assert not st.bend[v].any(), "the thief inherited its victim's bend words"
        assert st.inc[v] == key_b
        assert st.bend_tags([up], [TAG_B]) == [1, 0, 0]
        assert st.bend[v].tolist() == [key_b, up] and st.inc[v] == (key_b * up) >> 24, "the thief's first bend rests on its victim's key"
        st.block()
        assert st.wheel(CHAN, ONE) == [1, 0, st.n - 1]
        assert st.inc[v] == key_b and not st.bend.any(), "the centre restored the victim's key"
        assert st.bend_tags([up], [TAG_A]) == [0, 0, 0]                              # nobody carries the victim's tag
    elif name == "restrike":
        v, key_1, key_2 = 64, 40000003, 53393781
        st.strike([v], [TAG_A], [key_1])
        assert st.bend_tags([up], [TAG_A]) == [1, 0, 0] and st.bend[v, KEY] == key_1
        st.block()
        st.strike([v], [TAG_A], [key_2])
        assert st.inc[v] == key_2
        # the header's order: the note-on (above), then the channel's ratio on the new note
        assert st.bend_tags([up], [TAG_A]) == [1, 0, 0]
        assert st.bend[v, KEY] == key_2 and st.inc[v] == (key_2 * up) >> 24, "the key struck again is bent from the old note's key"
        st.block()
        assert st.wheel(CHAN, ONE) == [1, 0, st.n - 1] and st.inc[v] == key_2 and not st.bend.any()
    else:
        raise KeyError(name)
