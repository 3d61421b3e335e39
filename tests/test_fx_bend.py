"""The pitch wheel of the fixed-point bank on the GPU (skred_fxbank_bend_match / _bend_owned_each / _bend_tags_each / _bend_clear /
_download_bend, and the glide calls on a bank that has a bend array), byte for byte.

After every call the device is held to tests/fx_bend_model.py: download_bend == the model's words, download_glide and download_owners
== its glide and owner arrays on every voice, every word of the bank (skred_fxbank_download and _download_params, phase_inc among
them) == the oracle's bank after the model's stores, every d_result word == the model's count with the guard words past it untouched;
mixes and stems of every rendered block are compared bit for bit with oracle.cpuref.fx_render -- the integer mix is exact.  The clear
rule's scenes are tests/fx_bend_model.py's; tests/test_fx_bend_cpu.py asserts on the oracle alone that each of them bites.
"""
import ctypes as C

import numpy as np
import pytest

import chan_model as CM
import fx_bend_model as BM
import fx_chan_model as FCM
import fx_glide_model as GM
import fx_live_model as live
import fx_pedal_model as PM
import fx_steal_model as sm
from skred_amd import fxbank as fxb
from test_fx_chan import assert_same_bank, whole_bank
from test_fx_glide import DeviceFxStage, FILL, cs, dev_count, dev_list, mixed_glides, padded_tags, ptr, sync
from test_fx_glide_cpu import CUTS
from test_fx_live import dev_i32, host_of, open_fx

pytestmark = pytest.mark.gpu

BAD, RANGE = -2, -4
ONE, TOP = BM.ONE, 0xFFFFFFFF
KEY, RATIO = BM.KEY, BM.RATIO
SPAN = 256                                                       # SK_CONTROL_SPAN: voices or entries per workgroup of the bend kernels
N, FIRST, COUNT = 600, 37, 500                                  # the range starts off a 64-lane boundary and crosses a workgroup edge
G = GM.Glide
CH = 3
CHAN = CM.channel(CH)
EDGE_RATIOS = [1, ONE - 1, ONE, ONE + 1, 1 << 31, TOP]


class DeviceBendStage(DeviceFxStage, BM.FxBendStage):
    """fx_bend_model.FxBendStage with a device bank beside it: every call -- the glide calls of test_fx_glide.DeviceFxStage among them,
    which now run under the bend array on both sides -- runs on both, and the device is compared with the model."""

    def same(self, what):
        got = self.db.download_bend()
        bad = np.flatnonzero((got != self.bend).any(axis=1))
        assert not len(bad), f"{what}: bend words differ at {bad[:8].tolist()}: {got[bad[:4]].tolist()} / {self.bend[bad[:4]].tolist()}"
        super().same(what)

    def wheel(self, match, ratio, rng=None):
        first, count = rng or self.whole
        res = self.result(3)
        self.db.bend_match(first, count, match[0], match[1], ratio, res.data_ptr())
        return self.read(res, 3, f"bend_match to {ratio:#x}", super().wheel(match, ratio, rng))

    def bend_tags(self, ratios, tags, rng=None):
        first, count = rng or self.whole
        res = self.result(3)
        self.db.bend_tags_each(ratios, first, count, tags, res.data_ptr())
        return self.read(res, 3, f"bend_tags_each of {len(tags)}", super().bend_tags(ratios, tags, rng))

    def bend_list(self, ratios, entries, tags, count=None):
        dl, dc, res = dev_list(entries), dev_count(count), self.result(3)
        self.db.bend_owned_each(ratios, dl.data_ptr(), tags, ptr(dc), res.data_ptr())
        return self.read(res, 3, "bend_owned_each", super().bend_list(ratios, entries, tags, count))

    def bend_clear(self, snap, rng=None):
        first, count = rng or self.whole
        self.db.bend_clear(first, count, snap)
        super().bend_clear(snap, rng)
        self.same(f"bend_clear snap {snap}")


def stage(n=N, **kw):
    bank, pool, c0 = fxb.bank_fx(n)
    return DeviceBendStage(bank, pool, c0, **kw)


def mixed_ratios(gen, n):
    """n ratios: the edges, wheel positions on both sides of the centre, and whatever 32 bits hold"""
    wheel = [BM.ratio_of(s) for s in (-2.0, -0.37, 0.013, 1.0, 2.0, 12.0, -24.0)]
    kind = gen.integers(0, 3, n)
    return np.where(kind == 0, gen.choice(EDGE_RATIOS, n), np.where(kind == 1, gen.choice(wheel, n), gen.integers(1, 1 << 32, n))).astype(np.uint32)


def edge_increments(st, voices):
    """the increments of the CPU tests' list on some voices, through the host's own route, so that products of 0 and above 32 bits occur"""
    picks = [1, 2, 65535, 65536, 1 << 24, 0x7FFFFFFF, 0x80000000, TOP - 1, TOP]
    for k, v in enumerate(voices):
        one = dev_list([int(v)])
        st.db.ctl_list(fxb.fx_ctl(fxb.CTL_PHASE_INC, phase_inc=picks[k % len(picks)]), one.data_ptr(), 1)
        st.truth["phase_inc"][v] = picks[k % len(picks)]
    st.same("edge increments")


# ---------------------------------------------------------------------------------------------- the clear rule

@pytest.mark.parametrize("name", BM.SCENES)
def test_scene_on_the_device(name):
    """A thief's tag_list and a key struck again: fx_bend_model's scenes, which fail on a bank without the clear behind the tag launch.
    The scenes' own first bend creates the array; a never-bent bank downloads zeros."""
    st = stage()
    try:
        assert not st.db.download_bend().any()
        BM.run_scene(name, st)
    finally:
        st.close()


def mono_args(n, ch):
    iq = fxb.FxIdleQueryC(0, n, fxb.IDLE_ENV_DONE, 0, 0, 0)
    return iq, sm.Query(0, n, sm.OLDEST, 0, 0, max_out=1), CM.channel(ch)


def test_thief_and_restruck_key_through_note_on_channel():
    """Mono mode (cap 1, min_age 0) under a deflected wheel: the key is struck again through skred_fxbank_note_on_channel, so the new
    note takes the old note's voice and the call's own tag launch is the one that clears the words.  Then the header's order: the
    channel's ratio on the new note, a slide into it, and at the end the centre gives the new key's bits."""
    st = stage()
    tag, v = [(CH << 24) | 60], 300
    up = BM.ratio_of(1.5)
    try:
        st.strike([v], tag, [40000003])
        assert st.wheel(CHAN, up) == [1, 0, st.n - 1]
        st.block()
        iq, sq, chan = mono_args(st.n, CH)
        want, res, _ = FCM.burst(st.truth, st.now(), st.owner, iq, sq, chan, 1, 1)
        assert want.tolist() == [v] and res == [1, 0, 1, 1], "the new note must steal the channel's only voice"
        notes = [fxb.FxNoteC(53393781, 20000, 0x01234567, 700, 32000, fxb.NOTE_SET_PHASE | fxb.NOTE_SET_PAN)]
        da, dr = dev_i32(3), dev_i32(6)
        sync()
        st.db.note_on_channel(notes, iq, sq.c(), chan[0], chan[1], 1, tag, da.data_ptr(), dr.data_ptr())
        live.place_notes(st.truth, notes, want, 1, 0, st.now())
        GM.tag_list(st.owner, st.glide, want, tag)
        BM.tag_clear(st.bend, want, 1)
        sync()
        assert host_of(da).tolist() == [v, FILL, FILL] and host_of(dr).tolist() == res + [FILL, FILL]
        assert not st.bend[v].any() and st.inc[v] == 53393781
        st.same("the re-strike")
        st.block()
        assert st.bend_tags([up], tag) == [1, 0, 0] and st.bend[v].tolist() == [53393781, up], "the new note inherited the old note's key"
        u, d = GM.per_64(700.0)
        assert st.start([G(GM.FROM_SCALE, u, d, GM.scale_q16(-4))], tag) == [1, 0, 0]
        for _ in range(12):
            res = st.advance(64)
            st.block()
            if res == [0, 1]:
                break
        assert st.bend[v].tolist() == [53393781, up] and st.inc[v] == (53393781 * up) >> 24 and not st.glide.any()
        assert st.wheel(CHAN, ONE) == [1, 0, st.n - 1] and st.inc[v] == 53393781 and not st.bend.any()
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- every call against the model

@pytest.mark.parametrize("n", [1, 65, SPAN - 1, SPAN + 1])
def test_every_call_against_the_model_on_small_banks(n):
    """Banks of 1, 65, SK_CONTROL_SPAN - 1 and SK_CONTROL_SPAN + 1 voices: the channel wheel, the per-note calls with holes and
    out-of-bank entries and a d_count below n, the centre, the clears -- edge increments among the voices."""
    st = stage(n)
    gen = np.random.default_rng(n)
    try:
        v = np.arange(n, dtype=np.int32)
        tags = (((v % 2 + CH).astype(np.uint32)) << np.uint32(24)) | (1 + v).astype(np.uint32)   # channels 3 and 4 interleaved
        st.tag(v, tags)
        edge_increments(st, v[::3][:18])
        for r in (BM.ratio_of(2.0), TOP, 1, ONE + 1, BM.ratio_of(-2.0)):
            res = st.wheel(CHAN, r)
            assert res[0] + res[1] == (n + 1) // 2 and res[2] == n // 2
        rs = mixed_ratios(gen, n)
        perm = gen.permutation(n)
        lst = v[perm].tolist() + [-1, n, n + 7]
        ltags = tags[perm].tolist() + [5, 6, 7]
        if n > 1:
            ltags[0] ^= 1                                                             # a stolen voice: the owner differs
        lr = rs.tolist() + [ONE + 3] * 3
        res = st.bend_list(lr, lst, ltags, count=max(1, n // 2))
        assert sum(res) <= max(1, n // 2)                                             # (the centre on an unbent voice counts nothing)
        res = st.bend_list(lr, lst, ltags)
        assert sum(res) <= n and res[2] == (1 if n > 1 else 0)
        res = st.bend_list(lr, lst, ltags, count=5000)
        st.block()
        st.bend_clear(False, (0, max(1, n // 3)))
        st.bend_clear(True, (n // 3, n - n // 3))
        assert not st.bend.any()
        assert st.wheel(CHAN, ONE) == [0, 0, n // 2], "the centre on voices that are not bent stores nothing and counts nothing"
        take = min(n, 40)
        res = st.bend_tags(mixed_ratios(gen, take), tags[perm[:take]], (0, n))
        assert res[0] + res[1] <= take and res[2] == 0
        st.wheel((0, 0), ONE)                                                          # everyone's wheel to the centre
        assert not st.bend.any()
        st.block()
    finally:
        st.close()


def test_tag_counts_holes_and_glides_under_the_bend():
    """600 voices, the range [37, 537); 1, 2, 1023 and 1024 tags arriving in no order; then glides of all three forms on a bank where
    most voices are bent, advances of 1, 63, 64, 65 and 65536 frames, stops with and without snap, and bends of gliding voices."""
    st = stage()
    n, first, count = N, FIRST, COUNT
    rng = (first, count)
    heads = np.arange(first, first + count, dtype=np.int32)
    gen = np.random.default_rng(n + 11)
    try:
        tags = ((CH << 24) + 1 + np.arange(len(heads))).astype(np.uint32)
        tagged = np.arange(len(heads)) % 5 != 4
        st.tag(heads[tagged], tags[tagged])
        st.tag([0, n - 1], [(CH << 24) | 0xFFFF, (CH << 24) | 0xFFFE])
        own, own_tags = heads[tagged], tags[tagged]
        edge_increments(st, own[::23])
        order = gen.permutation(len(own))
        at = 0
        for m in (1, 2, 1023, 1024):
            pick = order[at:at + min(m, 150)]
            at += len(pick)
            t = padded_tags(own_tags[pick], m)
            p = gen.permutation(m)
            res = st.bend_tags(mixed_ratios(gen, m)[p], t[p], rng)                   # the ratios must follow their tags through the sort
            assert res[0] + res[1] <= len(pick) and res[2] == 0
        assert st.bend_tags([ONE + 9], [(CH << 24) | 0xFFFF], rng) == [0, 0, 0]      # carried below the range only
        assert int((st.bend[:, KEY] != 0).sum()) > 100
        st.block()
        for m in (1, 2, 1023, 1024):
            pick = gen.permutation(len(own))[:min(m, 120)]
            t = padded_tags(own_tags[pick], m)
            p = gen.permutation(m)
            gl = mixed_glides(gen, m)
            res = st.start([gl[k] for k in p], t[p], rng)
            assert res[0] + res[1] == len(pick) and res[2] == 0
        both = (st.bend[:, KEY] != 0) & (st.glide[:, 0] != 0)
        assert int(both.sum()) > 20, "voices that glide under a bend"
        for frames in (1, 63, 64):
            st.advance(frames, rng)
        st.block()
        st.wheel(CHAN, BM.ratio_of(-1.0), rng)                                        # the wheel moves while they glide
        for frames in (65, 65536, 64):
            st.advance(frames, rng)
        st.advance(64, (first, 1))
        st.block()
        st.stop(False, (first, 100))
        st.stop(True, (first + 100, count - 100))
        st.stop(True)
        assert not st.glide.any()
        st.wheel(CHAN, ONE)
        assert not st.bend.any()
        st.block()
    finally:
        st.close()


def test_three_workgroups_feed_the_counts():
    """3 x SK_CONTROL_SPAN + 7 voices: every workgroup of the channel wheel and of the per-entry call holds stored, withheld and
    unmatched voices, and the result words are exact.  Two calls in a row on one stream with no host wait in between."""
    n = 3 * SPAN + 7
    st = stage(n, stems=False)
    try:
        v = np.arange(n, dtype=np.int32)
        tags = (((v % 3 == 0) + CH).astype(np.uint32) << np.uint32(24)) | (1 + v).astype(np.uint32)   # every third voice on channel 4
        st.tag(v, tags)
        edge_increments(st, v[1::50])                                                 # channel 3 voices with products that do not fit
        up = BM.ratio_of(24.0)                                                        # x 4: withheld at and above 2^30
        want = BM.bend_match(st.owner.copy(), st.bend.copy(), st.inc.copy(), 0, n, CHAN, up)
        for g in range(3):
            probe = BM.bend_match(st.owner.copy(), st.bend.copy(), st.inc.copy(), g * SPAN, SPAN, CHAN, up)
            assert all(c > 0 for c in probe), (g, probe)
        assert st.wheel(CHAN, up) == want
        lst = v.copy()
        ltags = tags.copy()
        ltags[5::40] ^= np.uint32(0x00800000)                                         # owners that differ, in every workgroup
        bufs = [dev_i32(5) for _ in range(2)]
        dl = dev_list(lst)
        sync()
        for b in bufs:
            st.db.bend_owned_each(np.full(n, BM.ratio_of(36.0), np.uint32), dl.data_ptr(), ltags, 0, b.data_ptr())
        one = BM.bend_owned_each(st.owner, st.bend, st.inc, [BM.ratio_of(36.0)] * n, lst, ltags)
        two = BM.bend_owned_each(st.owner, st.bend, st.inc, [BM.ratio_of(36.0)] * n, lst, ltags)
        sync()
        assert one == two and all(c > 3 for c in one)
        for b, w in zip(bufs, (one, two)):
            assert host_of(b).view(np.uint32).tolist()[:3] == w and host_of(b).tolist()[3:] == [FILL, FILL]
        st.same("two per-entry bends")
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- twins

def test_wheel_up_wheel_to_centre_is_a_never_bent_twin():
    st = stage()
    twin = open_fx(st.bank, st.pool, st.now())
    try:
        v = np.arange(N, dtype=np.int32)
        tags = ((v % 16).astype(np.uint32) << np.uint32(24)) | (1 + v // 16).astype(np.uint32)
        st.tag(v, tags)
        dl = dev_list(v)
        twin.tag_list(dl.data_ptr(), tags)
        gen = np.random.default_rng(5)
        for k in range(40):
            res = st.wheel(CHAN, int(mixed_ratios(gen, 1)[0]) if k % 7 else BM.ratio_of(0.01 * k))
        st.wheel(CHAN, BM.ratio_of(1.0))
        st.block()                                                                     # the bent bank sounds another block
        twin.render_host(st.F, st.INTERP)
        res = st.wheel(CHAN, ONE)
        assert res[0] > 30 and res[1] == 0 and not st.bend.any()
        assert np.array_equal(st.inc, st.bank["phase_inc"]), "the centre gives every key's bits"
        for name in ("phase_inc",):
            got = whole_bank(twin, st.truth)
            assert np.array_equal(got[name], st.truth[name])
        # the phase a voice ran through under the bend is state: the twin takes it over, then the next block is bit-identical
        twin.upload(st.truth)
        mix, stems = st.block()
        got_mix, got_stems = twin.render_host(st.F, st.INTERP, want_stems=True)
        assert (got_mix == mix).all() and (got_stems == stems).all()
        assert_same_bank(whole_bank(twin, st.truth), st.truth, "the never-bent twin")
        assert not twin.download_bend().any()
    finally:
        st.close()
        twin.close()


def test_a_bent_chord_against_the_oracle_and_a_twin_driven_by_ctl_list():
    """Eight notes on a channel under a moving wheel; a twin never bends and receives the model's increments through
    skred_fxbank_ctl_list(SKRED_CTL_PHASE_INC) ahead of every block.  Mixes and stems are bit-equal, and both equal the oracle's."""
    st = stage()
    twin = open_fx(st.bank, st.pool, st.now())
    try:
        voices = np.array([5, 63, 64, 255, 256, 300, 511, 599], np.int32)
        tags = ((CH << 24) + 60 + np.arange(len(voices))).astype(np.uint32)
        st.tag(voices, tags)
        for k in range(10):
            if k < 8:
                assert st.wheel(CHAN, BM.ratio_of(2.0 * np.sin(k / 2.0) + 0.01))[0] == len(voices)
            elif k == 8:
                assert st.bend_tags([BM.ratio_of(-1.0 + 0.3 * j) for j in range(len(voices))], tags) == [len(voices), 0, 0]
            else:
                assert st.wheel(CHAN, ONE) == [len(voices), 0, N - len(voices)]
            for v in voices:
                one = dev_list([v])
                twin.ctl_list(fxb.fx_ctl(fxb.CTL_PHASE_INC, phase_inc=int(st.inc[v])), one.data_ptr(), 1)
            mix, stems = st.block()                                               # (the device's block is held to the oracle's inside)
            got_mix, got_stems = twin.render_host(st.F, st.INTERP, want_stems=True)
            assert (got_mix == mix).all() and (got_stems == stems).all(), f"block {k}: the twin renders another block"
        assert np.array_equal(st.inc[voices], st.bank["phase_inc"][voices]) and not st.bend.any()
        assert_same_bank(whole_bank(twin, st.truth), st.truth, "the twin")
        assert not twin.download_bend().any()
    finally:
        st.close()
        twin.close()


def test_a_glide_under_a_bend_over_three_block_cuttings():
    """1 500 voices (6 workgroups, the last one partial), every second one bent, 1 024 gliding.  512 frames advanced as 8 x 64, as
    1 x 512 and as 37 + 100 + 27 + 348 on three banks: each held to the model after every call, and to each other.  Then the voices
    that were sent to a known key land on (target * ratio) >> 24, and the centre gives the target's bits."""
    n = 1500
    stages = [stage(n, stems=False) for _ in CUTS]
    try:
        v = np.arange(n, dtype=np.int32)
        tags = (0x03000000 + 1 + v).astype(np.uint32)
        gen = np.random.default_rng(3)
        pick = gen.permutation(n)[:1024]
        glides = mixed_glides(np.random.default_rng(4), 1024)
        up, down = GM.per_64(2000.0)
        known = pick[:64]
        for k in range(64):
            glides[k] = G(GM.TO_INC, up, down, target_inc=30000001 + 977 * k)
        ratio = BM.ratio_of(1.25)
        for st, cut in zip(stages, CUTS):
            st.tag(v, tags)
            res = st.bend_list(np.full(n // 2, ratio, np.uint32), v[::2], tags[::2])
            assert res == [n // 2, 0, 0]
            res = st.start(glides, tags[pick])
            assert res[0] > 500 and res[0] + res[1] == 1024
            for frames in cut:
                st.advance(frames)
        a = stages[0]
        assert int((a.glide[:, 0] != 0).sum()) > 100, "some must still be on the way"
        p = BM.product(a.bend[:, KEY], a.bend[:, RATIO])
        fits = (a.bend[:, KEY] == 0) | ((p >= 1) & (p <= TOP))                     # a withheld re-derived store keeps the last product that fitted
        for st in stages[1:]:
            assert np.array_equal(st.glide, a.glide) and np.array_equal(st.bend, a.bend) and np.array_equal(st.inc[fits], a.inc[fits])
            assert np.array_equal(st.db.download_glide(), a.db.download_glide()) and np.array_equal(st.db.download_bend(), a.db.download_bend())
        for _ in range(40):
            if not a.glide[known, 0].any():
                break
            a.advance(512)
        want = 30000001 + 977 * np.arange(64)
        bent = known % 2 == 0
        assert not a.glide[known, 0].any() and bent.sum() > 10 and (~bent).sum() > 10
        assert np.array_equal(a.inc[known], np.where(bent, (want * ratio) >> 24, want)), "a glide under a bend lands on (target * ratio) >> 24"
        a.wheel((0, 0), ONE, (0, n))
        assert np.array_equal(a.inc[known], want) and not a.bend.any(), "the centre gives the target's bits"
        a.block()
    finally:
        for st in stages:
            st.close()


def test_calls_that_move_nothing_leave_the_bank_and_the_render_alone():
    """Bend calls that move nothing -- the centre on unbent voices, a match nobody satisfies, foreign tags, clears over nothing --
    leave every byte of the bank and the rendered blocks identical to a twin without them; a bank that never bends downloads zeros."""
    st = stage()
    bare = open_fx(st.bank, st.pool, st.now())
    try:
        bare.bend_clear(0, N, True)                                                     # no array: nothing to do
        assert not bare.download_bend().any() and not bare.download_owners().any()
        voices = np.arange(100, 140, dtype=np.int32)
        tags = ((CH << 24) + 1 + np.arange(40)).astype(np.uint32)
        dl = dev_list(voices)
        bare.tag_list(dl.data_ptr(), tags)
        st.tag(voices, tags)
        for k in range(4):
            if k == 1:
                assert st.wheel(CHAN, ONE) == [0, 0, N - 40]
                assert st.wheel(CM.channel(9), BM.ratio_of(2.0)) == [0, 0, N]
                assert st.bend_tags([BM.ratio_of(2.0)] * 3, [0x09000001, 0x09000002, 0x09000003]) == [0, 0, 0]
                assert st.bend_list([BM.ratio_of(1.0), ONE, 7], [100, 101, -1], [0x09000009, int(tags[1]), 5]) == [0, 0, 1]
            if k == 2:
                st.bend_clear(True)
                assert st.advance(64) == [0, 0]
            mix, stems = st.block()
            got_mix, got_stems = bare.render_host(st.F, st.INTERP, want_stems=True)
            assert (got_mix == mix).all() and (got_stems == stems).all(), f"block {k}: the bank without bend calls renders another block"
        assert_same_bank(whole_bank(bare, st.truth), st.truth, "the bank without bend calls")
        assert not st.bend.any() and not bare.download_bend().any()
    finally:
        st.close()
        bare.close()


def test_owner_pedal_glide_and_bend_arrays_at_once():
    """A bank that holds all four side arrays: one tag launch is followed by the pedal, glide and bend clears, each on the tagged
    voices only."""
    st = stage()
    try:
        v = np.arange(200, 232, dtype=np.int32)
        tags = ((CH << 24) + 1 + np.arange(32)).astype(np.uint32)
        st.strike(v, tags)
        pedal = PM.new(N)
        res = dev_i32(6)
        sync()
        st.db.release_tags_pedal(0, N, tags[:20], True, res.data_ptr())                # sustain is down: held back, PENDING
        want, stamped, _ = PM.release_tags_pedal(st.owner, pedal, st.truth, 0, N, tags[:20], True, st.now())
        sync()
        assert want == [0, 0, 0, 20] and host_of(res).tolist() == want + [FILL, FILL]
        assert st.wheel(CHAN, BM.ratio_of(1.0)) == [32, 0, N - 32]
        u, d = GM.per_64(100.0)
        assert st.start([G(GM.FROM_SCALE, u, d, GM.scale_q16(-3))] * 32, tags) == [32, 0, 0]
        assert st.advance(64) == [32, 0]
        assert np.array_equal(st.db.download_pedals(), pedal) and pedal[v[:20]].all()
        st.block()
        again = v[8:24]
        keys = st.bend[again, KEY].copy()
        st.tag(list(again) + [-1, N], list(tags[8:24] + np.uint32(0x100)) + [5, 6])   # new notes on sixteen of the voices
        pedal[again] = 0
        assert np.array_equal(st.db.download_pedals(), pedal), "the pedal words of the tagged voices, and only those"
        assert not st.bend[again].any() and not st.glide[again].any()
        assert st.bend[v[:8]].all() and st.glide[v[:8], 0].all() and st.bend[v[24:]].all() and pedal[v[:8]].all()
        assert st.advance(64) == [16, 0]
        assert st.wheel(CHAN, ONE) == [16, 0, N - 32], "the re-tagged voices have no key to restore"
        assert (st.inc[again] != keys).all()
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- a shard

def test_bends_through_a_shard():
    """One rank, local indices: the channel wheel, bends by id, a glide under the bend and the centre through skred_fxshard_bank()."""
    from skred_amd.sharded import _lib
    b, pool, c0 = fxb.bank_fx(N)
    L = fxb._bind(_lib())
    L.skred_shard_destroy.argtypes = [C.c_void_p]
    L.skred_shard_destroy.restype = None
    h = C.c_void_p()
    assert L.skred_fxshard_create(0, 0, 1, 0, b.n, C.byref(h)) == 0
    try:
        fx = fxb.DeviceFxBank.borrowed(L.skred_fxshard_bank(h), b.n)
        fx.set_tables(pool)
        cb = b.as_c()
        assert L.skred_fxshard_upload(h, C.byref(cb)) == 0
        fx.set_sample_count(c0)
        st = DeviceBendStage(b, pool, c0, db=fx)
        t = [(CH << 24) | (60 + k) for k in range(3)]
        st.strike([63, 64, 256], t)
        assert st.wheel(CHAN, BM.ratio_of(2.0), (FIRST, COUNT)) == [3, 0, COUNT - 3]
        st.block()
        assert st.bend_tags([BM.ratio_of(-1.0), ONE], t[:2], (FIRST, COUNT)) == [2, 0, 0]
        up, down = GM.per_64(300.0)
        assert st.start([G(GM.FROM_SCALE, up, down, GM.scale_q16(-12))], t[2:], (FIRST, COUNT)) == [1, 0, 0]
        assert st.advance(64, (FIRST, COUNT)) == [1, 0]
        st.block()
        st.stop(True)
        st.bend_clear(True, (0, 100))
        assert st.inc[63] == b["phase_inc"][63] and st.inc[64] == b["phase_inc"][64]
        assert st.inc[256] == (int(b["phase_inc"][256]) * BM.ratio_of(2.0)) >> 24
        assert st.wheel(CHAN, ONE) == [1, 0, N - 3] and np.array_equal(st.inc, b["phase_inc"])
        st.block()
    finally:
        L.skred_shard_destroy(h)


# ---------------------------------------------------------------------------------------------- refusals

def test_refusals_write_nothing():
    st = stage()
    n = st.n
    try:
        L = st.db.L
        st.tag([8, 16], [5, 6])
        assert st.bend_tags([BM.ratio_of(1.0)], [5]) == [1, 0, 0]                   # the array exists, voice 8 is bent
        dl = dev_list([8, 16, 24, 32])
        res = dev_i32(4)
        sync()
        good, zero, dup = fxb._tags([5, 6, 7, 8]), fxb._tags([5, 0, 7, 8]), fxb._tags([5, 6, 5, 8])
        ok, bad = fxb.bend_ratios([1, ONE, ONE + 1, TOP]), fxb.bend_ratios([1, ONE, ONE + 1, 0])
        m, never = fxb.OwnerMatchC(int(CHAN[0]), int(CHAN[1])), fxb.OwnerMatchC(1, 0xFF000000)
        h, d, rs, r, t = st.db.h, dl.data_ptr(), res.data_ptr(), ok.ctypes.data, good.ctypes.data
        BMt, BO, BT, BC, DB = (L.skred_fxbank_bend_match, L.skred_fxbank_bend_owned_each, L.skred_fxbank_bend_tags_each,
                               L.skred_fxbank_bend_clear, L.skred_fxbank_download_bend)
        assert BMt(None, 0, n, C.byref(m), ONE + 1, rs, None) == BAD and BMt(h, 0, n, None, ONE + 1, rs, None) == BAD
        assert BMt(h, 0, n, C.byref(m), 0, rs, None) == BAD and BMt(h, 0, n, C.byref(never), ONE + 1, rs, None) == BAD
        assert BMt(h, 0, n + 1, C.byref(m), 2, rs, None) == RANGE and BMt(h, 0, 0, C.byref(m), 2, rs, None) == RANGE
        assert BMt(h, -1, 4, C.byref(m), 2, rs, None) == RANGE and BMt(h, n, 1, C.byref(m), 2, rs, None) == RANGE
        assert BO(None, r, d, t, 4, None, rs, None) == BAD and BO(h, None, d, t, 4, None, rs, None) == BAD
        assert BO(h, r, None, t, 4, None, rs, None) == BAD and BO(h, r, d, None, 4, None, rs, None) == BAD
        assert BO(h, r, d, zero.ctypes.data, 4, None, rs, None) == BAD and BO(h, r, d, t, -1, None, rs, None) == BAD
        assert BO(h, bad.ctypes.data, d, t, 4, None, rs, None) == BAD
        assert BT(None, r, 0, n, t, 4, rs, None) == BAD and BT(h, None, 0, n, t, 4, rs, None) == BAD
        assert BT(h, r, 0, n, dup.ctypes.data, 4, rs, None) == BAD and BT(h, r, 0, n, zero.ctypes.data, 4, rs, None) == BAD
        assert BT(h, bad.ctypes.data, 0, n, t, 4, rs, None) == BAD and BT(h, bad.ctypes.data, 0, n + 1, t, 4, rs, None) == BAD
        assert BT(h, r, 0, n + 1, t, 4, rs, None) == RANGE and BT(h, r, -1, 4, t, 4, rs, None) == RANGE and BT(h, r, 0, 0, t, 4, rs, None) == RANGE
        assert BC(None, 0, n, 1, None) == BAD and BC(h, 8, n, 1, None) == RANGE and BC(h, 0, -1, 1, None) == RANGE
        out = np.full(16, 9, np.uint32)
        assert DB(h, out.ctypes.data, n - 2, 4) == RANGE and DB(h, None, 0, 4) == BAD and DB(h, out.ctypes.data, 0, -1) == BAD
        assert (out == 9).all()
        assert BO(h, r, d, t, 0, None, rs, None) == 0 and BT(h, r, 0, n, t, 0, rs, None) == 0 and BC(h, 0, 0, 1, None) == 0   # nothing to do
        sync()
        assert (host_of(res) == FILL).all()
        st.same("after the refusals")                                             # bend and glide words, owners and every word of the bank
        assert st.bend[8].tolist() == [int(st.bank["phase_inc"][8]), BM.ratio_of(1.0)]
        assert st.wheel((0, 0), ONE) == [1, 0, n - 2]                              # ... and the bank still answers
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- the staging ring

def test_more_bend_calls_than_the_ring_has_slots():
    """3 x SKRED_FX_RING_SLOTS bend_tags_each calls (two slots each) and as many bend_owned_each calls back to back on one stream, no
    host wait in between: a slot that is still in flight is waited for through its own event, and every ratio arrives."""
    st = stage()
    try:
        v = np.arange(N, dtype=np.int32)
        tags = (0x03000001 + v).astype(np.uint32)
        st.tag(v, tags)
        calls = 3 * fxb.FX_RING_SLOTS
        per = 12
        bufs, lists = [dev_i32(5) for _ in range(2 * calls)], []
        sync()
        want = []
        for c in range(calls):
            a = v[c * 2 * per:c * 2 * per + per][::-1].copy()                       # the tags in descending order
            b = v[c * 2 * per + per:(c + 1) * 2 * per]
            ra = [BM.ratio_of(0.1 * (c + 1)) + j for j in range(per)]
            rb = [BM.ratio_of(-0.1 * (c + 1)) - j for j in range(per)]
            lists.append(dev_list(b))
            st.db.bend_tags_each(ra, 0, N, tags[a], bufs[2 * c].data_ptr())
            st.db.bend_owned_each(rb, lists[-1].data_ptr(), tags[b], 0, bufs[2 * c + 1].data_ptr())
            want.append(BM.bend_tags_each(st.owner, st.bend, st.inc, ra, 0, N, tags[a])[0])
            want.append(BM.bend_owned_each(st.owner, st.bend, st.inc, rb, b, tags[b]))
        sync()
        for b, w in zip(bufs, want):
            assert w == [per, 0, 0] and host_of(b).tolist() == w + [FILL, FILL]
        st.same("the run of bends")
        assert int((st.bend[:, KEY] != 0).sum()) == 2 * per * calls
        st.block()
    finally:
        st.close()
