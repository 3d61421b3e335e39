"""Pedals on the fixed-point bank on the GPU (skred_fxbank_stamp_owned_pedal / _release_tags_pedal / _pedal_latch / _pedal_up /
_pedal_clear / _download_pedals), byte for byte.

After every call the device is held to tests/fx_pedal_model.py: download_pedals == the model's pedal array and download_owners == its
owner array on every voice, every word of the bank (skred_fxbank_download and _download_params, the time plane among them) == the
oracle's after fx_live_model's stamps, every d_result word == the model's count with the guard words past it untouched; mixes and
stems of every rendered block are compared bit for bit with oracle.cpuref.fx_render.  The scenes are tests/pedal_model.py's, the float
bank's, unchanged; tests/test_fx_pedal_cpu.py asserts on the oracle alone that each of them bites.
"""
import ctypes as C

import numpy as np
import pytest

import chan_model as CM
import fx_chan_model as FCM
import fx_live_model as live
import fx_pedal_model as FP
import fx_steal_model as sm
import pedal_model as PM
from skred_amd import device, fxbank as fxb
from test_fx_chan import assert_same_bank, whole_bank
from test_fx_live import dev_i32, host_of, open_fx
from test_fx_pedal_cpu import SCENE_VOICES

pytestmark = pytest.mark.gpu

REL, TRIG = fxb.STAMP_RELEASE, fxb.STAMP_TRIGGER
BAD, RANGE = -2, -4
FILL = -7
SUS, SOS, DOWN = FP.LIFT_SUSTAIN, FP.LIFT_SOSTENUTO, FP.SUSTAIN_DOWN
N, FIRST, COUNT = 600, 37, 500                                  # the range starts off a 64-lane boundary and crosses a 256-thread workgroup edge


def sync():
    import torch
    torch.cuda.synchronize()


def dev_list(entries):
    import torch
    return torch.from_numpy(np.array(entries, np.int32)).cuda()


def dev_count(count):
    import torch
    return None if count is None else torch.tensor([count, 4321], dtype=torch.int32, device="cuda")


def ptr(t):
    return t.data_ptr() if t is not None else 0


class DeviceFxStage(FP.FxStage):
    """fx_pedal_model.FxStage with a device bank beside it: every call runs on both, and the device is compared with the model."""

    def __init__(self, bank, pool, c0, db=None, stems=True):
        super().__init__(bank, pool, c0)
        self.db = db if db is not None else open_fx(bank, pool, c0)
        self.stems = stems

    def result(self, words):
        t = dev_i32(words + 2)
        sync()
        return t

    def read(self, t, words, what, want):
        sync()
        got = host_of(t)
        assert (got[words:] == FILL).all(), f"{what}: words past d_result were written"
        got = got[:words].view(np.uint32).tolist()
        print(f"{what}: d_result {got}, the model {want}")
        assert got == want, f"{what}: d_result {got}, the model says {want}"
        self.same(what)
        return want

    def same(self, what):
        for name, got, want in (("pedal", self.db.download_pedals(), self.pedal), ("owner", self.db.download_owners(), self.owner)):
            bad = np.flatnonzero(got != want)
            assert not len(bad), f"{what}: {name} words differ at {bad[:8].tolist()}: {got[bad[:8]].tolist()} / {want[bad[:8]].tolist()}"
        assert_same_bank(whole_bank(self.db, self.truth), self.truth, what)

    def tag(self, entries, tags, count=None):
        dl, dc, res = dev_list(entries), dev_count(count), self.result(2)
        self.db.tag_list(dl.data_ptr(), tags, ptr(dc), res.data_ptr())
        return self.read(res, 2, "tag_list", super().tag(entries, tags, count))

    def strike(self, slots, tags):
        dl = dev_list(slots)
        self.db.stamp_list(dl.data_ptr(), len(slots), TRIG)
        return super().strike(slots, tags)

    def off(self, tags, hold_all, rng=None):
        first, count = rng or self.whole
        res = self.result(4)
        self.db.release_tags_pedal(first, count, tags, hold_all, res.data_ptr())
        return self.read(res, 4, f"release_tags_pedal hold {hold_all}", super().off(tags, hold_all, rng))

    def off_list(self, entries, tags, hold_all, count=None):
        dl, dc, res = dev_list(entries), dev_count(count), self.result(4)
        self.db.stamp_owned_pedal(dl.data_ptr(), tags, hold_all, res.data_ptr(), ptr(dc))
        return self.read(res, 4, f"stamp_owned_pedal hold {hold_all}", super().off_list(entries, tags, hold_all, count))

    def plain_off(self, tags, rng=None):
        first, count = rng or self.whole
        res = self.result(3)
        self.db.release_tags(first, count, tags, REL, res.data_ptr())
        return self.read(res, 3, "release_tags", super().plain_off(tags, rng))

    def latch(self, match, rng=None):
        first, count = rng or self.whole
        res = self.result(2)
        self.db.pedal_latch(first, count, match[0], match[1], res.data_ptr())
        return self.read(res, 2, f"pedal_latch {match}", super().latch(match, rng))

    def up(self, match, flags, rng=None):
        first, count = rng or self.whole
        res = self.result(3)
        self.db.pedal_up(first, count, match[0], match[1], flags, res.data_ptr())
        return self.read(res, 3, f"pedal_up {match} flags {flags}", super().up(match, flags, rng))

    def pedal_clear(self, first, count):
        self.db.pedal_clear(first, count)
        super().pedal_clear(first, count)
        self.same("pedal_clear")

    def block(self):
        got_mix, got_stems = self.db.render_host(self.F, self.INTERP, want_stems=self.stems)
        mix, stems = super().block()
        assert (got_mix == mix).all(), "the mix differs from the oracle's"
        if self.stems:
            assert (got_stems == stems).all(), "the stems differ from the oracle's"
        assert self.db.sample_count() == self.now()
        self.same("a block")
        return mix, stems

    def close(self):
        self.db.close()


def stage(n=N, **kw):
    bank, pool, c0 = fxb.bank_fx(n)
    return DeviceFxStage(bank, pool, c0, **kw)


def padded_tags(tags, n):
    """`tags` first, then distinct tags nobody carries (every other one at or above 2^31), n in all."""
    extra = [(0x40000000 + 3 * k) | (0x80000000 if k & 1 else 0) for k in range(n - len(tags))]
    assert not set(extra) & set(int(t) for t in tags)
    return np.array(list(tags) + extra, np.uint32)[:n]


# ---------------------------------------------------------------------------------------------- the scenes

@pytest.mark.parametrize("name", PM.SCENES)
def test_scene_on_the_device(name):
    """The float bank's scenes (a) .. (f), unchanged, on 600 voices of the bank_fx recipe at one voice per slot."""
    st = stage()
    try:
        assert not st.db.download_pedals().any()                                   # no pedal call yet: zeros
        PM.run_scene(name, st, SCENE_VOICES)
    finally:
        st.close()


def mono_args(n, ch):
    iq = fxb.FxIdleQueryC(0, n, fxb.IDLE_ENV_DONE, 0, 0, 0)
    return iq, sm.Query(0, n, sm.OLDEST, 0, 0, max_out=1), CM.channel(ch)


def test_scene_b_through_note_on_channel():
    """Mono mode (cap 1, min_age 0): the key is struck again through skred_fxbank_note_on_channel while its note-off is pending, so the
    new note takes the old note's voice in the same block and the call's own tag launch is the one that clears the word."""
    st = stage()
    tag, v = [PM.tag_of(PM.CH, 60)], 300
    try:
        st.strike([v], tag)
        st.block()
        assert st.off(tag, True) == [0, 0, 0, 1] and st.word(v) == FP.PENDING
        iq, sq, chan = mono_args(st.n, PM.CH)
        want, res, _ = FCM.burst(st.truth, st.now(), st.owner, iq, sq, chan, 1, 1)
        assert want.tolist() == [v] and res == [1, 0, 1, 1], "the new note must steal the channel's only voice"
        notes = [fxb.FxNoteC(3000017, 20000, 0x01234567, 700, 32000, fxb.NOTE_SET_PHASE | fxb.NOTE_SET_PAN)]
        da, dr = dev_i32(3), dev_i32(6)
        sync()
        st.db.note_on_channel(notes, iq, sq.c(), chan[0], chan[1], 1, tag, da.data_ptr(), dr.data_ptr())
        live.place_notes(st.truth, notes, want, 1, 0, st.now())
        FP.tag_list(st.owner, st.pedal, want, tag)
        sync()
        assert host_of(da).tolist() == [v, FILL, FILL] and host_of(dr).tolist() == res + [FILL, FILL]
        assert st.word(v) == 0
        st.same("the re-strike")
        st.block()
        assert st.up(chan, SUS) == [0, 0, st.n - 1]
        assert st.release_clock(v) == 0, "the pedal-up released a key that is still down"
        st.block()
    finally:
        st.close()


def test_a_chord_sustained_across_a_theft():
    """A full bank (every voice sounds, none is idle).  Chord A's note-offs are held back; a burst of the same channel at its cap
    steals six of A's eight voices -- the thief's tags clear their bits --; the pedal-up releases the two notes A still has, and A's
    later note-offs find six tags that nobody carries."""
    st = stage()
    a_voices = [40, 63, 64, 200, 255, 256, 400, 599]
    a_tags = [PM.tag_of(PM.CH, 60 + k) for k in range(8)]
    b_tags = [PM.tag_of(PM.CH, 80 + k) for k in range(6)]
    try:
        st.strike(a_voices, a_tags)
        st.block()
        assert st.off_list(a_voices, a_tags, True) == [0, 0, 0, 8]
        st.block()
        iq, sq, chan = mono_args(st.n, PM.CH)
        want, res, idle = FCM.burst(st.truth, st.now(), st.owner, iq, sq, chan, 8, 6)
        assert idle == 0 and res == [6, 0, 6, 8] and set(want.tolist()) < set(a_voices)
        notes = [fxb.FxNoteC(3000017 + 40009 * i, 20000 + 23 * i, (0x01234567 * (i + 1)) & 0xFFFFFFFF, 700, 32000, fxb.NOTE_SET_PHASE)
                 for i in range(6)]
        da, dr = dev_i32(8), dev_i32(6)
        sync()
        st.db.note_on_channel(notes, iq, sq.c(), chan[0], chan[1], 8, b_tags, da.data_ptr(), dr.data_ptr())
        live.place_notes(st.truth, notes, want, 6, 0, st.now())
        FP.tag_list(st.owner, st.pedal, want, b_tags)                              # the thief's tag launch clears its victims' bits
        sync()
        assert host_of(da).tolist() == want.tolist() + [FILL, FILL] and host_of(dr).tolist() == res + [FILL, FILL]
        assert int((st.pedal != 0).sum()) == 2
        st.same("chord B")
        st.block()
        t_up = st.now()
        assert st.up(chan, SUS) == [2, 0, st.n - 8]
        for v in a_voices:
            assert st.release_clock(v) == (0 if v in want.tolist() else t_up), v
        st.block()
        assert st.off(a_tags, False) == [2, 0, 6, 0]                               # the victims' note-offs: nobody carries the tag
        assert st.off(b_tags, False) == [6, 0, 0, 0]
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- every call against the model

def test_every_call_against_the_model():
    """600 voices, the range [37, 537); lists with -1 holes, a voice beyond the bank, an untagged voice, a stolen voice, an entry named
    twice and a d_count below n; 1, 2, 1023 and 1024 tags."""
    st = stage()
    n, first, count = N, FIRST, COUNT
    rng = (first, count)
    heads = np.arange(first, first + count, dtype=np.int32)
    gen = np.random.default_rng(n + 1)
    try:
        # two channels interleaved, every fifth voice untagged; a voice below the range carries a tag of channel CH too
        chans = np.where(np.arange(len(heads)) % 2 == 0, PM.CH, PM.OTHER)
        tags = np.array([PM.tag_of(int(c), 1 + k) for k, c in enumerate(chans)], np.uint32)
        tagged = np.arange(len(heads)) % 5 != 4
        st.tag(heads[tagged], tags[tagged])
        st.tag([0, n - 1], [PM.tag_of(PM.CH, 0xFFFF), PM.tag_of(PM.CH, 0xFFFE)])
        ch = heads[tagged & (chans == PM.CH)]
        ch_tags = tags[tagged & (chans == PM.CH)]
        some = gen.permutation(len(ch))
        third = len(ch) // 3
        # note-offs by id: 1, 2, 1023 and 1024 tags (the list beyond the channel's notes: tags nobody carries), held back
        for m in (1, 2, 1023, 1024):
            pick = some[:min(m, third)]
            res = st.off(padded_tags(ch_tags[pick], m), True, rng)
            assert res[3] == len(pick) and res[0] == 0 and res[2] == m - len(pick)
        assert st.off([PM.tag_of(PM.CH, 0xFFFF)], True, rng) == [0, 0, 1, 0]       # carried below the range only
        # sostenuto: every held note of the channel that is not pending; a note released before is not caught
        gone = some[third:third + 2]
        assert st.plain_off(ch_tags[gone], rng)[0] == 2
        res = st.latch(CM.channel(PM.CH), rng)
        assert res[0] == len(ch) - third - 2 and res[1] == len(heads) - len(ch)
        assert st.latch(CM.channel(PM.CH), rng) == res                            # the same state gives the same counts
        # note-offs on a list with holes, a stolen voice (wrong tag), an untagged voice and a voice named twice; a count shorter than n
        kept = some[third + 2:]
        lst = [int(ch[kept[0]]), -1, int(ch[kept[1]]), int(heads[4]), n, int(ch[kept[0]]), int(ch[some[0]]), int(heads[1])]
        ltags = [int(ch_tags[kept[0]]), 5, 0x7FFFFFFF, 6, 7, int(ch_tags[kept[0]]), int(ch_tags[some[0]]), int(tags[1])]
        assert st.off_list(lst, ltags, False, count=7) == [1, 2, 2, 2]             # latched: held back without hold_all; pending alone: stamped
        assert st.off_list(lst, ltags, False) == [2, 2, 2, 2]                      # the other channel's note is stamped at once
        assert st.off_list(lst, ltags, False, count=5000) == [2, 2, 2, 2]          # a count above n
        st.block()
        # sustain up: everything pending that sostenuto does not keep
        assert st.up(CM.channel(PM.CH), SUS, rng) == [third, 1, len(heads) - len(ch)]
        st.up(CM.channel(PM.CH), SOS | DOWN, (first, 1))                           # a range of one voice
        res = st.up((0, 0), SOS | DOWN, rng)
        assert res[0] == 0 and res[1] == 1
        assert st.up((int(ch_tags[kept[0]]), 0xFFFFFFFF), SUS | SOS, rng) == [1, 0, len(heads) - 1]
        st.block()
        st.pedal_clear(first, 1)
        st.pedal_clear(0, n)
        assert not st.pedal.any()
    finally:
        st.close()


def test_many_workgroups_feed_the_counts():
    """70 000 voices on 16 channels, one channel's pedal: 274 workgroups of the range kernels add to the result words, which are exact.
    Each call runs twice in a row on one stream with no host wait in between: the same state gives the same answer, and the second
    starts from result words the stream cleared again."""
    n = 70000
    st = stage(n, stems=False)
    try:
        v = np.arange(n, dtype=np.int32)
        tags = ((v % 16).astype(np.uint32) << np.uint32(24)) | (1 + v // 16).astype(np.uint32)
        chan = CM.channel(PM.CH)
        mine = v % 16 == PM.CH
        st.tag(v, tags)
        down = v % 7 == 0
        # the list call, twice: the second finds the bits set and answers the same
        dl = dev_list(v[down])
        bufs = [dev_i32(6) for _ in range(2)]
        sync()
        for b in bufs:
            st.db.stamp_owned_pedal(dl.data_ptr(), tags[down], True, b.data_ptr())
        want = FP.stamp_owned_pedal(st.owner, st.pedal, st.truth, v[down], tags[down], None, True, st.now())[0]
        sync()
        assert want == [0, 0, 0, int(down.sum())]
        for b in bufs:
            assert host_of(b).tolist() == want + [FILL, FILL], (host_of(b).tolist(), want)
        st.same("two held-back lists")
        # latch twice
        bufs = [dev_i32(4) for _ in range(2)]
        sync()
        for b in bufs:
            st.db.pedal_latch(0, n, chan[0], chan[1], b.data_ptr())
        want = FP.latch(st.owner, st.pedal, st.truth, 0, n, chan)
        sync()
        assert want == [int((mine & ~down).sum()), int((~mine).sum())] and want[0] > 3000
        for b in bufs:
            assert host_of(b).tolist() == want + [FILL, FILL], (host_of(b).tolist(), want)
        st.same("two latches")
        # note-offs by id, twice, on a latched channel without hold_all: held back both times
        ids = tags[mine & ~down][:1024]
        bufs = [dev_i32(6) for _ in range(2)]
        sync()
        for b in bufs:
            st.db.release_tags_pedal(0, n, ids, False, b.data_ptr())
        want = FP.release_tags_pedal(st.owner, st.pedal, st.truth, 0, n, ids, False, st.now())[0]
        sync()
        assert want == [0, 0, 0, 1024]
        for b in bufs:
            assert host_of(b).tolist() == want + [FILL, FILL], (host_of(b).tolist(), want)
        st.same("two note-offs by id")
        # both pedals up twice: the first call releases, the second finds nothing
        bufs = [dev_i32(5) for _ in range(2)]
        sync()
        for b in bufs:
            st.db.pedal_up(0, n, chan[0], chan[1], SUS | SOS, b.data_ptr())
        one, _ = FP.up(st.owner, st.pedal, st.truth, 0, n, chan, SUS | SOS, st.now())
        two, _ = FP.up(st.owner, st.pedal, st.truth, 0, n, chan, SUS | SOS, st.now())
        sync()
        assert one == [int((mine & down).sum()) + 1024, 0, int((~mine).sum())] and two == [0, 0, one[2]]
        for b, w in zip(bufs, (one, two)):
            assert host_of(b).tolist() == w + [FILL, FILL], (host_of(b).tolist(), w)
        st.same("two pedal-ups")
        assert int((st.pedal != 0).sum()) == int((~mine & down).sum())             # the other channels' notes are still pending
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- twins

def test_twins_that_hold_nothing():
    """One bank lifts its chords through the pedal calls with hold_all = 0 and nothing latched, and moves pedals that hold nothing; a
    twin is driven by skred_fxbank_stamp_owned / _release_tags; a third receives the tags and the stamps and no pedal call at all.
    Result words 0 .. 2, every word of the bank, mixes and stems agree in every block; the banks without a pedal array download
    zeros."""
    st = stage()
    twin, bare = open_fx(st.bank, st.pool, st.now()), open_fx(st.bank, st.pool, st.now())
    try:
        chords = {1: np.arange(3, 250, 7, dtype=np.int32), 3: np.arange(256, 268, dtype=np.int32)}
        tagged = {}
        for k in range(7):
            if k in chords:
                voices = chords[k]
                tags = (0x80000000 + 100 * k + np.arange(len(voices))).astype(np.uint32)
                dl = dev_list(voices)
                for d in (twin, bare):
                    d.stamp_list(dl.data_ptr(), len(voices), TRIG)
                    d.tag_list(dl.data_ptr(), tags)
                st.strike(voices, tags)
                tagged[k] = (voices, tags, dl)
            r3 = dev_i32(5)
            if k == 2:                                                            # chord 1 is lifted through its list
                voices, tags, dl = tagged[1]
                assert st.off_list(voices, tags, False) == [len(voices), 0, 0, 0]
                twin.stamp_owned(dl.data_ptr(), tags, REL, r3.data_ptr())
                bare.stamp_list(dl.data_ptr(), len(voices), REL)
                sync()
                assert host_of(r3).tolist() == [len(voices), 0, 0, FILL, FILL]
            if k == 4:                                                            # pedals that hold nothing go down and up
                assert st.latch(CM.channel(99)) == [0, st.n]
                assert st.up(CM.channel(99), SUS | SOS) == [0, 0, st.n]
                assert st.up((0, 0), SUS | SOS) == [0, 0, st.n - len(chords[1]) - len(chords[3])]
            if k == 5:                                                            # chord 3 by id
                voices, tags, dl = tagged[3]
                assert st.off(tags, False, (FIRST, COUNT)) == [len(voices), 0, 0, 0]
                twin.release_tags(FIRST, COUNT, tags, REL, r3.data_ptr())
                bare.stamp_list(dl.data_ptr(), len(voices), REL)
                sync()
                assert host_of(r3).tolist() == [len(voices), 0, 0, FILL, FILL]
            mix, stems = st.block()                                               # (the device's block is held to the oracle's inside)
            for d, who in ((twin, "the twin"), (bare, "the bank without a pedal call")):
                got_mix, got_stems = d.render_host(st.F, st.INTERP, want_stems=True)
                assert (got_mix == mix).all() and (got_stems == stems).all(), f"block {k}: {who} renders another block"
                assert_same_bank(whole_bank(d, st.truth), st.truth, f"block {k}, {who}")
                assert np.array_equal(d.download_owners(), st.owner)
        assert not twin.download_pedals().any() and not bare.download_pedals().any() and not st.pedal.any()
        twin.pedal_clear()                                                         # nothing to do on a bank without the array
        assert not twin.download_pedals(FIRST, COUNT).any()
    finally:
        st.close()
        twin.close()
        bare.close()


# ---------------------------------------------------------------------------------------------- a shard

def test_pedals_through_a_shard():
    """One rank, local indices: a held-back note-off, the latch and the pedal-up through skred_fxshard_bank()."""
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
        st = DeviceFxStage(b, pool, c0, db=fx)
        t = [PM.tag_of(PM.CH, 60 + k) for k in range(3)]
        st.strike([63, 64, 256], t)
        st.block()
        assert st.latch(CM.channel(PM.CH), (FIRST, COUNT)) == [3, COUNT - 3]
        assert st.off(t[:2], False, (FIRST, COUNT)) == [0, 0, 0, 2]
        assert st.off(t[2:], True) == [0, 0, 0, 1]
        st.block()
        assert st.up(CM.channel(PM.CH), SOS | DOWN) == [0, 3, st.n - 3]
        assert st.up(CM.channel(PM.CH), SUS, (FIRST, COUNT)) == [3, 0, COUNT - 3]
        assert st.release_clock(256) == st.now()
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
        assert st.off([5], True) == [0, 0, 0, 1]                                   # the pedal array exists, voice 8 is pending
        assert st.latch((6, 0xFFFFFFFF)) == [1, n - 1]
        dl = dev_list([8, 16, 24, 32])
        res = dev_i32(4)
        sync()
        good, zero, dup = fxb._tags([5, 6, 7, 8]), fxb._tags([5, 0, 7, 8]), fxb._tags([5, 6, 5, 8])
        m, bad_m = device.owner_match(0, 0), device.owner_match(1, 0xFF000000)
        h, d, rs = st.db.h, dl.data_ptr(), res.data_ptr()
        SO, RT, LA, UP = L.skred_fxbank_stamp_owned_pedal, L.skred_fxbank_release_tags_pedal, L.skred_fxbank_pedal_latch, L.skred_fxbank_pedal_up
        assert SO(None, d, good.ctypes.data, 4, None, 1, rs, None) == BAD
        assert SO(h, None, good.ctypes.data, 4, None, 1, rs, None) == BAD
        assert SO(h, d, good.ctypes.data, 4, None, 1, None, None) == BAD
        assert SO(h, d, None, 4, None, 1, rs, None) == BAD
        assert SO(h, d, zero.ctypes.data, 4, None, 1, rs, None) == BAD
        assert SO(h, d, good.ctypes.data, -1, None, 1, rs, None) == BAD
        assert RT(h, 0, n, dup.ctypes.data, 4, 1, rs, None) == BAD
        assert RT(h, 0, n, zero.ctypes.data, 4, 1, rs, None) == BAD
        assert RT(h, 0, n, good.ctypes.data, 4, 1, None, None) == BAD
        assert RT(None, 0, n, good.ctypes.data, 4, 1, rs, None) == BAD
        assert RT(h, 0, n + 1, good.ctypes.data, 4, 1, rs, None) == RANGE
        assert RT(h, -1, 4, good.ctypes.data, 4, 1, rs, None) == RANGE
        assert RT(h, 0, 0, good.ctypes.data, 4, 1, rs, None) == RANGE
        assert LA(h, 0, n, None, rs, None) == BAD and LA(h, 0, n, C.byref(bad_m), rs, None) == BAD
        assert LA(h, 0, n, C.byref(m), None, None) == BAD and LA(None, 0, n, C.byref(m), rs, None) == BAD
        assert LA(h, 0, 0, C.byref(m), rs, None) == RANGE and LA(h, 1, n, C.byref(m), rs, None) == RANGE
        for flags in range(16):
            want = FP.up_flags_check(flags)
            if want:
                assert UP(h, 0, n, C.byref(m), flags, rs, None) == want, flags
        assert UP(h, 0, n, None, SUS, rs, None) == BAD and UP(h, 0, n, C.byref(bad_m), SUS, rs, None) == BAD
        assert UP(h, 0, n, C.byref(m), SUS, None, None) == BAD and UP(None, 0, n, C.byref(m), SUS, rs, None) == BAD
        assert UP(h, 0, n + 1, C.byref(m), SUS, rs, None) == RANGE and UP(h, n, 1, C.byref(m), SUS, rs, None) == RANGE
        assert L.skred_fxbank_pedal_clear(h, 8, n, None) == RANGE and L.skred_fxbank_pedal_clear(h, 0, -1, None) == RANGE
        out = np.full(4, 9, np.uint32)
        assert L.skred_fxbank_download_pedals(h, out.ctypes.data, n - 2, 4) == RANGE and L.skred_fxbank_download_pedals(h, None, 0, 4) == BAD
        assert (out == 9).all()
        assert SO(h, d, good.ctypes.data, 0, None, 1, rs, None) == 0 and RT(h, 0, n, good.ctypes.data, 0, 1, rs, None) == 0   # n == 0
        sync()
        assert (host_of(res) == FILL).all()
        st.same("after the refusals")                                             # pedal words, owners and every word of the bank
        assert st.word(8) == FP.PENDING and st.word(16) == FP.LATCHED
        assert st.up((0, 0), SUS | SOS) == [1, 0, n - 2]                           # ... and the bank still answers
        st.block()
    finally:
        st.close()
