"""Pedals on the device (skred_bank_stamp_owned_pedal / _release_tags_pedal / _pedal_latch / _pedal_up / _pedal_clear /
_download_pedals), byte for byte.

After every call the device is held to tests/pedal_model.py: download_pedals == the model's pedal array and download_owners == its
owner array on every voice, the envelope clocks the bank holds (download_env_clocks) == the oracle's after slot_model's stamps, every
d_result word == the model's count with the guard words past it untouched; state after a rendered block is compared with
oracle.cpuref.  The scenes are tests/pedal_model.py's; tests/test_pedal_cpu.py asserts on the oracle alone that each of them bites.
"""
import ctypes as C

import numpy as np
import pytest

import chan_model as CM
import owner_model as OM
import owner_scenes as OS
import pedal_model as PM
import slot_model as SM
import slot_steal_model as M
from oracle import cpuref
from skred_amd import device
from skred_amd.bank import slot_query
from steal_model import OLDEST, FIN, ENV
from test_idle import open_bank, render_blocks, traffic_bank
from test_slot_steal import plain_bank

REL, TRIG = SM.STAMP_RELEASE, SM.STAMP_TRIGGER
BAD, RANGE = -2, -4
FILL = -7
SUS, SOS, DOWN = PM.LIFT_SUSTAIN, PM.LIFT_SOSTENUTO, PM.SUSTAIN_DOWN


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


class DeviceStage(PM.Stage):
    """pedal_model.Stage with a device bank beside it: every call runs on both, and the device is compared with the model."""

    def __init__(self, dev, bank, tables, g, K, vmask, setup=None):
        super().__init__(bank, tables, g, K, vmask)
        self.db = open_bank(dev, bank, tables, g, setup)
        self.log = []

    def dev_list(self, entries):
        import torch
        return torch.from_numpy(np.array(entries, np.int32)).cuda()

    def result(self, words):
        import torch
        t = torch.full((words + 2,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return t

    def read(self, t, words, what, want):
        import torch
        torch.cuda.synchronize()
        got = t.cpu().numpy()
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
        start, release = self.db.download_env_clocks()
        e = self.truth["voice_amp_envelope"]
        assert start.tobytes() == e["sample_start"].astype(np.uint64).tobytes(), f"{what}: sample_start differs from the model"
        assert release.tobytes() == e["sample_release"].astype(np.uint64).tobytes(), f"{what}: sample_release differs from the model"

    def tag(self, entries, tags, count=None):
        import torch
        dl, res = self.dev_list(entries), self.result(2)
        dc = None if count is None else torch.tensor([count, 4321], dtype=torch.int32, device="cuda")
        self.db.tag_slots(dl.data_ptr(), tags, self.K, dc.data_ptr() if dc is not None else 0, res.data_ptr())
        return self.read(res, 2, "tag_slots", super().tag(entries, tags, count))

    def strike(self, slots, tags):
        dl = self.dev_list(slots)
        self.db.stamp_slots(dl.data_ptr(), len(slots), self.K, self.vmask, TRIG)
        return super().strike(slots, tags)

    def off(self, tags, hold_all, rng=None):
        first, count = rng or self.whole
        res = self.result(4)
        self.db.release_tags_pedal(first, count, self.K, self.vmask, tags, hold_all, res.data_ptr())
        return self.read(res, 4, f"release_tags_pedal hold {hold_all}", super().off(tags, hold_all, rng))

    def off_list(self, entries, tags, hold_all, count=None):
        import torch
        dl, res = self.dev_list(entries), self.result(4)
        dc = None if count is None else torch.tensor([count, 4321], dtype=torch.int32, device="cuda")
        self.db.stamp_owned_pedal(dl.data_ptr(), tags, self.K, self.vmask, hold_all, res.data_ptr(), dc.data_ptr() if dc is not None else 0)
        return self.read(res, 4, f"stamp_owned_pedal hold {hold_all}", super().off_list(entries, tags, hold_all, count))

    def plain_off(self, tags, rng=None):
        first, count = rng or self.whole
        res = self.result(3)
        self.db.release_tags(first, count, self.K, self.vmask, tags, REL, res.data_ptr())
        return self.read(res, 3, "release_tags", super().plain_off(tags, rng))

    def latch(self, match, rng=None):
        first, count = rng or self.whole
        res = self.result(2)
        self.db.pedal_latch(first, count, self.K, self.vmask, device.owner_match(*match), res.data_ptr())
        return self.read(res, 2, f"pedal_latch {match}", super().latch(match, rng))

    def up(self, match, flags, rng=None):
        first, count = rng or self.whole
        res = self.result(3)
        self.db.pedal_up(first, count, self.K, self.vmask, device.owner_match(*match), flags, res.data_ptr())
        return self.read(res, 3, f"pedal_up {match} flags {flags}", super().up(match, flags, rng))

    def pedal_clear(self, first, count):
        self.db.pedal_clear(first, count)
        super().pedal_clear(first, count)
        self.same("pedal_clear")

    def block(self):
        render_blocks(self.db, (self.F,))
        ref = super().block()
        a = self.bank.copy()
        self.db.download(a)
        assert not a.rw_equal(self.truth), f"state differs from the oracle: {a.rw_equal(self.truth)}"
        self.same("a block")
        return ref

    def close(self):
        self.db.close()


def padded_tags(tags, n):
    """`tags` first, then distinct tags nobody carries (every other one at or above 2^31), n in all."""
    extra = [(0x40000000 + 3 * k) | (0x80000000 if k & 1 else 0) for k in range(n - len(tags))]
    assert not set(extra) & set(int(t) for t in tags)
    return np.array(list(tags) + extra, np.uint32)[:n]


# ---------------------------------------------------------------------------------------------- the scenes

@pytest.mark.gpu
@pytest.mark.parametrize("name", PM.SCENES)
def test_scene_on_the_device(dev, name):
    """Scenes (a) .. (f) on tests/owner_scenes.py's bank: 3.sk tiled over 256 voices, K = 4."""
    bank, tables, g = OS.bank()
    st = DeviceStage(dev, bank, tables, g, OS.K, OS.VMASK)
    try:
        assert not st.db.download_pedals().any()                                   # no pedal call yet: zeros
        PM.run_scene(name, st, [int(x) for x in OS.others()[:8]])
        assert st.db.list_violations() == 0
    finally:
        st.close()


@pytest.mark.gpu
def test_scene_b_through_note_on_channel(dev):
    """Mono mode (cap 1, min_age 0): the key is struck again through skred_bank_note_on_channel while its note-off is pending, so the
    new note takes the old note's slot in the same block and the call's own tag launch is the one that clears the word."""
    import torch
    from test_slots import slot_notes
    bank, tables, g = OS.bank()
    K, N = OS.K, OS.N
    st = DeviceStage(dev, bank, tables, g, K, OS.VMASK)
    chan, tag = CM.channel(PM.CH), [PM.tag_of(PM.CH, 60)]
    try:
        slot = int(OS.others()[5])
        st.strike([slot], tag)
        st.block()
        assert st.off(tag, True) == [0, 0, 0, 1] and st.word(slot) == PM.PENDING
        iq = slot_query(0, N, K, OS.MMASK, FIN | ENV, OS.SETTLE, 0, 0)
        sq = M.SlotQuery(0, N, K, OS.MMASK, OLDEST, 0)
        want, res, _ = CM.burst(st.truth, st.now(), st.owner, iq, sq, chan, 1, 1)
        assert want.tolist() == [slot] and res == [1, 0, 1, 1], "the new note must steal the channel's only slot"
        notes = slot_notes(1, K, OS.VMASK, 3, [SM.SET_PHASE])
        da = torch.full((3,), FILL, dtype=torch.int32, device="cuda")
        dr = torch.full((6,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st.db.note_on_channel(notes, tag, iq, sq.c(), device.owner_match(*chan), 1, OS.VMASK, da.data_ptr(), dr.data_ptr())
        SM.store_notes((st.truth,), st.truth, notes, K, OS.VMASK, want, st.now())
        PM.tag_slots(st.owner, st.pedal, want, tag, None, K)
        torch.cuda.synchronize()
        assert da.cpu().numpy().tolist() == [slot, FILL, FILL] and dr.cpu().numpy().tolist() == res + [FILL, FILL]
        assert st.word(slot) == 0
        st.same("the re-strike")
        st.block()
        assert st.up(chan, SUS) == [0, 0, N // K - 1]
        assert st.release_clock(slot) == 0, "the pedal-up released a key that is still down"
        st.block()
    finally:
        st.close()


@pytest.mark.gpu
def test_a_chord_sustained_across_a_theft(dev):
    """tests/owner_scenes.py's story on the 3.sk bank with a pedal in it: chord A's note-off is held back, the bank fills up, chord B
    steals six of A's eight slots -- its tag launch clears their bits -- and the pedal-up releases the two notes A still has."""
    import torch
    story = OS.Story()
    st = DeviceStage(dev, story.bank, story.tables, story.g, OS.K, OS.VMASK)
    st.truth, st.gl, st.owner = story.truth, story.gl, story.owner                # the story's oracle is the stage's
    K, N = OS.K, OS.N
    try:
        want_a, _ = story.chord_a()
        da = torch.full((len(want_a),), FILL, dtype=torch.int32, device="cuda")
        dr = torch.full((3,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st.db.note_on_idle_slots(story.a_notes, OS.idle_q(), OS.VMASK, da.data_ptr(), dr.data_ptr())
        st.db.tag_slots(da.data_ptr(), OS.A_TAGS, K)
        st.block()
        assert st.off_list(want_a, OS.A_TAGS, True) == [0, 0, 0, 8]                # A's keys are lifted under the pedal
        dl = st.dev_list(OS.others())
        st.db.stamp_slots(dl.data_ptr(), len(OS.others()), K, OS.MMASK, TRIG)
        st.db.tag_slots(dl.data_ptr(), OS.c_tags(), K)
        story.fill_up()
        st.block()
        want_b, counts, _ = story.chord_b()
        dab = torch.full((OS.B_COUNT,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st.db.note_on_steal_slots(story.b_notes, OS.idle_q(), OS.steal_q().c(), OS.VMASK, dab.data_ptr(), dr.data_ptr())
        st.db.tag_slots(dab.data_ptr(), OS.B_TAGS, K)
        st.pedal[want_b] = 0                                                       # the thief's tag launch clears its victims' bits
        torch.cuda.synchronize()
        assert np.array_equal(dab.cpu().numpy(), want_b) and counts == (OS.B_COUNT, 0, OS.B_COUNT)
        stolen = sorted(set(want_a.tolist()) & set(want_b.tolist()))
        assert len(stolen) == OS.B_COUNT and int((st.pedal != 0).sum()) == len(want_a) - OS.B_COUNT
        st.same("chord B")
        st.block()
        t_up = st.now()
        assert st.up((0, 0), SUS) == [len(want_a) - OS.B_COUNT, 0, 0]
        for s in want_a.tolist():
            assert st.release_clock(s) == (0 if s in stolen else t_up), s
        st.block()
        assert st.off(OS.B_TAGS, False) == [OS.B_COUNT, 0, 0, 0]
        st.block()
        assert st.db.list_violations() == 0
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- every call against the model

# (n voices, K, first voice of the range): the range runs to the end of the bank, starts off a 64-voice boundary (K = 64: at 64) and
# crosses the 256-thread workgroup span of the range kernels; the list kernels' workgroups hold 256 / K entries
SHAPES = [(600, 1, 37), (600, 2, 38), (1500, 8, 40), (1500, 64, 64), (600, 8, 0), (1500, 1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,first", SHAPES)
def test_every_call_against_the_model(dev, n, K, first):
    bank, tables, g, now = plain_bank(n)
    vmask = 1 if K == 1 else (1 << (K - 1)) | 1                                   # the first and the last voice of a slot
    st = DeviceStage(dev, bank, tables, g, K, vmask)
    count = (n - n % K) - first
    rng = (first, count)
    heads = np.arange(first, first + count, K, dtype=np.int32)
    gen = np.random.default_rng(n + K)
    try:
        # two channels interleaved, every fifth slot untagged; a slot below the range carries a tag of channel CH too
        chans = np.where(np.arange(len(heads)) % 2 == 0, PM.CH, PM.OTHER)
        tags = np.array([PM.tag_of(int(c), 1 + k) for k, c in enumerate(chans)], np.uint32)
        tagged = np.arange(len(heads)) % 5 != 4
        st.tag(heads[tagged], tags[tagged])
        if first > 0:
            st.tag([0], [PM.tag_of(PM.CH, 0xFFFF)])
        ch = heads[tagged & (chans == PM.CH)]
        ch_tags = tags[tagged & (chans == PM.CH)]
        some = gen.permutation(len(ch))
        # note-offs by id: 1, 2, 1023 and 1024 tags (the list beyond the channel's notes: tags nobody carries), held back
        for m in (1, 2, 1023, 1024):
            pick = some[:min(m, len(ch) // 3)]
            res = st.off(padded_tags(ch_tags[pick], m), True, rng)
            assert res[3] == len(pick) and res[0] == 0 and res[2] == m - len(pick)
        # sostenuto: every held note of the channel that is not pending; a note released before is not caught
        gone = some[len(ch) // 3:len(ch) // 3 + 2]
        assert st.plain_off(ch_tags[gone], rng)[0] == 2
        res = st.latch(CM.channel(PM.CH), rng)
        assert res[0] == len(ch) - len(ch) // 3 - 2 and res[1] == len(heads) - len(ch)
        assert st.latch(CM.channel(PM.CH), rng) == res                            # the same state gives the same counts
        # note-offs on a list with holes, a stolen slot (wrong tag), an untagged slot and a slot named twice; a count shorter than n
        kept = some[len(ch) // 3 + 2:]
        lst = [int(ch[kept[0]]), -1, int(ch[kept[1]]), int(heads[4]), n, int(ch[kept[0]]), int(ch[some[0]]), int(heads[1])]
        ltags = [int(ch_tags[kept[0]]), 5, 0x7FFFFFFF, 6, 7, int(ch_tags[kept[0]]), int(ch_tags[some[0]]), int(tags[1])]
        assert st.off_list(lst, ltags, False, count=7) == [1, 2, 2, 2]             # latched: held back without hold_all; pending alone: stamped
        assert st.off_list(lst, ltags, False) == [2, 2, 2, 2]                      # the other channel's note is stamped at once
        st.block()
        # sustain up: everything pending that sostenuto does not keep
        res = st.up(CM.channel(PM.CH), SUS, rng)
        assert res == [len(ch) // 3, 1, len(heads) - len(ch)]
        res = st.up(CM.channel(PM.CH), SOS | DOWN, (first, K))                     # a range of one slot
        res = st.up((0, 0), SOS | DOWN, rng)
        assert res[0] == 0 and res[1] == 1
        res = st.up((int(ch_tags[kept[0]]), 0xFFFFFFFF), SUS | SOS, rng)           # one note
        assert res == [1, 0, len(heads) - 1]
        st.block()
        st.pedal_clear(first, K)
        st.pedal_clear(0, n)
        assert not st.pedal.any() and st.db.list_violations() == 0
    finally:
        st.close()


@pytest.mark.gpu
def test_many_workgroups_feed_the_counts(dev):
    """70 000 voices, K = 2: 137 workgroups of the range kernels add to the result words.  Each call runs twice in a row on one stream
    with no host wait in between: the second starts from result words the stream cleared again."""
    import torch
    n, K, vmask = 70000, 2, 3
    bank, tables, g, now = plain_bank(n)
    st = DeviceStage(dev, bank, tables, g, K, vmask)
    try:
        heads = np.arange(0, n, K, dtype=np.int32)
        k = np.arange(len(heads))
        tags = np.where(k % 3 == 1, PM.tag_of(PM.OTHER, 1), PM.tag_of(PM.CH, 1)).astype(np.uint32) + (k.astype(np.uint32) << 4)
        st.tag(heads, tags)
        down = k % 7 == 0
        res = st.off_list(heads[down], tags[down], True)
        assert res == [0, 0, 0, int(down.sum())]
        match = device.owner_match(*CM.channel(PM.CH))
        # latch twice
        bufs = [torch.full((4,), FILL, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for b in bufs:
            st.db.pedal_latch(0, n, K, vmask, match, b.data_ptr())
        want = PM.latch(st.owner, st.pedal, st.truth, 0, n, K, vmask, CM.channel(PM.CH))
        torch.cuda.synchronize()
        assert want[0] == int(((k % 3 != 1) & ~down).sum()) and want[1] == int((k % 3 == 1).sum())
        for b in bufs:
            assert b.cpu().numpy().tolist() == want + [FILL, FILL], (b.cpu().numpy().tolist(), want)
        st.same("two latches")
        # both pedals up twice: the first call releases, the second finds nothing
        torch.cuda.synchronize()
        bufs = [torch.full((5,), FILL, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for b in bufs:
            st.db.pedal_up(0, n, K, vmask, match, SUS | SOS, b.data_ptr())
        first, _ = PM.up(st.owner, st.pedal, st.truth, 0, n, K, vmask, CM.channel(PM.CH), SUS | SOS, st.now())
        second, _ = PM.up(st.owner, st.pedal, st.truth, 0, n, K, vmask, CM.channel(PM.CH), SUS | SOS, st.now())
        torch.cuda.synchronize()
        assert first[0] == int(((k % 3 != 1) & down).sum()) > 1000 and second[0] == 0
        for b, w in zip(bufs, (first, second)):
            assert b.cpu().numpy().tolist() == w + [FILL, FILL], (b.cpu().numpy().tolist(), w)
        st.same("two pedal-ups")
        assert int((st.pedal != 0).sum()) == int(((k % 3 == 1) & down).sum())      # the other channel's notes are still pending
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- twins

@pytest.mark.gpu
def test_twins_that_hold_nothing(dev):
    """tests/test_slots.py's in-place bank (4096 voices, two per lane, SKRED_OPT_IN_PLACE = 2).  One bank lifts its chords through the
    pedal calls with hold_all = 0 and nothing latched, and lifts pedals that hold nothing; a twin is driven by skred_bank_stamp_owned /
    _release_tags (and skred_bank_stamp_match where the other lifts a pedal: the same bound for the planner); a third bank receives
    the tags and the trigger stamps and no pedal call at all until the chords end.  Result words 0 .. 2, bank bytes, mix, kernel
    family, the in-place choice and the violation counter agree in every block."""
    import torch
    n, K, mask, F = 4096, 8, 0xFE, 64
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    st = DeviceStage(dev, bank, tables, g, K, mask, setup)
    twin, bare = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    nobody = device.owner_match(*CM.channel(99))
    try:
        chords = {1: np.arange(0, 40 * K, 2 * K, dtype=np.int32), 3: np.arange(1024, 1024 + 12 * K, K, dtype=np.int32)}
        tagged, taken = {}, []
        for k in range(7):
            if k in chords:
                slots = chords[k]
                tags = (0x80000000 + 100 * k + np.arange(len(slots))).astype(np.uint32)
                dl = st.dev_list(slots)
                for d in (twin, bare):
                    d.stamp_slots(dl.data_ptr(), len(slots), K, mask, TRIG)
                    d.tag_slots(dl.data_ptr(), tags, K)
                st.strike(slots, tags)
                tagged[k] = (slots, tags, dl)
            r3, r2 = st.result(3), st.result(2)
            if k == 2:                                                            # chord 1 is lifted through its list
                slots, tags, dl = tagged[1]
                assert st.off_list(slots, tags, False) == [len(slots), 0, 0, 0]
                twin.stamp_owned(dl.data_ptr(), tags, K, mask, REL, r3.data_ptr())
                bare.stamp_slots(dl.data_ptr(), len(slots), K, mask, REL)
                torch.cuda.synchronize()
                assert r3.cpu().numpy()[:3].tolist() == [len(slots), 0, 0]
            if k == 4:                                                            # pedals that hold nothing go down and up
                assert st.latch(CM.channel(99)) == [0, n // K]
                assert st.up(CM.channel(99), SUS | SOS) == [0, 0, n // K]
                twin.stamp_match(0, n, K, mask, nobody, REL, r2.data_ptr())
                bare.stamp_match(0, n, K, mask, nobody, REL, r2.data_ptr())
            if k == 5:                                                            # chord 3 by id
                slots, tags, dl = tagged[3]
                assert st.off(tags, False) == [len(slots), 0, 0, 0]
                twin.release_tags(0, n, K, mask, tags, REL, r3.data_ptr())
                bare.stamp_slots(dl.data_ptr(), len(slots), K, mask, REL)
                torch.cuda.synchronize()
                assert r3.cpu().numpy()[:3].tolist() == [len(slots), 0, 0]
            x, y, z = (render_blocks(d, (F,))[0] for d in (st.db, twin, bare))
            cpuref.render(st.truth, st.gl, st.tables, F, 0)
            taken.append((st.db.last_in_place(), twin.last_in_place(), bare.last_in_place()))
            assert x.tobytes() == y.tobytes() == z.tobytes(), f"block {k}: the mixes differ"
            assert st.db.last_kernel() == twin.last_kernel() == bare.last_kernel() == 3 and len(set(taken[-1])) == 1, (k, taken)
            a, b, c = bank.copy(), bank.copy(), bank.copy()
            st.db.download(a), twin.download(b), bare.download(c)
            assert not a.rw_equal(b) and not a.rw_equal(c) and not a.rw_equal(st.truth), (a.rw_equal(b), a.rw_equal(c), a.rw_equal(st.truth))
            for d in (twin, bare):
                assert np.array_equal(d.download_env_clocks()[1], st.db.download_env_clocks()[1])
            assert st.db.list_violations() == twin.list_violations() == bare.list_violations() == 0
        assert not twin.download_pedals().any() and not bare.download_pedals().any() and not st.pedal.any()
        print(f"in place per block: {taken}")
    finally:
        st.close()
        twin.close()
        bare.close()


# ---------------------------------------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_write_nothing(dev):
    import torch
    n, K = 256, 8
    bank, tables, g, now = plain_bank(n)
    st = DeviceStage(dev, bank, tables, g, K, 0xFF)
    try:
        L = st.db.L
        st.tag([8, 16], [5, 6])
        assert st.off([5], True) == [0, 0, 0, 1]                                   # the pedal array exists, slot 8 is pending
        assert st.latch((6, 0xFFFFFFFF)) == [1, n // K - 1]
        dl = st.dev_list([8, 16, 24, 32])
        res = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        good, zero, dup = device.tag_array([5, 6, 7, 8]), device.tag_array([5, 0, 7, 8]), device.tag_array([5, 6, 5, 8])
        m, bad_m = device.owner_match(0, 0), device.owner_match(1, 0xFF000000)
        h, d, rs = st.db.h, dl.data_ptr(), res.data_ptr()
        SO, RT, LA, UP = L.skred_bank_stamp_owned_pedal, L.skred_bank_release_tags_pedal, L.skred_bank_pedal_latch, L.skred_bank_pedal_up
        assert SO(None, d, good.ctypes.data, 4, None, K, 0xFF, 1, rs, None) == BAD
        assert SO(h, None, good.ctypes.data, 4, None, K, 0xFF, 1, rs, None) == BAD
        assert SO(h, d, good.ctypes.data, 4, None, K, 0xFF, 1, None, None) == BAD
        assert SO(h, d, None, 4, None, K, 0xFF, 1, rs, None) == BAD
        assert SO(h, d, zero.ctypes.data, 4, None, K, 0xFF, 1, rs, None) == BAD
        assert SO(h, d, good.ctypes.data, -1, None, K, 0xFF, 1, rs, None) == BAD
        assert SO(h, d, good.ctypes.data, 4, None, K, 0x1FF, 1, rs, None) == BAD
        assert SO(h, d, good.ctypes.data, 4, None, K, 0, 1, rs, None) == BAD
        assert SO(h, d, good.ctypes.data, 4, None, 12, 0xFF, 1, rs, None) == RANGE
        assert RT(h, 0, n, K, 0xFF, dup.ctypes.data, 4, 1, rs, None) == BAD
        assert RT(h, 0, n, K, 0xFF, zero.ctypes.data, 4, 1, rs, None) == BAD
        assert RT(h, 0, n, K, 0xFF, good.ctypes.data, 4, 1, None, None) == BAD
        assert RT(h, 0, n, K, 0x1FF, good.ctypes.data, 4, 1, rs, None) == BAD
        assert RT(h, 0, n, 3, 0x7, good.ctypes.data, 4, 1, rs, None) == RANGE
        assert RT(h, 4, 8, K, 0xFF, good.ctypes.data, 4, 1, rs, None) == RANGE
        assert RT(h, 0, n + K, K, 0xFF, good.ctypes.data, 4, 1, rs, None) == RANGE
        assert RT(h, 0, 0, K, 0xFF, good.ctypes.data, 4, 1, rs, None) == RANGE
        assert LA(h, 0, n, K, 0xFF, None, rs, None) == BAD and LA(h, 0, n, K, 0xFF, C.byref(bad_m), rs, None) == BAD
        assert LA(h, 0, n, K, 0xFF, C.byref(m), None, None) == BAD and LA(None, 0, n, K, 0xFF, C.byref(m), rs, None) == BAD
        assert LA(h, 0, n, K, 0, C.byref(m), rs, None) == BAD and LA(h, 0, n, 5, 1, C.byref(m), rs, None) == RANGE
        assert LA(h, 4, 8, K, 0xFF, C.byref(m), rs, None) == RANGE and LA(h, 0, 0, K, 0xFF, C.byref(m), rs, None) == RANGE
        assert LA(h, K, n, K, 0xFF, C.byref(m), rs, None) == RANGE
        for flags in range(16):
            want = PM.up_flags_check(flags)
            if want:
                assert UP(h, 0, n, K, 0xFF, C.byref(m), flags, rs, None) == want, flags
        assert UP(h, 0, n, K, 0xFF, None, SUS, rs, None) == BAD and UP(h, 0, n, K, 0xFF, C.byref(bad_m), SUS, rs, None) == BAD
        assert UP(h, 0, n, K, 0xFF, C.byref(m), SUS, None, None) == BAD and UP(None, 0, n, K, 0xFF, C.byref(m), SUS, rs, None) == BAD
        assert UP(h, 0, n, K, 0x100, C.byref(m), SUS, rs, None) == BAD and UP(h, 0, n, 64 * 2, 1, C.byref(m), SUS, rs, None) == RANGE
        assert UP(h, 0, n - 4, K, 0xFF, C.byref(m), SUS, rs, None) == RANGE and UP(h, n, K, K, 0xFF, C.byref(m), SUS, rs, None) == RANGE
        assert L.skred_bank_pedal_clear(h, 8, n, None) == RANGE and L.skred_bank_pedal_clear(h, 0, -1, None) == RANGE
        out = np.full(4, 9, np.uint32)
        assert L.skred_bank_download_pedals(h, out.ctypes.data, n - 2, 4) == RANGE and L.skred_bank_download_pedals(h, None, 0, 4) == BAD
        assert (out == 9).all()
        for call in (lambda: SO(h, d, good.ctypes.data, 0, None, K, 0xFF, 1, rs, None), lambda: RT(h, 0, n, K, 0xFF, good.ctypes.data, 0, 1, rs, None)):
            assert call() == 0                                                    # n == 0: nothing is done
        torch.cuda.synchronize()
        assert (res.cpu().numpy() == FILL).all()
        st.same("after the refusals")                                             # pedal words, owners and clocks as they were
        assert st.word(8) == PM.PENDING and st.word(16) == PM.LATCHED
        assert st.up((0, 0), SUS | SOS) == [1, 0, n // K - 2]                      # ... and the bank still answers
    finally:
        st.close()
