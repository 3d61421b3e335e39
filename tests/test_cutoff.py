"""Filter cutoff on the device (skred_bank_cutoff_match / _cutoff_owned_each / _cutoff_tags_each / _cutoff_advance / _cutoff_stop /
_download_cutoff), byte for byte.

After every call the device is held to tests/cutoff_model.py: download_cutoff == the model's eight words per voice; every controller
word of every voice (download_ctl: the five coefficient words and their neighbours velocity, smoothing and cz_distortion among them)
== the oracle's bank, which receives the model's coefficient stores; the owner, pedal, glide and bend words and the envelope clocks as
tests/test_bend.py's rig holds them; every d_result word == the model's count with the guard words past it untouched.  Blocks are
compared with oracle.cpuref.  Every w, q and product stays inside the box or is exactly 0, infinite or 3e38 (clamped or withheld).

The assertions marked CLEAR RULE fail on tests/cutoff_model.py with CLEAR_RULE = False -- and on a library whose tag launch does not
clear the cutoff words the device fails them against the model as it stands.
"""
import ctypes as C

import numpy as np
import pytest

import bend_model as BM
import cutoff_model as M
import ctl_model as CM
import glide_model as GM
import owner_scenes as OS
import slot_model as SM
from oracle import cpuref
from skred_amd import device
from skred_amd.device import ctl, filter_each
from test_bend import BendRig, strike
from test_cutoff_cpu import filtered
from test_glide import bank_words, banks_same
from test_idle import open_bank, render_blocks, traffic_bank
from test_owner import FILL, padded_tags
from test_slot_steal import plain_bank, playing_patch

F = 64
BAD, RANGE = -2, -4
f32 = np.float32
QM = M.SET_Q | M.SET_MODE
ANY = (0, 0)


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


class CutRig(BendRig):
    """tests/test_bend.py's rig with the model's cutoff words beside the bend words: every call runs on the device and on the model,
    whose coefficient stores go into the oracle's bank."""

    def __init__(self, dev, bank, tables, g, setup=None, db=None):
        super().__init__(dev, bank, tables, g, setup, db)
        self.cut = M.new(bank.n)

    def filt(self):
        return self.truth["voice_filter"]

    def same(self, tag):
        super().same(tag)                                            # (download_ctl against the oracle's bank: the coefficient words)
        got = self.db.download_cutoff()
        bad = np.flatnonzero((got != self.cut).any(axis=1))
        assert not len(bad), f"{tag}: cutoff words differ at {bad[:8].tolist()}: {got[bad[:8]].tolist()} / {self.cut[bad[:8]].tolist()}"

    def tag(self, entries, tags, K, count=None, tag=""):
        M.tag_clear(self.cut, entries, len(tags), count, K)
        super().tag(entries, tags, K, count, tag)

    def cut_match(self, first, count, K, fmask, m, rec, tag=""):
        res = self.result(4)
        self.db.cutoff_match(first, count, K, fmask, device.owner_match(*m), rec.c(), res.data_ptr())
        want = M.cutoff_match(self.owner, self.cut, self.bend, self.inc(), self.filt(), first, count, K, fmask, m, rec)
        return self.check(res, 4, want, tag or "cutoff_match")

    def cut_owned(self, recs, K, fmask, entries, tags, count=None, tag=""):
        import torch
        dl, res = self.dev_list(entries), self.result(4)
        dc = None if count is None else torch.tensor([count, 4321], dtype=torch.int32, device="cuda")
        self.db.cutoff_owned_each([r.c() for r in recs], K, fmask, dl.data_ptr(), tags, dc.data_ptr() if dc is not None else 0, res.data_ptr())
        want = M.cutoff_owned_each(self.owner, self.cut, self.bend, self.inc(), self.filt(), recs, K, fmask, entries, tags, count)
        return self.check(res, 4, want, tag or "cutoff_owned_each")

    def cut_tags(self, recs, first, count, K, fmask, tags, tag=""):
        res = self.result(4)
        self.db.cutoff_tags_each([r.c() for r in recs], first, count, K, fmask, tags, res.data_ptr())
        want, lst = M.cutoff_tags_each(self.owner, self.cut, self.bend, self.inc(), self.filt(), recs, first, count, K, fmask, tags)
        return self.check(res, 4, want, tag or "cutoff_tags_each"), lst

    def cut_advance(self, first, count, frames, tag=""):
        res = self.result(2)
        self.db.cutoff_advance(first, count, frames, res.data_ptr())
        return self.check(res, 2, M.advance(self.cut, self.filt(), first, count, frames), tag or f"cutoff_advance {frames}")

    def cut_stop(self, first, count, snap, tag=""):
        self.db.cutoff_stop(first, count, snap)
        M.stop(self.cut, self.filt(), first, count, snap)
        self.same(tag or f"cutoff_stop snap {snap}")


def sweeps(n, seed=0):
    """n records of every kind: first cutoffs, tracked ones, sweeps up and down, q or mode alone"""
    up, down = M.per_64(50.0)
    kinds = [lambda j: M.Rec(M.ABS | QM, 0.02 + 0.003 * (j % 900), 0.5 + 0.01 * (j % 70), 1 + j % 5),
             lambda j: M.Rec(M.TRACK | QM, 0.01 + 0.002 * (j % 40), 2.0, 1 + j % 5),
             lambda j: M.Rec(M.ABS | M.GLIDE | QM, 2.9 - 0.003 * (j % 900), 0.9, 2, up, down),
             lambda j: M.Rec(M.TRACK | M.GLIDE | M.SET_Q, 0.02 * (1 + j % 9), 8.0, rate_up=1.5, rate_down=0.5),
             lambda j: M.Rec(M.ABS | M.SET_MODE, 1.5707964, mode=4)]
    return [kinds[(k + seed) % 5](k + seed) for k in range(n)]


# ---------------------------------------------------------------------------------------------- 1. every call against the model

@pytest.mark.gpu
@pytest.mark.parametrize("n,K", [(1, 1), (65, 1), (255, 1), (257, 1), (1500, 4), (1472, 64)])
def test_every_call_against_the_model(dev, n, K):
    """Banks of 1, 65, 255 and 257 voices at K = 1, 1500 at K = 4 and 1472 at K = 64.  The channel sweep over the whole bank and, on the
    larger banks, over a range off the workgroup span that takes three workgroups; a filter_mask smaller than the patch's mask; records
    by note id with 1, 2, 1023 and 1024 tags; a list with a hole, a slot past the bank, a stolen slot and a count word; zero, huge and
    tiny increments under TRACK (withheld, clamped); advance in three lengths; stop with and without snap."""
    bank, tables, g, now = plain_bank(n)
    inc = bank["voice_phase_inc"]
    inc[5::23], inc[7::29], inc[13::37] = f32(0.0), f32(3e38), f32(1e-30)
    inc[11::31] *= f32(-1.0)
    r = CutRig(dev, bank, tables, g)
    slots = np.arange(0, n, K, dtype=np.int32)
    full = (1 << K) - 1
    part = full if K == 1 else (1 << (K - 1)) | 1
    gen = np.random.default_rng(70 + n + K)
    try:
        chan = (gen.integers(1, 4, len(slots)).astype(np.uint32) << np.uint32(24))
        all_tags = (chan + np.arange(len(slots), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        if len(slots) > 20:
            all_tags[::17] = 0                                       # untagged slots match nothing
        r.tag(slots, all_tags, K, tag="every slot")
        assert not r.db.download_cutoff().any()
        want = r.cut_match(0, n, K, full, ANY, M.Rec(M.ABS | M.SET_Q, 0.3, 0.9), tag="a first record without a mode")
        assert want[0] == 0 and want[1] == K * int((r.owner[slots] != 0).sum()) and not r.cut.any()
        want = r.cut_match(0, n, K, part, ANY, M.Rec(M.ABS | QM, 0.3, 0.9, 1), tag="every tagged slot, masked")
        assert want[0] > 0 and want[1] == 0
        want = r.cut_match(0, n, K, full, (2 << 24, 0xFF000000), M.Rec(M.TRACK | QM, 0.05, 1.5, 2), tag="channel 2 tracked")
        if n >= 255:
            assert want[1] > 0 and want[3] > 0 and want[2] > 0
        up, down = M.per_64(80.0)
        r.cut_match(0, n, K, full, ANY, M.Rec(M.ABS | M.GLIDE, 2.5, rate_up=up, rate_down=down), tag="a sweep up")
        r.cut_advance(0, n, 64)
        r.block("a block while sweeping")
        if n >= 1472:
            first, count = 36 // K * K, (636 - 36 // K * K) // K * K  # off the 256-voice span at both ends: three workgroups
            assert -(-count // 256) == 3
            want = r.cut_match(first, count, K, full, (1 << 24, 0xFF000000), M.Rec(M.TRACK | M.GLIDE, 0.08, rate_up=1.3, rate_down=0.6), tag="a range off the span")
            assert want[0] > 0 and want[2] > 0
            inside = slots[(slots >= first) & (slots < first + count) & (r.owner[slots] != 0)]
            order = gen.permutation(len(inside))
            at = 0
            for m in (1, 2, 1023, 1024):
                take = min(m, max(1, len(inside) // 5))
                pick = inside[order[at:at + take]]
                at += take
                tags = padded_tags(r.owner[pick], m)[gen.permutation(m)]   # (unsorted: the sort and the permutation have work to do)
                want, lst = r.cut_tags(sweeps(m, m), first, count, K, full if m != 2 else part, tags, tag=f"{m} tags")
                assert int((lst >= 0).sum()) == len(pick) and want[2] == 0 and want[0] > 0
            tagged = slots[r.owner[slots] != 0]
            rest = tagged[~np.isin(tagged, inside[order[:at]])]
            entries = np.array([rest[0], -1, n, rest[1], rest[2], rest[3]], np.int32)
            tags = np.array([r.owner[rest[0]], 5, 6, r.owner[rest[1]] ^ 0x00800000, r.owner[rest[2]], r.owner[rest[3]]], np.uint32)
            before = r.cut[rest[3]:rest[3] + K].copy()
            want = r.cut_owned(sweeps(6, 9), K, part, entries, tags, count=5, tag="a list")
            assert want[2] == 1 and (r.cut[rest[3]:rest[3] + K] == before).all()
        else:
            r.cut_tags(sweeps(1, 3), 0, n, K, full, all_tags[all_tags != 0][:1], tag="one tag")
        for frames in (37, 64, 411):
            r.cut_advance(0, n, frames)
        assert r.cut[:, M.W].any()
        r.cut_stop(0, max(K, (n // 2) // K * K), False)
        r.cut_stop(0, n, True)
        assert not r.cut[:, M.TARGET].any() and r.cut_advance(0, n, 64) == [0, 0]
        r.block("a block after the stop")
        assert r.db.list_violations() == 0
    finally:
        r.close()


@pytest.mark.gpu
def test_three_workgroups_feed_the_counts_and_one_channel_of_four(dev):
    """700 voices, K = 1: three workgroups of the match and advance passes add to the result words; two calls in a row on one stream
    with no host wait in between.  Then a sweep on channel 2 of four: the voices of the other three channels keep every byte."""
    import torch
    n, K = 700, 1
    bank, tables, g, now = plain_bank(n)
    r = CutRig(dev, bank, tables, g)
    try:
        heads = np.arange(n, dtype=np.int32)
        tags = ((np.uint32(1) + (heads % 4).astype(np.uint32) << np.uint32(24)) + heads.astype(np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(heads, tags, K, tag="every voice")
        bufs = [torch.full((6,), FILL, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        a, b = M.Rec(M.ABS | QM, 0.2, 0.9, 1), M.Rec(M.TRACK | M.GLIDE, 0.05, rate_up=1.1, rate_down=0.9)
        r.db.cutoff_match(0, n, K, 1, device.owner_match(*ANY), a.c(), bufs[0].data_ptr())
        r.db.cutoff_match(0, n, K, 1, device.owner_match(*ANY), b.c(), bufs[1].data_ptr())
        first = M.cutoff_match(r.owner, r.cut, r.bend, r.inc(), r.filt(), 0, n, K, 1, ANY, a)
        second = M.cutoff_match(r.owner, r.cut, r.bend, r.inc(), r.filt(), 0, n, K, 1, ANY, b)
        torch.cuda.synchronize()
        assert first == [n, 0, 0, 0] and second[0] == n
        for buf, w in zip(bufs, (first, second)):
            assert buf.cpu().numpy().view(np.uint32).tolist() == w + [FILL & 0xFFFFFFFF] * 2, (buf.cpu().numpy().tolist(), w)
        r.same("two calls")
        assert sum(r.cut_advance(0, n, 64)) == n
        before = bank_words(r.db, bank)
        cut_before = r.cut.copy()
        want = r.cut_match(0, n, K, 1, (2 << 24, 0xFF000000), M.Rec(M.ABS | QM, 1.0, 4.0, 3), tag="channel 2 of four")
        assert want[:3] == [n // 4, 0, n - n // 4]
        after = bank_words(r.db, bank)
        others = np.flatnonzero((r.owner >> 24) != 2)
        for c in M.COEFFS:
            assert after["voice_filter"][c][others].tobytes() == before["voice_filter"][c][others].tobytes(), c
        assert (r.cut[others] == cut_before[others]).all() and (r.db.download_cutoff()[others] == cut_before[others]).all()
        assert set(CM.words_differ(before, after)) <= {"voice_filter." + c for c in M.COEFFS}, CM.words_differ(before, after)
        r.block("after the channel sweep")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 2. cuttings, arrival, twins

@pytest.mark.gpu
@pytest.mark.parametrize("cuts", [(64,) * 8, (512,), (100, 412)])
def test_a_sweep_in_three_cuttings_lands_like_a_twin_set_at_the_target(dev, cuts):
    """512 frames of a sweep up on the even slots and down on the odd ones, in three block cuttings: after 512 frames the device holds
    what the (64,) * 8 model holds, every voice has landed on its target's bits, and its coefficient words equal those of a twin that
    was SET at the target with SKRED_CUTOFF_ABS."""
    n, K = 512, 4
    bank, tables, g, now = plain_bank(n)
    r = CutRig(dev, bank, tables, g)
    twin = open_bank(dev, bank, tables, g)
    try:
        heads = np.arange(0, n, K, dtype=np.int32)
        tags = (np.uint32(3 << 24) + np.arange(len(heads), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(heads, tags, K, tag="every slot")
        twin.tag_slots(r.dev_list(heads).data_ptr(), tags, K)
        even, odd = (3 << 24, 0xFF000001), ((3 << 24) | 1, 0xFF000001)
        r.cut_match(0, n, K, 0xF, even, M.Rec(M.ABS | QM, 0.05, 1.2, 1), tag="low")
        r.cut_match(0, n, K, 0xF, odd, M.Rec(M.ABS | QM, 2.0, 1.2, 1), tag="high")
        up, down = M.per_64(700.0)                                    # an octave per 64 frames: five octaves take five of the eight steps
        r.cut_match(0, n, K, 0xF, even, M.Rec(M.ABS | M.GLIDE, 1.6, rate_up=up, rate_down=down), tag="up")
        r.cut_match(0, n, K, 0xF, odd, M.Rec(M.ABS | M.GLIDE, 0.0625, rate_up=up, rate_down=down), tag="down")
        reference, rfilt = r.cut.copy(), r.filt().copy()
        for _ in range(8):
            M.advance(reference, rfilt, 0, n, 64)
        arrived = 0
        for f in cuts:
            arrived += r.cut_advance(0, n, f)[1]
        assert arrived == n and not r.cut[:, M.TARGET].any()
        assert r.cut.tobytes() == reference.tobytes() and r.filt().tobytes() == rfilt.tobytes(), "the cutting changed the curve"
        assert (r.cut[K:2 * K, M.W] == M.bits(f32(1.6))).all() and (r.cut[0:K, M.W] == M.bits(f32(0.0625))).all()   # (slot 0 carries tag ...1)
        m = device.owner_match
        twin.cutoff_match(0, n, K, 0xF, m(*even), M.Rec(M.ABS | QM, 1.6, 1.2, 1).c())
        twin.cutoff_match(0, n, K, 0xF, m(*odd), M.Rec(M.ABS | QM, 0.0625, 1.2, 1).c())
        banks_same(r.db, twin, bank, "landed against set")
        assert (twin.download_cutoff() == r.cut).all()
        r.block("landed")
    finally:
        r.close()
        twin.close()


@pytest.mark.gpu
def test_a_tracked_chord_against_the_per_entry_coefficient_route(dev):
    """3.sk over 64 copies with its carriers filtered.  Eight notes by note id get a tracked low-pass on their first carrier; a twin
    gets, through skred_bank_ctl_tags_each_filter, the coefficients skred_filter_coeffs_w gives for w = |inc| * value computed on the
    host from the increments the test knows.  Every byte of the two banks' downloads is equal."""
    n = 256
    bank, tables, g, K = playing_patch("3sk", n, (0, 1, 2))
    filtered(bank, K, (0, 1, 2))
    r = CutRig(dev, bank, tables, g)
    twin = open_bank(dev, bank, tables, g)
    try:
        slots = np.arange(0, n, K, dtype=np.int32)[3::7][:8]
        tags = (np.uint32(3 << 24) + np.arange(8, dtype=np.uint32) + np.uint32(60)).astype(np.uint32)
        r.tag(slots, tags, K, tag="the chord")
        twin.tag_slots(r.dev_list(slots).data_ptr(), tags, K)
        value = M.track_value(4.0, int(bank["voice_table_size"][0]))
        recs = [M.Rec(M.TRACK | QM, value, 0.8 + 0.1 * k, 1 + k % 5) for k in range(8)]
        want, lst = r.cut_tags(recs, 0, n, K, 0b0001, tags[::-1].copy(), tag="tracked, by note id")
        assert want == [8, 0, 0, 0]
        filt = []
        for k, s in enumerate(slots[::-1]):
            w = f32(abs(r.inc()[s])) * value
            assert M.W_MIN <= w <= M.W_MAX
            filt.append(filter_each(*device.filter_coeffs_w(recs[k].mode, float(w), float(recs[k].q))))
        twin.ctl_tags_each_filter(None, None, filt, 0, n, 0b0001, 0b0001, tags[::-1].copy(), K)
        banks_same(r.db, twin, bank, "the tracked chord against the host route")
        x, y = render_blocks(r.db, (F,))[0], render_blocks(twin, (F,))[0]
        cpuref.render(r.truth, r.gl, r.tables, F, 0)
        assert x.tobytes() == y.tobytes()
        banks_same(r.db, twin, bank, "a block later")
    finally:
        r.close()
        twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["one voice per lane", "two per lane"])
def test_swept_stems_against_the_oracle(dev, family):
    """A 256-voice bank of either kernel family, six blocks of 64 frames.  Three slots of one channel get a tracked cutoff, then a sweep
    (a new target in block 3); cutoff_advance runs ahead of every block.  The oracle's bank receives the model's coefficients block by
    block; the stems of the three slots through taps and the state of every voice must be the oracle's bit for bit."""
    import torch
    two = family == "two per lane"
    n = 256
    if two:
        K, vmask = 8, 0xFF
        bank, tables, g = traffic_bank(n)
        setup = lambda d: d.fast2_min_voices(0)   # noqa: E731
    else:
        bank, tables, g, K = playing_patch("3sk", n, (0, 1, 2))
        filtered(bank, K, (0, 1, 2))
        vmask = 0b0111
        setup = None
    r = CutRig(dev, bank, tables, g, setup)
    try:
        slots = [4 * K, 21 * K, 31 * K]
        if two:
            dl = r.dev_list(slots)
            r.db.stamp_slots(dl.data_ptr(), len(slots), K, 0xFE, SM.STAMP_TRIGGER)
            SM.stamp(r.truth, SM.stamp_voices(slots, len(slots), None, K, 0xFE, n), SM.STAMP_TRIGGER, r.now())
        tags = np.array([3 << 24 | 60, 3 << 24 | 64, 3 << 24 | 67], np.uint32)
        r.tag(slots, tags, K, tag="the chord")
        voices = np.array([s + l for s in slots for l in range(K)], np.int32)
        assert (r.truth["voice_filter_mode"][voices] != 0).any(), "the chord has no filtered voice"
        d_taps = torch.zeros((F, len(voices), 2), dtype=torch.float32, device="cuda")
        r.db.set_taps(voices, d_taps.data_ptr())
        chan = (3 << 24, 0xFF000000)
        value = f32(0.05) if two else M.track_value(8.0, 4096)
        want = r.cut_match(0, n, K, vmask, chan, M.Rec(M.TRACK | QM, value, 2.0, 1), tag="tracked")
        assert want[0] == 3 * bin(vmask).count("1") and want[1] == 0
        r.cut_match(0, n, K, vmask, chan, M.Rec(M.ABS | M.GLIDE, 2.0, rate_up=1.25, rate_down=0.8), tag="sweep up")
        kernels, differ = set(), 0
        for blk in range(6):
            if blk == 3:
                r.cut_tags([M.Rec(M.ABS | M.GLIDE | M.SET_Q, 0.05, 6.0, rate_up=1.25, rate_down=0.7)], 0, n, K, vmask, tags[1:2], tag="one note back down")
            before = r.filt().copy()
            r.cut_advance(0, n, F, tag=f"advance ahead of block {blk}")
            differ += before.tobytes() != r.filt().tobytes()
            render_blocks(r.db, (F,))
            ref = cpuref.render(r.truth, r.gl, r.tables, F, 0, want_stems=True)
            got = d_taps.cpu().numpy()
            assert r.db.last_taps() == len(voices)
            assert got.tobytes() == np.ascontiguousarray(ref["stems"][:, voices, :]).tobytes(), f"block {blk}: taps differ from the oracle"
            assert np.abs(got).sum() > 0
            kernels.add(r.db.last_kernel())
            a = bank.copy()
            r.db.download(a)
            assert not a.rw_equal(r.truth), f"block {blk}: state differs from the oracle: {a.rw_equal(r.truth)}"
        assert differ >= 4, "the sweep did not move the coefficients"
        assert (kernels == {3}) if two else (3 not in kernels), kernels
        assert r.db.list_violations() == 0
    finally:
        r.db.set_taps([], 0)
        r.close()


# ---------------------------------------------------------------------------------------------- 3. the clear rule

@pytest.mark.gpu
def test_a_thief_and_a_restruck_key_do_not_inherit_a_moving_cutoff(dev):
    """tests/owner_scenes.py's bank.  A key with a moving cutoff is struck again through skred_bank_note_on_channel -- the call's own
    tag launch clears the slot's cutoff words; then a note of another channel takes a slot whose cutoff moves.  In both the next
    advance moves nothing on the slot, the coefficients stay what they were, and the new note's first record needs q and mode."""
    from skred_amd.bank import slot_query
    import slot_steal_model as SSM
    from steal_model import ENV, FIN, OLDEST
    K, N = OS.K, OS.N
    bank, tables, g = OS.bank()
    filtered(bank, K, OS.MEMBERS)
    r = CutRig(dev, bank, tables, g)
    iq = slot_query(0, N, K, OS.MMASK, FIN | ENV, OS.SETTLE, 0, 0)
    sq = SSM.SlotQuery(0, N, K, OS.MMASK, OLDEST, 0)
    try:
        slot, other = int(OS.others()[5]), int(OS.others()[9])
        tag, tag2 = 3 << 24 | 60, 3 << 24 | 72
        r.tag([slot, other], [tag, tag2], K, tag="two keys")
        chan = (3 << 24, 0xFF000000)
        assert r.cut_match(0, N, K, OS.MMASK, chan, M.Rec(M.TRACK | QM, M.track_value(8.0, 4096), 1.1, 1), tag="tracked")[0] == 2 * len(OS.MEMBERS)
        r.cut_match(0, N, K, OS.MMASK, chan, M.Rec(M.ABS | M.GLIDE, 2.2, rate_up=1.1, rate_down=0.9), tag="a slow sweep")
        assert r.cut_advance(0, N, F) == [2 * len(OS.MEMBERS), 0]
        r.block("sweeping")
        held = r.filt()[slot:slot + K].copy()
        strike(r, iq, sq, (tag, 0xFFFFFFFF), tag, 3, slot)
        M.tag_clear(r.cut, [slot], 1, None, K)
        assert not r.cut[slot:slot + K].any()                        # CLEAR RULE
        r.same("the re-strike")                                      # CLEAR RULE (the device's words against the model's)
        assert r.cut_advance(0, N, F) == [len(OS.MEMBERS), 0]        # CLEAR RULE: the struck slot would move too
        assert r.filt()[slot:slot + K].tobytes() == held.tobytes()   # CLEAR RULE: the coefficients stay what they were
        assert r.cut_tags([M.Rec(M.ABS, 0.4)], 0, N, K, OS.MMASK, [tag], tag="no q, no mode")[0][:2] == [0, len(OS.MEMBERS)]   # CLEAR RULE
        # the thief
        held = r.filt()[other:other + K].copy()
        r.tag([other], [5 << 24 | 40], K, tag="the thief's tag")
        assert not r.cut[other:other + K].any()                      # CLEAR RULE
        assert r.cut_advance(0, N, F) == [0, 0]                      # CLEAR RULE
        assert r.filt()[other:other + K].tobytes() == held.tobytes()
        assert r.cut_tags([M.Rec(M.TRACK | QM, M.track_value(3.0, 4096), 0.7, 2)], 0, N, K, OS.MMASK, [5 << 24 | 40], tag="the thief's own cutoff")[0][0] == len(OS.MEMBERS)
        r.block("after the new notes")
        assert r.db.list_violations() == 0
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 4. purity

@pytest.mark.gpu
def test_cutoff_calls_leave_the_planner_alone(dev):
    """tests/test_slots.py's in-place bank (4096 voices, two per lane, SKRED_OPT_IN_PLACE = 2).  Block 0 .. 2: `plain` makes no cutoff
    call; the other bank allocates the array and sends calls that store nothing (a channel nobody is on, first records without a
    mode, advance and stop with nothing moving): the banks stay equal in every byte.  Block 3 ..: a chord sweeps; `plain` receives the
    model's coefficients through skred_bank_ctl_slots(SKRED_CTL_FILTER).  Mix, bank bytes, kernel family, in-place verdict and
    violation counter agree in every block."""
    n, K, mask = 4096, 8, 0xFE
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    r = CutRig(dev, bank, tables, g, setup)
    plain = open_bank(dev, bank, tables, g, setup)
    try:
        chord = np.arange(0, 40 * K, 2 * K, dtype=np.int32)
        tags = (np.uint32(0x03000000) + np.arange(len(chord), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        dl = r.dev_list(chord)
        lists = [r.dev_list([s]) for s in chord]
        taken = []
        for k in range(6):
            if k == 1:
                for d in (r.db, plain):
                    d.stamp_slots(dl.data_ptr(), len(chord), K, mask, SM.STAMP_TRIGGER)
                SM.stamp(r.truth, SM.stamp_voices(chord, len(chord), None, K, mask, n), SM.STAMP_TRIGGER, r.now())
                r.tag(chord, tags, K, tag="the chord")
                plain.tag_slots(dl.data_ptr(), tags, K)
            if 1 <= k < 3:
                before = bank_words(r.db, bank)
                assert r.cut_match(0, n, K, mask, (9 << 24, 0xFF000000), M.Rec(M.ABS | QM, 0.5, 0.9, 1), tag="a channel nobody is on") == [0, 0, n // K, 0]
                assert r.cut_match(0, n, K, mask, ANY, M.Rec(M.ABS | M.SET_Q, 0.5, 0.9), tag="no mode")[0] == 0
                assert r.cut_advance(0, n, F) == [0, 0]
                r.cut_stop(0, n, True)
                after = bank_words(r.db, bank)
                assert not CM.words_differ(before, after) and not before.rw_equal(after), "cutoff calls that store nothing changed the bank"
            if k == 3:
                assert r.cut_match(0, n, K, mask, (3 << 24, 0xFF000000), M.Rec(M.TRACK | QM, 0.05, 1.5, 1), tag="tracked")[0] == 7 * len(chord)
                r.cut_match(0, n, K, mask, (3 << 24, 0xFF000000), M.Rec(M.ABS | M.GLIDE, 2.4, rate_up=1.2, rate_down=0.8), tag="the sweep")
            if k >= 3:
                r.cut_advance(0, n, F)
                fl = r.filt()
                for s, one in zip(chord, lists):
                    plain.ctl_slots([ctl(CM.FILTER, **{c: float(fl[c][s + l]) for c in M.COEFFS}) if (mask >> l) & 1 else ctl(0) for l in range(K)],
                                    mask, one.data_ptr(), 1)
            x, y = render_blocks(r.db, (F,))[0], render_blocks(plain, (F,))[0]
            cpuref.render(r.truth, r.gl, r.tables, F, 0)
            taken.append((r.db.last_kernel(), plain.last_kernel(), r.db.last_in_place(), plain.last_in_place()))
            assert x.tobytes() == y.tobytes(), f"block {k}: the mixes differ"
            assert taken[-1][0] == taken[-1][1] == 3 and taken[-1][2] == taken[-1][3], (k, taken)
            banks_same(r.db, plain, bank, f"block {k}")
            assert r.db.list_violations() == plain.list_violations() == 0
        assert not plain.download_cutoff().any() and r.cut[:, M.W].any()
        print(f"(kernel, plain's, in place, plain's) per block: {taken}")
    finally:
        r.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- 5. every array at once, a shard

@pytest.mark.gpu
def test_all_five_side_arrays_at_once_and_more_calls_than_ring_slots(dev):
    """One bank with owner, pedal, glide, bend and cutoff arrays.  Forty cutoff_tags_each calls back to back with no host wait in
    between -- five times the staging ring's eight slots -- with advances in between, then a tag launch with the four clears behind
    it.  TRACK reads the key of the bent voices."""
    n, K = 512, 4
    bank, tables, g, now = plain_bank(n)
    r = CutRig(dev, bank, tables, g)
    try:
        heads = np.arange(0, n, K, dtype=np.int32)
        tags = (np.uint32(3 << 24) + np.arange(len(heads), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(heads, tags, K, tag="every slot")
        res = r.result(2)
        r.db.pedal_latch(0, n, K, 0xF, device.owner_match(9 << 24, 0xFF000000), res.data_ptr())     # the pedal array exists; nobody matches
        assert r.read(res, 2, "latch") == [0, n // K]
        up, down = GM.per_64(200.0)
        r.start_tags([GM.Glide(GM.TO_SCALE, up, down, 2.0)] * 8, 0, n, K, 0xF, tags[:8], tag="eight glides")
        r.tags_each(BM.ratio_of(np.linspace(0.5, 2.0, 16)), 0, n, K, 0xF, tags[4:20], tag="sixteen bends")
        assert r.bend[:, 0].any()
        want, _ = r.cut_tags([M.Rec(M.TRACK | QM, 0.05, 1.0, 1)] * 24, 0, n, K, 0xF, tags[:24], tag="tracked under the bends")
        assert want[0] == 24 * K
        bent = np.flatnonzero(r.bend[:, 0] != 0)
        assert (r.cut[bent, M.W] == M.bits(np.clip(np.abs(M.flt(r.bend[bent, 0])) * f32(0.05), M.W_MIN, M.W_MAX))).all(), "a bent voice tracks its key"
        assert (r.cut[bent, M.W] != M.bits(np.abs(r.inc()[bent]) * f32(0.05))).any()
        for j in range(40):
            pick = tags[(j * 3) % 100:(j * 3) % 100 + 16]
            recs = sweeps(16, j)
            r.db.cutoff_tags_each([x.c() for x in recs], 0, n, K, 0xF, pick)
            M.cutoff_tags_each(r.owner, r.cut, r.bend, r.inc(), r.filt(), recs, 0, n, K, 0xF, pick)
            if j % 4 == 3:
                r.db.cutoff_advance(0, n, F)
                M.advance(r.cut, r.filt(), 0, n, F)
        r.same("forty cutoff calls")
        r.advance(0, n, F, tag="the glides move")
        r.cut_advance(0, n, F, tag="the cutoffs move")
        assert r.glide[:, 0].any() and r.bend[:, 0].any() and r.cut[:, M.TARGET].any()
        r.tag(heads[:40], tags[:40] + np.uint32(0x1000), K, tag="forty new notes")
        assert not r.cut[:160].any() and not r.bend[:160].any() and not r.glide[:160].any() and r.cut[160:, M.W].any()
        r.block("all five arrays")
    finally:
        r.close()


@pytest.mark.gpu
def test_cutoffs_through_a_shard(dev):
    """One rank, local indices: the channel sweep, a record by note id and an advance through skred_shard_bank()."""
    from skred_amd.sharded import _lib
    n, K = 512, 4
    bank, tables, g, now = plain_bank(n)
    L = _lib()
    h = C.c_void_p()
    assert L.skred_shard_create(0, 0, 1, 0, n, C.byref(h)) == 0
    try:
        db = dev.DeviceBank.borrowed(L.skred_shard_bank(h), n)
        db.set_tables(tables)
        cb = bank.as_c()
        assert L.skred_shard_upload(h, C.byref(cb)) == 0
        db.set_globals(g)
        r = CutRig(dev, bank, tables, g, db=db)
        r.tag([8, 260, 508], [5, 6, 7], K, tag="three slots")
        assert r.cut_match(0, n, K, 0xF, ANY, M.Rec(M.TRACK | QM, 0.05, 0.9, 1), tag="tracked")[:3] == [12, 0, n // K - 3]
        assert r.cut_tags([M.Rec(M.ABS | M.GLIDE, 2.0, rate_up=4.0, rate_down=0.25), M.Rec(M.ABS, 0.7)], 0, n, K, 0xF, [7, 5], tag="by note id")[0][:2] == [8, 0]
        a, b = r.cut_advance(0, n, F), r.cut_advance(0, n, 8 * F)
        assert sum(a) == 4 and a[1] + b[1] == 4 and b[0] == 0
        r.block("a block on the shard's bank")
        r.cut_stop(0, n, True)
        r.block("after the stop")
    finally:
        L.skred_shard_destroy(h)


# ---------------------------------------------------------------------------------------------- 6. refusals

@pytest.mark.gpu
def test_refusals_write_nothing(dev):
    import torch
    n, K = 256, 8
    bank, tables, g, now = plain_bank(n)
    r = CutRig(dev, bank, tables, g)
    try:
        L = r.db.L
        r.tag([8, 16], [5, 6], K, tag="two slots")
        assert r.cut_tags([M.Rec(M.ABS | QM, 0.5, 0.9, 1)], 0, n, K, 0xFF, [5], tag="one cutoff")[0] == [8, 0, 0, 0]
        dl = r.dev_list([8, 16, 24, 32])
        res = torch.full((5,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        good, zero, dup = device.tag_array([5, 6, 7, 8]), device.tag_array([5, 0, 7, 8]), device.tag_array([5, 6, 5, 8])
        ok = device.cutoff_array([M.Rec(M.ABS | QM, 0.3, 0.9, 1).c()] * 4)
        h, d, rs, rp, tp = r.db.h, dl.data_ptr(), res.data_ptr(), C.cast(ok, C.c_void_p), good.ctypes.data
        m, wrong = device.owner_match(0, 0), device.owner_match(1, 0)
        MA, OE, TE, AD, ST, DL = (L.skred_bank_cutoff_match, L.skred_bank_cutoff_owned_each, L.skred_bank_cutoff_tags_each,
                                  L.skred_bank_cutoff_advance, L.skred_bank_cutoff_stop, L.skred_bank_download_cutoff)
        one = M.Rec(M.ABS | QM, 0.3, 0.9, 1).c()
        assert MA(None, 0, n, K, 0xFF, C.byref(m), C.byref(one), rs, None) == BAD and MA(h, 0, n, K, 0xFF, None, C.byref(one), rs, None) == BAD
        assert MA(h, 0, n, K, 0xFF, C.byref(m), None, rs, None) == BAD and MA(h, 0, n, 12, 0xFF, C.byref(m), C.byref(one), rs, None) == RANGE
        assert MA(h, 0, n, K, 0, C.byref(m), C.byref(one), rs, None) == BAD and MA(h, 0, n, K, 0x1FF, C.byref(m), C.byref(one), rs, None) == BAD
        assert MA(h, 4, 8, K, 0xFF, C.byref(m), C.byref(one), rs, None) == RANGE and MA(h, 0, n + K, K, 0xFF, C.byref(m), C.byref(one), rs, None) == RANGE
        assert MA(h, 0, 0, K, 0xFF, C.byref(m), C.byref(one), rs, None) == RANGE and MA(h, 0, n, K, 0xFF, C.byref(wrong), C.byref(one), rs, None) == BAD
        bads = [(M.Rec(M.ABS | M.TRACK, 0.3), BAD), (M.Rec(QM, 0.3, 0.9, 1), BAD), (M.Rec(M.ABS | 64, 0.3), BAD), (M.Rec(M.ABS, 0.3, reserved=(1, 0)), BAD),
                (M.Rec(M.ABS, float("nan")), BAD), (M.Rec(M.ABS, 3.5), RANGE), (M.Rec(M.TRACK, -1.0), RANGE), (M.Rec(M.ABS | M.SET_Q, 0.3, 2000.0), RANGE),
                (M.Rec(M.ABS | M.SET_MODE, 0.3, mode=9), RANGE), (M.Rec(M.ABS | M.GLIDE, 0.3, rate_up=1.0, rate_down=0.5), BAD),
                (M.Rec(M.ABS | M.GLIDE, 0.3, rate_up=2.0, rate_down=1.5), BAD), (M.Rec(M.ABS | M.GLIDE, 0.3, rate_up=20.0, rate_down=0.5), RANGE)]
        for rec, code in bads:
            c = rec.c()
            assert MA(h, 0, n, K, 0xFF, C.byref(m), C.byref(c), rs, None) == code, vars(rec)
            arr = device.cutoff_array([one, one, c, one])
            assert OE(h, C.cast(arr, C.c_void_p), K, 0xFF, d, tp, 4, None, rs, None) == code, vars(rec)
            assert TE(h, C.cast(arr, C.c_void_p), 0, n, K, 0xFF, tp, 4, rs, None) == code, vars(rec)
        assert OE(None, rp, K, 0xFF, d, tp, 4, None, rs, None) == BAD and OE(h, None, K, 0xFF, d, tp, 4, None, rs, None) == BAD
        assert OE(h, rp, K, 0xFF, None, tp, 4, None, rs, None) == BAD and OE(h, rp, K, 0xFF, d, None, 4, None, rs, None) == BAD
        assert OE(h, rp, K, 0xFF, d, zero.ctypes.data, 4, None, rs, None) == BAD and OE(h, rp, K, 0xFF, d, tp, -1, None, rs, None) == BAD
        assert OE(h, rp, K, 0x1FF, d, tp, 4, None, rs, None) == BAD and OE(h, rp, K, 0, d, tp, 4, None, rs, None) == BAD
        assert OE(h, rp, 12, 0xFF, d, tp, 4, None, rs, None) == RANGE
        assert TE(None, rp, 0, n, K, 0xFF, tp, 4, rs, None) == BAD and TE(h, rp, 0, n, K, 0xFF, dup.ctypes.data, 4, rs, None) == BAD
        assert TE(h, rp, 0, n, K, 0xFF, zero.ctypes.data, 4, rs, None) == BAD and TE(h, rp, 0, n, K, 0x1FF, tp, 4, rs, None) == BAD
        assert TE(h, rp, 0, n, 3, 0x7, tp, 4, rs, None) == RANGE and TE(h, rp, 4, 8, K, 0xFF, tp, 4, rs, None) == RANGE
        assert TE(h, rp, 0, n + K, K, 0xFF, tp, 4, rs, None) == RANGE and TE(h, rp, 0, 0, K, 0xFF, tp, 4, rs, None) == RANGE
        assert AD(None, 0, n, F, rs, None) == BAD and AD(h, 0, n, 0, rs, None) == BAD and AD(h, 0, n, 65537, rs, None) == BAD
        assert AD(h, 0, 0, F, rs, None) == RANGE and AD(h, 8, n, F, rs, None) == RANGE
        assert ST(None, 0, n, 1, None) == BAD and ST(h, 8, n, 1, None) == RANGE and ST(h, 0, -1, 0, None) == RANGE
        out = np.full(64, 9, np.uint32)
        assert DL(h, out.ctypes.data, n - 2, 4) == RANGE and DL(h, None, 0, 4) == BAD and DL(None, out.ctypes.data, 0, 4) == BAD
        assert (out == 9).all()
        assert OE(h, rp, K, 0xFF, d, tp, 0, None, rs, None) == 0 and TE(h, rp, 0, n, K, 0xFF, tp, 0, rs, None) == 0 and ST(h, 0, 0, 1, None) == 0
        torch.cuda.synchronize()
        assert (res.cpu().numpy() == FILL).all()
        r.same("after the refusals")
        assert r.cut_match(0, n, K, 0xFF, ANY, M.Rec(M.ABS, 0.8), tag="the bank still answers") == [8, 8, n // K - 2, 0]
        r.block("after the refusals")
    finally:
        r.close()
