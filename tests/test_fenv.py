"""The filter envelope on the device (skred_bank_fenv_match / _fenv_owned_each / _fenv_tags_each / _download_fenv, and the cutoff calls
on a bank that has an fenv array), byte for byte.

After every call the device is held to tests/fenv_model.py on top of tests/cutoff_model.py: download_fenv == the model's eight words
per voice, download_cutoff == the model's cutoff words, every controller word of every voice (download_ctl: the five coefficient
words and their neighbours) == the oracle's bank, which receives the model's coefficient stores; the owner, pedal, glide and bend
words and the envelope clocks likewise; every d_result word == the model's count with the guard words past it untouched.  Blocks are
compared with oracle.cpuref.  The release clock the advance pass reads is the oracle's sample_release, which every stamp of the
control plane moves on the device and on the model together.

The assertions marked CLEAR RULE fail on tests/fenv_model.py with CLEAR_RULE = False, those marked READ THE CLOCK with
READ_RELEASE_CLOCK = False -- and on a library without the rule the device fails them against the model as it stands.
"""
import ctypes as C

import numpy as np
import pytest

import bend_model as BM
import chan_model as CHM
import cutoff_model as M
import ctl_model as CM
import fenv_model as FM
import glide_model as GM
import owner_model as OM
import owner_scenes as OS
import pedal_model as PM
import slot_model as SM
from oracle import cpuref
from skred_amd import device
from test_bend import strike
from test_cutoff import CutRig, sweeps
from test_cutoff_cpu import filtered
from test_fenv_cpu import contours
from test_glide import GlideRig, bank_words, banks_same
from test_idle import open_bank, render_blocks, traffic_bank
from test_owner import FILL, padded_tags
from test_slot_steal import plain_bank, playing_patch

F = 64
BAD, RANGE = -2, -4
f32 = np.float32
QM = M.SET_Q | M.SET_MODE
ANY = (0, 0)
REL, TRIG = SM.STAMP_RELEASE, SM.STAMP_TRIGGER
CONTOUR = FM.Rec(FM.REL, 8.0, 2.0, 1.0, 1.5, 0.9, 0.8)


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


class FenvRig(CutRig):
    """tests/test_cutoff.py's rig with the model's fenv words beside the cutoff words and a pedal array that may be used: every call
    runs on the device and on the model, whose coefficient stores go into the oracle's bank."""

    def __init__(self, dev, bank, tables, g, setup=None, db=None):
        super().__init__(dev, bank, tables, g, setup, db)
        self.fenv, self.pedal = FM.new(bank.n), PM.new(bank.n)

    def rel(self):
        return self.truth["voice_amp_envelope"]["sample_release"]

    def same(self, tag):
        GlideRig.same(self, tag)                                     # owner words, envelope clocks, glide words, increments
        for name, got, want in (("bend", self.db.download_bend(), self.bend), ("cutoff", self.db.download_cutoff(), self.cut),
                                ("fenv", self.db.download_fenv(), self.fenv)):
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), f"{tag}: {name} words differ at {bad[:8].tolist()}: {got[bad[:8]].tolist()} / {want[bad[:8]].tolist()}"
        a = self.bank.copy()
        self.db.download_ctl(a)
        assert not CM.words_differ(a, self.truth), f"{tag}: controller words differ from the model: {CM.words_differ(a, self.truth)}"
        got = self.db.download_pedals()
        assert (got == self.pedal).all(), f"{tag}: pedal words differ at {np.flatnonzero(got != self.pedal)[:8].tolist()}"

    def tag(self, entries, tags, K, count=None, tag=""):
        FM.tag_clear(self.fenv, entries, len(tags), count, K)
        for e in OM.looked(entries, len(tags), count):
            if CM.slot_valid(e, K, self.n):
                self.pedal[e] = 0
        super().tag(entries, tags, K, count, tag)

    # the cutoff calls on a bank with the array: the model's, ending the contours they touch
    def cut_match(self, *a, **k):
        with FM.cutoff_ends(self.fenv):
            return super().cut_match(*a, **k)

    def cut_owned(self, *a, **k):
        with FM.cutoff_ends(self.fenv):
            return super().cut_owned(*a, **k)

    def cut_tags(self, *a, **k):
        with FM.cutoff_ends(self.fenv):
            return super().cut_tags(*a, **k)

    def cut_advance(self, first, count, frames, tag=""):
        res = self.result(2)
        self.db.cutoff_advance(first, count, frames, res.data_ptr())
        return self.check(res, 2, FM.advance(self.cut, self.fenv, self.rel(), self.filt(), first, count, frames), tag or f"cutoff_advance {frames}")

    def cut_stop(self, first, count, snap, tag=""):
        self.db.cutoff_stop(first, count, snap)
        FM.stop(self.cut, self.fenv, self.filt(), first, count, snap)
        self.same(tag or f"cutoff_stop snap {snap}")

    # the record calls
    def fenv_match(self, first, count, K, fmask, m, rec, tag=""):
        res = self.result(4)
        self.db.fenv_match(first, count, K, fmask, device.owner_match(*m), rec.c(), res.data_ptr())
        want = FM.fenv_match(self.owner, self.cut, self.fenv, self.filt(), first, count, K, fmask, m, rec)
        return self.check(res, 4, want, tag or "fenv_match")

    def fenv_owned(self, recs, K, fmask, entries, tags, count=None, tag=""):
        import torch
        dl, res = self.dev_list(entries), self.result(4)
        dc = None if count is None else torch.tensor([count, 4321], dtype=torch.int32, device="cuda")
        self.db.fenv_owned_each([r.c() for r in recs], K, fmask, dl.data_ptr(), tags, dc.data_ptr() if dc is not None else 0, res.data_ptr())
        want = FM.fenv_owned_each(self.owner, self.cut, self.fenv, self.filt(), recs, K, fmask, entries, tags, count)
        return self.check(res, 4, want, tag or "fenv_owned_each")

    def fenv_tags(self, recs, first, count, K, fmask, tags, tag=""):
        res = self.result(4)
        self.db.fenv_tags_each([r.c() for r in recs], first, count, K, fmask, tags, res.data_ptr())
        want, lst = FM.fenv_tags_each(self.owner, self.cut, self.fenv, self.filt(), recs, first, count, K, fmask, tags)
        return self.check(res, 4, want, tag or "fenv_tags_each"), lst

    # the note-off paths the release can come through
    def trigger(self, slots, K, mask):
        dl = self.dev_list(slots)
        self.db.stamp_slots(dl.data_ptr(), len(slots), K, mask, TRIG)
        SM.stamp(self.truth, SM.stamp_voices(slots, len(slots), None, K, mask, self.n), TRIG, self.now())

    def stamp_match(self, first, count, K, mask, m, tag=""):
        res = self.result(2)
        self.db.stamp_match(first, count, K, mask, device.owner_match(*m), REL, res.data_ptr())
        heads = np.arange(first, first + count, K)
        hit = CHM.matches(self.owner[heads], m)
        voices = np.array([int(e) + l for e in heads[hit] for l in SM.lanes(mask, K)], np.int32)
        SM.stamp(self.truth, voices, REL, self.now())
        return self.check(res, 2, [int(hit.sum()), int((~hit).sum())], tag or "stamp_match")

    def off_pedal(self, first, count, K, mask, tags, hold_all, tag=""):
        res = self.result(4)
        self.db.release_tags_pedal(first, count, K, mask, tags, hold_all, res.data_ptr())
        want = PM.release_tags_pedal(self.owner, self.pedal, self.truth, first, count, K, mask, tags, hold_all, self.now())[0]
        return self.check(res, 4, want, tag or "release_tags_pedal")

    def pedal_up(self, first, count, K, mask, m, flags, tag=""):
        res = self.result(3)
        self.db.pedal_up(first, count, K, mask, device.owner_match(*m), flags, res.data_ptr())
        want = PM.up(self.owner, self.pedal, self.truth, first, count, K, mask, m, flags, self.now())[0]
        return self.check(res, 3, want, tag or "pedal_up")


# ---------------------------------------------------------------------------------------------- 1. every call against the model

@pytest.mark.gpu
@pytest.mark.parametrize("n,K", [(1, 1), (65, 1), (255, 1), (257, 1), (1500, 4), (1472, 64)])
def test_every_call_against_the_model(dev, n, K):
    """Banks of 1, 65, 255 and 257 voices at K = 1, 1500 at K = 4 and 1472 at K = 64.  A record on a bank without any side array (all
    withheld); the channel sweep over the whole bank and, on the larger banks, over a range off the workgroup span that takes three
    workgroups; a filter_mask smaller than the patch's mask; records by note id with 1, 2, 1023 and 1024 tags; a list with a hole, a
    slot past the bank, a stolen slot and a count word; clamped and withheld voices; advances in several lengths with a note-off of
    one channel in between; stop with and without snap."""
    bank, tables, g, now = plain_bank(n)
    inc = bank["voice_phase_inc"]
    inc[5::23], inc[7::29], inc[13::37] = f32(0.0), f32(3e38), f32(1e-30)
    r = FenvRig(dev, bank, tables, g)
    slots = np.arange(0, n, K, dtype=np.int32)
    full = (1 << K) - 1
    part = full if K == 1 else (1 << (K - 1)) | 1
    gen = np.random.default_rng(170 + n + K)
    try:
        chan = (gen.integers(1, 4, len(slots)).astype(np.uint32) << np.uint32(24))
        all_tags = (chan + np.arange(len(slots), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        if len(slots) > 20:
            all_tags[::17] = 0                                       # untagged slots match nothing
        r.trigger(slots, K, full)
        r.tag(slots, all_tags, K, tag="every slot")
        assert not r.db.download_fenv().any()
        tagged = int((r.owner[slots] != 0).sum())
        want = r.fenv_match(0, n, K, full, ANY, CONTOUR, tag="a record on a bank without a cutoff")
        assert want[:2] == [0, K * tagged] and not r.fenv.any() and not r.cut.any()
        r.cut_match(0, n, K, full, ANY, M.Rec(M.TRACK | QM, 0.05, 0.9, 1), tag="a tracked base")
        want = r.fenv_match(0, n, K, part, ANY, FM.Rec(FM.REL | FM.START, 8.0, 2.0, 1.0, 1.5, 0.9, 0.8, start=0.5), tag="every tagged slot, masked")
        assert want[0] > 0 and (K != 1 or n < 255 or (want[1] > 0 and want[3] > 0))
        r.cut_advance(0, n, 64)
        r.block("a block in the attack")
        r.fenv_match(0, n, K, full, (2 << 24, 0xFF000000), FM.Rec(FM.ABS, 2.5, 2.5, 0.01, 2.0, 0.5, 0.7), tag="channel 2: peak == sustain")
        if n >= 1472:
            first, count = 36 // K * K, (636 - 36 // K * K) // K * K  # off the 256-voice span at both ends: three workgroups
            assert -(-count // 256) == 3
            want = r.fenv_match(first, count, K, full, (1 << 24, 0xFF000000), FM.Rec(FM.ABS | FM.START, 0.02, 0.3, 1.5, 0.8, 1.2, 1.3, start=1.0), tag="a range off the span")
            assert want[0] > 0 and want[2] > 0
            inside = slots[(slots >= first) & (slots < first + count) & (r.owner[slots] != 0)]
            order = gen.permutation(len(inside))
            at = 0
            for m in (1, 2, 1023, 1024):
                take = min(m, max(1, len(inside) // 5))
                pick = inside[order[at:at + take]]
                at += take
                tags = padded_tags(r.owner[pick], m)[gen.permutation(m)]   # (unsorted: the sort and the permutation have work to do)
                want, lst = r.fenv_tags(contours(m, m), first, count, K, full if m != 2 else part, tags, tag=f"{m} tags")
                assert int((lst >= 0).sum()) == len(pick) and want[2] == 0 and want[0] + want[1] > 0
            tg = slots[r.owner[slots] != 0]
            rest = tg[~np.isin(tg, inside[order[:at]])]
            entries = np.array([rest[0], -1, n, rest[1], rest[2], rest[3]], np.int32)
            tags = np.array([r.owner[rest[0]], 5, 6, r.owner[rest[1]] ^ 0x00800000, r.owner[rest[2]], r.owner[rest[3]]], np.uint32)
            before = r.fenv[rest[3]:rest[3] + K].copy()
            want = r.fenv_owned(contours(6, 9), K, part, entries, tags, count=5, tag="a list")
            assert want[2] == 1 and (r.fenv[rest[3]:rest[3] + K] == before).all()
        else:
            r.fenv_tags(contours(1, 3), 0, n, K, full, all_tags[all_tags != 0][:1], tag="one tag")
        for frames in (37, 64, 411):
            r.cut_advance(0, n, frames)
        assert r.now() > 0
        r.stamp_match(0, n, K, full, (1 << 24, 0xFF000000), tag="channel 1: note-off")
        stages = set()
        for frames in (64, 200, 27, 4096):
            r.cut_advance(0, n, frames)
            stages |= set(r.fenv[:, 0].tolist())
        print(f"stages seen after the note-off: {sorted(stages)}")
        r.block("a block after the note-off")
        r.cut_stop(0, max(K, (n // 2) // K * K), False)
        r.cut_stop(0, n, True)
        assert not r.fenv.any() and not r.cut[:, M.TARGET].any() and r.cut_advance(0, n, 64) == [0, 0]
        r.block("a block after the stop")
        assert r.db.list_violations() == 0
    finally:
        r.close()


@pytest.mark.gpu
def test_three_workgroups_feed_the_counts_and_one_channel_of_four(dev):
    """700 voices, K = 1: three workgroups of the record and advance passes add to the result words; two record calls in a row on one
    stream with no host wait in between.  Then a contour on channel 2 of four: the voices of the other three channels keep every byte."""
    import torch
    n, K = 700, 1
    bank, tables, g, now = plain_bank(n)
    r = FenvRig(dev, bank, tables, g)
    try:
        heads = np.arange(n, dtype=np.int32)
        tags = ((np.uint32(1) + (heads % 4).astype(np.uint32) << np.uint32(24)) + heads.astype(np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(heads, tags, K, tag="every voice")
        r.cut_match(0, n, K, 1, ANY, M.Rec(M.ABS | QM, 0.2, 0.9, 1), tag="the base")
        bufs = [torch.full((6,), FILL, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        a, b = FM.Rec(FM.ABS, 1.0, 0.5, 0.1, 1.5, 0.9, 0.8), FM.Rec(FM.REL | FM.START, 20.0, 2.0, 1.0, 1.1, 0.9, 0.8, start=0.001)
        r.db.fenv_match(0, n, K, 1, device.owner_match(*ANY), a.c(), bufs[0].data_ptr())
        r.db.fenv_match(0, n, K, 1, device.owner_match(*ANY), b.c(), bufs[1].data_ptr())
        first = FM.fenv_match(r.owner, r.cut, r.fenv, r.filt(), 0, n, K, 1, ANY, a)
        second = FM.fenv_match(r.owner, r.cut, r.fenv, r.filt(), 0, n, K, 1, ANY, b)
        torch.cuda.synchronize()
        assert first == [n, 0, 0, 0] and second == [n, 0, 0, n]       # 0.2 * 20 and 0.2 * 0.001: every voice clamped, counted once
        for buf, w in zip(bufs, (first, second)):
            assert buf.cpu().numpy().view(np.uint32).tolist() == w + [FILL & 0xFFFFFFFF] * 2, (buf.cpu().numpy().tolist(), w)
        r.same("two calls")
        assert r.cut_advance(0, n, 64) == [n, 0]
        before = bank_words(r.db, bank)
        cut_before, fenv_before = r.cut.copy(), r.fenv.copy()
        want = r.fenv_match(0, n, K, 1, (2 << 24, 0xFF000000), FM.Rec(FM.ABS | FM.START, 1.0, 0.5, 0.1, 1.5, 0.9, 0.8, start=0.05), tag="channel 2 of four")
        assert want == [n // 4, 0, n - n // 4, 0]
        after = bank_words(r.db, bank)
        others = np.flatnonzero((r.owner >> 24) != 2)
        for c in M.COEFFS:
            assert after["voice_filter"][c][others].tobytes() == before["voice_filter"][c][others].tobytes(), c
        assert (r.cut[others] == cut_before[others]).all() and (r.db.download_cutoff()[others] == cut_before[others]).all()
        assert (r.fenv[others] == fenv_before[others]).all() and (r.db.download_fenv()[others] == fenv_before[others]).all()
        assert set(CM.words_differ(before, after)) <= {"voice_filter." + c for c in M.COEFFS}, CM.words_differ(before, after)
        r.block("after the channel's contour")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 2. cuttings

CUTTINGS = [(64,) * 24, (512, 1024), (100, 412, 300, 724)]


@pytest.mark.gpu
@pytest.mark.parametrize("cuts", CUTTINGS)
def test_a_contour_in_three_cuttings(dev, cuts):
    """A record at frame 0, a note-off of the whole channel at frame 512 (a block cut in every cutting), 1536 frames in all.  The
    device is held to the model after every pass, and at 512 and 1536 frames to the model run in 64-frame blocks: the cutting does
    not change the curve.  At the end every contour has ended on its w_end."""
    n, K = 512, 4
    bank, tables, g, now = plain_bank(n)
    r = FenvRig(dev, bank, tables, g)
    try:
        heads = np.arange(0, n, K, dtype=np.int32)
        tags = (np.uint32(3 << 24) + np.arange(len(heads), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        r.trigger(heads, K, 0xF)
        r.tag(heads, tags, K, tag="every slot")
        render_blocks(r.db, (F,))                                     # (the clock leaves 0: a release stamp of 0 is no release)
        cpuref.render(r.truth, r.gl, r.tables, F, 0)
        r.cut_match(0, n, K, 0xF, ANY, M.Rec(M.TRACK | QM, 0.05, 1.2, 1), tag="the base")
        r.fenv_match(0, n, K, 0xF, ANY, FM.Rec(FM.REL, 9.0, 3.0, 0.5, 1.3, 0.91, 0.8), tag="the contour")
        ref_cut, ref_fenv, ref_filt = r.cut.copy(), r.fenv.copy(), r.filt().copy()
        assert not r.rel().any()
        at, seen = 0, {}
        for f in cuts:
            if at == 512:
                assert r.stamp_match(0, n, K, 0xF, (3 << 24, 0xFF000000), tag="the note-off")[0] == n // K
                assert (r.rel() != 0).any()
            r.cut_advance(0, n, f)
            at += f
            if at in (512, 1536):
                seen[at] = (r.cut.copy(), r.fenv.copy(), r.filt().copy())
        ref_rel = np.zeros_like(r.rel())
        for k in range(24):                                           # the same performance in 64-frame blocks, on the model
            if k == 8:
                ref_rel = r.rel()
            FM.advance(ref_cut, ref_fenv, ref_rel, ref_filt, 0, n, 64)
            if 64 * (k + 1) in seen:
                c, e, fl = seen[64 * (k + 1)]
                assert ref_cut.tobytes() == c.tobytes() and ref_fenv.tobytes() == e.tobytes() and ref_filt.tobytes() == fl.tobytes(), f"the cutting changed the curve at {64 * (k + 1)}"
        released = r.rel() != 0
        assert set(seen) == {512, 1536} and (seen[512][1][:, 0] != 0).any() and released.any() and not r.fenv[released].any()
        r.block("after the contour")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 3. stems against the oracle

@pytest.mark.gpu
@pytest.mark.parametrize("family", ["one voice per lane", "two per lane"])
def test_a_full_contours_stems_against_the_oracle(dev, family):
    """A 256-voice bank of either kernel family, ten blocks of 64 frames.  Three slots of one channel get a tracked cutoff and a
    contour; cutoff_advance runs ahead of every block; one note is released in block 4 through release_tags and its contour closes.
    The oracle's bank receives the model's coefficients block by block; the stems of the three slots through taps and the state of
    every voice must be the oracle's bit for bit."""
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
    r = FenvRig(dev, bank, tables, g, setup)
    try:
        slots = [4 * K, 21 * K, 31 * K]
        r.trigger(slots, K, vmask & 0xFE if two else vmask)
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
        want, _ = r.fenv_tags([FM.Rec(FM.REL | FM.START, 6.0, 2.0, 0.5, 2.0, 0.7, 0.6, start=0.5)] * 3, 0, n, K, vmask, tags, tag="the contours")
        assert want[0] == 3 * bin(vmask).count("1")
        kernels, differ, stages = set(), 0, set()
        for blk in range(10):
            if blk == 4:
                r.release(0, n, K, vmask, tags[1:2], REL, tag="one note-off")
            before = r.filt().copy()
            r.cut_advance(0, n, F, tag=f"advance ahead of block {blk}")
            stages |= set(r.fenv[voices, 0].tolist())
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
        assert differ >= 6, "the contour did not move the coefficients"
        assert {1, 2, 3, 4} <= stages, stages                        # READ THE CLOCK (stage 4 is entered from the clock alone)
        assert (kernels == {3}) if two else (3 not in kernels), kernels
        assert r.db.list_violations() == 0
    finally:
        r.db.set_taps([], 0)
        r.close()


# ---------------------------------------------------------------------------------------------- 4. every note-off path

@pytest.mark.gpu
@pytest.mark.parametrize("path", ["stamp_owned", "release_tags", "stamp_match", "pedal_up"])
def test_the_release_comes_through(dev, path):
    """tests/owner_scenes.py's bank with its carriers filtered.  Two keys with contours rest in sustain; one gets its note-off through
    the named path.  The pass behind the stamp enters its release; the other key rests on.  Under the pedal the held-back note-off
    releases nothing until the pedal-up stamps."""
    K, N = OS.K, OS.N
    bank, tables, g = OS.bank()
    filtered(bank, K, OS.MEMBERS)
    r = FenvRig(dev, bank, tables, g)
    try:
        slot, other = int(OS.others()[5]), int(OS.others()[9])
        tag, tag2 = 3 << 24 | 60, 5 << 24 | 72
        r.trigger([slot, other], K, OS.MMASK)
        r.tag([slot, other], [tag, tag2], K, tag="two keys")
        r.block("the clock leaves 0")
        assert r.cut_match(0, N, K, OS.MMASK, ANY, M.Rec(M.TRACK | QM, M.track_value(4.0, 4096), 1.1, 1), tag="tracked")[0] == 2 * len(OS.MEMBERS)
        assert r.fenv_tags([FM.Rec(FM.REL, 6.0, 2.0, 1.0, 2.0, 0.7, 0.6)] * 2, 0, N, K, OS.MMASK, [tag, tag2], tag="two contours")[0][0] == 2 * len(OS.MEMBERS)
        vs, vo = slot + np.array(OS.MEMBERS), other + np.array(OS.MEMBERS)
        base = r.cut[vs, M.W].copy()
        for _ in range(10):
            r.cut_advance(0, N, F)
        assert (r.fenv[vs, 0] == 3).all() and (r.fenv[vo, 0] == 3).all()
        r.block("resting")
        if path == "stamp_owned":
            assert r.stamp([slot], [tag], K, OS.MMASK, REL, tag="stamp_owned")[0][0] == 1
        elif path == "release_tags":
            assert r.release(0, N, K, OS.MMASK, [tag], REL, tag="release_tags")[0][0] == 1
        elif path == "stamp_match":
            assert r.stamp_match(0, N, K, OS.MMASK, CHM.channel(3))[0] == 1
        else:
            assert r.off_pedal(0, N, K, OS.MMASK, [tag], True, tag="held back") == [0, 0, 0, 1]
            assert r.cut_advance(0, N, F) == [0, 0] and (r.fenv[vs, 0] == 3).all()
            r.block("under the pedal")
            assert r.pedal_up(0, N, K, OS.MMASK, CHM.channel(3), PM.LIFT_SUSTAIN)[:2] == [1, 0]
        assert (r.rel()[vs] != 0).all() and (r.rel()[vo] == 0).all()
        assert r.cut_advance(0, N, F) == [len(OS.MEMBERS), 0]        # READ THE CLOCK
        assert (r.fenv[vs, 0] == 4).all() and (r.fenv[vo, 0] == 3).all()   # READ THE CLOCK
        r.block("releasing")
        for _ in range(6):
            r.cut_advance(0, N, F)
        assert not r.fenv[vs].any() and (r.cut[vs, M.W] == base).all() and (r.fenv[vo, 0] == 3).all()   # READ THE CLOCK
        r.block("released")
        assert r.db.list_violations() == 0
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 5. who ends an envelope

@pytest.mark.gpu
def test_a_thief_and_a_restruck_key_inherit_no_contour(dev):
    """tests/owner_scenes.py's bank.  A key with a contour is struck again through skred_bank_note_on_channel -- the call's own tag
    launch clears the slot's fenv words; then a note of another channel takes a slot whose contour rests.  The new notes get their
    own base cutoff, and neither a later advance nor the victim's release clock moves them."""
    from skred_amd.bank import slot_query
    import slot_steal_model as SSM
    from steal_model import ENV, FIN, OLDEST
    K, N = OS.K, OS.N
    bank, tables, g = OS.bank()
    filtered(bank, K, OS.MEMBERS)
    r = FenvRig(dev, bank, tables, g)
    iq = slot_query(0, N, K, OS.MMASK, FIN | ENV, OS.SETTLE, 0, 0)
    sq = SSM.SlotQuery(0, N, K, OS.MMASK, OLDEST, 0)
    try:
        slot, other = int(OS.others()[5]), int(OS.others()[9])
        tag, tag2 = 3 << 24 | 60, 3 << 24 | 72
        r.tag([slot, other], [tag, tag2], K, tag="two keys")
        chan = (3 << 24, 0xFF000000)
        assert r.cut_match(0, N, K, OS.MMASK, chan, M.Rec(M.TRACK | QM, M.track_value(8.0, 4096), 1.1, 1), tag="tracked")[0] == 2 * len(OS.MEMBERS)
        assert r.fenv_match(0, N, K, OS.MMASK, chan, FM.Rec(FM.REL, 4.0, 2.0, 1.0, 1.1, 0.95, 0.8), tag="two contours")[0] == 2 * len(OS.MEMBERS)
        assert r.cut_advance(0, N, F) == [2 * len(OS.MEMBERS), 0]
        r.block("in the attack")
        strike(r, iq, sq, (tag, 0xFFFFFFFF), tag, 3, slot)
        M.tag_clear(r.cut, [slot], 1, None, K)
        FM.tag_clear(r.fenv, [slot], 1, None, K)
        assert not r.fenv[slot:slot + K].any()                       # CLEAR RULE
        r.same("the re-strike")                                      # CLEAR RULE (the device's words against the model's)
        assert r.cut_tags([M.Rec(M.ABS | QM, 0.3, 0.9, 1)], 0, N, K, OS.MMASK, [tag], tag="the new note's own cutoff")[0][0] == len(OS.MEMBERS)
        held = r.filt()[slot:slot + K].copy()
        assert r.cut_advance(0, N, F) == [len(OS.MEMBERS), 0]        # CLEAR RULE: the struck slot's attack would run on
        assert r.filt()[slot:slot + K].tobytes() == held.tobytes()   # CLEAR RULE
        # the thief
        r.tag([other], [5 << 24 | 40], K, tag="the thief's tag")
        assert not r.fenv[other:other + K].any() and not r.cut[other:other + K].any()   # CLEAR RULE
        assert r.cut_tags([M.Rec(M.TRACK | QM, M.track_value(3.0, 4096), 0.7, 2)], 0, N, K, OS.MMASK, [5 << 24 | 40], tag="the thief's own cutoff")[0][0] == len(OS.MEMBERS)
        r.block("the clock moves")
        r.stamp([other], [5 << 24 | 40], K, OS.MMASK, REL, tag="the thief's note-off")
        held = r.filt()[other:other + K].copy()                      # (behind the block: rendering moves the filter's memory)
        assert r.cut_advance(0, N, F) == [0, 0]                      # CLEAR RULE: the victim's release would start on the thief
        assert r.filt()[other:other + K].tobytes() == held.tobytes()   # CLEAR RULE
        assert r.fenv_tags([CONTOUR], 0, N, K, OS.MMASK, [5 << 24 | 40], tag="the thief's own contour")[0][0] == len(OS.MEMBERS)
        r.block("after the new notes")
        assert r.db.list_violations() == 0
    finally:
        r.close()


@pytest.mark.gpu
def test_a_cutoff_call_on_an_enveloped_voice_ends_the_contour(dev):
    """512 voices, K = 4, every slot enveloped.  cutoff_tags_each sets one note, starts a glide on another and is withheld on a third
    (TRACK on a zero increment): the first two lose their contours, the third keeps it.  cutoff_stop ends the contours of its range."""
    n, K = 512, 4
    bank, tables, g, now = plain_bank(n)
    bank["voice_phase_inc"][8:12] = f32(0.0)
    r = FenvRig(dev, bank, tables, g)
    try:
        heads = np.arange(0, n, K, dtype=np.int32)
        tags = (np.uint32(3 << 24) + np.arange(len(heads), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(heads, tags, K, tag="every slot")
        r.cut_match(0, n, K, 0xF, ANY, M.Rec(M.ABS | QM, 0.1, 0.9, 1), tag="the base")
        assert r.fenv_match(0, n, K, 0xF, ANY, FM.Rec(FM.ABS, 1.0, 0.5, 0.05, 1.5, 0.9, 0.8), tag="contours")[0] == n
        r.cut_advance(0, n, F)
        recs = [M.Rec(M.ABS, 0.3), M.Rec(M.ABS | M.GLIDE, 2.0, rate_up=1.2, rate_down=0.8), M.Rec(M.TRACK, 3.0)]
        want, _ = r.cut_tags(recs, 0, n, K, 0xF, tags[:3], tag="set, glide, withheld")
        assert want[:2] == [2 * K, K]
        assert not r.fenv[:2 * K].any() and (r.fenv[2 * K:3 * K, 0] == 1).all() and (r.fenv[3 * K:, 0] == 1).all()
        assert r.cut_advance(0, n, F) == [n - K, 0]                   # the glide moves by the cutoff's rule, the others by the envelope's
        r.cut_stop(2 * K, 64, False, tag="stop over enveloped voices")
        assert not r.fenv[2 * K:2 * K + 64].any() and (r.fenv[2 * K + 64:, 0] != 0).all()
        r.block("after the stop")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 6. purity

@pytest.mark.gpu
def test_a_twin_without_fenv_calls_is_the_bank_as_it_was(dev):
    """tests/test_slots.py's in-place bank (4096 voices, two per lane).  Both banks get the same cutoff calls; `r` also gets fenv calls
    that start nothing (a channel nobody is on: the array exists, nothing is enveloped).  Blocks, bank bytes, cutoff words, the
    advance's d_result, kernel family and in-place verdict agree block by block: cutoff_advance through the envelope instantiation
    writes the bytes the plain one writes."""
    n, K, mask = 4096, 8, 0xFE
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    r = FenvRig(dev, bank, tables, g, setup)
    plain = open_bank(dev, bank, tables, g, setup)
    try:
        chord = np.arange(0, 40 * K, 2 * K, dtype=np.int32)
        tags = (np.uint32(0x03000000) + np.arange(len(chord), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        dl = r.dev_list(chord)
        m = device.owner_match
        taken = []
        for k in range(6):
            if k == 1:
                for d in (r.db, plain):
                    d.stamp_slots(dl.data_ptr(), len(chord), K, mask, TRIG)
                SM.stamp(r.truth, SM.stamp_voices(chord, len(chord), None, K, mask, n), TRIG, r.now())
                r.tag(chord, tags, K, tag="the chord")
                plain.tag_slots(dl.data_ptr(), tags, K)
                assert r.fenv_match(0, n, K, mask, (9 << 24, 0xFF000000), CONTOUR, tag="a channel nobody is on") == [0, 0, n // K, 0]
                assert not r.db.download_fenv().any()
            if k == 2:
                r.cut_match(0, n, K, mask, (3 << 24, 0xFF000000), M.Rec(M.TRACK | QM, 0.05, 1.5, 1), tag="tracked")
                plain.cutoff_match(0, n, K, mask, m(3 << 24, 0xFF000000), M.Rec(M.TRACK | QM, 0.05, 1.5, 1).c())
                sweep = M.Rec(M.ABS | M.GLIDE, 2.4, rate_up=1.2, rate_down=0.8)
                r.cut_match(0, n, K, mask, (3 << 24, 0xFF000000), sweep, tag="the sweep")
                plain.cutoff_match(0, n, K, mask, m(3 << 24, 0xFF000000), sweep.c())
            if k >= 2:
                want = r.cut_advance(0, n, F)
                res = r.result(2)
                plain.cutoff_advance(0, n, F, res.data_ptr())
                assert r.read(res, 2, "the twin's advance") == want
                if k == 4:
                    assert r.fenv_match(0, n, K, mask, (9 << 24, 0xFF000000), CONTOUR, tag="nobody again") == [0, 0, n // K, 0]
            x, y = render_blocks(r.db, (F,))[0], render_blocks(plain, (F,))[0]
            cpuref.render(r.truth, r.gl, r.tables, F, 0)
            taken.append((r.db.last_kernel(), plain.last_kernel(), r.db.last_in_place(), plain.last_in_place()))
            assert x.tobytes() == y.tobytes(), f"block {k}: the mixes differ"
            assert taken[-1][0] == taken[-1][1] == 3 and taken[-1][2] == taken[-1][3], (k, taken)
            banks_same(r.db, plain, bank, f"block {k}")
            assert (plain.download_cutoff() == r.cut).all(), f"block {k}: the cutoff words differ"
            assert r.db.list_violations() == plain.list_violations() == 0
        assert not plain.download_fenv().any() and not r.fenv.any() and r.cut[:, M.TARGET].any()
        print(f"(kernel, plain's, in place, plain's) per block: {taken}")
    finally:
        r.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- 7. every array at once

@pytest.mark.gpu
def test_all_six_side_arrays_at_once_and_more_calls_than_ring_slots(dev):
    """One bank with owner, pedal, glide, bend, cutoff and fenv arrays.  Forty fenv_tags_each calls back to back with no host wait in
    between -- five times the staging ring's eight slots -- with advances in between, then a tag launch with the five clears behind
    it.  REL levels stand on a base that tracked the key of the bent voices."""
    n, K = 512, 4
    bank, tables, g, now = plain_bank(n)
    r = FenvRig(dev, bank, tables, g)
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
        want, _ = r.cut_tags([M.Rec(M.TRACK | QM, 0.05, 1.0, 1)] * 110, 0, n, K, 0xF, tags[:110], tag="tracked under the bends")
        assert want[0] == 110 * K
        bent = np.flatnonzero(r.bend[:, 0] != 0)
        for j in range(40):
            pick = tags[(j * 3) % 100:(j * 3) % 100 + 16]
            recs = contours(16, j)
            r.db.fenv_tags_each([x.c() for x in recs], 0, n, K, 0xF, pick)
            FM.fenv_tags_each(r.owner, r.cut, r.fenv, r.filt(), recs, 0, n, K, 0xF, pick)
            if j % 4 == 3:
                r.db.cutoff_advance(0, n, F)
                FM.advance(r.cut, r.fenv, r.rel(), r.filt(), 0, n, F)
        r.same("forty fenv calls")
        assert r.fenv[bent, 0].any(), "bent voices carry contours"
        r.advance(0, n, F, tag="the glides move")
        r.cut_advance(0, n, F, tag="the contours move")
        assert r.glide[:, 0].any() and r.bend[:, 0].any() and r.cut[:, M.TARGET].any() and r.fenv[:, 0].any()
        r.tag(heads[:40], tags[:40] + np.uint32(0x1000), K, tag="forty new notes")
        assert not r.fenv[:160].any() and not r.cut[:160].any() and not r.bend[:160].any() and not r.glide[:160].any() and r.fenv[160:, 0].any()
        r.block("all six arrays")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 8. refusals

@pytest.mark.gpu
def test_refusals_write_nothing(dev):
    import torch
    n, K = 256, 8
    bank, tables, g, now = plain_bank(n)
    r = FenvRig(dev, bank, tables, g)
    try:
        L = r.db.L
        r.tag([8, 16], [5, 6], K, tag="two slots")
        r.cut_tags([M.Rec(M.ABS | QM, 0.25, 0.9, 1)], 0, n, K, 0xFF, [5], tag="one cutoff")
        assert r.fenv_tags([CONTOUR], 0, n, K, 0xFF, [5], tag="one contour")[0] == [8, 0, 0, 0]
        dl = r.dev_list([8, 16, 24, 32])
        res = torch.full((5,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        good, zero, dup = device.tag_array([5, 6, 7, 8]), device.tag_array([5, 0, 7, 8]), device.tag_array([5, 6, 5, 8])
        one = CONTOUR.c()
        ok = device.fenv_array([one] * 4)
        h, d, rs, rp, tp = r.db.h, dl.data_ptr(), res.data_ptr(), C.cast(ok, C.c_void_p), good.ctypes.data
        m, wrong = device.owner_match(0, 0), device.owner_match(1, 0)
        MA, OE, TE, DL = L.skred_bank_fenv_match, L.skred_bank_fenv_owned_each, L.skred_bank_fenv_tags_each, L.skred_bank_download_fenv
        assert MA(None, 0, n, K, 0xFF, C.byref(m), C.byref(one), rs, None) == BAD and MA(h, 0, n, K, 0xFF, None, C.byref(one), rs, None) == BAD
        assert MA(h, 0, n, K, 0xFF, C.byref(m), None, rs, None) == BAD and MA(h, 0, n, 12, 0xFF, C.byref(m), C.byref(one), rs, None) == RANGE
        assert MA(h, 0, n, K, 0, C.byref(m), C.byref(one), rs, None) == BAD and MA(h, 0, n, K, 0x1FF, C.byref(m), C.byref(one), rs, None) == BAD
        assert MA(h, 4, 8, K, 0xFF, C.byref(m), C.byref(one), rs, None) == RANGE and MA(h, 0, n + K, K, 0xFF, C.byref(m), C.byref(one), rs, None) == RANGE
        assert MA(h, 0, 0, K, 0xFF, C.byref(m), C.byref(one), rs, None) == RANGE and MA(h, 0, n, K, 0xFF, C.byref(wrong), C.byref(one), rs, None) == BAD
        nan = float("nan")
        bads = [(FM.Rec(FM.ABS | FM.REL, 2.0, 0.5, 0.1, 1.5, 0.9, 0.8), BAD), (FM.Rec(0, 2.0, 0.5, 0.1, 1.5, 0.9, 0.8), BAD),
                (FM.Rec(FM.ABS | 8, 2.0, 0.5, 0.1, 1.5, 0.9, 0.8), BAD), (FM.Rec(FM.ABS, 2.0, 0.5, 0.1, 1.5, 0.9, 0.8, start=0.2), BAD),
                (FM.Rec(FM.ABS, nan, 0.5, 0.1, 1.5, 0.9, 0.8), BAD), (FM.Rec(FM.ABS, 2.0, 0.5, 0.1, 1.5, nan, 0.8), BAD),
                (FM.Rec(FM.ABS, 3.5, 0.5, 0.1, 1.5, 0.9, 0.8), RANGE), (FM.Rec(FM.ABS | FM.START, 2.0, 0.5, 0.1, 1.5, 0.9, 0.8), RANGE),
                (FM.Rec(FM.REL, 2.0, 0.0, 1.0, 1.5, 0.9, 0.8), RANGE), (FM.Rec(FM.REL, 2.0, 0.5, -1.0, 1.5, 0.9, 0.8), RANGE),
                (FM.Rec(FM.ABS, 2.0, 0.5, 0.1, 20.0, 0.9, 0.8), RANGE), (FM.Rec(FM.ABS, 2.0, 0.5, 0.1, 1.5, 0.9, 0.01), RANGE),
                (FM.Rec(FM.ABS, 2.0, 0.5, 0.1, 1.0, 0.9, 0.8), BAD), (FM.Rec(FM.ABS, 2.0, 0.5, 0.1, 1.5, 1.0, 0.8), BAD),
                (FM.Rec(FM.ABS, 2.0, 0.5, 0.1, 1.5, 0.9, 1.0), BAD)]
        for rec, code in bads:
            assert FM.check([rec], K, 0xFF, 0xFF) == code, vars(rec)
            c = rec.c()
            assert MA(h, 0, n, K, 0xFF, C.byref(m), C.byref(c), rs, None) == code, vars(rec)
            arr = device.fenv_array([one, one, c, one])
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
        out = np.full(64, 9, np.uint32)
        assert DL(h, out.ctypes.data, n - 2, 4) == RANGE and DL(h, None, 0, 4) == BAD and DL(None, out.ctypes.data, 0, 4) == BAD
        assert (out == 9).all()
        assert OE(h, rp, K, 0xFF, d, tp, 0, None, rs, None) == 0 and TE(h, rp, 0, n, K, 0xFF, tp, 0, rs, None) == 0
        torch.cuda.synchronize()
        assert (res.cpu().numpy() == FILL).all()
        r.same("after the refusals")
        assert r.fenv_match(0, n, K, 0xFF, ANY, CONTOUR, tag="the bank still answers") == [8, 8, n // K - 2, 0]
        r.block("after the refusals")
    finally:
        r.close()
