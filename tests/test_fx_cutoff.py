"""Filter cutoff on the fixed-point bank on the GPU (skred_fxbank_cutoff_match / _cutoff_owned_each / _cutoff_tags_each / _cutoff_advance
/ _cutoff_stop / _download_cutoff), byte for byte.

After every call the device is held to tests/fx_cutoff_model.py: download_cutoff == the model's eight words on every voice, the bend,
glide and owner arrays == the model's, every word of the bank (skred_fxbank_download and _download_params, the five coefficient words
among them) == the oracle's bank after the model's stores, every d_result word == the model's count with the guard words past it
untouched; mixes and stems of every rendered block are compared bit for bit with oracle.cpuref.fx_render driven through the model.
The randomised performance is tests/fx_cutoff_scenes.py's, whose conditions tests/test_fx_cutoff_cpu.py asserts on the model alone; the
clear rule's scenes are the model's, and the CPU tests assert that each of them bites.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import chan_model as CM
import fx_bend_model as BM
import fx_chan_model as FCM
import fx_cutoff_model as M
import fx_cutoff_scenes as S
import fx_glide_model as GM
import fx_live_model as live
import fx_pedal_model as PM
import fx_steal_model as sm
from skred_amd import fxbank as fxb
from test_fx_bend import DeviceBendStage, mono_args
from test_fx_chan import assert_same_bank, whole_bank
from test_fx_glide import FILL, dev_count, dev_list, padded_tags, ptr, sync
from test_fx_cutoff_cpu import CUTS
from test_fx_live import dev_i32, host_of, open_fx

pytestmark = pytest.mark.gpu

BAD, RANGE = -2, -4
SPAN = 256                                                       # SK_CONTROL_SPAN: voices or entries per workgroup of the cutoff kernels
N = 600
R = M.Rec
BOTH = M.BOTH
CH = S.CH
CHAN = S.CHAN
G = GM.Glide


def cs(recs):
    return [r.c() for r in recs]


class DeviceCutoffStage(DeviceBendStage, M.FxCutoffStage):
    """fx_cutoff_model.FxCutoffStage with a device bank beside it: every call runs on both, and the device is compared with the model."""

    def same(self, what):
        got = self.db.download_cutoff()
        bad = np.flatnonzero((got != self.cut).any(axis=1))
        assert not len(bad), f"{what}: cutoff words differ at {bad[:8].tolist()}: {got[bad[:4]].tolist()} / {self.cut[bad[:4]].tolist()}"
        super().same(what)

    def cut_match(self, match, rec, rng=None):
        first, count = rng or self.whole
        res = self.result(4)
        self.db.cutoff_match(first, count, match[0], match[1], rec.c(), res.data_ptr())
        return self.read(res, 4, "cutoff_match", super().cut_match(match, rec, rng))

    def cut_tags(self, recs, tags, rng=None):
        first, count = rng or self.whole
        res = self.result(4)
        self.db.cutoff_tags_each(cs(recs), first, count, tags, res.data_ptr())
        return self.read(res, 4, f"cutoff_tags_each of {len(tags)}", super().cut_tags(recs, tags, rng))

    def cut_list(self, recs, entries, tags, count=None):
        dl, dc, res = dev_list(entries), dev_count(count), self.result(4)
        self.db.cutoff_owned_each(cs(recs), dl.data_ptr(), tags, ptr(dc), res.data_ptr())
        return self.read(res, 4, "cutoff_owned_each", super().cut_list(recs, entries, tags, count))

    def cut_advance(self, frames, rng=None):
        first, count = rng or self.whole
        res = self.result(2)
        self.db.cutoff_advance(first, count, frames, res.data_ptr())
        return self.read(res, 2, f"cutoff_advance by {frames}", super().cut_advance(frames, rng))

    def cut_stop(self, snap, rng=None):
        first, count = rng or self.whole
        self.db.cutoff_stop(first, count, snap)
        super().cut_stop(snap, rng)
        self.same(f"cutoff_stop snap {snap}")


def stage(n=N, **kw):
    bank, pool, c0 = fxb.bank_fx(n)
    return DeviceCutoffStage(S.silent_voice(bank), pool, c0, **kw)


# ---------------------------------------------------------------------------------------------- the clear rule, stealing

@pytest.mark.parametrize("name", M.SCENES)
def test_scene_on_the_device(name):
    """A thief's tag_list and a key struck again: the model's scenes, which fail on a bank without the clear behind the tag launch.  The
    scenes' own first record creates the array; a bank that never set a cutoff downloads zeros."""
    st = stage()
    try:
        assert not st.db.download_cutoff().any()
        M.run_scene(name, st)
    finally:
        st.close()


def test_thief_and_restruck_key_through_note_on_channel():
    """Mono mode (cap 1, min_age 0) under a sweeping cutoff: the key is struck again through skred_fxbank_note_on_channel, so the new
    note takes the old note's voice and the call's own tag launch is the one that clears the eight words; the coefficients stay.  Then
    the header's order: the tracked cutoff on the new note, and a sweep that lands."""
    st = stage()
    tag, v = [(CH << 24) | 60], 300
    up, down = M.rate_q32(400.0)
    try:
        st.strike([v], tag, [40000003])
        assert st.cut_tags([R(M.TRACK | BOTH, M.track_q24(1), 2 << 16, 1)], tag) == [1, 0, 0, 0]
        assert st.cut_tags([R(M.TRACK | M.GLIDE, M.track_q24(16), up_q32=up, down_q32=down)], tag) == [1, 0, 0, 0]
        assert st.cut_advance(64) == [1, 0]
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
        M.tag_clear(st.cut, want, 1)
        sync()
        assert host_of(da).tolist() == [v, FILL, FILL] and host_of(dr).tolist() == res + [FILL, FILL]
        assert not st.cut[v].any()
        st.same("the re-strike")
        assert st.cut_advance(64) == [0, 0]
        st.block()
        assert st.cut_tags([R(M.TRACK, M.track_q24(2))], tag) == [0, 1, 0, 0], "the new note inherited the old note's q and mode"
        assert st.cut_tags([R(M.TRACK | BOTH, M.track_q24(2), 3 << 16, 1)], tag) == [1, 0, 0, 0]
        assert st.cut[v, M.W] == (53393781 * M.track_q24(2)) >> 27
        assert st.cut_tags([R(M.TRACK | M.GLIDE, M.track_q24(4), up_q32=up, down_q32=down)], tag) == [1, 0, 0, 0]
        for _ in range(12):
            res = st.cut_advance(64)
            st.block()
            if res == [0, 1]:
                break
        assert res == [0, 1] and st.cut[v].tolist() == [(53393781 * M.track_q24(4)) >> 27, 0, 0, 0, 0, 3 << 16, 1, 0]
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- every call against the model

@pytest.mark.parametrize("n", [1, 65, SPAN - 1, SPAN + 1, 1500])
def test_every_call_against_the_model(n):
    """Banks of 1, 65, 255, 257 and 1 500 voices through the shared performance: a channel of two interleaved (the sweep's range spans
    every workgroup of the match kernel: six at 1 500), records per note with holes, entries outside the bank, a stolen voice and a
    d_count below and above n, sweeps up and down that land and that go on, stops with and without snap, rendered blocks between."""
    st = stage(n, stems=n <= SPAN + 1)
    try:
        tally = S.random_performance(st, np.random.default_rng(n))
        print(tally)
        if n >= 65:
            assert tally["landed"] >= 1 and tally["still"] >= 1 and tally["up"] >= 1 and tally["down"] >= 1
    finally:
        st.close()


def test_tag_counts_holes_stolen_tags_and_a_channel_of_four():
    """1 500 voices, the range [37, 737) -- three workgroups of the match kernel; 1, 2, 1 023 and 1 024 tags arriving in no order with
    tags nobody carries (holes) and tags whose voice lies outside the range; four channels interleaved, one of them swept."""
    n, rng = 1500, (37, 700)
    st = stage(n, stems=False)
    gen = np.random.default_rng(n + 11)
    try:
        heads = np.arange(rng[0], rng[0] + rng[1], dtype=np.int32)
        tags = ((((heads % 4) + CH).astype(np.uint32)) << np.uint32(24)) | (1 + np.arange(len(heads))).astype(np.uint32)
        tagged = np.arange(len(heads)) % 5 != 4
        st.tag(heads[tagged], tags[tagged])
        st.tag([0, n - 1], [(CH << 24) | 0xFFFF, (CH << 24) | 0xFFFE])
        own, own_tags = heads[tagged], tags[tagged]
        res = st.cut_match(CHAN, R(M.TRACK | BOTH, M.track_q24(3), 1 << 16, 2), rng)
        mine = int(((own_tags >> 24) == CH).sum())
        assert res[0] + res[1] == mine and res[2] == rng[1] - mine and mine > 100
        order, at = gen.permutation(len(own)), 0
        for m in (1, 2, 1023, 1024):
            pick = order[at:at + min(m, 150)]
            at += len(pick)
            t = padded_tags(own_tags[pick], m)
            recs = [R(M.TRACK | BOTH, M.track_q24(int(gen.choice(S.HARMONICS))), int(np.exp2(gen.uniform(10, 26))), 1 + k % 5) for k in range(m)]
            p = gen.permutation(m)
            res = st.cut_tags([recs[i] for i in p], t[p], rng)                       # the records must follow their tags through the sort
            assert res[0] + res[1] == len(pick) and res[2] == 0
        assert st.cut_tags([R(M.ABS | BOTH, 1 << 24, 1 << 16, 1)], [(CH << 24) | 0xFFFF], rng) == [0, 0, 0, 0]      # carried below the range only
        st.tag(own[:3], own_tags[:3] + np.uint32(0x100))                              # three voices stolen: the old tags find nobody
        assert st.cut_tags([R(M.ABS | BOTH, 1 << 24, 1 << 16, 1)] * 3, own_tags[:3], rng) == [0, 0, 0, 0]
        assert int((st.cut[:, M.W] != 0).sum()) > 300
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- cuttings, arrival

def test_three_block_cuttings_and_arrival_equals_an_abs_twin():
    """1 024 frames advanced as one block, as 16 x 64 and as 100 + 28 + 512 + 1 + 383 on three banks: each held to the model after every
    call -- so the 16 x 64 bank equals the model at EVERY multiple of 64, and tests/test_fx_cutoff_cpu.py holds the model there to the
    plain loop -- and every pair of banks is compared at every multiple of 64 both stop at (128, 640 and 1 024 between 16 x 64 and
    the uneven cutting, 1 024 with the single block).  Then the sweeps run out, and every voice
    that landed holds the bits of a twin voice set with ABS at the target."""
    n = 320
    at64, stages = [], []
    try:
        for cutting in CUTS:
            st = stage(n, stems=False)
            stages.append(st)
            v = np.arange(n, dtype=np.int32)
            tags = (0x03000001 + v).astype(np.uint32)
            st.tag(v, tags)
            gen = np.random.default_rng(5)
            w0 = [int(np.exp2(gen.uniform(20, 30))) for _ in range(n)]
            assert st.cut_tags([R(M.ABS | BOTH, w, 3 << 15, 1 + k % 5) for k, w in enumerate(w0)], tags) == [n, 0, 0, 0]
            fast, slow = M.rate_q32(150.0), M.rate_q32(5.0)
            movers = v[v % 2 == 0]
            targets = [min(M.W_MAX, 3 * w0[x]) if x % 4 == 0 else max(M.W_MIN, w0[x] // 3) for x in movers]
            rates = [fast if x % 8 < 4 else slow for x in movers]
            assert st.cut_tags([R(M.ABS | M.GLIDE, t, up_q32=r[0], down_q32=r[1]) for t, r in zip(targets, rates)], tags[movers]) == [len(movers), 0, 0, 0]
            seen, t = {}, 0
            for frames in cutting:
                res = st.cut_advance(frames)
                t += frames
                if t % 64 == 0:
                    seen[t] = (st.db.download_cutoff()[:, :2].copy(), whole_bank(st.db, st.truth))
            assert 1 <= res[0] < len(movers), "some voice landed and some voice still moves"
            at64.append(seen)
        assert set(at64[0]) == {1024} and set(at64[1]) == set(range(64, 1025, 64)) and set(at64[2]) == {128, 640, 1024}
        compared = []
        for a, b in itertools.combinations(range(3), 2):                             # every pair, at every multiple of 64 both stop at
            for t in sorted(set(at64[a]) & set(at64[b])):
                assert np.array_equal(at64[a][t][0], at64[b][t][0]), (a, b, t)
                assert_same_bank(at64[b][t][1], at64[a][t][1], f"cuttings {a} and {b} at frame {t}")
                compared.append((a, b, t))
        assert compared == [(0, 1, 1024), (0, 2, 1024), (1, 2, 128), (1, 2, 640), (1, 2, 1024)]
        st = stages[0]
        for _ in range(60):
            if st.cut_advance(4096) == [0, 0]:
                break
        assert not st.cut[:, M.TARGET].any()
        twin = stages[1]
        twin.cut_stop(False)
        assert twin.cut_tags([R(M.ABS, int(st.cut[x, M.W])) for x in movers], tags[movers]) == [len(movers), 0, 0, 0]
        assert np.array_equal(twin.db.download_cutoff()[movers], st.db.download_cutoff()[movers])
        a, b = whole_bank(st.db, st.truth), whole_bank(twin.db, twin.truth)
        for name in M.COEFFS:
            assert np.array_equal(a[name][movers], b[name][movers]), name
    finally:
        for st in stages:
            st.close()


# ---------------------------------------------------------------------------------------------- the parent's route, rendered sweeps

def test_a_tracked_chord_against_the_parents_route():
    """Eight notes with a cutoff at 4 x their own pitch: one cutoff_tags_each(TRACK) here; on a twin bank the same w turned into
    coefficients by the model and sent through skred_fxbank_ctl_tags_each_filter.  The banks download identically and render
    identically, block after block, through a sweep."""
    st = stage()
    twin = open_fx(st.bank, st.pool, st.now())
    try:
        v = np.array([10, 64, 65, 255, 256, 300, 511, 599], np.int32)
        tags = ((CH << 24) + 60 + np.arange(8)).astype(np.uint32)
        st.strike(v, tags)
        twin.stamp_list(dev_list(v).data_ptr(), len(v), fxb.STAMP_TRIGGER)
        twin.tag_list(dev_list(v).data_ptr(), tags)
        modes = [1 + k % 5 for k in range(8)]
        up, down = M.rate_q32(200.0)
        assert st.cut_tags([R(M.TRACK | BOTH, M.track_q24(4), 3 << 16, m) for m in modes], tags) == [8, 0, 0, 0]
        assert st.cut_tags([R(M.TRACK | M.GLIDE, M.track_q24(1), up_q32=up, down_q32=down)] * 8, tags) == [8, 0, 0, 0]
        for k in range(6):
            if k:
                st.cut_advance(64)
            filt = [fxb.fx_filter_each(*M.coeffs(int(st.cut[x, M.MODE]), int(st.cut[x, M.W]), int(st.cut[x, M.Q]))) for x in v]
            twin.ctl_tags_each_filter(None, None, filt, 0, N, tags)
            mix, stems = st.block()
            got_mix, got_stems = twin.render_host(st.F, st.INTERP, want_stems=True)
            assert (got_mix == mix).all() and (got_stems == stems).all(), f"block {k}: the parent's route renders another block"
            assert_same_bank(whole_bank(twin, st.truth), st.truth, f"the parent's route, block {k}")
        assert (st.cut[v, M.W] < [(int(st.bank['phase_inc'][x]) * M.track_q24(4)) >> 27 for x in v]).all()
    finally:
        st.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- purity

def test_calls_that_list_nobody_leave_the_bank_and_the_render_alone():
    """Cutoff calls that reach nobody -- a match nobody satisfies, foreign tags, advances and stops over nothing -- leave every byte of
    the bank and the rendered blocks identical to a twin without cutoff calls; a bank that never set a cutoff downloads zeros."""
    st = stage()
    bare = open_fx(st.bank, st.pool, st.now())
    try:
        bare.cutoff_stop(0, N, True)                                                    # no array: nothing to do
        res = dev_i32(4)
        sync()
        bare.cutoff_advance(0, N, 64, res.data_ptr())
        sync()
        assert host_of(res).tolist() == [0, 0, FILL, FILL]
        assert not bare.download_cutoff().any() and not bare.download_owners().any()
        voices = np.arange(100, 140, dtype=np.int32)
        tags = ((CH << 24) + 1 + np.arange(40)).astype(np.uint32)
        bare.tag_list(dev_list(voices).data_ptr(), tags)
        st.tag(voices, tags)
        rec = R(M.ABS | BOTH, 1 << 26, 1 << 16, 1)
        for k in range(4):
            if k == 1:
                assert st.cut_match(CM.channel(9), rec) == [0, 0, N, 0]
                assert st.cut_tags([rec] * 3, [0x09000001, 0x09000002, 0x09000003]) == [0, 0, 0, 0]
                assert st.cut_list([rec] * 3, [100, 101, -1], [0x09000009, int(tags[1]) ^ 1, 5]) == [0, 0, 2, 0]
            if k == 2:
                st.cut_stop(True)
                assert st.cut_advance(64) == [0, 0]
            mix, stems = st.block()
            got_mix, got_stems = bare.render_host(st.F, st.INTERP, want_stems=True)
            assert (got_mix == mix).all() and (got_stems == stems).all(), f"block {k}: the bank without cutoff calls renders another block"
        assert_same_bank(whole_bank(bare, st.truth), st.truth, "the bank without cutoff calls")
        assert not st.cut.any() and not bare.download_cutoff().any()
    finally:
        st.close()
        bare.close()


# ---------------------------------------------------------------------------------------------- combinations

def test_owner_pedal_glide_bend_and_cutoff_arrays_at_once():
    """A bank that holds all five side arrays: TRACK reads the key under the bend while the voice glides; one tag launch is followed by
    the pedal, glide, bend and cutoff clears, each on the tagged voices only."""
    st = stage()
    try:
        v = np.arange(200, 232, dtype=np.int32)
        tags = ((CH << 24) + 1 + np.arange(32)).astype(np.uint32)
        st.strike(v, tags)
        pedal = PM.new(N)
        res = dev_i32(6)
        sync()
        st.db.release_tags_pedal(0, N, tags[:20], True, res.data_ptr())                # sustain is down: held back, PENDING
        want, _, _ = PM.release_tags_pedal(st.owner, pedal, st.truth, 0, N, tags[:20], True, st.now())
        sync()
        assert want == [0, 0, 0, 20] and host_of(res).tolist() == want + [FILL, FILL]
        assert st.wheel(CHAN, BM.ratio_of(7.0)) == [32, 0, N - 32]
        u, d = GM.per_64(100.0)
        assert st.start([G(GM.FROM_SCALE, u, d, GM.scale_q16(-3))] * 32, tags) == [32, 0, 0]
        assert st.advance(64) == [32, 0]
        assert st.cut_match(CHAN, R(M.TRACK | BOTH, M.track_q24(2), 1 << 16, 1)) == [32, 0, N - 32, 0]
        assert (st.cut[v, M.W] == [(int(k) * M.track_q24(2)) >> 27 for k in st.bend[v, 0]]).all(), "TRACK reads the key, which the glide moves"
        cu, cd = M.rate_q32(100.0)
        assert st.cut_tags([R(M.TRACK | M.GLIDE, M.track_q24(6), up_q32=cu, down_q32=cd)] * 32, tags) == [32, 0, 0, 0]
        assert st.cut_advance(64) == [32, 0]
        assert np.array_equal(st.db.download_pedals(), pedal) and pedal[v[:20]].all()
        st.block()
        again = v[8:24]
        st.tag(list(again) + [-1, N], list(tags[8:24] + np.uint32(0x100)) + [5, 6])   # new notes on sixteen of the voices
        pedal[again] = 0
        assert np.array_equal(st.db.download_pedals(), pedal), "the pedal words of the tagged voices, and only those"
        assert not st.cut[again].any() and not st.bend[again].any() and not st.glide[again].any()
        assert st.cut[v[:8], M.TARGET].all() and st.cut[v[24:], M.TARGET].all()
        assert st.cut_advance(64) == [16, 0] and st.advance(64) == [16, 0]
        st.block()
    finally:
        st.close()


def test_cutoffs_through_a_shard():
    """One rank, local indices: the channel sweep, records by id, a sweep that lands and a stop through skred_fxshard_bank()."""
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
        st = DeviceCutoffStage(b, pool, c0, db=fx)
        t = [(CH << 24) | (60 + k) for k in range(3)]
        st.strike([63, 64, 256], t)
        assert st.cut_match(CHAN, R(M.TRACK | BOTH, M.track_q24(2), 1 << 16, 1), (37, 500)) == [3, 0, 497, 0]
        st.block()
        up, down = M.rate_q32(900.0)
        assert st.cut_tags([R(M.TRACK | M.GLIDE, M.track_q24(3), up_q32=up, down_q32=down), R(M.ABS, 1 << 27)], t[:2], (37, 500)) == [2, 0, 0, 0]
        res = st.cut_advance(128, (37, 500))
        assert res == [0, 1] and st.cut[63].tolist() == [(int(b["phase_inc"][63]) * M.track_q24(3)) >> 27, 0, 0, 0, 0, 1 << 16, 1, 0]
        st.block()
        st.cut_stop(True)
        st.block()
    finally:
        L.skred_shard_destroy(h)


def test_refusals_write_nothing():
    st = stage()
    n = st.n
    try:
        L = st.db.L
        st.tag([8, 16], [5, 6])
        assert st.cut_tags([R(M.ABS | BOTH, 1 << 25, 1 << 16, 1)], [5]) == [1, 0, 0, 0]      # the array exists, voice 8 has a cutoff
        dl = dev_list([8, 16, 24, 32])
        res = dev_i32(5)
        sync()
        good, zero, dup = fxb._tags([5, 6, 7, 8]), fxb._tags([5, 0, 7, 8]), fxb._tags([5, 6, 5, 8])
        ok = fxb.fx_cutoff_array(cs([R(M.ABS | BOTH, 1 << 24, 1 << 16, 1)] * 4))
        bad = fxb.fx_cutoff_array(cs([R(M.ABS | BOTH, 1 << 24, 1 << 16, 1)] * 3 + [R(M.ABS | M.GLIDE, 1 << 24, up_q32=0, down_q32=5)]))
        far = fxb.fx_cutoff_array(cs([R(M.ABS, M.W_MAX + 1)]))
        m, never = fxb.OwnerMatchC(int(CHAN[0]), int(CHAN[1])), fxb.OwnerMatchC(1, 0xFF000000)
        vp = lambda a: C.cast(a, C.c_void_p)
        h, d, rs, r, t = st.db.h, dl.data_ptr(), res.data_ptr(), vp(ok), good.ctypes.data
        CMt, CO, CT, CA, CS, DC = (L.skred_fxbank_cutoff_match, L.skred_fxbank_cutoff_owned_each, L.skred_fxbank_cutoff_tags_each,
                                   L.skred_fxbank_cutoff_advance, L.skred_fxbank_cutoff_stop, L.skred_fxbank_download_cutoff)
        assert CMt(None, 0, n, C.byref(m), r, rs, None) == BAD and CMt(h, 0, n, None, r, rs, None) == BAD and CMt(h, 0, n, C.byref(m), None, rs, None) == BAD
        assert CMt(h, 0, n, C.byref(m), vp(far), rs, None) == RANGE and CMt(h, 0, n, C.byref(never), r, rs, None) == BAD
        assert CMt(h, 0, n + 1, C.byref(m), r, rs, None) == RANGE and CMt(h, 0, 0, C.byref(m), r, rs, None) == RANGE
        assert CMt(h, -1, 4, C.byref(m), r, rs, None) == RANGE and CMt(h, n, 1, C.byref(m), r, rs, None) == RANGE
        assert CO(None, r, d, t, 4, None, rs, None) == BAD and CO(h, None, d, t, 4, None, rs, None) == BAD
        assert CO(h, r, None, t, 4, None, rs, None) == BAD and CO(h, r, d, None, 4, None, rs, None) == BAD
        assert CO(h, r, d, zero.ctypes.data, 4, None, rs, None) == BAD and CO(h, r, d, t, -1, None, rs, None) == BAD
        assert CO(h, vp(bad), d, t, 4, None, rs, None) == BAD
        assert CT(None, r, 0, n, t, 4, rs, None) == BAD and CT(h, None, 0, n, t, 4, rs, None) == BAD
        assert CT(h, r, 0, n, dup.ctypes.data, 4, rs, None) == BAD and CT(h, r, 0, n, zero.ctypes.data, 4, rs, None) == BAD
        assert CT(h, vp(bad), 0, n, t, 4, rs, None) == BAD and CT(h, vp(bad), 0, n + 1, t, 4, rs, None) == BAD
        assert CT(h, r, 0, n + 1, t, 4, rs, None) == RANGE and CT(h, r, -1, 4, t, 4, rs, None) == RANGE and CT(h, r, 0, 0, t, 4, rs, None) == RANGE
        assert CA(None, 0, n, 64, rs, None) == BAD and CA(h, 0, n, 0, rs, None) == BAD and CA(h, 0, n, 65537, rs, None) == BAD
        assert CA(h, 1, n, 64, rs, None) == RANGE and CA(h, 0, 0, 64, rs, None) == RANGE
        assert CS(None, 0, n, 1, None) == BAD and CS(h, 8, n, 1, None) == RANGE and CS(h, 0, -1, 1, None) == RANGE
        out = np.full(64, 9, np.uint32)
        assert DC(h, out.ctypes.data, n - 2, 4) == RANGE and DC(h, None, 0, 4) == BAD and DC(h, out.ctypes.data, 0, -1) == BAD
        assert (out == 9).all()
        assert CO(h, r, d, t, 0, None, rs, None) == 0 and CT(h, r, 0, n, t, 0, rs, None) == 0 and CS(h, 0, 0, 1, None) == 0   # nothing to do
        sync()
        assert (host_of(res) == FILL).all()
        st.same("after the refusals")                                             # cutoff, bend and glide words, owners, every word of the bank
        assert st.cut[8].tolist() == [1 << 25, 0, 0, 0, 0, 1 << 16, 1, 0]
        assert st.cut_match((0, 0), R(M.ABS, 1 << 26)) == [1, 1, n - 2, 0]           # ... and the bank still answers
        st.block()
    finally:
        st.close()


def test_more_cutoff_calls_than_the_ring_has_slots():
    """3 x SKRED_FX_RING_SLOTS cutoff_tags_each calls (two slots each) and as many cutoff_owned_each calls back to back on one stream,
    no host wait in between: a slot that is still in flight is waited for through its own event, and every record arrives."""
    st = stage()
    try:
        v = np.arange(N, dtype=np.int32)
        tags = (0x03000001 + v).astype(np.uint32)
        st.tag(v, tags)
        calls, per = 3 * fxb.FX_RING_SLOTS, 12
        bufs, lists = [dev_i32(6) for _ in range(2 * calls)], []
        sync()
        want = []
        for c in range(calls):
            a = v[c * 2 * per:c * 2 * per + per][::-1].copy()                       # the tags in descending order
            b = v[c * 2 * per + per:(c + 1) * 2 * per]
            if 5 in a or 5 in b:                                                    # (the voice without pitch)
                st.truth["phase_inc"][5] = 1 << 20
                st.db.ctl_list(fxb.fx_ctl(fxb.CTL_PHASE_INC, phase_inc=1 << 20), dev_list([5]).data_ptr(), 1)
            ra = [R(M.TRACK | BOTH, M.track_q24(1) + 1000 * c + j, (1 << 16) + j, 1 + j % 5) for j in range(per)]
            rb = [R(M.ABS | BOTH, (1 << 24) + 100 * c + j, (1 << 14) + c, 1 + (j + c) % 5) for j in range(per)]
            lists.append(dev_list(b))
            st.db.cutoff_tags_each(cs(ra), 0, N, tags[a], bufs[2 * c].data_ptr())
            st.db.cutoff_owned_each(cs(rb), lists[-1].data_ptr(), tags[b], 0, bufs[2 * c + 1].data_ptr())
            want.append(M.cutoff_tags_each(st.owner, st.cut, st.bend, st.inc, st.filt, ra, 0, N, tags[a])[0])
            want.append(M.cutoff_owned_each(st.owner, st.cut, st.bend, st.inc, st.filt, rb, b, tags[b]))
        sync()
        for b, w in zip(bufs, want):
            assert w[:3] == [per, 0, 0] and host_of(b).tolist() == w + [FILL, FILL]
        st.same("the run of records")
        assert int((st.cut[:, M.W] != 0).sum()) == 2 * per * calls
        st.block()
    finally:
        st.close()
