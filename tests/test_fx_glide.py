"""Portamento on the fixed-point bank on the GPU (skred_fxbank_glide_owned / _glide_tags / _glide_advance / _glide_stop /
_download_glide), byte for byte.

After every call the device is held to tests/fx_glide_model.py: download_glide == the model's words and download_owners == its owner
array on every voice, every word of the bank (skred_fxbank_download and _download_params, phase_inc among them) == the oracle's bank
after the model's stores, every d_result word == the model's count with the guard words past it untouched; mixes and stems of every
rendered block are compared bit for bit with oracle.cpuref.fx_render -- the integer mix is exact.  The clear rule's scenes are
tests/fx_glide_model.py's; tests/test_fx_glide_cpu.py asserts on the oracle alone that each of them bites.
"""
import ctypes as C

import numpy as np
import pytest

import chan_model as CM
import fx_chan_model as FCM
import fx_glide_model as GM
import fx_live_model as live
import fx_steal_model as sm
from skred_amd import fxbank as fxb
from test_fx_chan import assert_same_bank, whole_bank
from test_fx_live import dev_i32, host_of, open_fx
from test_fx_glide_cpu import CUTS

pytestmark = pytest.mark.gpu

TRIG = fxb.STAMP_TRIGGER
BAD, RANGE = -2, -4
FILL = -7
N, FIRST, COUNT = 600, 37, 500                                  # the range starts off a 64-lane boundary and crosses a 256-thread workgroup edge
G = GM.Glide
CH = 3


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


def cs(glides):
    return [g.c() for g in glides]


class DeviceFxStage(GM.FxStage):
    """fx_glide_model.FxStage with a device bank beside it: every call runs on both, and the device is compared with the model."""

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
        got = self.db.download_glide()
        bad = np.flatnonzero((got != self.glide).any(axis=1))
        assert not len(bad), f"{what}: glide words differ at {bad[:8].tolist()}: {got[bad[:4]].tolist()} / {self.glide[bad[:4]].tolist()}"
        got = self.db.download_owners()
        assert np.array_equal(got, self.owner), f"{what}: owner words differ at {np.flatnonzero(got != self.owner)[:8].tolist()}"
        assert_same_bank(whole_bank(self.db, self.truth), self.truth, what)

    def tag(self, entries, tags, count=None):
        dl, dc, res = dev_list(entries), dev_count(count), self.result(2)
        self.db.tag_list(dl.data_ptr(), tags, ptr(dc), res.data_ptr())
        return self.read(res, 2, "tag_list", super().tag(entries, tags, count))

    def strike(self, voices, tags, incs=None):
        dl = dev_list(voices)
        if incs is not None:
            for v, inc in zip(voices, incs):                                       # the key's increment, as the host knows it
                one = dev_list([v])
                self.db.ctl_list(fxb.fx_ctl(fxb.CTL_PHASE_INC, phase_inc=int(inc)), one.data_ptr(), 1)
        self.db.stamp_list(dl.data_ptr(), len(voices), TRIG)
        return super().strike(voices, tags, incs)

    def start(self, glides, tags, rng=None):
        first, count = rng or self.whole
        res = self.result(3)
        self.db.glide_tags(cs(glides), first, count, tags, res.data_ptr())
        return self.read(res, 3, f"glide_tags of {len(tags)}", super().start(glides, tags, rng))

    def start_list(self, glides, entries, tags, count=None):
        dl, dc, res = dev_list(entries), dev_count(count), self.result(3)
        self.db.glide_owned(cs(glides), dl.data_ptr(), tags, ptr(dc), res.data_ptr())
        return self.read(res, 3, "glide_owned", super().start_list(glides, entries, tags, count))

    def advance(self, frames, rng=None):
        first, count = rng or self.whole
        res = self.result(2)
        self.db.glide_advance(first, count, frames, res.data_ptr())
        return self.read(res, 2, f"glide_advance by {frames}", super().advance(frames, rng))

    def stop(self, snap, rng=None):
        first, count = rng or self.whole
        self.db.glide_stop(first, count, snap)
        super().stop(snap, rng)
        self.same(f"glide_stop snap {snap}")

    def block(self, frames=None):
        frames = frames or self.F
        got_mix, got_stems = self.db.render_host(frames, self.INTERP, want_stems=self.stems)
        mix, stems = super().block(frames)
        assert (got_mix == mix).all(), "the mix differs from the oracle's"
        if self.stems:
            assert (got_stems == stems).all(), "the stems differ from the oracle's"
        assert self.db.sample_count() == self.now()
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


def mixed_glides(gen, n, incs=None):
    """n entries of all three forms; rates from crawling to jumping; targets and scales on both sides of where the voice is."""
    out = []
    for k in range(n):
        up, down = int(gen.choice([1, 1 << 18, 1 << 24, 1 << 28, 0xFFFFFFFF])), int(gen.choice([1, 1 << 18, 1 << 24, 1 << 28, 0xFFFFFFFF]))
        form = int(gen.integers(0, 3))
        if form == 0:
            out.append(G(GM.FROM_SCALE, up, down, int(gen.choice([1, 30000, 65535, 65536, 65537, 98304, 0xFFFFFFFF]))))
        elif form == 1:
            out.append(G(GM.TO_SCALE, up, down, int(gen.choice([1, 30000, 65535, 65536, 65537, 98304, 0xFFFFFFFF]))))
        else:
            out.append(G(GM.TO_INC, up, down, target_inc=int(gen.choice([1, 70000, 30000001, 0x80000000, 0xFFFFFFFF]))))
    return out


# ---------------------------------------------------------------------------------------------- the clear rule

@pytest.mark.parametrize("name", GM.SCENES)
def test_scene_on_the_device(name):
    """A thief's tag_list and a key struck again: fx_glide_model's scenes, which fail on a bank without the clear behind the tag launch."""
    st = stage()
    try:
        assert not st.db.download_glide().any()                                    # no glide yet: zeros
        # the array must exist before the scene's tag launches: one start that nobody owns
        dl = dev_list([5])
        st.db.glide_owned(cs([G(GM.TO_INC, 1, 1, target_inc=9)]), dl.data_ptr(), [0x7FFFFFF0])
        GM.run_scene(name, st)
    finally:
        st.close()


def mono_args(n, ch):
    iq = fxb.FxIdleQueryC(0, n, fxb.IDLE_ENV_DONE, 0, 0, 0)
    return iq, sm.Query(0, n, sm.OLDEST, 0, 0, max_out=1), CM.channel(ch)


def test_restrike_through_note_on_channel():
    """Mono mode (cap 1, min_age 0): the key is struck again through skred_fxbank_note_on_channel while its glide is under way, so the
    new note takes the old note's voice and the call's own tag launch is the one that clears the words.  Then the legato the header
    orders: note_on_channel, then glide_tags(FROM_SCALE)."""
    st = stage()
    tag, v = [(CH << 24) | 60], 300
    up, down = GM.per_64(700.0)
    try:
        st.strike([v], tag, [40000003])
        assert st.start([G(GM.TO_INC, up, down, target_inc=90000001)], tag) == [1, 0, 0]
        assert st.advance(64) == [1, 0]
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
        sync()
        assert host_of(da).tolist() == [v, FILL, FILL] and host_of(dr).tolist() == res + [FILL, FILL]
        assert not st.glide[v].any()
        st.same("the re-strike")
        assert st.advance(64) == [0, 0] and st.inc[v] == 53393781, "the key struck again inherited the old note's glide"
        st.block()
        assert st.start([G(GM.FROM_SCALE, up, down, GM.scale_q16(-4))], tag) == [1, 0, 0]
        for _ in range(12):
            res = st.advance(64)
            st.block()
            if res == [0, 1]:
                break
        assert st.inc[v] == 53393781 and not st.glide.any()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- every call against the model

def test_every_call_against_the_model():
    """600 voices, the range [37, 537); 1, 2, 1023 and 1024 tags; lists with -1 holes, a voice beyond the bank, an untagged voice, a
    stolen voice and a d_count below n; all three forms, withheld starts among them; advances of 1, 63, 64, 65 and 65536 frames."""
    st = stage()
    n, first, count = N, FIRST, COUNT
    rng = (first, count)
    heads = np.arange(first, first + count, dtype=np.int32)
    gen = np.random.default_rng(n + 7)
    try:
        tags = ((CH << 24) + 1 + np.arange(len(heads))).astype(np.uint32)
        tagged = np.arange(len(heads)) % 5 != 4
        st.tag(heads[tagged], tags[tagged])
        st.tag([0, n - 1], [(CH << 24) | 0xFFFF, (CH << 24) | 0xFFFE])
        own, own_tags = heads[tagged], tags[tagged]
        order = gen.permutation(len(own))
        at = 0
        for m in (1, 2, 1023, 1024):
            pick = order[at:at + min(m, 90)]
            at += len(pick)
            t = padded_tags(own_tags[pick], m)
            t = t[gen.permutation(m)]                                               # the tags arrive in no order: the entries must follow them
            res = st.start(mixed_glides(gen, m), t, rng)
            assert res[0] + res[1] == len(pick) and res[2] == 0
        assert st.start([G(GM.TO_INC, 1, 1, target_inc=5)], [(CH << 24) | 0xFFFF], rng) == [0, 0, 0]   # carried below the range only
        assert int((st.glide[:, 0] != 0).sum()) > 100
        for frames in (1, 63, 64):
            st.advance(frames, rng)
        st.block()
        # a list with holes, a stolen voice (wrong tag), an untagged voice, a voice beyond the bank; a count shorter than n
        a, b, c, d = (int(k) for k in order[200:204])                              # voices no start has touched: their increments are the recipe's
        lst = [int(own[a]), -1, int(own[b]), int(heads[4]), n, int(own[c]), int(own[d])]
        ltags = [int(own_tags[a]), 5, 0x7FFFFFFF, 6, 7, int(own_tags[c]), int(own_tags[d])]
        gl = [G(GM.TO_INC, 1 << 24, 1 << 24, target_inc=30000001), G(GM.TO_INC, 1, 1, target_inc=1), G(GM.TO_INC, 1, 1, target_inc=1),
              G(GM.TO_INC, 1, 1, target_inc=1), G(GM.TO_INC, 1, 1, target_inc=1), G(GM.FROM_SCALE, 5, 5, 0xFFFFFFFF), G(GM.TO_SCALE, 7, 7, 98304)]
        assert st.start_list(gl, lst, ltags, count=6) == [1, 1, 2]                  # (FROM_SCALE by 65535.99..: above 32 bits, withheld)
        assert st.start_list(gl, lst, ltags) == [2, 1, 2]
        assert st.start_list(gl, lst, ltags, count=5000) == [2, 1, 2]               # a count above n; the bend composes on the old target
        for frames in (65, 65536, 64):
            st.advance(frames, rng)
        st.advance(64, (first, 1))                                                  # a range of one voice
        st.advance(64)
        st.block()
        st.stop(False, (first, 100))
        st.stop(True, (first + 100, count - 100))
        st.stop(True)
        assert not st.glide.any()
        st.block()
    finally:
        st.close()


def test_fifteen_hundred_voices_and_three_block_cuttings():
    """1 500 voices (6 workgroups, the last one partial), 1 024 of them gliding at rates from crawling to jumping.  512 frames advanced as
    8 x 64, as 1 x 512 and as 37 + 100 + 27 + 348 on three banks: each held to the model after every call, and to each other."""
    n = 1500
    stages = [stage(n, stems=False) for _ in CUTS]
    try:
        v = np.arange(n, dtype=np.int32)
        tags = (0x05000000 + 1 + v).astype(np.uint32)
        pick = np.random.default_rng(3).permutation(n)[:1024]
        glides = mixed_glides(np.random.default_rng(4), 1024)
        for st, cut in zip(stages, CUTS):
            st.tag(v, tags)
            res = st.start(glides, tags[pick])
            assert res[0] > 500 and res[0] + res[1] == 1024
            for frames in cut:
                st.advance(frames)
        a = stages[0]
        assert int((a.glide[:, 0] != 0).sum()) > 100, "some must still be on the way"
        for st in stages[1:]:
            assert np.array_equal(st.glide, a.glide) and np.array_equal(st.inc, a.inc)
            assert np.array_equal(st.db.download_glide(), a.db.download_glide())
        a.block()
    finally:
        for st in stages:
            st.close()


def test_many_workgroups_feed_the_counts():
    """70 000 voices: 274 workgroups of the range kernels add to the result words, which are exact.  The advance runs twice in a row on
    one stream with no host wait in between: the second starts from result words the stream cleared again."""
    n = 70000
    st = stage(n, stems=False)
    try:
        v = np.arange(n, dtype=np.int32)
        tags = ((v % 16).astype(np.uint32) << np.uint32(24)) | (1 + v // 16).astype(np.uint32)
        st.tag(v, tags)
        up, down = GM.per_64(300.0)
        mine = v[v % 16 == CH]
        for lo in range(0, len(mine), 1024):
            part = mine[lo:lo + 1024]
            far = np.where(part % 32 == CH, st.inc[part] + 3, (st.inc[part].astype(np.uint64) * 3 // 2).clip(1, 0xFFFFFFFF))
            gl = [G(GM.TO_INC, up, down, target_inc=int(t)) for t in far]
            dl = dev_list(part)
            st.db.glide_owned(cs(gl), dl.data_ptr(), tags[part])
            assert GM.start_owned(st.owner, st.glide, st.inc, gl, part, tags[part]) == [len(part), 0, 0]
        st.same("the channel's glides")
        bufs = [dev_i32(4) for _ in range(2)]
        sync()
        for b in bufs:
            st.db.glide_advance(0, n, 64, b.data_ptr())
        one, two = GM.advance(st.glide, st.inc, 0, n, 64), GM.advance(st.glide, st.inc, 0, n, 64)
        sync()
        assert one[0] + one[1] == len(mine) and one[1] > 1000 and two == [one[0], 0] and one[0] > 1000
        for b, w in zip(bufs, (one, two)):
            assert host_of(b).tolist() == w + [FILL, FILL], (host_of(b).tolist(), w)
        st.same("two advances")
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- twins

def test_a_twin_driven_by_ctl_list_renders_the_same_bits():
    """One bank glides on the device; a twin never makes a glide call and receives the model's increments through
    skred_fxbank_ctl_list(SKRED_CTL_PHASE_INC) ahead of every block.  Mixes and stems are bit-equal, and both equal the oracle's."""
    st = stage()
    twin = open_fx(st.bank, st.pool, st.now())
    try:
        voices = np.array([5, 63, 64, 255, 256, 300, 511, 599], np.int32)
        tags = (0x03000000 + 60 + np.arange(len(voices))).astype(np.uint32)
        st.tag(voices, tags)
        up, down = GM.per_64(500.0)
        gl = [G(GM.FROM_SCALE, up, down, GM.scale_q16(-7 + 2 * k)) for k in range(len(voices))]
        assert st.start(gl, tags) == [len(voices), 0, 0]
        arrived = 0
        for k in range(24):
            if k:
                arrived += st.advance(64)[1]
            for v in voices:
                one = dev_list([v])
                twin.ctl_list(fxb.fx_ctl(fxb.CTL_PHASE_INC, phase_inc=int(st.inc[v])), one.data_ptr(), 1)
            mix, stems = st.block()                                               # (the device's block is held to the oracle's inside)
            got_mix, got_stems = twin.render_host(st.F, st.INTERP, want_stems=True)
            assert (got_mix == mix).all() and (got_stems == stems).all(), f"block {k}: the twin renders another block"
        assert arrived == len(voices) and np.array_equal(st.inc[voices], st.bank["phase_inc"][voices]), "every slide landed on its key"
        assert_same_bank(whole_bank(twin, st.truth), st.truth, "the twin")
        assert not twin.download_glide().any()
    finally:
        st.close()
        twin.close()


def test_calls_that_start_nothing_leave_the_render_alone():
    """A bank whose glide calls start nothing (wrong tags, withheld starts, advances and stops over nothing) renders blocks bit-identical
    to a twin without them; a bank without the array gets SKRED_OK and a cleared d_result from advance, zeros from the download."""
    st = stage()
    bare = open_fx(st.bank, st.pool, st.now())
    try:
        res = dev_i32(4)
        sync()
        bare.glide_advance(FIRST, COUNT, 64, res.data_ptr())
        bare.glide_advance(0, N, 65536)                                             # no result asked for
        bare.glide_stop(0, N, True)
        sync()
        assert host_of(res).tolist() == [0, 0, FILL, FILL] and not bare.download_glide().any() and not bare.download_owners().any()
        voices = np.arange(100, 140, dtype=np.int32)
        tags = (0x03000001 + np.arange(40)).astype(np.uint32)
        dl = dev_list(voices)
        bare.tag_list(dl.data_ptr(), tags)
        st.tag(voices, tags)
        for k in range(4):
            if k == 1:
                assert st.start([G(GM.TO_INC, 9, 9, target_inc=77)] * 3, [0x09000001, 0x09000002, 0x09000003]) == [0, 0, 0]
                assert st.start_list([G(GM.FROM_SCALE, 9, 9, 0xFFFFFFFF)] * 2 + [G(GM.TO_INC, 9, 9, target_inc=5)], [100, 101, 102],
                                     [int(tags[0]), int(tags[1]), 0x09000009]) == [0, 2, 1]
            if k >= 1:
                assert st.advance(64) == [0, 0]
            if k == 3:
                st.stop(True)
            mix, stems = st.block()
            got_mix, got_stems = bare.render_host(st.F, st.INTERP, want_stems=True)
            assert (got_mix == mix).all() and (got_stems == stems).all(), f"block {k}: the bank without glide calls renders another block"
        assert_same_bank(whole_bank(bare, st.truth), st.truth, "the bank without glide calls")
        assert not st.glide.any()
    finally:
        st.close()
        bare.close()


# ---------------------------------------------------------------------------------------------- a shard

def test_glides_through_a_shard():
    """One rank, local indices: a start by id, advances and a snap through skred_fxshard_bank()."""
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
        t = [(CH << 24) | (60 + k) for k in range(3)]
        st.strike([63, 64, 256], t)
        up, down = GM.per_64(300.0)
        assert st.start([G(GM.FROM_SCALE, up, down, GM.scale_q16(-12))] * 3, t, (FIRST, COUNT)) == [3, 0, 0]
        st.block()
        assert st.advance(64, (FIRST, COUNT)) == [3, 0]
        st.block()
        st.stop(True, (0, 100))
        assert st.inc[63] == b["phase_inc"][63] and st.inc[64] == b["phase_inc"][64] and st.inc[256] != b["phase_inc"][256]
        assert st.advance(640) == [1, 0]
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
        assert st.start([G(GM.TO_INC, 1 << 20, 1 << 20, target_inc=70000)], [5]) == [1, 0, 0]   # the array exists, voice 8 glides
        dl = dev_list([8, 16, 24, 32])
        res = dev_i32(4)
        sync()
        good, zero, dup = fxb._tags([5, 6, 7, 8]), fxb._tags([5, 0, 7, 8]), fxb._tags([5, 6, 5, 8])
        ok = fxb.glide_array(cs([G(GM.TO_INC, 1, 1, target_inc=9)] * 4))
        bad_sets = [G(3, 1, 1, 1, 1), G(0, 1, 1, 1, 1), G(1, 0, 1, 1), G(2, 1, 0, 1), G(1, 1, 1, 0), G(2, 1, 1, 0), G(4, 1, 1, 1, 0),
                    G(1, 1, 1, 1, reserved=(0, 1, 0))]
        h, d, rs, g, t = st.db.h, dl.data_ptr(), res.data_ptr(), C.cast(ok, C.c_void_p), good.ctypes.data
        GO, GT, AD, SP, DG = (L.skred_fxbank_glide_owned, L.skred_fxbank_glide_tags, L.skred_fxbank_glide_advance, L.skred_fxbank_glide_stop,
                              L.skred_fxbank_download_glide)
        assert GO(None, g, d, t, 4, None, rs, None) == BAD and GO(h, None, d, t, 4, None, rs, None) == BAD
        assert GO(h, g, None, t, 4, None, rs, None) == BAD and GO(h, g, d, None, 4, None, rs, None) == BAD
        assert GO(h, g, d, zero.ctypes.data, 4, None, rs, None) == BAD and GO(h, g, d, t, -1, None, rs, None) == BAD
        assert GT(None, g, 0, n, t, 4, rs, None) == BAD and GT(h, None, 0, n, t, 4, rs, None) == BAD
        assert GT(h, g, 0, n, dup.ctypes.data, 4, rs, None) == BAD and GT(h, g, 0, n, zero.ctypes.data, 4, rs, None) == BAD
        assert GT(h, g, 0, n + 1, t, 4, rs, None) == RANGE and GT(h, g, -1, 4, t, 4, rs, None) == RANGE and GT(h, g, 0, 0, t, 4, rs, None) == RANGE
        for b in bad_sets:
            arr = fxb.glide_array(cs([G(GM.TO_INC, 1, 1, target_inc=9)] * 3 + [b]))
            assert GO(h, C.cast(arr, C.c_void_p), d, t, 4, None, rs, None) == BAD and GT(h, C.cast(arr, C.c_void_p), 0, n, t, 4, rs, None) == BAD
            assert fxb.fx_glide_check(arr) == BAD == GM.check([b])
        assert AD(None, 0, n, 64, rs, None) == BAD and AD(h, 0, n, 0, rs, None) == BAD and AD(h, 0, n, 65537, rs, None) == BAD
        assert AD(h, 0, n + 1, 64, rs, None) == RANGE and AD(h, 0, 0, 64, rs, None) == RANGE and AD(h, n, 1, 64, rs, None) == RANGE
        assert SP(None, 0, n, 1, None) == BAD and SP(h, 8, n, 1, None) == RANGE and SP(h, 0, -1, 1, None) == RANGE
        out = np.full(16, 9, np.uint32)
        assert DG(h, out.ctypes.data, n - 2, 4) == RANGE and DG(h, None, 0, 4) == BAD and DG(h, out.ctypes.data, 0, -1) == BAD
        assert (out == 9).all()
        assert GO(h, g, d, t, 0, None, rs, None) == 0 and GT(h, g, 0, n, t, 0, rs, None) == 0 and SP(h, 0, 0, 1, None) == 0   # nothing to do
        sync()
        assert (host_of(res) == FILL).all()
        st.same("after the refusals")                                             # glide words, owners and every word of the bank
        assert st.glide[8, 0] == 70000
        assert st.advance(64) == [1, 0]                                            # ... and the bank still answers
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- the staging ring

def test_more_start_calls_than_the_ring_has_slots():
    """3 x SKRED_FX_RING_SLOTS glide_tags calls (two slots each) and as many glide_owned calls back to back on one stream, no host wait
    in between: a slot that is still in flight is waited for through its own event, and every entry arrives."""
    st = stage()
    try:
        v = np.arange(N, dtype=np.int32)
        tags = (0x03000001 + v).astype(np.uint32)
        st.tag(v, tags)
        calls = 3 * fxb.FX_RING_SLOTS
        per = 12
        up, down = GM.per_64(200.0)
        bufs, lists = [dev_i32(5) for _ in range(2 * calls)], []
        sync()
        want = []
        for c in range(calls):
            a = v[c * 2 * per:c * 2 * per + per][::-1].copy()                       # the tags in descending order
            b = v[c * 2 * per + per:(c + 1) * 2 * per]
            ga = [G(GM.TO_INC, up, down, target_inc=int(st.inc[x]) * 3 // 2 + c) for x in a]
            gb = [G(GM.FROM_SCALE, up, down, 65536 - 3000 - c) for _ in b]
            lists.append(dev_list(b))
            st.db.glide_tags(cs(ga), 0, N, tags[a], bufs[2 * c].data_ptr())
            st.db.glide_owned(cs(gb), lists[-1].data_ptr(), tags[b], 0, bufs[2 * c + 1].data_ptr())
            want.append(GM.start_tags(st.owner, st.glide, st.inc, ga, 0, N, tags[a])[0])
            want.append(GM.start_owned(st.owner, st.glide, st.inc, gb, b, tags[b]))
        sync()
        for b, w in zip(bufs, want):
            assert w == [per, 0, 0] and host_of(b).tolist() == w + [FILL, FILL]
        st.same("the run of starts")
        assert st.advance(64) == [2 * per * calls, 0]
        st.block()
    finally:
        st.close()
