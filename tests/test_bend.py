"""The pitch wheel on the device (skred_bank_bend_match / _bend_owned_each / _bend_tags_each / _bend_clear / _download_bend, and the
glide calls on a bank that has a bend array), byte for byte.

After every call the device is held to tests/bend_model.py: download_bend == the model's words, every controller word of every voice
(download_ctl: voice_phase_inc among them) == the oracle's bank, which receives the model's increments, the glide, pedal and owner
words and the envelope clocks as tests/test_glide.py's rig holds them, every d_result word == the model's count with the guard words
past it untouched.  Blocks are compared with oracle.cpuref; a twin driven through skred_bank_ctl_slots(SKRED_CTL_PHASE_INC) with the
model's increments must hold the same bytes.  Increments, keys and products stay in the normal fp32 range or are exactly 0, 3e38 or
the smallest denormal (tests/bend_model.py says why).

The assertions marked CLEAR RULE fail on tests/bend_model.py with CLEAR_RULE = False -- and on a library whose tag launch does not
clear the bend words the device fails them against the model as it stands.
"""
import ctypes as C

import numpy as np
import pytest

import bend_model as BM
import chan_model as CHM
import ctl_model as CM
import glide_model as GM
import owner_model as OM
import owner_scenes as OS
import slot_model as SM
import slot_steal_model as M
from oracle import cpuref
from skred_amd import device
from skred_amd.bank import slot_query
from skred_amd.device import ctl
from steal_model import ENV, FIN, OLDEST
from test_glide import GlideRig, bank_words, banks_same
from test_idle import open_bank, render_blocks, traffic_bank
from test_owner import FILL, padded_tags
from test_slot_steal import plain_bank, playing_patch

F = 64
BAD, RANGE = -2, -4
SEMI = 2.0 ** (1.0 / 12.0)
FROM, TO = GM.FROM_SCALE, GM.TO_SCALE
TINY = np.array([1], np.uint32).view(np.float32)[0]


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


class BendRig(GlideRig):
    """tests/test_glide.py's rig with the model's bend words beside the glide words: every call runs on the device and on the model."""

    def __init__(self, dev, bank, tables, g, setup=None, db=None):
        super().__init__(dev, bank, tables, g, setup, db)
        self.bend = BM.new(bank.n)

    def same(self, tag):
        super().same(tag)
        got = self.db.download_bend()
        bad = np.flatnonzero((got != self.bend).any(axis=1))
        assert not len(bad), f"{tag}: bend words differ at {bad[:8].tolist()}: {got[bad[:8]].tolist()} / {self.bend[bad[:8]].tolist()}"
        a = self.bank.copy()
        self.db.download_ctl(a)
        assert not CM.words_differ(a, self.truth), f"{tag}: controller words differ from the model: {CM.words_differ(a, self.truth)}"
        assert not self.db.download_pedals().any(), f"{tag}: a pedal word was written"

    def tag(self, entries, tags, K, count=None, tag=""):
        BM.tag_clear(self.bend, entries, len(tags), count, K)
        super().tag(entries, tags, K, count, tag)

    def match(self, first, count, K, vmask, m, ratio, tag=""):
        res = self.result(3)
        self.db.bend_match(first, count, K, vmask, device.owner_match(*m), float(np.float32(ratio)), res.data_ptr())
        return self.check(res, 3, BM.bend_match(self.owner, self.bend, self.inc(), first, count, K, vmask, m, ratio), tag or f"match {ratio}")

    def owned_each(self, ratios, K, vmask, entries, tags, count=None, tag=""):
        import torch
        dl, res = self.dev_list(entries), self.result(3)
        dc = None if count is None else torch.tensor([count, 4321], dtype=torch.int32, device="cuda")
        self.db.bend_owned_each(ratios, K, vmask, dl.data_ptr(), tags, dc.data_ptr() if dc is not None else 0, res.data_ptr())
        return self.check(res, 3, BM.bend_owned_each(self.owner, self.bend, self.inc(), ratios, K, vmask, entries, tags, count), tag)

    def tags_each(self, ratios, first, count, K, vmask, tags, tag=""):
        res = self.result(3)
        self.db.bend_tags_each(ratios, first, count, K, vmask, tags, res.data_ptr())
        want, lst = BM.bend_tags_each(self.owner, self.bend, self.inc(), ratios, first, count, K, vmask, tags)
        return self.check(res, 3, want, tag), lst

    def bend_clear(self, first, count, snap, tag=""):
        self.db.bend_clear(first, count, snap)
        BM.clear(self.bend, self.inc(), first, count, snap)
        self.same(tag or f"bend_clear snap {snap}")

    # the glide calls: the model's under a bend array
    def start_owned(self, glides, K, vmask, entries, tags, count=None, tag=""):
        import torch
        dl, res = self.dev_list(entries), self.result(3)
        dc = None if count is None else torch.tensor([count, 4321], dtype=torch.int32, device="cuda")
        self.db.glide_owned([g.c() for g in glides], K, vmask, dl.data_ptr(), tags, dc.data_ptr() if dc is not None else 0, res.data_ptr())
        return self.check(res, 3, BM.glide_start_owned(self.owner, self.glide, self.bend, self.inc(), glides, K, vmask, entries, tags, count), tag)

    def start_tags(self, glides, first, count, K, vmask, tags, tag=""):
        res = self.result(3)
        self.db.glide_tags([g.c() for g in glides], first, count, K, vmask, tags, res.data_ptr())
        want, lst = BM.glide_start_tags(self.owner, self.glide, self.bend, self.inc(), glides, first, count, K, vmask, tags)
        return self.check(res, 3, want, tag), lst

    def advance(self, first, count, frames, tag=""):
        res = self.result(2)
        self.db.glide_advance(first, count, frames, res.data_ptr())
        return self.check(res, 2, BM.glide_advance(self.glide, self.bend, self.inc(), first, count, frames), tag or f"advance {frames}")

    def stop(self, first, count, snap, tag=""):
        self.db.glide_stop(first, count, snap)
        BM.glide_stop(self.glide, self.bend, self.inc(), first, count, snap)
        self.same(tag or f"stop snap {snap}")


def wheel(n, seed):
    """n wheel positions within two semitones of the centre, none at it"""
    r = np.atleast_1d(BM.ratio_of(np.random.default_rng(seed).uniform(-2.0, 2.0, n)))
    r[r == 1.0] = np.float32(SEMI)
    return r


def odd_increments(inc):
    inc[5::23] = np.float32(0.0)                                     # withheld: a zero key
    inc[7::29] = np.float32(3e38)                                    # withheld upwards: the product overflows
    inc[11::31] *= np.float32(-1.0)                                  # negative increments bend on their side of zero
    inc[13::37] = TINY                                               # the smallest denormal: times 0.25 it is zero, withheld
    assert (np.abs(inc[(inc != 0) & (inc != TINY)]) > 1e-30).all()


# ---------------------------------------------------------------------------------------------- 1. every call against the model

@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 4, 64])
def test_every_call_against_the_model(dev, K):
    """1500 voices (1472 at K = 64: whole slots).  The channel wheel over the whole bank, with a mask that leaves voices out, and over
    a range off the workgroup span (slots 9 .. 133 at K = 4; the same voices' slots at the other K); per-note bends by note id with 1,
    2, 1023 and 1024 tags, and on a list with a hole, a slot past the bank, a stolen slot and a count word; zero, huge, negative and
    denormal increments; the centre; clear with and without snap."""
    n = 1500 // K * K
    bank, tables, g, now = plain_bank(n)
    odd_increments(bank["voice_phase_inc"])
    r = BendRig(dev, bank, tables, g)
    slots = np.arange(0, n, K, dtype=np.int32)
    full = (1 << K) - 1
    part = full if K == 1 else (1 << (K - 1)) | 1
    gen = np.random.default_rng(40 + K)
    try:
        chan = (gen.integers(1, 4, len(slots)).astype(np.uint32) << np.uint32(24))
        all_tags = (chan + np.arange(len(slots), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        all_tags[::17] = 0                                           # untagged slots match nothing
        r.tag(slots, all_tags, K, tag="every slot")
        assert not r.db.download_bend().any()
        original = r.inc().copy()
        want = r.match(0, n, K, full, (2 << 24, 0xFF000000), 1.5, tag="channel 2 up")
        assert want[0] > 50 and want[1] > 0 and want[2] > len(slots) // 2
        want = r.match(0, n, K, part, (0, 0), 0.25, tag="every tagged slot down, masked")
        assert want[1] > 0
        first, count = (36 // K * K, (536 - 36 // K * K) // K * K)   # slots 9 .. 133 at K = 4: off the 256-voice span at both ends
        if K == 4:
            assert (first, count) == (36, 500)
        want = r.match(first, count, K, full, (1 << 24, 0xFF000000), float(np.float32(SEMI)), tag="a range off the span")
        assert want[0] > 0 and want[2] > 0
        out = np.r_[0:first, first + count:n]
        r.block("a block while bent")
        inside = slots[(slots >= first) & (slots < first + count) & (r.owner[slots] != 0)]
        order = gen.permutation(len(inside))
        at = 0
        for m in (1, 2, 1023, 1024):
            take = min(m, max(1, len(inside) // 5))
            pick = inside[order[at:at + take]]
            at += take
            tags = padded_tags(r.owner[pick], m)[gen.permutation(m)]  # (the tags unsorted: the sort and the permutation have work to do)
            ratios = wheel(m, m)
            ratios[::5] = np.float32(1.0)                            # the centre among them
            want, lst = r.tags_each(ratios, first, count, K, full if m != 2 else part, tags, tag=f"{m} tags")
            assert int((lst >= 0).sum()) == len(pick) and want[2] == 0
        tagged = slots[r.owner[slots] != 0]
        rest = tagged[~np.isin(tagged, inside[order[:at]])]
        entries = np.array([rest[0], -1, n, rest[1], rest[2], rest[3]], np.int32)
        tags = np.array([r.owner[rest[0]], 5, 6, r.owner[rest[1]] ^ 0x00800000, r.owner[rest[2]], r.owner[rest[3]]], np.uint32)
        before = r.bend[rest[3]:rest[3] + K].copy()
        want = r.owned_each(wheel(6, 9), K, part, entries, tags, count=5, tag="a list")
        assert want[2] == 1 and (r.bend[rest[3]:rest[3] + K] == before).all()
        assert r.bend[:, 0].any() and r.inc()[out].tobytes() != original[out].tobytes()
        r.bend_clear(first, (count // 2) // K * K, False)
        r.bend_clear(0, K, True)
        want = r.match(0, n, K, full, (0, 0), 1.0, tag="the centre")
        assert want[1] == 0 and not r.bend.any()
        r.block("a block after the centre")
        assert r.db.list_violations() == 0
    finally:
        r.close()


@pytest.mark.gpu
def test_many_workgroups_feed_the_counts(dev):
    """70 000 voices, K = 2: 274 workgroups of the match pass add to the result words.  Two bends in a row on one stream with no host
    wait in between: the second starts from result words the stream cleared again."""
    import torch
    n, K = 70000, 2
    bank, tables, g, now = plain_bank(n)
    r = BendRig(dev, bank, tables, g)
    try:
        heads = np.arange(0, n, K, dtype=np.int32)
        k = np.arange(len(heads))
        tags = ((np.uint32(1) + (k % 3).astype(np.uint32) << np.uint32(24)) + k.astype(np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(heads, tags, K, tag="every slot")
        original = r.inc().copy()
        bufs = [torch.full((5,), FILL, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        m = (2 << 24, 0xFF000000)
        r.db.bend_match(0, n, K, 3, device.owner_match(*m), 1.25, bufs[0].data_ptr())
        r.db.bend_match(0, n, K, 3, device.owner_match(0, 0), 0.75, bufs[1].data_ptr())
        first = BM.bend_match(r.owner, r.bend, r.inc(), 0, n, K, 3, m, 1.25)
        second = BM.bend_match(r.owner, r.bend, r.inc(), 0, n, K, 3, (0, 0), 0.75)
        torch.cuda.synchronize()
        assert first[0] > 20000 and first[2] > 20000 and second == [n, 0, 0]
        for b, w in zip(bufs, (first, second)):
            assert b.cpu().numpy().tolist() == w + [FILL, FILL], (b.cpu().numpy().tolist(), w)
        r.same("two bends")
        r.match(0, n, K, 3, (0, 0), 1.0, tag="the centre")
        assert r.inc().tobytes() == original.tobytes() and not r.bend.any()
        r.block("back at the keys")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 2. twins, taps, the oracle

@pytest.mark.gpu
@pytest.mark.parametrize("family", ["one voice per lane", "two per lane"])
def test_a_bent_chord_against_the_oracle_and_a_twin(dev, family):
    """tests/test_glide.py's two banks.  Three slots of one channel follow the wheel (bend_match ahead of every block; the last
    message is the centre), one of them with a per-note bend on top in some blocks.  A twin never hears of a bend: it receives the
    model's increments through skred_bank_ctl_slots(SKRED_CTL_PHASE_INC) ahead of every block.  The stems of the three slots through
    taps must be the oracle's bit for bit; state, taps, mix and kernel family must be the twin's.  After the centre the bank is, in
    every byte of its download, a twin's that was never bent, and the bend words are zero."""
    import torch
    two = family == "two per lane"
    if two:
        n, K, vmask = 512, 8, 0xFF
        bank, tables, g = traffic_bank(n)
        setup = lambda d: d.fast2_min_voices(0)   # noqa: E731
    else:
        n, K, vmask = 256, 4, 0xF
        bank, tables, g, K = playing_patch("3sk", n, (0, 1, 2))
        setup = None
    r = BendRig(dev, bank, tables, g, setup)
    twin = open_bank(dev, bank, tables, g, setup)
    try:
        slots = [4 * K, 21 * K, 63 * K]
        if two:
            dl = r.dev_list(slots)
            for d in (r.db, twin):
                d.stamp_slots(dl.data_ptr(), len(slots), K, 0xFE, SM.STAMP_TRIGGER)
            SM.stamp(r.truth, SM.stamp_voices(slots, len(slots), None, K, 0xFE, n), SM.STAMP_TRIGGER, r.now())
        tags = np.array([3 << 24 | 60, 3 << 24 | 64, 3 << 24 | 67], np.uint32)
        r.tag(slots, tags, K, tag="the chord")
        original = r.inc().copy()
        voices = np.array([s + l for s in slots for l in range(K)], np.int32)
        d_taps, t_taps = (torch.zeros((F, len(voices), 2), dtype=torch.float32, device="cuda") for _ in range(2))
        r.db.set_taps(voices, d_taps.data_ptr())
        twin.set_taps(voices, t_taps.data_ptr())
        lists = [r.dev_list([s]) for s in slots]
        positions = [0.5, 1.0, 2.0, 1.3, -0.7, -2.0, -1.0, 0.0]
        kernels = set()
        for blk, semis in enumerate(positions):
            want = r.match(0, n, K, vmask, (3 << 24, 0xFF000000), BM.ratio_of(semis), tag=f"wheel at {semis}")
            assert want[0] == 3 * K and want[1] == 0
            if blk in (2, 3):
                r.tags_each([BM.ratio_of(semis + 0.25)], 0, n, K, vmask, tags[1:2], tag="a per-note bend on top")
            for s, dl in zip(slots, lists):
                twin.ctl_slots([ctl(CM.PHASE_INC, phase_inc=float(r.inc()[s + l])) for l in range(K)], vmask, dl.data_ptr(), 1)
            x, y = render_blocks(r.db, (F,))[0], render_blocks(twin, (F,))[0]
            ref = cpuref.render(r.truth, r.gl, r.tables, F, 0, want_stems=True)
            got = d_taps.cpu().numpy()
            assert r.db.last_taps() == twin.last_taps() == len(voices)
            assert got.tobytes() == np.ascontiguousarray(ref["stems"][:, voices, :]).tobytes(), f"block {blk}: taps differ from the oracle"
            assert got.tobytes() == t_taps.cpu().numpy().tobytes(), f"block {blk}: taps differ from the twin's"
            assert x.tobytes() == y.tobytes(), f"block {blk}: the mix differs from the twin's"
            assert r.db.last_kernel() == twin.last_kernel()
            kernels.add(r.db.last_kernel())
            banks_same(r.db, twin, bank, f"block {blk}")
            a = bank.copy()
            r.db.download(a)
            assert not a.rw_equal(r.truth), f"block {blk}: state differs from the oracle: {a.rw_equal(r.truth)}"
        assert (kernels == {3}) if two else (3 not in kernels), kernels
        assert r.inc().tobytes() == original.tobytes() and not r.bend.any() and not r.db.download_bend().any()
        assert r.db.list_violations() == twin.list_violations() == 0
    finally:
        r.db.set_taps([], 0)
        twin.set_taps([], 0)
        r.close()
        twin.close()


@pytest.mark.gpu
def test_wheel_up_wheel_to_centre_is_the_never_bent_bank(dev):
    """200 wheel messages on a channel, the last at centre: every byte of the bank's download equals a twin's that made no bend call,
    and the bend words are zero.  (The INC_SCALE route does not return: tests/test_bend_cpu.py counts the voices.)"""
    n, K = 1024, 4
    bank, tables, g, now = plain_bank(n)
    r = BendRig(dev, bank, tables, g)
    twin = open_bank(dev, bank, tables, g)
    try:
        heads = np.arange(0, n, K, dtype=np.int32)
        tags = (np.uint32(3 << 24) + np.arange(len(heads), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(heads, tags, K, tag="every slot")
        twin.tag_slots(r.dev_list(heads).data_ptr(), tags, K)
        m = device.owner_match(3 << 24, 0xFF000000)
        for ratio in wheel(199, 7):
            r.db.bend_match(0, n, K, 0xF, m, float(ratio))
            BM.bend_match(r.owner, r.bend, r.inc(), 0, n, K, 0xF, (3 << 24, 0xFF000000), ratio)
        r.same("199 messages")
        assert r.bend[:, 0].all() and r.inc().tobytes() != bank["voice_phase_inc"].tobytes()
        assert r.match(0, n, K, 0xF, (3 << 24, 0xFF000000), 1.0, tag="the centre") == [n, 0, 0]
        banks_same(r.db, twin, bank, "after the centre")
        assert not r.db.download_bend().any() and r.inc().tobytes() == bank["voice_phase_inc"].tobytes()
        x, y = render_blocks(r.db, (F,))[0], render_blocks(twin, (F,))[0]
        assert x.tobytes() == y.tobytes()
        banks_same(r.db, twin, bank, "a block later")
    finally:
        r.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 3. glides under a bend, the clear rule

def channel_scene(dev):
    bank, tables, g = OS.bank()
    r = BendRig(dev, bank, tables, g)
    iq = slot_query(0, OS.N, OS.K, OS.MMASK, FIN | ENV, OS.SETTLE, 0, 0)
    sq = M.SlotQuery(0, OS.N, OS.K, OS.MMASK, OLDEST, 0)
    return r, iq, sq


def strike(r, iq, sq, match, tag, seed, expect_slot):
    """one note through skred_bank_note_on_channel under cap 1 on `match`, on the device and on the models; returns the slot"""
    import torch
    from test_slots import slot_notes
    K = OS.K
    want, res, _ = CHM.burst(r.truth, r.now(), r.owner, iq, sq, match, 1, 1)
    assert want.tolist() == [expect_slot], (want, res)
    notes = slot_notes(1, K, OS.VMASK, seed, [SM.SET_PHASE])
    da = torch.full((3,), FILL, dtype=torch.int32, device="cuda")
    dr = torch.full((6,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.db.note_on_channel(notes, [tag], iq, sq.c(), device.owner_match(*match), 1, OS.VMASK, da.data_ptr(), dr.data_ptr())
    SM.store_notes((r.truth,), r.truth, notes, K, OS.VMASK, want, r.now())
    OM.tag_slots(r.owner, want, [tag], None, K)
    GM.tag_clear(r.glide, want, 1, None, K)
    BM.tag_clear(r.bend, want, 1, None, K)
    torch.cuda.synchronize()
    assert da.cpu().numpy().tolist() == [expect_slot, FILL, FILL] and dr.cpu().numpy().tolist() == res + [FILL, FILL]
    return np.array([np.float32(notes[l].phase_inc) for l in range(K)], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("cuts", [(64,) * 8, (37, 100, 27, 348)])
def test_a_glide_under_a_bend_lands_on_target_times_ratio(dev, cuts):
    """A note struck under a deflected wheel in the documented order -- skred_bank_note_on_channel, skred_bank_bend_tags_each with the
    channel's ratio, skred_bank_glide_tags(FROM_SCALE) last -- and advanced over 512 frames in two cuttings: it lands on target *
    ratio bit for bit, and the wheel at centre then gives the note-on's bits."""
    r, iq, sq = channel_scene(dev)
    K, N = OS.K, OS.N
    try:
        slot = int(OS.others()[5])
        tag = 3 << 24 | 60
        r.tag([slot], [tag], K, tag="the old key")
        struck = strike(r, iq, sq, (tag, 0xFFFFFFFF), tag, 3, slot)
        r.same("the note-on")
        ratio = BM.ratio_of(1.5)
        assert r.tags_each([ratio], 0, N, K, OS.VMASK, [tag], tag="the wheel's position")[0] == [K, 0, 0]
        up, down = GM.per_64(450.0)                                   # 0.65 semitones per step: three semitones take five of the eight steps
        assert r.start_tags([GM.Glide(FROM, up, down, np.float32(SEMI ** -3))], 0, N, K, OS.VMASK, [tag], tag="slide into the note")[0] == [K, 0, 0]
        vs = np.arange(slot, slot + K)
        assert (r.glide[vs, 0] == struck.view(np.uint32)).all() and (r.bend[vs, 1] == BM.bits(ratio)).all()
        arrived = 0
        for f in cuts:
            arrived += r.advance(0, N, f)[1]
            assert (r.inc().view(np.uint32)[vs] == BM.mul(r.bend[vs, 0], r.bend[vs, 1])).all()
        assert arrived == K and not r.glide.any()
        assert r.inc()[vs].tobytes() == (struck * ratio).astype(np.float32).tobytes(), "not target * ratio"
        r.block("landed under the wheel")
        assert r.match(0, N, K, OS.VMASK, (3 << 24, 0xFF000000), 1.0, tag="the centre")[0] == K
        assert r.inc()[vs].tobytes() == struck.tobytes() and not r.bend.any()
        # ... and TO_SCALE with a snap: the key stays, the target is the key's; the snap stores target * ratio
        r.tags_each([ratio], 0, N, K, OS.VMASK, [tag], tag="up again")
        assert r.start_tags([GM.Glide(TO, up, down, np.float32(SEMI ** 2))], 0, N, K, OS.VMASK, [tag], tag="legato")[0] == [K, 0, 0]
        assert (r.bend[vs, 0] == struck.view(np.uint32)).all()
        r.advance(0, N, 64)
        r.stop(0, N, True, tag="snap")
        two = (struck * np.float32(SEMI ** 2)).astype(np.float32)
        assert (r.bend[vs, 0] == two.view(np.uint32)).all() and r.inc()[vs].tobytes() == (two * ratio).astype(np.float32).tobytes()
        r.block("after the snap")
        assert r.db.list_violations() == 0
    finally:
        r.close()


@pytest.mark.gpu
def test_a_thief_and_a_restruck_key_do_not_inherit_a_bend(dev):
    """tests/owner_scenes.py's bank.  Mono mode (cap 1 on the key's own match): a bent key is struck again through
    skred_bank_note_on_channel -- the call's own tag launch clears the slot's bend words, and the wheel back at centre must leave the
    NEW key's increments.  Then a note of another channel takes a bent slot (its trigger stamp, its increments, its tag call); its
    first bend and the centre behind it must return the THIEF's increments, not restore its victim's key."""
    r, iq, sq = channel_scene(dev)
    K, N = OS.K, OS.N
    try:
        slot, other = int(OS.others()[5]), int(OS.others()[9])
        tag, tag2 = 3 << 24 | 60, 3 << 24 | 72
        r.tag([slot, other], [tag, tag2], K, tag="two keys")
        assert r.match(0, N, K, OS.VMASK, (3 << 24, 0xFF000000), 0.8, tag="the wheel down") == [2 * K, 0, len(OS.others()) + len(OS.A_SLOTS) - 2]
        r.block("bent")
        struck = strike(r, iq, sq, (tag, 0xFFFFFFFF), tag, 3, slot)
        assert not r.bend[slot:slot + K].any()                       # CLEAR RULE
        r.same("the re-strike")                                      # CLEAR RULE (the device's words against the model's)
        assert r.match(0, N, K, OS.VMASK, (3 << 24, 0xFF000000), 1.0, tag="the centre")[0] == K      # CLEAR RULE: 2 * K would be restored
        assert r.inc()[slot:slot + K].tobytes() == struck.tobytes(), "the new key was set back to the old key's increments"   # CLEAR RULE
        # the thief
        r.match(0, N, K, OS.VMASK, (3 << 24, 0xFF000000), 1.25, tag="the wheel up")
        dl = r.dev_list([other])
        r.db.stamp_slots(dl.data_ptr(), 1, K, OS.VMASK, SM.STAMP_TRIGGER)
        SM.stamp(r.truth, np.arange(other, other + K), SM.STAMP_TRIGGER, r.now())
        mine = (r.bank["voice_phase_inc"][other:other + K] * np.float32(1.7)).astype(np.float32)
        r.db.ctl_slots([ctl(CM.PHASE_INC, phase_inc=float(x)) for x in mine], OS.VMASK, dl.data_ptr(), 1)
        r.inc()[other:other + K] = mine
        r.tag([other], [5 << 24 | 40], K, tag="the thief's tag")
        assert not r.bend[other:other + K].any()                     # CLEAR RULE
        assert r.tags_each([1.5], 0, N, K, OS.VMASK, [5 << 24 | 40], tag="the thief's first bend")[0] == [K, 0, 0]
        assert (r.bend[other:other + K, 0] == mine.view(np.uint32)).all()     # CLEAR RULE: the victim's key would stand here
        assert r.match(0, N, K, OS.VMASK, (5 << 24, 0xFF000000), 1.0, tag="the thief's centre")[0] == K
        assert r.inc()[other:other + K].tobytes() == mine.tobytes(), "the thief was set to its victim's key"                 # CLEAR RULE
        r.block("after the new notes")
        assert r.db.list_violations() == 0
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 4. purity

@pytest.mark.gpu
def test_bend_calls_that_move_nothing_leave_the_bank_and_the_planner_alone(dev):
    """tests/test_slots.py's in-place bank (4096 voices, two per lane, SKRED_OPT_IN_PLACE = 2).  `plain` makes no bend call; the other
    bank allocates the array and, ahead of every block, sends the centre to every tagged slot, a bend to a channel nobody is on and a
    per-note centre.  Mix, bank bytes, kernel family, in-place verdict and violation counter agree in every block."""
    n, K, mask = 4096, 8, 0xFE
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    r = BendRig(dev, bank, tables, g, setup)
    plain = open_bank(dev, bank, tables, g, setup)
    try:
        chord = np.arange(0, 40 * K, 2 * K, dtype=np.int32)
        tags = (np.uint32(0x03000000) + np.arange(len(chord), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        dl = r.dev_list(chord)
        taken = []
        for k in range(5):
            if k == 1:
                for d in (r.db, plain):
                    d.stamp_slots(dl.data_ptr(), len(chord), K, mask, SM.STAMP_TRIGGER)
                SM.stamp(r.truth, SM.stamp_voices(chord, len(chord), None, K, mask, n), SM.STAMP_TRIGGER, r.now())
                r.tag(chord, tags, K, tag="the chord")
                plain.tag_slots(dl.data_ptr(), tags, K)
            if k >= 1:
                before = bank_words(r.db, bank)
                assert r.match(0, n, K, mask, (0, 0), 1.0, tag="the centre on voices that are not bent") == [0, 0, n // K - len(chord)]
                assert r.match(0, n, K, mask, (9 << 24, 0xFF000000), 1.5, tag="a channel nobody is on") == [0, 0, n // K]
                assert r.tags_each([1.0, 1.0], 0, n, K, mask, tags[:2], tag="a per-note centre")[0] == [0, 0, 0]
                r.bend_clear(0, n, True)
                after = bank_words(r.db, bank)
                assert not CM.words_differ(before, after) and not before.rw_equal(after), "bend calls that move nothing changed the bank"
            x, y = render_blocks(r.db, (F,))[0], render_blocks(plain, (F,))[0]
            cpuref.render(r.truth, r.gl, r.tables, F, 0)
            taken.append((r.db.last_kernel(), plain.last_kernel(), r.db.last_in_place(), plain.last_in_place()))
            assert x.tobytes() == y.tobytes(), f"block {k}: the mixes differ"
            assert taken[-1][0] == taken[-1][1] == 3 and taken[-1][2] == taken[-1][3], (k, taken)
            banks_same(r.db, plain, bank, f"block {k}")
            assert r.db.list_violations() == plain.list_violations() == 0
        assert not plain.download_bend().any()
        print(f"(kernel, plain's, in place, plain's) per block: {taken}")
    finally:
        r.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- 5. every array at once, a shard

@pytest.mark.gpu
def test_owner_pedal_glide_and_bend_arrays_at_once(dev):
    """One bank with all four side arrays.  Forty bend calls back to back with no host wait in between -- five times the staging
    ring's eight slots -- then a tag launch with the three clears behind it."""
    n, K = 512, 4
    bank, tables, g, now = plain_bank(n)
    r = BendRig(dev, bank, tables, g)
    try:
        heads = np.arange(0, n, K, dtype=np.int32)
        tags = (np.uint32(3 << 24) + np.arange(len(heads), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(heads, tags, K, tag="every slot")
        res = r.result(2)
        r.db.pedal_latch(0, n, K, 0xF, device.owner_match(9 << 24, 0xFF000000), res.data_ptr())     # the pedal array exists; nobody matches
        assert r.read(res, 2, "latch") == [0, n // K]
        up, down = GM.per_64(200.0)
        r.start_tags([GM.Glide(TO, up, down, 2.0)] * 8, 0, n, K, 0xF, tags[:8], tag="eight glides")
        for j in range(40):
            pick = tags[(j * 3) % 100:(j * 3) % 100 + 16]
            ratios = wheel(16, j)
            r.db.bend_tags_each(ratios, 0, n, K, 0xF, pick)
            BM.bend_tags_each(r.owner, r.bend, r.inc(), ratios, 0, n, K, 0xF, pick)
        r.same("forty bend calls")
        r.advance(0, n, F, tag="the glides move under the bends")
        assert r.glide[:, 0].any() and r.bend[:, 0].any()
        r.tag(heads[:40], tags[:40] + np.uint32(0x1000), K, tag="forty new notes")
        assert not r.bend[:160].any() and not r.glide[:160].any() and r.bend[160:, 0].any()
        r.block("all four arrays")
    finally:
        r.close()


@pytest.mark.gpu
def test_bends_through_a_shard(dev):
    """One rank, local indices: the channel wheel, a per-note bend and a glide under it through skred_shard_bank()."""
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
        r = BendRig(dev, bank, tables, g, db=db)
        r.tag([8, 260, 508], [5, 6, 7], K, tag="three slots")
        assert r.match(0, n, K, 0xF, (0, 0), 1.5, tag="the wheel") == [12, 0, n // K - 3]
        assert r.tags_each([0.75, 1.0], 0, n, K, 0xF, [7, 5], tag="by note id")[0] == [8, 0, 0]
        assert r.start_tags([GM.Glide(FROM, 2.0, 0.5, 0.5)], 0, n, K, 0xF, [6], tag="a glide under the bend")[0] == [4, 0, 0]
        assert r.advance(0, n, F) == [0, 4]
        r.block("a block on the shard's bank")
        r.bend_clear(0, n, True)
        assert r.inc().tobytes() == bank["voice_phase_inc"].tobytes()
        r.block("back at the keys")
    finally:
        L.skred_shard_destroy(h)


# ---------------------------------------------------------------------------------------------- 6. refusals

@pytest.mark.gpu
def test_refusals_write_nothing(dev):
    import torch
    n, K = 256, 8
    bank, tables, g, now = plain_bank(n)
    r = BendRig(dev, bank, tables, g)
    try:
        L = r.db.L
        r.tag([8, 16], [5, 6], K, tag="two slots")
        assert r.tags_each([1.5], 0, n, K, 0xFF, [5], tag="one bend")[0] == [8, 0, 0]
        dl = r.dev_list([8, 16, 24, 32])
        res = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        good, zero, dup = device.tag_array([5, 6, 7, 8]), device.tag_array([5, 0, 7, 8]), device.tag_array([5, 6, 5, 8])
        ok = np.array([1.0, 1.5, 0.5, 2.0], np.float32)
        h, d, rs, rp, tp = r.db.h, dl.data_ptr(), res.data_ptr(), ok.ctypes.data, good.ctypes.data
        m, wrong = device.owner_match(0, 0), device.owner_match(1, 0)
        BMa, BO, BT, BC, DB = (L.skred_bank_bend_match, L.skred_bank_bend_owned_each, L.skred_bank_bend_tags_each, L.skred_bank_bend_clear,
                               L.skred_bank_download_bend)
        assert BMa(None, 0, n, K, 0xFF, C.byref(m), 1.5, rs, None) == BAD and BMa(h, 0, n, K, 0xFF, None, 1.5, rs, None) == BAD
        assert BMa(h, 0, n, 12, 0xFF, C.byref(m), 1.5, rs, None) == RANGE and BMa(h, 0, n, K, 0, C.byref(m), 1.5, rs, None) == BAD
        assert BMa(h, 0, n, K, 0x1FF, C.byref(m), 1.5, rs, None) == BAD and BMa(h, 0, n, K, 0xFF, C.byref(wrong), 1.5, rs, None) == BAD
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert BMa(h, 0, n, K, 0xFF, C.byref(m), bad, rs, None) == BAD, bad
            ratios = np.array([1.0, 1.5, bad, 2.0], np.float32)
            assert BO(h, ratios.ctypes.data, K, 0xFF, d, tp, 4, None, rs, None) == BAD, bad
            assert BT(h, ratios.ctypes.data, 0, n, K, 0xFF, tp, 4, rs, None) == BAD, bad
        assert BMa(h, 4, 8, K, 0xFF, C.byref(m), 1.5, rs, None) == RANGE and BMa(h, 0, n + K, K, 0xFF, C.byref(m), 1.5, rs, None) == RANGE
        assert BMa(h, 0, 0, K, 0xFF, C.byref(m), 1.5, rs, None) == RANGE
        assert BO(None, rp, K, 0xFF, d, tp, 4, None, rs, None) == BAD and BO(h, None, K, 0xFF, d, tp, 4, None, rs, None) == BAD
        assert BO(h, rp, K, 0xFF, None, tp, 4, None, rs, None) == BAD and BO(h, rp, K, 0xFF, d, None, 4, None, rs, None) == BAD
        assert BO(h, rp, K, 0xFF, d, zero.ctypes.data, 4, None, rs, None) == BAD and BO(h, rp, K, 0xFF, d, tp, -1, None, rs, None) == BAD
        assert BO(h, rp, K, 0x1FF, d, tp, 4, None, rs, None) == BAD and BO(h, rp, K, 0, d, tp, 4, None, rs, None) == BAD
        assert BO(h, rp, 12, 0xFF, d, tp, 4, None, rs, None) == RANGE
        assert BT(None, rp, 0, n, K, 0xFF, tp, 4, rs, None) == BAD and BT(h, rp, 0, n, K, 0xFF, dup.ctypes.data, 4, rs, None) == BAD
        assert BT(h, rp, 0, n, K, 0xFF, zero.ctypes.data, 4, rs, None) == BAD and BT(h, rp, 0, n, K, 0x1FF, tp, 4, rs, None) == BAD
        assert BT(h, rp, 0, n, 3, 0x7, tp, 4, rs, None) == RANGE and BT(h, rp, 4, 8, K, 0xFF, tp, 4, rs, None) == RANGE
        assert BT(h, rp, 0, n + K, K, 0xFF, tp, 4, rs, None) == RANGE and BT(h, rp, 0, 0, K, 0xFF, tp, 4, rs, None) == RANGE
        assert BC(None, 0, n, 1, None) == BAD and BC(h, 8, n, 1, None) == RANGE and BC(h, 0, -1, 0, None) == RANGE
        out = np.full(16, 9, np.uint32)
        assert DB(h, out.ctypes.data, n - 2, 4) == RANGE and DB(h, None, 0, 4) == BAD and DB(None, out.ctypes.data, 0, 4) == BAD
        assert (out == 9).all()
        assert BO(h, rp, K, 0xFF, d, tp, 0, None, rs, None) == 0 and BT(h, rp, 0, n, K, 0xFF, tp, 0, rs, None) == 0 and BC(h, 0, 0, 1, None) == 0
        torch.cuda.synchronize()
        assert (res.cpu().numpy() == FILL).all()
        r.same("after the refusals")
        assert r.match(0, n, K, 0xFF, (0, 0), 1.0, tag="the bank still answers") == [8, 0, n // K - 2]
        r.block("after the refusals")
    finally:
        r.close()
