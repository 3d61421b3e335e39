"""Portamento on the device (skred_bank_glide_owned / _glide_tags / _glide_advance / _glide_stop / _download_glide), byte for byte.

After every call the device is held to tests/glide_model.py: download_glide == the model's glide words and voice_phase_inc (through
download_ctl) == the model's increments on every voice, the owner words and envelope clocks as tests/test_owner.py's rig holds them,
every d_result word == the model's count with the guard words past it untouched.  Blocks are compared with oracle.cpuref, whose bank
receives the model's increments; a twin driven block by block through skred_bank_ctl_slots(SKRED_CTL_PHASE_INC) must hold the same
bytes.  Increments, targets and products stay in the normal fp32 range or are exactly 0 or 3e38 (tests/glide_model.py says why).

The assertions marked CLEAR RULE fail on tests/glide_model.py with CLEAR_RULE = False -- and on a library whose tag launch does not
clear the glide words the device fails them against the model as it stands.
"""
import ctypes as C

import numpy as np
import pytest

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
from test_idle import open_bank, render_blocks, traffic_bank
from test_owner import FILL, Rig, padded_tags
from test_slot_steal import plain_bank, playing_patch

F = 64
BAD, RANGE = -2, -4
SEMI = 2.0 ** (1.0 / 12.0)
FROM, TO = GM.FROM_SCALE, GM.TO_SCALE


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


class GlideRig(Rig):
    """tests/test_owner.py's rig with the model's glide words beside the owner array: every call runs on the device and on the model."""

    def __init__(self, dev, bank, tables, g, setup=None, db=None):
        if db is None:
            super().__init__(dev, bank, tables, g, setup)
        else:
            self.db, self.bank, self.tables = db, bank, tables
            self.truth, self.gl, self.owner, self.n = bank.copy(), g.copy(), OM.new(bank.n), bank.n
        self.glide = GM.new(bank.n)

    def inc(self):
        return self.truth["voice_phase_inc"]

    def same(self, tag):
        super().same(tag)
        got = self.db.download_glide()
        bad = np.flatnonzero((got != self.glide).any(axis=1))
        assert not len(bad), f"{tag}: glide words differ at {bad[:8].tolist()}: {got[bad[:8]].tolist()} / {self.glide[bad[:8]].tolist()}"
        a = self.bank.copy()
        self.db.download_ctl(a)
        got, want = a["voice_phase_inc"].view(np.uint32), self.inc().view(np.uint32)
        bad = np.flatnonzero(got != want)
        assert not len(bad), f"{tag}: voice_phase_inc differs at {bad[:8].tolist()}: {a['voice_phase_inc'][bad[:8]].tolist()} / {self.inc()[bad[:8]].tolist()}"

    def tag(self, entries, tags, K, count=None, tag=""):
        GM.tag_clear(self.glide, entries, len(tags), count, K)
        super().tag(entries, tags, K, count, tag)

    def check(self, res, words, want, tag):
        got = self.read(res, words, tag)
        print(f"{tag}: d_result {got}, the model {want}")
        assert got == want, f"{tag}: d_result {got}, the model says {want}"
        self.same(tag)
        return want

    def start_owned(self, glides, K, vmask, entries, tags, count=None, tag=""):
        import torch
        dl, res = self.dev_list(entries), self.result(3)
        dc = None if count is None else torch.tensor([count, 4321], dtype=torch.int32, device="cuda")
        self.db.glide_owned([g.c() for g in glides], K, vmask, dl.data_ptr(), tags, dc.data_ptr() if dc is not None else 0, res.data_ptr())
        return self.check(res, 3, GM.start_owned(self.owner, self.glide, self.inc(), glides, K, vmask, entries, tags, count), tag)

    def start_tags(self, glides, first, count, K, vmask, tags, tag=""):
        res = self.result(3)
        self.db.glide_tags([g.c() for g in glides], first, count, K, vmask, tags, res.data_ptr())
        want, lst = GM.start_tags(self.owner, self.glide, self.inc(), glides, first, count, K, vmask, tags)
        return self.check(res, 3, want, tag), lst

    def advance(self, first, count, frames, tag=""):
        res = self.result(2)
        self.db.glide_advance(first, count, frames, res.data_ptr())
        return self.check(res, 2, GM.advance(self.glide, self.inc(), first, count, frames), tag or f"advance {frames}")

    def stop(self, first, count, snap, tag=""):
        self.db.glide_stop(first, count, snap)
        GM.stop(self.glide, self.inc(), first, count, snap)
        self.same(tag or f"stop snap {snap}")


def bank_words(db, like):
    a = like.copy()
    db.download(a)
    db.download_ctl(a)
    return a


def banks_same(x, y, like, tag):
    a, b = bank_words(x, like), bank_words(y, like)
    assert not CM.words_differ(a, b) and not a.rw_equal(b), f"{tag}: the two banks differ: {CM.words_differ(a, b)} {a.rw_equal(b)}"


def glides_for(n, seed=0):
    """n entries: both modes, rates from a semitone per step down to the smallest above 1, a rate of exactly 2 with scales that are
    powers of two (every product exact: the arrival falls ON a step, the increment level with the target)"""
    out = []
    for k in range(n):
        j = k + seed
        if j % 4 == 0:
            out.append(GM.Glide(FROM if j % 8 else TO, 2.0, 0.5, 0.125 if j % 8 else 8.0))
        else:
            up = np.float32((SEMI, 1.003, 1.0 + 2.0 ** -23)[j % 3])
            out.append(GM.Glide(FROM if j % 2 else TO, up, np.float32(1.0) / up if j % 3 != 2 else np.float32(1.0 - 2.0 ** -24),
                                np.float32(SEMI ** ((j % 25) - 12)) if j % 25 != 12 else np.float32(0.75)))
    return out


# ---------------------------------------------------------------------------------------------- 1. every call against the model

@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 4, 64])
def test_every_call_against_the_model(dev, K):
    """600 voices.  Glides by note id with 1, 2, 1023 and 1024 tags, on a list with holes, a stolen slot and a count word; the advance
    over [37, 537) -- off the 64-voice boundary, across two workgroup spans -- by 1, 63, 64, 100 and 512 frames; an arrival exactly on
    a step (rate 2 from an eighth: the third product is the target) and one in the middle of a 512-frame call's loop; a zero, a
    huge and a negative increment; stop with and without snap."""
    n = 600
    bank, tables, g, now = plain_bank(n)
    inc = bank["voice_phase_inc"]
    inc[5::23] = np.float32(0.0)                                     # a start from zero is withheld
    inc[7::29] = np.float32(3e38)                                    # FROM_SCALE up, TO_SCALE up: the product overflows
    inc[11::31] *= np.float32(-1.0)                                  # negative increments glide on their side of zero
    assert (np.abs(inc[inc != 0]) > 1e-30).all()
    r = GlideRig(dev, bank, tables, g)
    slots = np.arange(0, n - K + 1, K, dtype=np.int32)
    full = (1 << K) - 1
    part = full if K == 1 else (1 << (K - 1)) | 1
    gen = np.random.default_rng(K)
    try:
        all_tags = (np.uint32(0x0B000000) + np.arange(len(slots), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(slots, all_tags, K, tag="every slot")
        res = r.result(2)
        r.db.glide_advance(37, 500, 64, res.data_ptr())              # no glide array yet: the result is cleared, nothing else happens
        assert r.read(res, 2, "advance before any glide") == [0, 0] and not r.db.download_glide().any()
        r.same("advance before any glide")
        first, count = (37, 500) if K == 1 else (K, (len(slots) - 1) * K)
        inside = slots[(slots >= first) & (slots < first + count)]
        order = gen.permutation(len(inside))
        at = 0
        for m in (1, 2, 1023, 1024):
            take = min(m, max(1, len(inside) // 5))
            pick = inside[order[at:at + take]]
            at += take
            tags = padded_tags(r.owner[pick], m)[gen.permutation(m)]  # (the tags unsorted: the sort and the permutation have work to do)
            want, lst = r.start_tags(glides_for(m, m), first, count, K, full if m != 2 else part, tags, tag=f"{m} tags")
            assert want[0] + want[1] == len(pick) * bin(full if m != 2 else part).count("1") and want[0] > 0 and int((lst >= 0).sum()) == len(pick)
        # a list: a hole, a slot past the bank, a stolen slot, a slot outside the range above, a count word that cuts the last entry off
        rest = slots[~np.isin(slots, inside[order[:at]])]
        entries = np.array([rest[0], -1, n, rest[1], rest[2], rest[3]], np.int32)
        tags = np.array([r.owner[rest[0]], 5, 6, r.owner[rest[1]] ^ 0x00800000, r.owner[rest[2]], r.owner[rest[3]]], np.uint32)
        want = r.start_owned(glides_for(6, 1), K, part, entries, tags, count=5, tag="a list")
        assert want[2] == 1 and want[0] + want[1] == 2 * bin(part).count("1") and not r.glide[rest[3]].any()
        assert r.glide[:, 0].any() and int((r.glide[:, 0] != 0).sum()) > 20
        seen = [0, 0]
        for frames in (1, 63, 64, 100, 512, 64, 64, 512, 1, 63):
            still, arrived = r.advance(37, 500, frames)
            seen = [seen[0] + still, seen[1] + arrived]
        out = np.r_[0:37, 537:n]
        assert r.glide[out, 3].sum() == 0, "a voice outside [37, 537) moved"
        assert seen[0] > 50 and seen[1] > 5, seen
        # legato onto a new key while gliding: the targets compose
        moving = [int(s) for s in inside if r.glide[s, 0]][:3]
        if moving:
            old = r.glide[moving, 0].copy()
            r.start_owned([GM.Glide(TO, SEMI, 1 / SEMI, np.float32(SEMI ** 3))] * len(moving), K, 1, moving, r.owner[moving], tag="legato")
            assert (r.glide[moving, 0] == GM.mul(old, GM.bits(np.float32(SEMI ** 3)))).all() and not r.glide[moving, 3].any()
        r.advance(0, n, 100, tag="the whole bank")
        r.block("a block while gliding")
        r.stop(first, count // 2 if K == 1 else (count // 2) // K * K, True)
        r.advance(0, n, 64)
        r.stop(0, n, False)
        assert not r.glide.any()
        assert r.advance(0, n, 512, tag="nothing glides") == [0, 0]
        r.block("a block after the glides")
        assert r.db.list_violations() == 0 and np.isfinite(r.inc()[np.isfinite(bank["voice_phase_inc"])]).all()
    finally:
        r.close()


@pytest.mark.gpu
def test_arrivals_on_a_step_and_inside_a_loop(dev):
    """Rate 2 from an eighth below (three exact doublings) and rate 1/2 from eight times above: voice 0's slot advances by 64 frames
    three times and arrives ON the third step; voice 8's slot by one call of 512 frames and arrives at the third of its eight steps;
    voice 16's slot by 63 + 1 + 127 + 1 frames: the carry brings the third step due inside the last call."""
    n, K = 64, 8
    bank, tables, g, now = plain_bank(n)
    r = GlideRig(dev, bank, tables, g)
    try:
        struck = r.inc().copy()
        slots = [0, 8, 16, 24]
        tags = [11, 12, 13, 14]
        r.tag(slots, tags, K, tag="four slots")
        up, down = GM.Glide(FROM, 2.0, 0.5, 0.125), GM.Glide(FROM, 2.0, 0.5, 8.0)
        assert r.start_owned([up, down, up, down], K, 0xFF, slots, tags, tag="start") == [32, 0, 0]
        assert (r.inc()[:8] == struck[:8] * np.float32(0.125)).all() and (r.inc()[8:16] == struck[8:16] * np.float32(8.0)).all()
        assert r.advance(0, 8, 64) == [8, 0] and r.advance(0, 8, 64) == [8, 0]
        assert r.advance(0, 8, 64) == [0, 8] and r.inc()[:8].tobytes() == struck[:8].tobytes()
        assert r.advance(8, 8, 512) == [0, 8] and r.inc()[8:16].tobytes() == struck[8:16].tobytes()
        assert r.advance(16, 8, 63) == [8, 0] and r.glide[16, 3] == 63 and (r.inc()[16:24] == struck[16:24] * np.float32(0.125)).all()
        assert r.advance(16, 8, 1) == [8, 0] and r.glide[16, 3] == 0 and (r.inc()[16:24] == struck[16:24] * np.float32(0.25)).all()
        assert r.advance(16, 8, 127) == [8, 0] and r.glide[16, 3] == 63
        assert r.advance(16, 8, 1) == [0, 8] and r.inc()[16:24].tobytes() == struck[16:24].tobytes()
        assert r.advance(0, n, 65536) == [0, 8] and r.inc().tobytes() == struck.tobytes() and not r.glide.any()
        r.block("landed")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 2. twins, taps, the oracle

@pytest.mark.gpu
@pytest.mark.parametrize("family", ["one voice per lane", "two per lane"])
def test_a_glided_chord_against_the_oracle_and_a_twin(dev, family):
    """One voice per lane: 3.sk over 64 copies (K = 4, its modulated carriers keep it off the two-per-lane kernels).  Two per lane:
    tests/test_idle.py's traffic bank (512 voices, K = 8, kernel family 3), the chord's free voices triggered first.  Three slots slide
    into a new key (FROM_SCALE by note id: a fifth up, an octave down, a semitone up) and are advanced ahead of every block of 64
    frames.  A twin never hears of a glide: it receives the model's increments through skred_bank_ctl_slots(SKRED_CTL_PHASE_INC) ahead
    of every block.  The stems of the three slots through taps must be the oracle's bit for bit; state, taps, mix and kernel family
    must be the twin's (the device sums the mix in another order than the oracle: the mix is held to the twin, as tests/test_expr.py
    holds it)."""
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
    r = GlideRig(dev, bank, tables, g, setup)
    twin = open_bank(dev, bank, tables, g, setup)
    try:
        slots = [4 * K, 21 * K, 63 * K]                               # (3.sk: sounding copies, copy % 4 != 0); the last slot of the bank among them
        if two:
            dl = r.dev_list(slots)
            for d in (r.db, twin):
                d.stamp_slots(dl.data_ptr(), len(slots), K, 0xFE, SM.STAMP_TRIGGER)
            SM.stamp(r.truth, SM.stamp_voices(slots, len(slots), None, K, 0xFE, n), SM.STAMP_TRIGGER, r.now())
        tags = np.array([3 << 24 | 60, 3 << 24 | 64, 3 << 24 | 67], np.uint32)
        r.tag(slots, tags, K, tag="the chord")
        voices = np.array([s + l for s in slots for l in range(K)], np.int32)
        d_taps, t_taps = (torch.zeros((F, len(voices), 2), dtype=torch.float32, device="cuda") for _ in range(2))
        r.db.set_taps(voices, d_taps.data_ptr())
        twin.set_taps(voices, t_taps.data_ptr())
        up, down = GM.per_64(700.0)                                  # about a semitone per block
        glides = [GM.Glide(FROM, up, down, np.float32(SEMI ** -7)), GM.Glide(FROM, up, down, np.float32(2.0)), GM.Glide(FROM, up, down, np.float32(1 / SEMI))]
        want, lst = r.start_tags(glides, 0, n, K, vmask, tags[::-1].copy(), tag="the chord glides")
        assert want == [3 * K, 0, 0] and lst.tolist() == slots[::-1]
        lists = [r.dev_list([s]) for s in slots]
        kernels, heard, blocks = set(), 0, 0
        while True:
            still, arrived = r.advance(0, n, F)
            for s, dl in zip(slots, lists):
                twin.ctl_slots([ctl(CM.PHASE_INC, phase_inc=float(r.inc()[s + l])) for l in range(K)], vmask, dl.data_ptr(), 1)
            x, y = render_blocks(r.db, (F,))[0], render_blocks(twin, (F,))[0]
            ref = cpuref.render(r.truth, r.gl, r.tables, F, 0, want_stems=True)
            got = d_taps.cpu().numpy()
            assert r.db.last_taps() == twin.last_taps() == len(voices)
            assert got.tobytes() == np.ascontiguousarray(ref["stems"][:, voices, :]).tobytes(), f"block {blocks}: taps differ from the oracle"
            assert got.tobytes() == t_taps.cpu().numpy().tobytes(), f"block {blocks}: taps differ from the twin's"
            assert x.tobytes() == y.tobytes(), f"block {blocks}: the mix differs from the twin's"
            assert r.db.last_kernel() == twin.last_kernel()
            kernels.add(r.db.last_kernel())
            banks_same(r.db, twin, bank, f"block {blocks}")
            a = bank.copy()
            r.db.download(a)
            assert not a.rw_equal(r.truth), f"block {blocks}: state differs from the oracle: {a.rw_equal(r.truth)}"
            heard += np.abs(got).sum() > 0
            blocks += 1
            if still == 0 and blocks > 14:
                break
            assert blocks < 40
        assert heard == blocks and ((kernels == {3}) if two else (3 not in kernels)), (heard, blocks, kernels)
        print(f"{family}: {blocks} blocks, kernel family {kernels}")
        assert not r.glide.any() and r.db.list_violations() == twin.list_violations() == 0
    finally:
        r.db.set_taps([], 0)
        twin.set_taps([], 0)
        r.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 3. the clear rule

@pytest.mark.gpu
def test_a_restruck_key_and_a_thief_do_not_inherit_a_glide(dev):
    """tests/owner_scenes.py's bank (3.sk over 256 voices, K = 4).  Mono mode (cap 1, min_age 0): a key glides, and the next key is
    struck through skred_bank_note_on_channel before it has arrived -- the new note takes the old note's slot in the same block, and
    the call's own tag launch clears the slot's glide words.  Then a note of ANOTHER channel takes a gliding slot (its trigger stamp
    and its tag call: the launch a thief's burst ends with).  Neither new note's increment may move at the next advance."""
    import torch
    from test_slots import slot_notes
    bank, tables, g = OS.bank()
    K, N = OS.K, OS.N
    r = GlideRig(dev, bank, tables, g)
    chan, tag = CHM.channel(3), [3 << 24 | 60]
    try:
        slot, other = int(OS.others()[5]), int(OS.others()[9])
        r.tag([slot, other], [tag[0], 3 << 24 | 72], K, tag="two keys")
        up, down = GM.per_64(50.0)
        slow = GM.Glide(FROM, up, down, np.float32(0.5))
        assert r.start_tags([slow, slow], 0, N, K, OS.VMASK, [tag[0], 3 << 24 | 72], tag="both glide")[0] == [2 * K, 0, 0]
        assert r.advance(0, N, F) == [2 * K, 0]
        r.block("gliding")
        # the key is struck again
        iq = slot_query(0, N, K, OS.MMASK, FIN | ENV, OS.SETTLE, 0, 0)
        sq = M.SlotQuery(0, N, K, OS.MMASK, OLDEST, 0)
        one = (int(tag[0]), 0xFFFFFFFF)                              # mono on this key's own match: the burst must take its slot
        want, res, _ = CHM.burst(r.truth, r.now(), r.owner, iq, sq, one, 1, 1)
        assert want.tolist() == [slot] and res == [1, 0, 1, 1], "the new note must steal the note's own slot"
        notes = slot_notes(1, K, OS.VMASK, 3, [SM.SET_PHASE])
        da = torch.full((3,), FILL, dtype=torch.int32, device="cuda")
        dr = torch.full((6,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.db.note_on_channel(notes, tag, iq, sq.c(), device.owner_match(*one), 1, OS.VMASK, da.data_ptr(), dr.data_ptr())
        SM.store_notes((r.truth,), r.truth, notes, K, OS.VMASK, want, r.now())
        OM.tag_slots(r.owner, want, tag, None, K)
        GM.tag_clear(r.glide, want, 1, None, K)
        torch.cuda.synchronize()
        assert da.cpu().numpy().tolist() == [slot, FILL, FILL] and dr.cpu().numpy().tolist() == res + [FILL, FILL]
        assert not r.glide[slot:slot + K].any()                      # CLEAR RULE
        r.same("the re-strike")                                      # CLEAR RULE (the device's words against the model's)
        struck = r.inc()[slot:slot + K].copy()
        assert struck.tolist() == [np.float32(notes[l].phase_inc) for l in range(K)]
        # a thief of another channel takes the other gliding slot
        dl = r.dev_list([other])
        r.db.stamp_slots(dl.data_ptr(), 1, K, OS.VMASK, SM.STAMP_TRIGGER)
        SM.stamp(r.truth, np.arange(other, other + K), SM.STAMP_TRIGGER, r.now())
        mid = r.inc()[other:other + K].copy()
        r.tag([other], [5 << 24 | 40], K, tag="the thief's tag")
        assert not r.glide[other:other + K].any()                    # CLEAR RULE
        assert r.advance(0, N, F) == [0, 0]                          # CLEAR RULE: 2 * K voices would still glide
        assert r.inc()[slot:slot + K].tobytes() == struck.tobytes(), "the new note inherited the old note's glide"     # CLEAR RULE
        assert r.inc()[other:other + K].tobytes() == mid.tobytes(), "the thief inherited its victim's glide"            # CLEAR RULE
        r.block("after the new notes")
        # the order for mono legato: note_on_channel, THEN the glide
        assert r.start_tags([slow], 0, N, K, OS.VMASK, tag, tag="legato after the note-on")[0] == [K, 0, 0]
        assert r.advance(0, N, F) == [K, 0]
        r.block("gliding again")
        assert r.db.list_violations() == 0
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 4. purity

@pytest.mark.gpu
def test_a_bank_where_nothing_glides_is_the_bank_without_glide_calls(dev):
    """tests/test_slots.py's in-place bank (4096 voices, two per lane, SKRED_OPT_IN_PLACE = 2).  `plain` makes no glide call; `idle`
    allocates the glide array (a TO_SCALE of scale 1 on one slot, stopped at once: no plane word changes) and advances the whole bank
    ahead of every block.  Mix, bank bytes, kernel family, in-place verdict and violation counter agree in every block, and an advance
    leaves every word of the bank as it was."""
    n, K, mask = 4096, 8, 0xFE
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    r = GlideRig(dev, bank, tables, g, setup)
    plain = open_bank(dev, bank, tables, g, setup)
    try:
        chord = np.arange(0, 40 * K, 2 * K, dtype=np.int32)
        tags = (np.uint32(0x80000000) + np.arange(len(chord), dtype=np.uint32)).astype(np.uint32)
        dl = r.dev_list(chord)
        taken = []
        for k in range(5):
            if k == 1:
                for d in (r.db, plain):
                    d.stamp_slots(dl.data_ptr(), len(chord), K, mask, SM.STAMP_TRIGGER)
                SM.stamp(r.truth, SM.stamp_voices(chord, len(chord), None, K, mask, n), SM.STAMP_TRIGGER, r.now())
                r.tag(chord, tags, K, tag="the chord")
                plain.tag_slots(dl.data_ptr(), tags, K)
                before = bank_words(r.db, bank)
                assert r.start_owned([GM.Glide(TO, 1.5, 0.5, 1.0)], K, mask, chord[:1], tags[:1], tag="a glide to where it is")[0] == 7
                r.stop(0, n, False)
                after = bank_words(r.db, bank)
                assert not CM.words_differ(before, after) and not before.rw_equal(after)
            if k >= 1:
                before = bank_words(r.db, bank)
                assert r.advance(0, n, F) == [0, 0]
                after = bank_words(r.db, bank)
                assert not CM.words_differ(before, after) and not before.rw_equal(after), "an advance with nothing gliding changed the bank"
            x, y = render_blocks(r.db, (F,))[0], render_blocks(plain, (F,))[0]
            cpuref.render(r.truth, r.gl, r.tables, F, 0)
            taken.append((r.db.last_kernel(), plain.last_kernel(), r.db.last_in_place(), plain.last_in_place()))
            assert x.tobytes() == y.tobytes(), f"block {k}: the mixes differ"
            assert taken[-1][0] == taken[-1][1] == 3 and taken[-1][2] == taken[-1][3], (k, taken)
            banks_same(r.db, plain, bank, f"block {k}")
            assert r.db.list_violations() == plain.list_violations() == 0
        assert not plain.download_glide().any()
        print(f"(kernel, plain's, in place, plain's) per block: {taken}")
    finally:
        r.close()
        plain.close()


@pytest.mark.gpu
def test_glide_calls_leave_the_planner_alone(dev):
    """tests/test_timbre.py's planner scene (2048 voices, two per lane, SKRED_OPT_IN_PLACE = 2, a chord of 40 slots of 7 voices: the
    verdict CAN move, as that test's control shows).  The chord's glides start behind block 2 and advance ahead of every later block;
    `plain` never hears of them.  The in-place verdict and skred_bank_last_kernel of every block equal plain's.  Block 3 lies behind
    the start call and the first advance: the chord's 280 listed voices and 280 more from a call that told the planner about its
    voices would be 560, over the bound of 405, so that block must also BE in place, as block 2 ahead of the calls is.  The later
    blocks, behind an advance each, are held to plain's verdict only, whatever that is: plain itself, which makes no call after
    the chord's tags, is not in place from block 4 on (an MI355X run: True for blocks 2 and 3, False for blocks 4 to 6, on both banks)."""
    n, K, mask, CHORD = 2048, 8, 0xFE, 40
    assert CHORD * 7 <= n // 6 + 64 < 2 * CHORD * 7
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    r = GlideRig(dev, bank, tables, g, setup)
    plain = open_bank(dev, bank, tables, g, setup)
    try:
        chord = np.arange(0, CHORD * 2 * K, 2 * K, dtype=np.int32)
        tags = (np.uint32(3 << 24) + np.arange(len(chord), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        dl = r.dev_list(chord)
        up, down = GM.per_64(300.0)
        taken = []
        for k in range(7):
            if k == 1:
                for d in (r.db, plain):
                    d.stamp_slots(dl.data_ptr(), len(chord), K, mask, SM.STAMP_TRIGGER)
                SM.stamp(r.truth, SM.stamp_voices(chord, len(chord), None, K, mask, n), SM.STAMP_TRIGGER, r.now())
                r.tag(chord, tags, K, tag="the chord")
                plain.tag_slots(dl.data_ptr(), tags, K)
            if k == 3:
                glides = [GM.Glide(FROM if j % 2 else TO, up, down, np.float32(SEMI ** (j % 7 - 3.5))) for j in range(len(chord))]
                want, _ = r.start_tags(glides, 0, n, K, mask, tags, tag="the chord glides")
                assert want == [len(chord) * 7, 0, 0]
            if k >= 3:
                still, arrived = r.advance(0, n, F)
                assert still + arrived > 0 or k > 3
            for d in (r.db, plain):
                render_blocks(d, (F,))
            cpuref.render(r.truth, r.gl, r.tables, F, 0)
            taken.append((r.db.last_kernel(), plain.last_kernel(), r.db.last_in_place(), plain.last_in_place()))
            assert taken[-1][0] == taken[-1][1] and taken[-1][2] == taken[-1][3], (k, taken)
            a = bank.copy()
            r.db.download(a)
            assert not a.rw_equal(r.truth), (k, a.rw_equal(r.truth))
            assert r.db.list_violations() == plain.list_violations() == 0
        print(f"(kernel, plain's, in place, plain's) per block: {taken}")
        assert taken[2][2] and taken[3][2], f"the block behind the glide start and the first advance was not in place: {taken}"
    finally:
        r.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- 5. many workgroups, a shard

@pytest.mark.gpu
def test_many_workgroups_feed_the_counts(dev):
    """70 000 voices, K = 2: 274 workgroups of the advance pass add to the result words.  The advance runs twice in a row on one
    stream with no host wait in between: the second starts from result words the stream cleared again."""
    import torch
    n, K, vmask = 70000, 2, 3
    bank, tables, g, now = plain_bank(n)
    r = GlideRig(dev, bank, tables, g)
    try:
        heads = np.arange(0, n, K, dtype=np.int32)
        k = np.arange(len(heads))
        tags = (np.uint32(0x01000000) + k.astype(np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(heads, tags, K, tag="every slot")
        some = k % 3 == 0
        glides = [GM.Glide(FROM, 2.0, 0.5, (0.5, 0.25, 4.0)[j % 3]) for j in range(int(some.sum()))]
        assert r.start_owned(glides, K, vmask, heads[some], tags[some], tag="a third of the bank") == [2 * int(some.sum()), 0, 0]
        bufs = [torch.full((4,), FILL, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for b in bufs:
            r.db.glide_advance(0, n, F, b.data_ptr())
        first, second = GM.advance(r.glide, r.inc(), 0, n, F), GM.advance(r.glide, r.inc(), 0, n, F)
        torch.cuda.synchronize()
        third = 2 * int(some.sum()) // 3
        assert abs(first[1] - third) <= 2 and first[0] + first[1] == 2 * int(some.sum()) and second[1] > 1000 and second[0] == 0
        for b, w in zip(bufs, (first, second)):
            assert b.cpu().numpy().tolist() == w + [FILL, FILL], (b.cpu().numpy().tolist(), w)
        r.same("two advances")
        assert r.inc().tobytes() == bank["voice_phase_inc"].tobytes() and not r.glide.any()
        r.block("landed")
    finally:
        r.close()


@pytest.mark.gpu
def test_glides_through_a_shard(dev):
    """One rank, local indices: glides by note id and the advance through skred_shard_bank()."""
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
        r = GlideRig(dev, bank, tables, g, db=db)
        r.tag([8, 260, 508], [5, 6, 7], K, tag="three slots")
        up, down = GM.per_64(700.0)
        assert r.start_tags([GM.Glide(FROM, up, down, 0.5), GM.Glide(TO, up, down, 1.5), GM.Glide(FROM, 2.0, 0.5, 2.0)], 0, n, K, 0xF,
                            [7, 5, 6], tag="by note id")[0] == [12, 0, 0]
        assert r.advance(0, n, F) == [8, 4]
        r.block("a block on the shard's bank")
        # slot 260 landed in the first pass (one halving); slot 508 climbs an octave at 700 semitones a second, 1.016 per 64 frames:
        # 1 + 8 steps are 9.1 of its 12 semitones, so it is still under way; slot 8 lies below the range
        assert r.advance(100, 412, 512) == [4, 0]
        r.stop(0, n, True)
        r.block("stopped")
    finally:
        L.skred_shard_destroy(h)


# ---------------------------------------------------------------------------------------------- 6. refusals

@pytest.mark.gpu
def test_refusals_write_nothing(dev):
    import torch
    n, K = 256, 8
    bank, tables, g, now = plain_bank(n)
    r = GlideRig(dev, bank, tables, g)
    try:
        L = r.db.L
        r.tag([8, 16], [5, 6], K, tag="two slots")
        slow = GM.Glide(FROM, 1.001, 0.999, 0.5)
        assert r.start_tags([slow], 0, n, K, 0xFF, [5], tag="one glide")[0] == [8, 0, 0]
        dl = r.dev_list([8, 16, 24, 32])
        res = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        good, zero, dup = device.tag_array([5, 6, 7, 8]), device.tag_array([5, 0, 7, 8]), device.tag_array([5, 6, 5, 8])
        G = device.glide
        ok = device.glide_array([G(FROM, 1.01, 0.99, 0.5)] * 4)
        h, d, rs, gp = r.db.h, dl.data_ptr(), res.data_ptr(), C.cast(ok, C.c_void_p)
        GO, GT, AD, ST, DG = (L.skred_bank_glide_owned, L.skred_bank_glide_tags, L.skred_bank_glide_advance, L.skred_bank_glide_stop,
                              L.skred_bank_download_glide)
        assert GO(None, gp, K, 0xFF, d, good.ctypes.data, 4, None, rs, None) == BAD
        assert GO(h, None, K, 0xFF, d, good.ctypes.data, 4, None, rs, None) == BAD
        assert GO(h, gp, K, 0xFF, None, good.ctypes.data, 4, None, rs, None) == BAD
        assert GO(h, gp, K, 0xFF, d, None, 4, None, rs, None) == BAD
        assert GO(h, gp, K, 0xFF, d, zero.ctypes.data, 4, None, rs, None) == BAD
        assert GO(h, gp, K, 0xFF, d, good.ctypes.data, -1, None, rs, None) == BAD
        assert GO(h, gp, K, 0x1FF, d, good.ctypes.data, 4, None, rs, None) == BAD
        assert GO(h, gp, K, 0, d, good.ctypes.data, 4, None, rs, None) == BAD
        assert GO(h, gp, 12, 0xFF, d, good.ctypes.data, 4, None, rs, None) == RANGE
        for entry in ((0, 1.01, 0.99, 0.5), (3, 1.01, 0.99, 0.5), (FROM, 1.0, 0.99, 0.5), (FROM, 1.01, 1.0, 0.5), (FROM, 1.01, 0.0, 0.5),
                      (TO, 1.01, 0.99, 0.0), (TO, 1.01, 0.99, -2.0), (TO, float("nan"), 0.99, 2.0), (TO, 1.01, 0.99, float("inf"))):
            bad = device.glide_array([G(FROM, 1.01, 0.99, 0.5)] * 3 + [G(*entry)])
            assert GO(h, C.cast(bad, C.c_void_p), K, 0xFF, d, good.ctypes.data, 4, None, rs, None) == BAD, entry
            assert GT(h, C.cast(bad, C.c_void_p), 0, n, K, 0xFF, good.ctypes.data, 4, rs, None) == BAD, entry
        rsv = device.glide_array([G(FROM, 1.01, 0.99, 0.5)])
        rsv[0].reserved[3] = 1
        assert GO(h, C.cast(rsv, C.c_void_p), K, 0xFF, d, good.ctypes.data, 1, None, rs, None) == BAD
        assert GT(h, gp, 0, n, K, 0xFF, dup.ctypes.data, 4, rs, None) == BAD
        assert GT(h, gp, 0, n, K, 0xFF, zero.ctypes.data, 4, rs, None) == BAD
        assert GT(h, gp, 0, n, K, 0x1FF, good.ctypes.data, 4, rs, None) == BAD
        assert GT(h, gp, 0, n, 3, 0x7, good.ctypes.data, 4, rs, None) == RANGE
        assert GT(h, gp, 4, 8, K, 0xFF, good.ctypes.data, 4, rs, None) == RANGE
        assert GT(h, gp, 0, n + K, K, 0xFF, good.ctypes.data, 4, rs, None) == RANGE
        assert GT(h, gp, 0, 0, K, 0xFF, good.ctypes.data, 4, rs, None) == RANGE
        assert GT(None, gp, 0, n, K, 0xFF, good.ctypes.data, 4, rs, None) == BAD
        assert AD(None, 0, n, 64, rs, None) == BAD and AD(h, 0, n, 0, rs, None) == BAD and AD(h, 0, n, 65537, rs, None) == BAD
        assert AD(h, 0, 0, 64, rs, None) == RANGE and AD(h, 37, n, 64, rs, None) == RANGE and AD(h, -1, 8, 64, rs, None) == RANGE
        assert ST(None, 0, n, 1, None) == BAD and ST(h, 8, n, 1, None) == RANGE and ST(h, 0, -1, 0, None) == RANGE
        out = np.full(16, 9, np.uint32)
        assert DG(h, out.ctypes.data, n - 2, 4) == RANGE and DG(h, None, 0, 4) == BAD and DG(None, out.ctypes.data, 0, 4) == BAD
        assert (out == 9).all()
        assert GO(h, gp, K, 0xFF, d, good.ctypes.data, 0, None, rs, None) == 0 and GT(h, gp, 0, n, K, 0xFF, good.ctypes.data, 0, rs, None) == 0
        assert ST(h, 0, 0, 1, None) == 0
        torch.cuda.synchronize()
        assert (res.cpu().numpy() == FILL).all()
        r.same("after the refusals")                                  # glide words, increments, owners and clocks as they were
        # ... and the bank still answers: 65536 frames are 1024 steps of 1.001, a factor of 2.78, past the octave the glide has to climb
        assert r.glide[8:16, 0].all() and r.advance(0, n, 65536) == [0, 8]
        r.block("after the refusals")
    finally:
        r.close()
