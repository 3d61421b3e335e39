"""Note owners on the device (skred_bank_tag_slots / _find_owned / _stamp_owned / _release_tags / _ctl_owned / _owner_clear /
_download_owners), byte for byte.

After every call the device is held to tests/owner_model.py: DeviceBank.download_owners == the model's owner array on every voice,
d_slots_out (guard entries included) == the model's list, every d_result word == the model's count, and the envelope clocks the bank
holds (download_env_clocks) == the oracle's after slot_model's stamps.  State after a rendered block is compared with oracle.cpuref
on the model's stamps.  The theft scene is tests/owner_scenes.py's; tests/test_owner_cpu.py asserts on the oracle alone that it steals.
"""
import ctypes as C

import numpy as np
import pytest

import ctl_model as CM
import owner_model as OM
import owner_scenes as S
import slot_model as SM
import slot_steal_scenes as SS
from oracle import cpuref
from skred_amd import banks, device
from skred_amd.device import ctl
from test_idle import open_bank, render_blocks, traffic_bank
from test_slot_steal import plain_bank

REL, TRIG = SM.STAMP_RELEASE, SM.STAMP_TRIGGER
DIRTY_PARAMS, DIRTY_PAN = 1, 8
BAD, RANGE = -2, -4
FILL = -7
F = 64


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


class Rig:
    """A bank on the device, the oracle's copy of it and the model's owner array, moved together."""

    def __init__(self, dev, bank, tables, g, setup=None):
        self.db = open_bank(dev, bank, tables, g, setup)
        self.bank, self.tables = bank, tables
        self.truth, self.gl = bank.copy(), g.copy()
        self.owner = OM.new(bank.n)
        self.n = bank.n

    def now(self):
        return int(self.gl.synth_sample_count)

    def dev_list(self, entries):
        import torch
        return torch.from_numpy(np.array(entries, np.int32)).cuda()

    def result(self, words):
        import torch
        t = torch.full((words + 2,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return t

    def read(self, t, words, tag):
        import torch
        torch.cuda.synchronize()
        got = t.cpu().numpy()
        assert (got[words:] == FILL).all(), f"{tag}: words past d_result were written"
        return got[:words].view(np.uint32).tolist()

    def same(self, tag):
        """the owner array and the envelope clocks, every voice"""
        got = self.db.download_owners()
        bad = np.flatnonzero(got != self.owner)
        assert not len(bad), f"{tag}: owner words differ at {bad[:8].tolist()}: {got[bad[:8]].tolist()} / {self.owner[bad[:8]].tolist()}"
        start, release = self.db.download_env_clocks()
        e = self.truth["voice_amp_envelope"]
        assert start.tobytes() == e["sample_start"].astype(np.uint64).tobytes(), f"{tag}: sample_start differs from the model"
        assert release.tobytes() == e["sample_release"].astype(np.uint64).tobytes(), f"{tag}: sample_release differs from the model"

    def tag(self, entries, tags, K, count=None, tag=""):
        import torch
        dl, res = self.dev_list(entries), self.result(2)
        dc = None if count is None else torch.tensor([count, 4321], dtype=torch.int32, device="cuda")
        self.db.tag_slots(dl.data_ptr(), tags, K, dc.data_ptr() if dc is not None else 0, res.data_ptr())
        want = OM.tag_slots(self.owner, entries, tags, count, K)
        got = self.read(res, 2, tag)
        print(f"{tag}: tag_slots d_result {got}, the model {want}")
        assert got == want, f"{tag}: tag_slots d_result {got}, the model says {want}"
        self.same(tag)

    def find(self, first, count, K, tags, tag=""):
        import torch
        out = torch.full((len(tags) + 8,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.db.find_owned(first, count, K, tags, out.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = OM.find_owned(self.owner, first, count, K, tags)
        bad = np.flatnonzero(got[:len(tags)] != want)
        assert not len(bad), f"{tag}: d_slots_out differs at {bad[:8].tolist()}: {got[bad[:8]].tolist()} / {want[bad[:8]].tolist()}"
        assert (got[len(tags):] == FILL).all(), f"{tag}: entries past n were written"
        return want

    def stamp(self, entries, tags, K, mask, stamps, count=None, tag=""):
        import torch
        dl, res = self.dev_list(entries), self.result(3)
        dc = None if count is None else torch.tensor([count, 4321], dtype=torch.int32, device="cuda")
        self.db.stamp_owned(dl.data_ptr(), tags, K, mask, stamps, res.data_ptr(), dc.data_ptr() if dc is not None else 0)
        want, voices = OM.stamp_owned(self.owner, self.truth, entries, tags, count, K, mask, stamps, self.now())
        got = self.read(res, 3, tag)
        print(f"{tag}: stamp_owned d_result {got}, the model {want}")
        assert got == want, f"{tag}: stamp_owned d_result {got}, the model says {want}"
        self.same(tag)
        return want, voices

    def release(self, first, count, K, mask, tags, stamps, tag=""):
        res = self.result(3)
        self.db.release_tags(first, count, K, mask, tags, stamps, res.data_ptr())
        want, voices, lst = OM.release_tags(self.owner, self.truth, first, count, K, mask, tags, stamps, self.now())
        got = self.read(res, 3, tag)
        print(f"{tag}: release_tags d_result {got}, the model {want}")
        assert got == want, f"{tag}: release_tags d_result {got}, the model says {want}"
        self.same(tag)
        return want, voices, lst

    def clear(self, first, count, tag=""):
        self.db.owner_clear(first, count)
        OM.clear(self.owner, first, count)
        self.same(tag)

    def block(self, tag="", stems=False):
        if stems:
            x, xs = self.db.render_host(F, 2, 0, want_stems=True)
        else:
            render_blocks(self.db, (F,))
        ref = cpuref.render(self.truth, self.gl, self.tables, F, 0, want_stems=stems)
        if stems:
            assert xs.tobytes() == ref["stems"].tobytes(), f"{tag}: stems differ from the oracle"
        a = self.bank.copy()
        self.db.download(a)
        assert not a.rw_equal(self.truth), f"{tag}: state differs from the oracle: {a.rw_equal(self.truth)}"
        self.same(tag)

    def close(self):
        self.db.close()


def padded_tags(tags, n):
    """`tags` first, then distinct tags nobody carries (every other one at or above 2^31), n in all."""
    extra = [(0x40000000 + 3 * k) | (0x80000000 if k & 1 else 0) for k in range(n - len(tags))]
    assert not set(extra) & set(int(t) for t in tags)
    return np.array(list(tags) + extra, np.uint32)[:n]


# ---------------------------------------------------------------------------------------------- 1. every call against the model

# (n voices, K, first, count): one wavefront; a range that starts at a multiple of K that is no multiple of 256 and ends ragged;
# K = 64 over seventeen voice workgroups; 2079 slots of K = 2 from voice 2: nine workgroups of the find pass, the last one ragged
SHAPES = [(64, 1, 0, 64), (320, 8, 24, 296), (4160, 64, 64, 4096), (4160, 2, 2, 4158)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,first,count", SHAPES)
def test_every_call_against_the_model(dev, n, K, first, count):
    bank, tables, g, now = plain_bank(n)
    r = Rig(dev, bank, tables, g)
    mask = 1 if K == 1 else (1 << (K - 1)) | 1                       # the first and the last voice of a slot
    last = first + count - K
    mid = first + (count // K // 2) * K
    outside = 0 if first > 0 else None                               # a slot of the bank below the range
    try:
        assert not r.db.download_owners().any()                      # nothing was ever tagged: zeros
        r.same("before")
        # the range's first and last slot, two slots with ONE tag (mid and the slot after it), tags at or above 2^31, holes
        t_first, t_last, t_twice, t_out = 0x80000000, 0xFFFFFFFF, 7, 0x12345678
        entries = [last, -1, first, mid + K, n, mid, first + 1 if K > 1 else -5, 2**31 - 64]
        tags = [t_last, 91, t_first, t_twice, 92, t_twice, 93, 94]
        if outside is not None:
            entries.append(outside)
            tags.append(t_out)
        r.tag(entries, tags, K, tag="tags with holes")
        assert r.owner[first] == t_first and r.owner[last] == t_last and r.owner[mid] == r.owner[mid + K] == t_twice
        for m in (1, 2, 1023, 1024):
            want = r.find(first, count, K, padded_tags([t_twice, t_last, t_first, t_out][:max(m, 1)], m), tag=f"find {m} tags")
            assert want[0] == mid                                    # the LOWER of the two slots that carry the tag
            if m >= 4:
                assert want[1] == last and want[2] == first and want[3] == -1     # (carried outside the range, or by nobody)
        a = r.find(first, count, K, padded_tags([t_last, t_twice], 700), tag="again")
        b = r.find(first, count, K, padded_tags([t_last, t_twice], 700), tag="and again")   # the same state gives the same bytes
        assert a.tobytes() == b.tobytes()
        r.find(mid, K, K, [t_twice, t_first], tag="a range of one slot")
        # a note-off on a list with holes, a stolen slot (wrong tag) and an untagged one; a count shorter than n
        free = first + K if first + K not in (mid, mid + K, last) else first + 2 * K
        off = [first, -1, last, mid, free, n - K + 1 if K > 1 else n, mid + K]
        off_tags = [t_first, 5, 0x7FFFFFFF, t_twice, 6, 8, t_twice]
        want, voices = r.stamp(off, off_tags, K, mask, REL, count=6, tag="note-off, count 6 of 7")
        assert want == [2, 2, 2] and sum(want) == 6
        want, _ = r.stamp(off, off_tags, K, mask, REL | TRIG, tag="trigger and release, no count")
        assert want == [3, 2, 2]
        # tag 0 clears the owner: the same note-off then misses
        r.tag([first], [0], K, tag="tag 0")
        want, _ = r.stamp([first], [t_first], K, mask, REL, tag="after tag 0")
        assert want == [0, 1, 0]
        r.block("a block after the stamps")
        # note-off by id: the lower slot of the two, the last slot, a tag nobody carries, a tag carried outside the range
        want, voices, lst = r.release(first, count, K, mask, [t_twice, 0x55, t_last, t_out], TRIG, tag="release_tags")
        assert want == [2, 0, 2] and lst.tolist() == [mid, -1, last, -1]
        assert mid + K + (K - 1) not in voices.tolist() and len(voices) == 2 * bin(mask).count("1")
        r.release(first, count, K, mask, padded_tags([t_last], 1024), REL, tag="release 1024 tags")
        r.block("a block after release_tags")
        r.clear(mid, K, tag="owner_clear of one slot")
        assert r.find(first, count, K, [t_twice], tag="after the clear")[0] == mid + K
        r.clear(0, n, tag="owner_clear of the bank")
        assert not r.owner.any()
        assert r.db.list_violations() == 0
    finally:
        r.close()


@pytest.mark.gpu
def test_on_a_scene_with_every_kind_of_slot(dev):
    """tests/slot_steal_scenes.py's bank (idle, released, finished and dead slots): the guard looks at the owner word alone, the
    stamps are skred_bank_stamp_slots' -- a release on a voice at rest stores nothing."""
    n, K, mask = 320, 8, 0x55
    bank, tables, g, truth, now, kind = SS.scene(n, K, mask)
    r = Rig(dev, bank, tables, g)
    try:
        for f in SS.FRAMES:
            render_blocks(r.db, (f,))
            cpuref.render(r.truth, r.gl, r.tables, f, 0)
        heads = np.arange(0, n, K, dtype=np.int32)
        tags = (0x80000000 + np.arange(len(heads))).astype(np.uint32)
        r.tag(heads, tags, K, tag="every slot")
        rng = np.random.default_rng(5)
        pick = rng.permutation(len(heads))[:24]
        wrong = tags[pick].copy()
        wrong[::5] += 1000                                                         # every fifth note-off carries a stale tag
        want, voices = r.stamp(heads[pick], wrong, K, mask, REL, tag="a chord of 24")
        assert want == [24 - 5, 5, 0]
        want, _, _ = r.release(0, n, K, mask, tags[::3], REL, tag="every third by id")
        assert want == [len(tags[::3]), 0, 0]
        r.block("the scene")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 2. the theft

@pytest.mark.gpu
def test_a_stolen_chord_keeps_its_notes(dev):
    import torch
    st = S.Story()
    r = Rig(dev, st.bank, st.tables, st.g)
    r.truth, r.gl, r.owner = st.truth, st.gl, st.owner                           # the story's oracle is the rig's
    K, N = S.K, S.N
    try:
        # chord A on the idle slots, tagged from its d_assigned
        want_a, tagged = st.chord_a()
        da = torch.full((len(want_a) + 8,), FILL, dtype=torch.int32, device="cuda")
        dr = torch.full((3,), FILL, dtype=torch.int32, device="cuda")
        ta = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.db.note_on_idle_slots(st.a_notes, S.idle_q(), S.VMASK, da.data_ptr(), dr.data_ptr())
        r.db.tag_slots(da.data_ptr(), S.A_TAGS, K, 0, ta.data_ptr())              # same stream, nothing waited for
        torch.cuda.synchronize()
        assert np.array_equal(da.cpu().numpy()[:len(want_a)], want_a) and ta.cpu().numpy().tolist() == tagged
        r.same("chord A")
        r.block("after A", stems=True)
        # the bank fills up: every other slot is played again, and tagged
        dl = r.dev_list(S.others())
        r.db.stamp_slots(dl.data_ptr(), len(S.others()), K, S.MMASK, TRIG)
        r.db.tag_slots(dl.data_ptr(), S.c_tags(), K)
        assert st.fill_up() == [56, 0]
        r.same("filled up")
        r.block("after the fill", stems=True)
        # chord B steals
        want_b, counts, tagged = st.chord_b()
        dab = torch.full((S.B_COUNT + 8,), FILL, dtype=torch.int32, device="cuda")
        tb = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.db.note_on_steal_slots(st.b_notes, S.idle_q(), S.steal_q().c(), S.VMASK, dab.data_ptr(), dr.data_ptr())
        r.db.tag_slots(dab.data_ptr(), S.B_TAGS, K, 0, tb.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(dab.cpu().numpy()[:S.B_COUNT], want_b), (dab.cpu().numpy().tolist(), want_b.tolist())
        assert tuple(dr.cpu().numpy().tolist()) == counts == (S.B_COUNT, 0, S.B_COUNT) and tb.cpu().numpy().tolist() == tagged
        r.same("chord B")
        stolen = len(set(want_a.tolist()) & set(want_b.tolist()))
        assert stolen == S.B_COUNT
        # A's key is lifted: the note-off on A's own d_assigned, with A's tags
        res = r.result(3)
        r.db.stamp_owned(da.data_ptr(), S.A_TAGS, K, S.VMASK, REL, res.data_ptr())
        want, voices = st.a_off()
        got = r.read(res, 3, "A's note-off")
        assert got == want == [len(want_a) - stolen, stolen, 0], (got, want)
        r.same("A's note-off")
        _, release = r.db.download_env_clocks()
        b_voices = np.concatenate([np.arange(s, s + K) for s in want_b])
        assert (release[b_voices] == 0).all(), "a note of chord B was released by A's note-off"
        r.block("after A's note-off", stems=True)                                 # B's voices: the oracle WITHOUT the release
        # ... and B is released by its tags alone
        want, voices, lst = r.release(0, N, K, S.VMASK, S.B_TAGS, REL, tag="B's note-off by id")
        assert want == [S.B_COUNT, 0, 0] and np.array_equal(lst, want_b) and sorted(voices.tolist()) == sorted(b_voices.tolist())
        r.block("after B's note-off", stems=True)
        assert r.db.list_violations() == 0
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 3. controllers under the guard

@pytest.mark.gpu
def test_ctl_owned_against_the_model_and_the_host_route(dev):
    import torch
    n, K, mask = 320, 8, 0x55
    bank, tables, g = banks.bank_c2(n)
    bank["voice_amp"][2::16] = 0.0                                                # voices the AMP guard leaves alone
    r = Rig(dev, bank, tables, g)
    twin = open_bank(dev, bank, tables, g)
    mirror = bank.copy()
    try:
        chord = np.array([8, 312, 16, 160], np.int32)
        tags = np.array([0x80000010, 0x11, 0x12, 0xFFFFFFFE], np.uint32)
        r.tag(chord, tags, K, tag="the chord")
        r.tag([16], [0x99], K, tag="slot 16 is stolen")
        entries = np.array([8, -1, 312, 16, 4, 160, 320, 24], np.int32)
        etags = np.array([0x80000010, 1, 0x11, 0x12, 2, 0xFFFFFFFE, 3, 4], np.uint32)
        for i, (bits, count) in enumerate(((CM.AMP | CM.FILTER | CM.PAN | CM.PHASE_INC, None), (CM.ALL & ~CM.PHASE_INC, 6), (CM.FILTER, None))):
            co = banks.biquad_coeffs(np.array([1]), np.array([800.0 + 50 * i], np.float32), np.array([1.1], np.float32), 48000)
            ctls = [ctl(bits, phase_inc=0.2 + 0.01 * l, inc_scale=1.0594631, amp=0.3 + 0.01 * l, pan_left=0.2, pan_right=0.7,
                        b0=float(co["b0"][0]), b1=float(co["b1"][0]), b2=float(co["b2"][0]), a1=float(co["a1"][0]), a2=float(co["a2"][0]),
                        attack_time=30.0, decay_time=60.0 + l, sustain_level=0.5, release_time=400.0, velocity=0.7, smoothing=0.25,
                        fm_depth=0.05, freq_scale=1.0, am_depth=0.1, pan_depth=0.1, cz_depth=0.2, cz_dist=0.3) for l in range(K)]
            dl, res = r.dev_list(entries), r.result(3)
            dc = None if count is None else torch.tensor([count, 99], dtype=torch.int32, device="cuda")
            r.db.ctl_owned(ctls, mask, dl.data_ptr(), etags, dc.data_ptr() if dc is not None else 0, res.data_ptr())
            want, touched = OM.ctl_owned(r.owner, (r.truth, mirror), ctls, mask, entries, etags, count)
            got = r.read(res, 3, f"ctl_owned {i}")
            print(f"ctl_owned {i}: d_result {got}, the model {want}")
            assert got == want and want[2] == (2 if count is None else 1)         # slot 16 (stolen), slot 24 (untagged)
            a = bank.copy()
            r.db.download(a)
            r.db.download_ctl(a)
            assert not CM.words_differ(a, mirror), f"ctl_owned {i}: controller words differ from the model: {CM.words_differ(a, mirror)}"
            for field, sub in CM.CTL_WORDS:                                       # the stolen slot's words are unchanged
                assert CM.word(a, field, sub)[16:24].tobytes() == CM.word(bank, field, sub)[16:24].tobytes(), (field, sub)
            twin.update(mirror, touched, DIRTY_PARAMS | DIRTY_PAN)
            b = bank.copy()
            twin.download(b)
            twin.download_ctl(b)
            assert not CM.words_differ(a, b) and not a.rw_equal(b), (CM.words_differ(a, b), a.rw_equal(b))
            x, y = render_blocks(r.db, (F,))[0], render_blocks(twin, (F,))[0]
            cpuref.render(r.truth, r.gl, r.tables, F, 0)
            assert x.tobytes() == y.tobytes(), f"ctl_owned {i}: the mixes of the two routes differ"
            assert r.db.last_kernel() == twin.last_kernel()
            a = bank.copy()
            r.db.download(a)
            assert not a.rw_equal(r.truth), a.rw_equal(r.truth)
        r.same("after the controllers")
        assert want[1] >= 0 and r.db.list_violations() == twin.list_violations() == 0
    finally:
        r.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 4. the planner's shadow

@pytest.mark.gpu
def test_a_twin_without_owner_calls_renders_the_same_blocks(dev):
    """tests/test_slots.py's in-place bank (4096 voices, two per lane, SKRED_OPT_IN_PLACE = 2).  One bank tags its chords and
    releases them through stamp_owned and release_tags; its twin receives no owner call, only the equivalent stamp_slots.  Mix,
    state, kernel family, the in-place choice and the violation counter agree in every block."""
    n, K, mask = 4096, 8, 0xFE
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    r = Rig(dev, bank, tables, g, setup)
    twin = open_bank(dev, bank, tables, g, setup)
    try:
        chords = {1: np.arange(0, 40 * K, 2 * K, dtype=np.int32), 3: np.arange(1024, 1024 + 12 * K, K, dtype=np.int32)}
        tagged = {}
        taken = []
        for k in range(7):
            if k in chords:
                slots = chords[k]
                tags = (0x80000000 + 100 * k + np.arange(len(slots))).astype(np.uint32)
                dl = r.dev_list(slots)
                r.db.stamp_slots(dl.data_ptr(), len(slots), K, mask, TRIG)
                twin.stamp_slots(dl.data_ptr(), len(slots), K, mask, TRIG)
                SM.stamp(r.truth, SM.stamp_voices(slots, len(slots), None, K, mask, n), TRIG, r.now())
                r.tag(slots, tags, K, tag=f"chord {k}")
                tagged[k] = (slots, tags, dl)
            if k == 2:                                                            # chord 1 is lifted through its list
                slots, tags, dl = tagged[1]
                want, _ = r.stamp(slots, tags, K, mask, REL, tag="chord 1 off")
                assert want == [len(slots), 0, 0]
                twin.stamp_slots(dl.data_ptr(), len(slots), K, mask, REL)
            if k == 5:                                                            # chord 3 by id
                slots, tags, dl = tagged[3]
                want, _, lst = r.release(0, n, K, mask, tags, REL, tag="chord 3 off")
                assert want == [len(slots), 0, 0]
                twin.stamp_slots(dl.data_ptr(), len(slots), K, mask, REL)
            x, y = render_blocks(r.db, (F,))[0], render_blocks(twin, (F,))[0]
            cpuref.render(r.truth, r.gl, r.tables, F, 0)
            taken.append((r.db.last_in_place(), twin.last_in_place()))
            assert x.tobytes() == y.tobytes(), f"block {k}: the mixes differ"
            assert r.db.last_kernel() == twin.last_kernel() == 3 and taken[-1][0] == taken[-1][1], (k, taken)
            a, b = bank.copy(), bank.copy()
            r.db.download(a)
            twin.download(b)
            assert not a.rw_equal(b) and not a.rw_equal(r.truth), (a.rw_equal(b), a.rw_equal(r.truth))
            assert r.db.list_violations() == twin.list_violations() == 0
        assert not twin.download_owners().any()                                   # the twin was never tagged: zeros
        print(f"in place per block: {taken}")
    finally:
        r.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 5. refusals

@pytest.mark.gpu
def test_refusals_write_nothing(dev):
    import torch
    n, K = 256, 8
    bank, tables, g, now = plain_bank(n)
    r = Rig(dev, bank, tables, g)
    try:
        L = r.db.L
        r.tag([8, 16], [5, 6], K, tag="two tags")
        dl = r.dev_list([8, 16, 24, 32])
        out = torch.full((8,), FILL, dtype=torch.int32, device="cuda")
        res = torch.full((3,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        good, zero, dup = device.tag_array([5, 6, 7, 8]), device.tag_array([5, 0, 7, 8]), device.tag_array([5, 6, 5, 8])
        arr = device.ctl_array([ctl(device.CTL_PAN, pan_left=0.5, pan_right=0.5)] * K)
        p = C.cast(arr, C.c_void_p)
        h, d, o, rs = r.db.h, dl.data_ptr(), out.data_ptr(), res.data_ptr()
        assert L.skred_bank_tag_slots(h, d, good.ctypes.data, 4, None, 12, rs, None) == RANGE
        assert L.skred_bank_tag_slots(h, d, None, 4, None, K, rs, None) == BAD
        assert L.skred_bank_find_owned(h, 0, n, K, zero.ctypes.data, 4, o, None) == BAD
        assert L.skred_bank_find_owned(h, 0, n, K, dup.ctypes.data, 4, o, None) == BAD
        assert L.skred_bank_find_owned(h, 4, 8, K, good.ctypes.data, 4, o, None) == RANGE
        assert L.skred_bank_find_owned(h, 0, n + K, K, good.ctypes.data, 4, o, None) == RANGE
        assert L.skred_bank_find_owned(h, 0, 0, K, good.ctypes.data, 4, o, None) == RANGE
        assert L.skred_bank_stamp_owned(h, d, zero.ctypes.data, 4, None, K, 0xFF, REL, rs, None) == BAD
        assert L.skred_bank_stamp_owned(h, d, good.ctypes.data, 4, None, K, 0xFF, REL, None, None) == BAD
        assert L.skred_bank_stamp_owned(h, d, good.ctypes.data, 4, None, K, 0x1FF, REL, rs, None) == BAD
        assert L.skred_bank_stamp_owned(h, d, good.ctypes.data, 4, None, K, 0xFF, 1, rs, None) == BAD
        assert L.skred_bank_release_tags(h, 0, n, K, 0xFF, dup.ctypes.data, 4, REL, rs, None) == BAD
        assert L.skred_bank_release_tags(h, 0, n, 3, 0x7, good.ctypes.data, 4, REL, rs, None) == RANGE
        assert L.skred_bank_ctl_owned(h, p, K, 0xFF, d, zero.ctypes.data, 4, None, rs, None) == BAD
        assert L.skred_bank_ctl_owned(h, p, K, 0, d, good.ctypes.data, 4, None, rs, None) == BAD
        assert L.skred_bank_owner_clear(h, 8, n, None) == RANGE
        for call in (lambda: L.skred_bank_find_owned(h, 0, n, K, good.ctypes.data, 0, o, None),
                     lambda: L.skred_bank_stamp_owned(h, d, good.ctypes.data, 0, None, K, 0xFF, REL, rs, None),
                     lambda: L.skred_bank_release_tags(h, 0, n, K, 0xFF, good.ctypes.data, 0, REL, rs, None)):
            assert call() == 0                                                    # n == 0: nothing is done
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == FILL).all() and (res.cpu().numpy() == FILL).all()
        r.same("after the refusals")                                              # owners and clocks as they were
        assert r.find(0, n, K, [6, 5], tag="the bank still answers").tolist() == [16, 8]
    finally:
        r.close()
