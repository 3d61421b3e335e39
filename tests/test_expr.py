"""Channels and per-note expression on the device (skred_bank_find_match / _find_match_host / _stamp_match / _ctl_match /
_ctl_owned_each / _ctl_tags_each), byte for byte.

After every call the device is held to tests/expr_model.py: the list and the count word of a find, every d_result word, the owner
array and the envelope clocks (download_owners, download_env_clocks), and every word a controller can store (download, download_ctl)
against the oracle's bank with the model's stores.  State after a rendered block is compared with oracle.cpuref.  The channel scene is
tests/expr_scenes.py's; tests/test_expr_cpu.py asserts on the oracle alone that it steals.
"""
import numpy as np
import pytest

import ctl_model as CM
import expr_model as EM
import expr_scenes as XS
import owner_scenes as S
import slot_model as SM
from oracle import cpuref
from skred_amd import banks, device
from skred_amd.device import ctl, ctl_each, owner_match
from test_idle import open_bank, render_blocks, traffic_bank
from test_owner import FILL, Rig
from test_slot_steal import plain_bank

REL, TRIG = SM.STAMP_RELEASE, SM.STAMP_TRIGGER
DIRTY_PARAMS, DIRTY_PAN = 1, 8
F = 64
CH = 0xFF000000


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def words_same(r, tag):
    """every word a controller can store, as the device holds it, against the oracle's bank"""
    a = r.bank.copy()
    r.db.download(a)
    r.db.download_ctl(a)
    assert not CM.words_differ(a, r.truth), f"{tag}: controller words differ from the model: {CM.words_differ(a, r.truth)}"


def find(r, first, count, K, value, mask, max_out, tag):
    import torch
    want, total = EM.find_match(r.owner, first, count, K, value, mask, max_out)
    out = torch.full((max_out + 8,), FILL, dtype=torch.int32, device="cuda")
    cnt = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.db.find_match(first, count, K, owner_match(value, mask), max_out, out.data_ptr() if max_out else 0, cnt.data_ptr())
    torch.cuda.synchronize()
    got, c = out.cpu().numpy(), cnt.cpu().numpy()
    print(f"{tag}: max_out {max_out}: d_count {c[0]}, the model's total {total}, written {len(want)}")
    assert c[0] == total and (c[1:] == FILL).all(), f"{tag}: d_count {c.tolist()}, the model's total {total}"
    assert np.array_equal(got[:len(want)], want), f"{tag}: the list differs from the model"
    assert (got[len(want):] == FILL).all(), f"{tag}: entries past min(total, max_out) were written"
    assert (np.diff(want) > 0).all()
    lst, t = r.db.find_match_host(first, count, K, owner_match(value, mask), max_out)
    assert t == total and np.array_equal(lst, want), f"{tag}: find_match_host differs from the model"
    return want, total


def stamp_match(r, first, count, K, vmask, value, mask, stamps, tag):
    res = r.result(2)
    r.db.stamp_match(first, count, K, vmask, owner_match(value, mask), stamps, res.data_ptr())
    want, voices = EM.stamp_match(r.owner, r.truth, first, count, K, vmask, value, mask, stamps, r.now())
    got = r.read(res, 2, tag)
    print(f"{tag}: stamp_match d_result {got}, the model {want}")
    assert got == want, f"{tag}: stamp_match d_result {got}, the model says {want}"
    r.same(tag)
    return want, voices


def ctl_match(r, ctls, first, count, vmask, value, mask, tag):
    res = r.result(3)
    r.db.ctl_match(ctls, first, count, vmask, owner_match(value, mask), res.data_ptr())
    want, touched = EM.ctl_match(r.owner, (r.truth,), ctls, first, count, vmask, value, mask)
    got = r.read(res, 3, tag)
    print(f"{tag}: ctl_match d_result {got}, the model {want}")
    assert got == want, f"{tag}: ctl_match d_result {got}, the model says {want}"
    words_same(r, tag)
    return want, touched


# ---------------------------------------------------------------------------------------------- 1. matches against the model

# (n voices, K, first, count).  The find pass takes one lane per SLOT, 256 to a workgroup; the stamps and the controller one per voice.
# K = 1 and K = 2: ranges inside the bank of three full workgroups of slots and a ragged fourth.  K = 8 and K = 64: every slot of
# banks of 64 * K .. 2048 voices, and a range inside one, eight workgroups of voices with a ragged last one.
SHAPES = [(64, 1, 0, 64), (2048, 1, 5, 1000), (2048, 2, 2, 1610), (512, 8, 0, 512), (2048, 8, 24, 2000), (2048, 64, 64, 1920)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,first,count", SHAPES)
def test_matches_against_the_model(dev, n, K, first, count):
    bank, tables, g, now = plain_bank(n)
    bank["voice_amp"][3::7] = 0.0                                    # voices the AMP guard leaves alone
    r = Rig(dev, bank, tables, g)
    full = (1 << K) - 1
    part = full if K == 1 else (1 << (K - 1)) | 1
    try:
        # a find on a never-tagged bank allocates the array and matches nothing
        assert find(r, first, count, K, 0, 0, 4, "never tagged")[1] == 0
        heads = np.arange(first, first + count, K, dtype=np.int32)
        s = np.arange(len(heads), dtype=np.uint32)
        # of every five slots: untagged, channel 1, channel 2, channel 0xFF, channel 1 -- untagged slots between tagged ones
        tags = np.select([s % 5 == 0, s % 5 == 2, s % 5 == 3], [np.uint32(0), np.uint32(2 << 24) | (s + 1), np.uint32(CH) | (s + 1)],
                         np.uint32(1 << 24) | (s + 1)).astype(np.uint32)
        if len(heads) > 8:
            tags[8] = 0xFFFFFFFF                                     # (slot 8 is on channel 0xFF: every bit set)
        r.tag(heads, tags, K, tag="channels")
        if first > 0:
            r.tag([0], [1 << 24 | 0x77], K, tag="a slot of channel 1 below the range")
        one = int(tags[min(6, len(tags) - 1)])
        for value, mask, name in ((0, 0, "every tagged slot"), (1 << 24, CH, "channel 1"), (one, 0xFFFFFFFF, "one note"),
                                  (7 << 24, CH, "nobody"), (0xFFFFFFFF, 0xFFFFFFFF, "all ones"), (0xFF << 24, CH, "channel 0xFF")):
            total = EM.find_match(r.owner, first, count, K, value, mask, 0)[1]
            for max_out in sorted({0, 1, total, total + 5}):
                find(r, first, count, K, value, mask, max_out, name)
        assert EM.find_match(r.owner, first, count, K, one, 0xFFFFFFFF, 9)[1] == 1
        find(r, first + K, K, K, 1 << 24, CH, 3, "a range of one slot")
        # all notes off on channel 1 (partial mask), a trigger and release on everything tagged, a channel nobody is on
        want, _ = stamp_match(r, first, count, K, part, 1 << 24, CH, REL, "channel 1 off")
        assert want[0] == int((tags >> 24 == 1).sum()) and sum(want) == count // K
        stamp_match(r, first, count, K, full, 0, 0, TRIG | REL, "every tagged slot, trigger and release")
        assert stamp_match(r, first, count, K, full, 7 << 24, CH, REL, "nobody")[0] == [0, count // K]
        r.block("a block after the stamps")
        # controllers by channel: words that list nobody, then every word but PHASE_INC on another channel
        co = banks.biquad_coeffs(np.array([1]), np.array([850.0], np.float32), np.array([1.1], np.float32), 48000)
        vals = dict(phase_inc=0.2, inc_scale=1.0594631, amp=0.3, pan_left=0.2, pan_right=0.7, b0=float(co["b0"][0]), b1=float(co["b1"][0]),
                    b2=float(co["b2"][0]), a1=float(co["a1"][0]), a2=float(co["a2"][0]), attack_time=30.0, decay_time=60.0, sustain_level=0.5,
                    release_time=400.0, velocity=0.7, smoothing=0.25, fm_depth=0.05, freq_scale=1.0, am_depth=0.1, pan_depth=0.1,
                    cz_depth=0.2, cz_dist=0.3)
        quiet = [ctl(CM.FILTER | CM.PAN, **dict(vals, pan_left=0.01 * l)) for l in range(K)]
        loud = [ctl(CM.ALL & ~CM.PHASE_INC, **dict(vals, amp=0.3 + 0.01 * l)) for l in range(K)]
        want, _ = ctl_match(r, quiet, first, count, full, 2 << 24, CH, "channel 2: filter and pan")
        assert want[0] == int((tags >> 24 == 2).sum()) * K and want[1] == 0
        want, touched = ctl_match(r, loud, first, count, part, 0xFF << 24, CH, "channel 0xFF: every word")
        assert want[1] == int((bank["voice_amp"][touched] == 0).sum())     # the withheld amps on zero-amp voices
        assert ctl_match(r, quiet, first, count, full, 7 << 24, CH, "nobody")[0] == [0, 0, count // K]
        r.block("a block after the controllers")
        r.same("the owner array is only read")
        assert r.db.list_violations() == 0
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 2. per-entry controller values

@pytest.mark.gpu
@pytest.mark.parametrize("n_entries,K", [(1, 8), (2, 64), (255, 1), (256, 2), (257, 2), (1024, 2)])
def test_per_entry_values_against_the_model(dev, n_entries, K):
    n = 2048
    bank, tables, g, now = plain_bank(n)
    bank["voice_amp"][5::11] = 0.0                                   # zero-amp voices: the AMP guard withholds
    slots = np.arange(0, n, K, dtype=np.int32)
    rng = np.random.default_rng(n_entries)
    pick = rng.permutation(len(slots))[:min(n_entries, len(slots))]
    hot = int(slots[pick[0]])
    bank["voice_phase_inc"][hot:hot + K] = np.float32(3e38)          # an increment whose bend overflows
    r = Rig(dev, bank, tables, g)
    full = (1 << K) - 1
    part = full if K == 1 else (1 << (K - 1)) | 1
    try:
        r.tag(slots, (np.uint32(0x0B000000) + np.arange(len(slots), dtype=np.uint32) + np.uint32(1)).astype(np.uint32), K, tag="every slot")
        entries = np.full(n_entries, -1, np.int32)
        entries[:len(pick)] = slots[pick]                            # (n_entries beyond the slots the bank has: -1 entries)
        tags = np.array([r.owner[e] if e >= 0 else 0x70000000 + k for k, e in enumerate(entries)], np.uint32)
        if n_entries > 2:
            entries[3::7] = -1                                       # holes: the -1 of a dropped note
            tags[4::5] ^= 0x00800000                                 # stolen: the slot carries somebody else's tag
        assert len(set(tags.tolist())) == n_entries
        bits = [EM.EACH_INC_SCALE, EM.EACH_AMP_SCALE, EM.EACH_VELOCITY, EM.EACH_PAN, EM.EACH_ALL]
        each = [ctl_each(bits[k % 5], inc_scale=float(np.float32(2.0 ** ((k % 25 - 12) / 12.0))), amp_scale=0.25 + 0.001 * k,
                         velocity=0.3 + 0.0005 * k, pan_left=0.001 * (k % 1000), pan_right=0.9) for k in range(n_entries)]
        each[0] = ctl_each(EM.EACH_ALL, inc_scale=2.0, amp_scale=1e-45, velocity=0.5, pan_left=0.5, pan_right=0.5)
        recs = [ctl(CM.AMP | CM.FILTER | CM.SMOOTHING, amp=0.5 + 0.005 * l, b0=0.4, b1=0.1, b2=0.05, a1=-0.2, a2=0.1, smoothing=0.3) for l in range(K)]
        for i, (ctls, ee, vmask) in enumerate(((recs, each, full), (recs, each, part),
                                               (None, [ctl_each(int(e.set) & ~EM.EACH_AMP_SCALE or EM.EACH_PAN, inc_scale=e.inc_scale,
                                                                velocity=e.velocity, pan_left=e.pan_left, pan_right=e.pan_right) for e in each], part))):
            dl, res = r.dev_list(entries), r.result(3)
            r.db.ctl_owned_each(ctls, ee, vmask, dl.data_ptr(), tags, K, 0, res.data_ptr())
            want, touched = EM.ctl_owned_each(r.owner, (r.truth,), ctls, ee, K, vmask, entries, tags, None)
            got = r.read(res, 3, f"ctl_owned_each {i}")
            print(f"ctl_owned_each {i}: d_result {got}, the model {want}")
            assert got == want, f"ctl_owned_each {i}: d_result {got}, the model says {want}"
            words_same(r, f"ctl_owned_each {i}")
            if i == 0:
                # the overflowing bend (every voice of the slot) and the amp product that rounds to 0 (0.5 * 1e-45, voice 0) were
                # withheld and counted, the words kept
                assert np.all(r.truth["voice_phase_inc"][hot:hot + K] == np.float32(3e38)) and want[1] >= K + 1
                assert r.truth["voice_amp"][hot] == bank["voice_amp"][hot]
        # a count word shorter than the list
        if n_entries > 2:
            import torch
            dl, res = r.dev_list(entries), r.result(3)
            dc = torch.tensor([n_entries // 2, 99], dtype=torch.int32, device="cuda")
            r.db.ctl_owned_each(recs, each, full, dl.data_ptr(), tags, K, dc.data_ptr(), res.data_ptr())
            want, _ = EM.ctl_owned_each(r.owner, (r.truth,), recs, each, K, full, entries, tags, n_entries // 2)
            assert r.read(res, 3, "a count word") == want
            words_same(r, "a count word")
        # by note id: the tags travel sorted, every entry stays with its tag; a stolen tag is carried by nobody
        res = r.result(3)
        r.db.ctl_tags_each(recs, each, 0, n, part, tags, K, res.data_ptr())
        want, touched, lst = EM.ctl_tags_each(r.owner, (r.truth,), recs, each, 0, n, K, part, tags)
        got = r.read(res, 3, "ctl_tags_each")
        print(f"ctl_tags_each: d_result {got}, the model {want}, {int((lst >= 0).sum())} of {n_entries} tags found")
        assert got == want and want[2] == 0
        words_same(r, "ctl_tags_each")
        r.block("a block after the expression")
        r.same("the owner array is only read")
        assert r.db.list_violations() == 0
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 3. the channel scene

@pytest.mark.gpu
def test_two_channels_share_a_range_and_one_steals(dev):
    import torch
    st = XS.Story()
    r = Rig(dev, st.bank, st.tables, st.g)
    twin = open_bank(dev, st.bank, st.tables, st.g)                  # the host route: skred_bank_update and stamps on lists
    r.truth, r.gl, r.owner = st.truth, st.gl, st.owner
    K, N = XS.K, XS.N

    def both_blocks(tag):
        (x, xs), (y, ys) = r.db.render_host(F, 2, 0, want_stems=True), twin.render_host(F, 2, 0, want_stems=True)
        ref = cpuref.render(r.truth, r.gl, r.tables, F, 0, want_stems=True)
        assert xs.tobytes() == ref["stems"].tobytes(), f"{tag}: stems differ from the oracle"
        assert x.tobytes() == y.tobytes() and xs.tobytes() == ys.tobytes(), f"{tag}: the mixes or stems of the two routes differ"
        assert r.db.last_kernel() == twin.last_kernel(), f"{tag}: the kernel families differ"
        a, b = st.bank.copy(), st.bank.copy()
        r.db.download(a)
        twin.download(b)
        assert not a.rw_equal(b) and not a.rw_equal(r.truth), f"{tag}: {a.rw_equal(b)} / {a.rw_equal(r.truth)}"
        r.same(tag)
        return ref

    try:
        want_a, _ = st.chord_a()
        da = torch.full((len(want_a),), FILL, dtype=torch.int32, device="cuda")
        dr = torch.full((3,), FILL, dtype=torch.int32, device="cuda")
        for d in (r.db, twin):
            d.note_on_idle_slots(st.a_notes, S.idle_q(), S.VMASK, da.data_ptr(), dr.data_ptr())
        r.db.tag_slots(da.data_ptr(), XS.A_TAGS, K)
        both_blocks("after A")
        dl = r.dev_list(S.others())
        for d in (r.db, twin):
            d.stamp_slots(dl.data_ptr(), len(S.others()), K, S.MMASK, TRIG)
        r.db.tag_slots(dl.data_ptr(), XS.C_TAGS, K)
        st.fill_up()
        both_blocks("after the fill")
        want_b, counts, _ = st.chord_b()
        dab = torch.full((S.B_COUNT,), FILL, dtype=torch.int32, device="cuda")
        for d in (r.db, twin):
            d.note_on_steal_slots(st.b_notes, S.idle_q(), S.steal_q().c(), S.VMASK, dab.data_ptr(), dr.data_ptr())
        r.db.tag_slots(dab.data_ptr(), XS.B_TAGS, K)
        torch.cuda.synchronize()
        assert np.array_equal(dab.cpu().numpy(), want_b) and counts == (S.B_COUNT, 0, S.B_COUNT)
        r.same("chord B")
        survivors = sorted(set(want_a.tolist()) - set(want_b.tolist()))
        assert len(survivors) == len(want_a) - S.B_COUNT
        for ch, lst in ((XS.CH_A, survivors), (XS.CH_B, sorted(want_b.tolist()))):
            got, total = r.db.find_match_host(0, N, K, XS.channel(ch), N)
            assert got.tolist() == lst and total == len(lst)
        # all notes off on channel A: A's survivors, none of B
        want, voices = stamp_match(r, 0, N, K, S.VMASK, XS.CH_A << 24, XS.CH_MASK, REL, "all notes off on A")
        assert want == [len(survivors), N // K - len(survivors)]
        sl = r.dev_list(survivors)
        twin.stamp_slots(sl.data_ptr(), len(survivors), K, S.VMASK, REL)
        _, release = r.db.download_env_clocks()
        b_voices = np.concatenate([np.arange(s, s + K) for s in want_b])
        assert (release[b_voices] == 0).all(), "a note of channel B was released by A's all-notes-off"
        both_blocks("after A's all-notes-off")
        # B's mod wheel, then B's per-note bends by note id
        want, touched = ctl_match(r, XS.sweep(), 0, N, S.MMASK, XS.CH_B << 24, XS.CH_MASK, "B's sweep")
        assert want == [S.B_COUNT * 3, 0, N // K - S.B_COUNT] and set(touched.tolist()) <= set(b_voices.tolist())
        twin.update(r.truth, touched, DIRTY_PARAMS | DIRTY_PAN)
        both_blocks("after B's sweep")
        res = r.result(3)
        r.db.ctl_tags_each(None, XS.bends(), 0, N, S.MMASK, XS.B_TAGS, K, res.data_ptr())
        want, touched, lst = st.b_bends()
        assert r.read(res, 3, "B's bends") == want == [S.B_COUNT * 3, 0, 0] and np.array_equal(lst, want_b)
        words_same(r, "B's bends")
        twin.update(r.truth, touched, DIRTY_PARAMS | DIRTY_PAN)
        both_blocks("after B's bends")
        both_blocks("one block later")
        assert r.db.list_violations() == twin.list_violations() == 0
    finally:
        r.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 4. the planner's shadow

@pytest.mark.gpu
def test_the_planner_sees_what_the_unguarded_calls_show_it(dev):
    """tests/test_owner.py's in-place bank (two per lane, SKRED_OPT_IN_PLACE = 2) at 2048 voices.  One bank plays by channel; `host`
    never calls an entry point of this section -- it receives the same changes through stamp_slots and ctl_slots on the chord's list --
    and must render the same bytes; `plain` never hears of the filter sweep at all, and after a ctl_match that names only FILTER the
    planner of the first bank stands where plain's stands.

    The all-notes-off: stamp_match grows the motion-list bound by the whole RANGE (the host cannot know how many slots match), so the
    twins stamp a list of as many entries -- the chord's slots, then -1 holes, which stamp_slots skips and still counts into its bound.
    Their planners then stand where stamp_match leaves the first bank's, and mix, state, kernel family and in-place choice agree in
    every block."""
    n, K, mask = 2048, 8, 0xFE
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    r = Rig(dev, bank, tables, g, setup)
    host, plain = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    co = banks.biquad_coeffs(np.array([1]), np.array([700.0], np.float32), np.array([1.3], np.float32), 48000)
    filt = [ctl(CM.FILTER, b0=float(co["b0"][0]), b1=float(co["b1"][0]), b2=float(co["b2"][0]), a1=float(co["a1"][0]), a2=float(co["a2"][0]))
            for _ in range(K)]
    try:
        chord = np.arange(0, 40 * K, 2 * K, dtype=np.int32)
        tags = (np.uint32(3 << 24) + np.arange(len(chord), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        dl = r.dev_list(chord)
        padded = r.dev_list(np.concatenate([chord, np.full(n // K - len(chord), -1, np.int32)]))
        taken = []
        for k in range(6):
            if k == 1:
                for d in (r.db, host, plain):
                    d.stamp_slots(dl.data_ptr(), len(chord), K, mask, TRIG)
                SM.stamp(r.truth, SM.stamp_voices(chord, len(chord), None, K, mask, n), TRIG, r.now())
                r.tag(chord, tags, K, tag="the chord, on channel 3")
            if k == 3:                                                            # a filter sweep of the channel: lists nobody
                want, touched = ctl_match(r, filt, 0, n, mask, 3 << 24, CH, "filter only")
                assert want == [len(chord) * 7, 0, n // K - len(chord)]
                host.ctl_slots(filt, mask, dl.data_ptr(), len(chord))
            if k == 4:                                                            # all notes off on the channel
                want, _ = stamp_match(r, 0, n, K, mask, 3 << 24, CH, REL, "channel 3 off")
                assert want == [len(chord), n // K - len(chord)]
                for d in (host, plain):
                    d.stamp_slots(padded.data_ptr(), n // K, K, mask, REL)
            x, y = render_blocks(r.db, (F,))[0], render_blocks(host, (F,))[0]
            render_blocks(plain, (F,))
            cpuref.render(r.truth, r.gl, r.tables, F, 0)
            taken.append((r.db.last_kernel(), plain.last_kernel(), r.db.last_in_place(), plain.last_in_place()))
            assert x.tobytes() == y.tobytes(), f"block {k}: the mixes of the two routes differ"
            assert r.db.last_kernel() == host.last_kernel() == plain.last_kernel(), (k, taken)
            assert r.db.last_in_place() == host.last_in_place() == plain.last_in_place(), (k, taken)   # behind the filter sweep too: as if nothing was said
            a, b = bank.copy(), bank.copy()
            r.db.download(a)
            host.download(b)
            assert not a.rw_equal(b) and not a.rw_equal(r.truth), (a.rw_equal(b), a.rw_equal(r.truth))
            assert r.db.list_violations() == host.list_violations() == plain.list_violations() == 0
        print(f"(kernel, plain's kernel, in place, plain's in place) per block: {taken}")
        assert not host.download_owners().any() and not plain.download_owners().any()
    finally:
        r.close()
        host.close()
        plain.close()
