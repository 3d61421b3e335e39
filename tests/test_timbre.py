"""Per-note timbre on the device (skred_bank_ctl_owned_each_filter / _ctl_tags_each_filter), byte for byte.

After every call the device is held to tests/timbre_model.py: all three d_result words, the owner array and the envelope clocks,
every word a controller can store (download, download_ctl) and the whole read-write state -- the filter memory with it -- against
the oracle's bank with the model's stores.  Banks of 600 voices at K = 1, 4 and 64, lists of 1, 2, 1023 and 1024 entries with -1
holes and stolen slots, filter_mask equal to voice_mask and a strict subset of it, a count word shorter than the list, the range
[37, 537) at K = 1.  A twin driven by n single skred_bank_ctl_owned calls must hold the same bytes; with `each` given, every word but
the five coefficient words must be what skred_bank_ctl_owned_each alone leaves on another twin.  End to end: a chord through
skred_bank_note_on_channel on 3.sk with filtered carriers, one cutoff per note by note id, two blocks of 64 frames, the stems of the chord through
taps bit for bit against the oracle, the state after each block too, and the mix bit for bit against a bank on the host route."""
import numpy as np
import pytest

import ctl_model as CM
import expr_model as EM
import owner_model as OM
import slot_model as SM
import timbre_model as TM
from oracle import cpuref
from skred_amd import device
from skred_amd.bank import slot_query
from skred_amd.device import ctl, ctl_each, filter_each
from steal_model import ENV, FIN, OLDEST, RELEASED_FIRST
from test_idle import open_bank, render_blocks, traffic_bank
from test_owner import FILL, Rig
from test_slot_steal import patch_notes, plain_bank, playing_patch

F = 64
N = 600
RATE = 44100.0
DIRTY_PARAMS = 1
MEMORY = ("x1", "x2", "y1", "y2")


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def cutoff(k, mode=1):
    """the k-th of a ladder of cutoffs, as skred_filter_coeffs makes them"""
    return filter_each(*device.filter_coeffs(mode, 110.0 * 2.0 ** ((k % 72) / 12.0), 0.7 + 0.01 * (k % 50), RATE))


def bank_words(db, like):
    a = like.copy()
    db.download(a)
    db.download_ctl(a)
    return a


def whole_bank_same(r, tag):
    """every word the device holds against the oracle's bank: what a controller can store, the read-write state, owners and clocks"""
    a = bank_words(r.db, r.bank)
    assert not CM.words_differ(a, r.truth), f"{tag}: controller words differ from the model: {CM.words_differ(a, r.truth)}"
    assert not a.rw_equal(r.truth), f"{tag}: state differs from the model: {a.rw_equal(r.truth)}"
    for m in MEMORY:
        assert a["voice_filter"][m].tobytes() == r.truth["voice_filter"][m].tobytes(), f"{tag}: the filter memory {m} changed"
    r.same(tag)
    return a


def banks_same(x, y, like, tag, but=()):
    a, b = bank_words(x, like), bank_words(y, like)
    bad = {k: v for k, v in CM.words_differ(a, b).items() if k not in but}
    assert not bad and not a.rw_equal(b), f"{tag}: the two banks differ: {bad} {a.rw_equal(b)}"


def as_ctl(r):
    return ctl(int(r.set), **{f: float(getattr(r, f)) for f in EM.Rec.FIELDS})


def single_calls(twin, dl, ctls, each, filt, K, vmask, fmask, entries, tags, count=None):
    """the parent's only route: one skred_bank_ctl_owned per entry, with the records the entry leaves (the amp product made here)"""
    for k in range(len(tags) if count is None else min(count, len(tags))):
        recs = [ctl(0)] * K
        mask = 0
        for l in CM.lanes(vmask, K):
            r, _ = TM.lay_over(ctls[l] if ctls is not None else None, each[k] if each is not None else None,
                               filt[k] if (fmask >> l) & 1 else None)
            if r.set:
                recs = recs[:l] + [as_ctl(r)] + recs[l + 1:]
                mask |= 1 << l
        if mask and entries[k] >= 0:
            twin.ctl_owned(recs, mask, dl.data_ptr() + 4 * k, [tags[k]])


# ---------------------------------------------------------------------------------------------- 1. against the model and the twins

@pytest.mark.gpu
@pytest.mark.parametrize("n_entries,K", [(1, 4), (2, 64), (1023, 1), (1024, 1), (1024, 4)])
def test_per_entry_coefficients_against_the_model(dev, n_entries, K):
    import torch
    bank, tables, g, now = plain_bank(N)
    bank["voice_amp"][5::11] = 0.0                                   # zero-amp voices: the AMP guard withholds
    r = Rig(dev, bank, tables, g)
    singles, plain_each = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    slots = np.arange(0, N - K + 1, K, dtype=np.int32)
    full = (1 << K) - 1
    part = full if K == 1 else (1 << (K - 1)) | 1                    # voices 0 and K - 1
    sub = 1 if K == 1 else 1 << (K - 1)                              # a strict subset of `part` (K = 1 has none)
    rng = np.random.default_rng(n_entries + K)
    try:
        all_tags = (np.uint32(0x0B000000) + np.arange(len(slots), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(slots, all_tags, K, tag="every slot")
        dl = r.dev_list(slots)
        for d in (singles, plain_each):
            d.tag_slots(dl.data_ptr(), all_tags, K)
        pick = rng.permutation(len(slots))[:min(n_entries, len(slots))]
        entries = np.full(n_entries, -1, np.int32)
        entries[:len(pick)] = slots[pick]                            # (more entries than the bank has slots: -1 entries)
        tags = np.array([r.owner[e] if e >= 0 else 0x70000000 + k for k, e in enumerate(entries)], np.uint32)
        if n_entries > 2:
            entries[3::7] = -1                                       # holes: the -1 of a dropped note
            tags[4::5] ^= 0x00800000                                 # stolen: the slot carries somebody else's tag
        assert len(set(tags.tolist())) == n_entries
        filt = [cutoff(k, 1 + k % 5) for k in range(n_entries)]
        bits = [EM.EACH_INC_SCALE, EM.EACH_AMP_SCALE, EM.EACH_VELOCITY, EM.EACH_PAN, EM.EACH_ALL]
        each = [ctl_each(bits[k % 5], inc_scale=float(np.float32(2.0 ** ((k % 25 - 12) / 12.0))), amp_scale=0.25 + 0.001 * k,
                         velocity=0.3 + 0.0005 * k, pan_left=0.001 * (k % 1000), pan_right=0.9) for k in range(n_entries)]
        recs = [ctl(CM.AMP | CM.SMOOTHING, amp=0.5 + 0.005 * l, smoothing=0.3) for l in range(K)]
        # the records of the lanes outside filter_mask may name FILTER themselves: a set of their own
        own = [ctl(CM.AMP | CM.FILTER, amp=0.4, b0=0.4, b1=0.1, b2=0.05, a1=-0.2, a2=0.1) if not (sub >> l) & 1 else recs[l] for l in range(K)]
        dl = r.dev_list(entries)
        memory = {m: r.truth["voice_filter"][m].copy() for m in MEMORY}
        steps = [("records, entries, filter_mask == voice_mask", recs, each, full, full, None),
                 ("a strict subset", own if K > 1 else recs, each, part, sub, None),
                 ("coefficients only", None, None, part, sub, None),
                 ("a count word", recs, each, full, full, n_entries // 2 if n_entries > 2 else None)]
        for name, ctls, ee, vmask, fmask, count in steps:
            before = r.truth.copy()
            res = r.result(3)
            dc = torch.tensor([count, 99], dtype=torch.int32, device="cuda") if count is not None else None
            r.db.ctl_owned_each_filter(ctls, ee, filt, vmask, fmask, dl.data_ptr(), tags, K, dc.data_ptr() if dc is not None else 0, res.data_ptr())
            want, touched = TM.ctl_owned_each_filter(r.owner, (r.truth,), ctls, ee, filt, K, vmask, fmask, entries, tags, count)
            got = r.read(res, 3, name)
            print(f"{name}: d_result {got}, the model {want}")
            assert got == want, f"{name}: d_result {got}, the model says {want}"
            assert want[0] == (len(touched)) and (n_entries <= 2 or want[2] > 0)
            whole_bank_same(r, name)
            for m in MEMORY:
                assert r.truth["voice_filter"][m].tobytes() == memory[m].tobytes()
            if ctls is None and ee is None:
                # the five words and nothing else: on the voices of filter_mask of the written slots
                diff = CM.words_differ(r.truth, before)
                assert set(diff) <= {"voice_filter." + c for c in TM.COEFFS}, diff
                lanes_f = set(CM.lanes(fmask, K))
                assert all((v % K) in lanes_f for f in TM.COEFFS for v in np.flatnonzero(r.truth["voice_filter"][f] != before["voice_filter"][f]))
            single_calls(singles, dl, ctls, ee, filt, K, vmask, fmask, entries, tags, count)
            banks_same(r.db, singles, bank, f"{name}: the twin of single ctl_owned calls")
            if ee is not None:
                plain_each.ctl_owned_each(ctls, ee, vmask, dl.data_ptr(), tags, K, dc.data_ptr() if dc is not None else 0)
            if name.startswith("records"):
                banks_same(r.db, plain_each, bank, f"{name}: ctl_owned_each alone on a twin", but={"voice_filter." + c for c in TM.COEFFS})
        # by note id: the tags travel sorted, every set of coefficients stays with its tag; [37, 537) at K = 1
        first, count = (37, 500) if K == 1 else (K, (len(slots) - 1) * K)
        for name, ctls, ee, vmask, fmask in (("tags", recs, each, part, sub), ("tags, coefficients only", None, None, full, full)):
            res = r.result(3)
            r.db.ctl_tags_each_filter(ctls, ee, filt, first, count, vmask, fmask, tags, K, res.data_ptr())
            want, touched, lst = TM.ctl_tags_each_filter(r.owner, (r.truth,), ctls, ee, filt, first, count, K, vmask, fmask, tags)
            got = r.read(res, 3, name)
            print(f"{name}: d_result {got}, the model {want}, {int((lst >= 0).sum())} of {n_entries} tags found")
            assert got == want and want[2] == 0, f"{name}: d_result {got}, the model says {want}"
            assert all(first <= e < first + count for e in lst if e >= 0)
            whole_bank_same(r, name)
        r.block("a block after the calls")
        assert r.db.list_violations() == 0
    finally:
        r.close()
        singles.close()
        plain_each.close()


# ---------------------------------------------------------------------------------------------- 2. end to end

@pytest.mark.gpu
def test_a_chord_with_one_cutoff_per_note(dev):
    """3.sk over 64 copies (K = 4) with its three carriers filtered.  A three-note chord on channel 3 through note_on_channel; the
    oracle's bank receives what d_assigned says was placed (the placement itself is tests/test_chan.py's subject); then one cutoff per
    note by note id.  Two blocks of 64 frames: the taps of the chord's carriers (the stems the reference would store for them) and the
    state of every voice bit for bit against the oracle, the mix bit for bit against a bank that got the same coefficients through
    skred_bank_update; a third block with every voice's stem (taps and the full stem buffer exclude one another)."""
    import torch
    n, members = 256, (0, 1, 2)
    bank, tables, g, K = playing_patch("3sk", n, members)
    sel = np.isin(np.arange(n) % K, members)
    bank["voice_filter_mode"][sel] = 1
    base = device.filter_coeffs(1, 2000.0, 0.707, RATE)
    for c, v in zip(TM.COEFFS, base):
        bank["voice_filter"][c][sel] = v
    mmask = vmask = 0b0111
    r = Rig(dev, bank, tables, g)
    twin = open_bank(dev, bank, tables, g)
    try:
        for _ in range(4):
            r.block("before the chord", stems=True)
            twin.render_host(F, 2, 0)
        count = 3
        tags = np.array([3 << 24 | 60, 3 << 24 | 64, 3 << 24 | 67], np.uint32)
        notes = patch_notes(count, K, vmask, 1)
        iq = slot_query(0, n, K, mmask, FIN | ENV, 1e-3, 0, 0)
        sq = __import__("slot_steal_model").SlotQuery(0, n, K, mmask, OLDEST, RELEASED_FIRST)
        das = []
        for d in (r.db, twin):
            da = torch.full((count,), FILL, dtype=torch.int32, device="cuda")
            dr = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
            d.note_on_channel(notes, tags, iq, sq.c(), device.owner_match(3 << 24, 0xFF000000), 8, vmask, da.data_ptr(), dr.data_ptr())
            torch.cuda.synchronize()
            das.append(da.cpu().numpy())
            assert dr.cpu().numpy()[:2].tolist() == [count, 0]
        assigned = das[0]
        assert np.array_equal(das[0], das[1]) and (assigned >= 0).all() and len(set(assigned.tolist())) == count
        SM.store_notes((r.truth,), r.truth, notes, K, vmask, assigned, r.now())
        OM.tag_slots(r.owner, assigned, tags, None, K)
        whole_bank_same(r, "after the chord")
        filt = [filter_each(*device.filter_coeffs(1, f, 0.9, RATE)) for f in (400.0, 1600.0, 6400.0)]
        res = r.result(3)
        r.db.ctl_tags_each_filter(None, None, filt, 0, n, vmask, vmask, tags[::-1].copy(), K, res.data_ptr())     # (the tags descending: the sort has work to do)
        want, touched, lst = TM.ctl_tags_each_filter(r.owner, (r.truth,), None, None, filt, 0, n, K, vmask, vmask, tags[::-1].copy())
        assert r.read(res, 3, "one cutoff per note") == want == [count * 3, 0, 0] and np.array_equal(lst, assigned[::-1])
        for k, s in enumerate(assigned[::-1]):
            assert r.truth["voice_filter"]["b0"][s] == np.float32(filt[k].b0)
        whole_bank_same(r, "one cutoff per note")
        twin.update(r.truth, touched, DIRTY_PARAMS)                  # the host route: no owner call, no per-entry call
        carriers = np.array([s + l for s in assigned for l in members], np.int32)
        d_taps = torch.zeros((F, len(carriers), 2), dtype=torch.float32, device="cuda")
        r.db.set_taps(carriers, d_taps.data_ptr())
        for k in range(2):
            x, y = render_blocks(r.db, (F,))[0], render_blocks(twin, (F,))[0]
            ref = cpuref.render(r.truth, r.gl, r.tables, F, 0, want_stems=True)
            assert r.db.last_taps() == len(carriers)
            assert d_taps.cpu().numpy().tobytes() == np.ascontiguousarray(ref["stems"][:, carriers, :]).tobytes(), f"block {k}: taps differ from the oracle"
            assert x.tobytes() == y.tobytes(), f"block {k}: the mix differs from the host route's"
            assert np.abs(ref["stems"][:, carriers, :]).sum() > 0
            whole_bank_same(r, f"block {k}")
        r.db.set_taps([], 0)
        r.block("every stem of a third block", stems=True)
        # three notes, three timbres: the first carriers of the three slots hold three different sets of coefficients
        assert len({r.truth["voice_filter"]["a1"][s].tobytes() for s in assigned}) == 3
        assert r.db.list_violations() == 0
    finally:
        r.db.set_taps([], 0)
        r.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 3. the planner's shadow

@pytest.mark.gpu
def test_coefficients_alone_leave_the_planner_alone(dev):
    """tests/test_expr.py's in-place bank (two per lane, SKRED_OPT_IN_PLACE = 2, 2048 voices), with a chord sized so that the verdict
    CAN move.  With SKRED_OPT_IN_PLACE = 2 a block is rendered in place while the bound on its motion list -- the length the previous
    block reported plus the voices control calls touched since -- stays at or below n / 6 + 64 = 405 (skred_bank_plan.c).  The chord
    is 40 slots of 7 voices: 280 voices, listed from their trigger on and through attack and decay (some 50 blocks), so every block
    behind the trigger reports 280 and is in place.  A call that told the planner about its voices adds 40 * 7 = 280: 560, not in place.

    `plain` never hears of the filter calls; `control` makes the first of them with SKRED_EACH_VELOCITY beside the coefficients, a
    listing word.  FILTER is not a listing word, so the block behind the filter call must be chosen as plain's is -- the same kernel
    family, in place -- while control's block behind its call must NOT be in place: that is what shows the scene can see a filter call
    that grew the bound.  The second call (coefficients and a pan, block 4) is held to plain's verdict only, whatever that is.  The bank
    exports no list length; the verdict under this bound is its observable."""
    n, K, mask, CHORD = 2048, 8, 0xFE, 40
    assert CHORD * 7 <= n // 6 + 64 < 2 * CHORD * 7
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    r = Rig(dev, bank, tables, g, setup)
    plain, control = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    try:
        chord = np.arange(0, CHORD * 2 * K, 2 * K, dtype=np.int32)
        tags = (np.uint32(3 << 24) + np.arange(len(chord), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        dl = r.dev_list(chord)
        filt = [cutoff(k) for k in range(len(chord))]
        pans = [ctl_each(EM.EACH_PAN, pan_left=0.2, pan_right=0.7)] * len(chord)
        taken = []
        for k in range(6):
            if k == 1:
                for d in (r.db, plain, control):
                    d.stamp_slots(dl.data_ptr(), len(chord), K, mask, SM.STAMP_TRIGGER)
                SM.stamp(r.truth, SM.stamp_voices(chord, len(chord), None, K, mask, n), SM.STAMP_TRIGGER, r.now())
                r.tag(chord, tags, K, tag="the chord")
                control.tag_slots(dl.data_ptr(), tags, K)
            if k in (3, 4):
                res = r.result(3)
                if k == 3:
                    r.db.ctl_tags_each_filter(None, None, filt, 0, n, mask, 0x0E, tags, K, res.data_ptr())
                    want, _, _ = TM.ctl_tags_each_filter(r.owner, (r.truth,), None, None, filt, 0, n, K, mask, 0x0E, tags)
                    control.ctl_tags_each_filter(None, [ctl_each(EM.EACH_VELOCITY, velocity=0.5)] * len(chord), filt, 0, n, mask, 0x0E, tags, K)
                else:
                    r.db.ctl_owned_each_filter(None, pans, filt, mask, mask, dl.data_ptr(), tags, K, 0, res.data_ptr())
                    want, _ = TM.ctl_owned_each_filter(r.owner, (r.truth,), None, pans, filt, K, mask, mask, chord, tags, None)
                assert r.read(res, 3, f"block {k}") == want == [len(chord) * 7, 0, 0]
            for d in (r.db, plain, control):
                render_blocks(d, (F,))
            cpuref.render(r.truth, r.gl, r.tables, F, 0)
            taken.append((r.db.last_kernel(), plain.last_kernel(), control.last_kernel(), r.db.last_in_place(), plain.last_in_place(),
                          control.last_in_place()))
            assert r.db.last_kernel() == plain.last_kernel() and r.db.last_in_place() == plain.last_in_place(), (k, taken)
            a = bank.copy()
            r.db.download(a)
            assert not a.rw_equal(r.truth), (k, a.rw_equal(r.truth))
            assert r.db.list_violations() == plain.list_violations() == control.list_violations() == 0
        print(f"(kernel, plain's, control's, in place, plain's, control's) per block: {taken}")
        assert taken[2][3] and taken[3][3], f"the block behind the coefficients-only call was not in place: {taken}"
        assert taken[2][5] and not taken[3][5], f"the control's listing call did not move its verdict: the scene shows nothing: {taken}"
    finally:
        r.close()
        plain.close()
        control.close()


# ---------------------------------------------------------------------------------------------- 4. refusals

@pytest.mark.gpu
def test_refusals_write_nothing(dev):
    bank, tables, g, now = plain_bank(N)
    r = Rig(dev, bank, tables, g)
    try:
        r.tag([0, 8], [5, 6], 8, tag="two slots")
        dl, res = r.dev_list([0, 8]), r.result(3)
        good = [cutoff(0), cutoff(1)]
        inf = [cutoff(0), filter_each(0.1, float("inf"), 0.1, 0.1, 0.1)]
        resv = [cutoff(0), cutoff(1)]
        resv[1].reserved[2] = 1
        names = [ctl(CM.FILTER, b0=0.5)] * 8
        o = lambda **kw: r.db.ctl_owned_each_filter(kw.get("ctls"), None, kw.get("filt", good), kw.get("vm", 0xFF), kw.get("fm", 0xFF), dl.data_ptr(),   # noqa: E731
                                                    kw.get("tags", [5, 6]), 8, 0, res.data_ptr())
        t = lambda **kw: r.db.ctl_tags_each_filter(kw.get("ctls"), None, kw.get("filt", good), 0, kw.get("count", 600), kw.get("vm", 0xFF),   # noqa: E731
                                                   kw.get("fm", 0xFF), kw.get("tags", [5, 6]), 8, res.data_ptr())
        for call in (o, t):
            for kw in (dict(fm=0), dict(vm=0x0F, fm=0x1F), dict(filt=inf), dict(filt=resv), dict(ctls=names), dict(tags=[5, 0])):
                with pytest.raises(device.SkredAmdError):
                    call(**kw)
        with pytest.raises(device.SkredAmdError):
            t(tags=[5, 5])
        with pytest.raises(device.SkredAmdError):
            t(count=604)
        assert r.read(res, 3, "refusals") == [FILL & 0xFFFFFFFF] * 3
        whole_bank_same(r, "after the refusals")
        o()
        want, _ = TM.ctl_owned_each_filter(r.owner, (r.truth,), None, None, good, 8, 0xFF, 0xFF, [0, 8], [5, 6], None)
        assert r.read(res, 3, "the accepted call") == want == [16, 0, 0]
        whole_bank_same(r, "after the accepted call")
    finally:
        r.close()
