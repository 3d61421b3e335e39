"""Patch notes on the device (skred_bank_find_idle_slots / _notes_on_slots / _note_on_idle_slots / _stamp_slots).

Every comparison is byte for byte against tests/slot_model.py on the ORACLE's bank (cpuref.render of the same blocks, the notes and
stamps stored into it as the model states them).  DeviceBank.download returns the read-write fields only; the increments,
velocities and envelope clocks a note stores show in the state they produce a block later, so every placement is followed by a
block on both sides.  The scenes come from tests/slot_scenes.py; tests/test_slots_cpu.py asserts that none of them is vacuous.
Lists are pre-filled with -7: entries past `written` must keep it.
"""
import ctypes as C

import numpy as np
import pytest

import slot_model as M
import slot_scenes as S
from oracle import cpuref
from skred_amd import banks, device
from skred_amd.bank import slot_query
from test_idle import open_bank, render_blocks, traffic_bank

DIRTY_PARAMS, DIRTY_PHASE, DIRTY_PAN = 1, 2, 8
REL, TRIG = M.STAMP_RELEASE, M.STAMP_TRIGGER
BAD, RANGE = -2, -4
NAN = float("nan")
FILL = -7


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def reach(dev, n, K, mask, with_amp=True, setup=None):
    """(bank on the device after the scene's blocks, host bank, tables, a copy of the oracle's bank there, its globals)."""
    bank, tables, g, truth, gl = S.scene(n, K, mask, with_amp)
    db = open_bank(dev, bank, tables, g, setup)
    render_blocks(db, S.FRAMES)
    return db, bank, tables, truth.copy(), gl.copy()


def buffers(room, words=2):
    import torch
    return (torch.full((room + 8,), FILL, dtype=torch.int32, device="cuda"), torch.full((words,), FILL, dtype=torch.int32, device="cuda"))


def run_query(db, q):
    import torch
    dv, dc = buffers(q.max_out)
    torch.cuda.synchronize()
    db.find_idle_slots(q, dv.data_ptr(), dc.data_ptr())
    torch.cuda.synchronize()
    return dv.cpu().numpy(), dc.cpu().numpy()


def check_query(db, truth, first, count, K, mask, which, settle, start, max_out):
    want = M.idle_slots(truth, first, count, K, mask, which, settle, start)
    q = slot_query(first, count, K, mask, which, float(settle), start, max_out)
    dv, dc = run_query(db, q)
    total, written = len(want), min(len(want), max_out)
    tag = f"[{first},+{count}) K {K} mask 0x{mask:x} which 0x{which:x} from {start} max_out {max_out}"
    print(f"{tag}: total {total}, written {written}")
    assert (int(dc[0]), int(dc[1])) == (written, total), f"{tag}: d_count {dc.tolist()}, expected ({written}, {total})"
    assert np.array_equal(dv[:written], want[:written]), f"{tag}: got {dv[:written].tolist()}, expected {want[:written].tolist()}"
    assert (dv[written:] == FILL).all(), f"{tag}: entries past `written` were touched"
    dv2, dc2 = run_query(db, q)
    assert dv.tobytes() == dv2.tobytes() and dc.tobytes() == dc2.tobytes(), f"{tag}: two identical queries differ"
    return want


def slot_notes(n, K, voice_mask, seed, flags=M.SET_PHASE, junk=True):
    """n * K records: distinct finite values where voice_mask has a bit; elsewhere -- with `junk` -- records skred_notes_check would
    refuse (non-finite values, unknown flags, reserved words): the library must not look at them."""
    out = []
    for k in range(n):
        for l in range(K):
            if (voice_mask >> l) & 1 or not junk:
                f = flags if isinstance(flags, int) else flags[(k + l) % len(flags)]
                out.append(device.NoteC(np.float32(0.31 + 0.007 * k + 0.013 * l + 0.001 * seed), np.float32(0.2 + 0.01 * k + 0.02 * l),
                                        np.float32(0.25 * ((k + l) % 3)) if f & M.SET_PHASE else NAN,
                                        np.float32(0.1 + 0.01 * l) if f & M.SET_PAN else NAN,
                                        np.float32(0.9 - 0.01 * l) if f & M.SET_PAN else NAN, f))
            else:
                out.append(device.NoteC(NAN, float("inf"), NAN, NAN, NAN, 0xFFFF, (C.c_uint32 * 2)(7, 9)))
    return out


def state_is(db, truth, like, tag):
    a = like.copy()
    db.download(a)
    assert not a.rw_equal(truth), f"{tag}: state differs from the oracle: {a.rw_equal(truth)}"
    return a


def block(db, truth, gl, tables, frames, like, tag):
    """One block on the device and on the oracle; the states must agree afterwards."""
    render_blocks(db, (frames,))
    cpuref.render(truth, gl, tables, frames, 0)
    return state_is(db, truth, like, tag)


# ---------------------------------------------------------------------------------------------- 1. the query

@pytest.mark.gpu
@pytest.mark.parametrize("n,K,name", S.QUERY_CASES + [S.BIG_CASE])
def test_queries(dev, n, K, name):
    mask = S.masks(K)[name]
    db, bank, tables, truth, gl = reach(dev, n, K, mask)
    try:
        state_is(db, truth, bank, "after the scene's blocks")
        args = (0, n, K, mask, S.WHICH_ALL, S.SETTLE)
        lst = check_query(db, truth, *args, None, n // K)
        total = len(lst)
        assert 0 < total < n // K
        starts = [0, int(lst[total // 2]), ((n // K) // 2) * K, n - K]          # the first slot, a listed one, a middle one, the last (the wrap)
        if n > 256:
            starts.append(256 + (40 // K) * K)                                   # inside the second workgroup
        for start in starts:
            check_query(db, truth, *args, start, n // K)
        for mo in (0, 1, max(total - 1, 1), total, total + 5):
            check_query(db, truth, *args, starts[1], mo)
        check_query(db, truth, *args, n - K, max(total - 1, 1))
        if K > 1:                                                                # other criteria, the level of ENV_DONE
            check_query(db, truth, 0, n, K, mask, M.ENV, 0.0, None, n // K)
            check_query(db, truth, 0, n, K, mask, M.FIN | M.AMP, 0.0, starts[2], n // K)
        voices, tot = db.find_idle_slots_host(slot_query(*args, starts[2], 3))   # the host form waits for the stream only
        want = M.idle_slots(truth, *args, starts[2])
        assert tot == len(want) and np.array_equal(voices, want[:3])
        voices, tot = db.find_idle_slots_host(slot_query(*args, None, 0))
        assert tot == len(want) and len(voices) == 0
    finally:
        db.close()


@pytest.mark.gpu
def test_a_range_off_the_64_boundaries(dev):
    K, mask = 8, 0x55
    db, bank, tables, truth, gl = reach(dev, 320, K, mask)
    try:
        for start in (24, 160, 312):
            for mo in (37, 2):
                check_query(db, truth, 24, 296, K, mask, S.WHICH_ALL, S.SETTLE, start, mo)
        check_query(db, truth, 312, 8, K, mask, S.WHICH_ALL, S.SETTLE, 312, 4)   # one slot
    finally:
        db.close()


@pytest.mark.gpu
def test_no_slot_idle_and_all_slots_idle(dev):
    n, K = 320, 8
    bank, tables, g = banks.bank_c2(n)                    # every voice sounds
    rest = bank.copy()
    rest["voice_amp_envelope"]["is_active"][:] = 0        # every envelope at rest, gain exactly 0
    for b, total in ((bank, 0), (rest, n // K)):
        db = open_bank(dev, b, tables, g)
        try:
            for mask in (0xFF, 0x01, 0x80, 0x55):
                want = check_query(db, b, 0, n, K, mask, S.WHICH_ALL, 0.0, 160, n // K)
                assert len(want) == total
                check_query(db, b, 24, 296, K, mask, S.WHICH_NOTES, 0.0, 312, 5)
        finally:
            db.close()


# ---------------------------------------------------------------------------------------------- 2. K = 1: the per-voice calls

@pytest.mark.gpu
def test_one_voice_slots_are_the_voice_calls(dev):
    """find_idle_slots / notes_on_slots / stamp_slots with K = 1, mask 1 against find_idle / notes_on_list / stamp_list on a twin
    bank: lists, counts, d_assigned, result words and the downloaded state, byte for byte, and the next block's mix."""
    import torch
    n, F = 1088, 128
    bank, tables, g, truth0, gl0 = S.scene(n, 1, 1, False)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    truth, gl = truth0.copy(), gl0.copy()
    try:
        render_blocks(db, S.FRAMES); render_blocks(twin, S.FRAMES)
        for first, count, start, mo in ((0, n, None, n), (0, n, 700, 20), (5, 1000, 1004, 0), (5, 1000, 300, 1000)):
            sv, sc = buffers(mo)
            vv, vc = buffers(mo)
            torch.cuda.synchronize()
            db.find_idle_slots(slot_query(first, count, 1, 1, S.WHICH_NOTES, float(S.SETTLE), start, mo), sv.data_ptr(), sc.data_ptr())
            twin.find_idle(first, count, S.WHICH_NOTES, float(S.SETTLE), start, mo, vv.data_ptr(), vc.data_ptr())
            torch.cuda.synchronize()
            assert sv.cpu().numpy().tobytes() == vv.cpu().numpy().tobytes() and sc.cpu().numpy().tobytes() == vc.cpu().numpy().tobytes()
        lst = M.idle_slots(truth, 0, n, 1, 1, S.WHICH_NOTES, S.SETTLE, 700)
        listed = 20
        assert len(lst) > listed
        sv, sc = buffers(listed)
        vv, vc = buffers(listed)
        torch.cuda.synchronize()
        db.find_idle_slots(slot_query(0, n, 1, 1, S.WHICH_NOTES, float(S.SETTLE), 700, listed), sv.data_ptr(), sc.data_ptr())
        twin.find_idle(0, n, S.WHICH_NOTES, float(S.SETTLE), 700, listed, vv.data_ptr(), vc.data_ptr())
        for count, first_entry in ((12, 0), (12, 12), (300, 3)):                 # placed, partly dropped, more than one workgroup
            notes = slot_notes(count, 1, 1, count, [M.SET_PHASE, M.SET_PAN, 0, M.SET_PHASE | M.SET_PAN])
            sa, sr = buffers(count)
            va, vr = buffers(count)
            torch.cuda.synchronize()
            db.notes_on_slots(notes, 1, 1, sv.data_ptr(), sc.data_ptr(), first_entry, sa.data_ptr(), sr.data_ptr())
            twin.notes_on_list(notes, vv.data_ptr(), vc.data_ptr(), first_entry, va.data_ptr(), vr.data_ptr())
            torch.cuda.synchronize()
            assert sa.cpu().numpy().tobytes() == va.cpu().numpy().tobytes(), (count, first_entry)
            assert sr.cpu().numpy().tobytes() == vr.cpu().numpy().tobytes(), (count, first_entry)
            got = sa.cpu().numpy()[:count]
            assert np.array_equal(got, M.place(count, 1, lst, listed, first_entry, n))
            M.store_notes((truth,), truth, notes, 1, 1, got, gl.synth_sample_count)
            a, b = state_is(db, truth, bank, "notes"), bank.copy()
            twin.download(b)
            assert not a.rw_equal(b), a.rw_equal(b)
        x, y = render_blocks(db, (F,))[0], render_blocks(twin, (F,))[0]
        assert x.tobytes() == y.tobytes()
        cpuref.render(truth, gl, tables, F, 0)
        state_is(db, truth, bank, "a block after the notes")
        # stamps: the list with holes, with the count and without it
        holes = np.array([-1, int(lst[0]), n, int(lst[1]), 2**31 - 1, int(lst[2]), 8, 16], np.int32)
        dh = torch.from_numpy(holes).cuda()
        cnt = torch.tensor([6, 0], dtype=torch.int32, device="cuda")
        for stamps, dc, m in ((REL, cnt, 6), (TRIG | REL, None, None)):
            db.stamp_slots(dh.data_ptr(), len(holes), 1, 1, stamps, dc.data_ptr() if dc is not None else 0)
            twin.stamp_list(dh.data_ptr(), len(holes), stamps, dc.data_ptr() if dc is not None else 0)
            M.stamp(truth, M.stamp_voices(holes, len(holes), m, 1, 1, n), stamps, gl.synth_sample_count)
        x, y = render_blocks(db, (F,))[0], render_blocks(twin, (F,))[0]
        assert x.tobytes() == y.tobytes()
        cpuref.render(truth, gl, tables, F, 0)
        a, b = state_is(db, truth, bank, "a block after the stamps"), bank.copy()
        twin.download(b)
        assert not a.rw_equal(b), a.rw_equal(b)
        assert db.last_kernel() == twin.last_kernel()
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 3. notes

@pytest.mark.gpu
@pytest.mark.parametrize("n,K,name,vname,counts", [(1088, 2, "low", "all", (5, None, "+", 300)), (1088, 2, "all", "high", (300, "+")),
                                                    (4160, 64, "alt", "alt", (2, None, "+", 40)), (320, 8, "alt", "all", (1, None, "+"))])
def test_notes_below_at_and_above_the_listed_count(dev, n, K, name, vname, counts):
    """note_on_idle_slots with fewer notes than idle slots, as many ("None"), and more ("+"); 300 notes at K = 2 and 40 at K = 64 are
    more than one workgroup of the notes kernel.  Dropped notes are -1 in d_assigned, d_result sums to the batch, the stores are the
    model's."""
    import torch
    mask, vmask = S.masks(K)[name], S.masks(K)[vname]
    db, bank, tables, truth, gl = reach(dev, n, K, mask, False)
    try:
        start = ((n // K) // 3) * K
        for i, count in enumerate(counts):
            lst = M.idle_slots(truth, 0, n, K, mask, S.WHICH_NOTES, S.SETTLE, start)
            assert len(lst) > 2, "the scene ran out of idle slots"
            count = len(lst) if count is None else len(lst) + 7 if count == "+" else count     # as many as listed, more, or a fixed batch
            notes = slot_notes(count, K, vmask, i, [M.SET_PHASE, M.SET_PHASE | M.SET_PAN])
            assert device.slot_notes_check(notes, K, vmask) == 0
            da, dr = buffers(count)
            torch.cuda.synchronize()
            db.note_on_idle_slots(notes, slot_query(0, n, K, mask, S.WHICH_NOTES, float(S.SETTLE), start, -5), vmask, da.data_ptr(), dr.data_ptr())
            torch.cuda.synchronize()
            got, res = da.cpu().numpy(), dr.cpu().numpy()
            want = M.place(count, K, lst, min(len(lst), count), 0, n)
            placed = int((want >= 0).sum())
            print(f"n {n} K {K}: {count} notes on {len(lst)} idle slots -> placed {placed}")
            assert np.array_equal(got[:count], want) and (got[count:] == FILL).all(), (got.tolist(), want.tolist())
            assert res.tolist() == [placed, count - placed] and placed == min(count, len(lst))
            M.store_notes((truth,), truth, notes, K, vmask, want, gl.synth_sample_count)
            state_is(db, truth, bank, f"the stores of batch {i}")
            block(db, truth, gl, tables, 64, bank, f"a block after batch {i}")
            # the slots that took a note sound now: the next query does not list them (where a member received one)
            if vmask & mask:
                again = M.idle_slots(truth, 0, n, K, mask, S.WHICH_NOTES, S.SETTLE, start)
                assert not set(again) & set(want[want >= 0])
            # make room for the next batch: release what was placed and let it end
            dl = torch.from_numpy(want).cuda()
            db.stamp_slots(dl.data_ptr(), count, K, vmask, REL)
            M.stamp(truth, M.stamp_voices(want, count, None, K, vmask, n), REL, gl.synth_sample_count)
            block(db, truth, gl, tables, 512, bank, f"the release after batch {i}")
    finally:
        db.close()


@pytest.mark.gpu
def test_cursor_shares_one_query(dev):
    import torch
    n, K, mask, vmask = 1088, 2, 1, 3
    db, bank, tables, truth, gl = reach(dev, n, K, mask, False)
    try:
        lst = M.idle_slots(truth, 0, n, K, mask, S.WHICH_NOTES, S.SETTLE, 512)[:20]
        assert len(lst) == 20
        dv, dc = buffers(20)
        outs = [buffers(8) for _ in range(3)]
        batches = [slot_notes(8, K, vmask, 20 + i) for i in range(3)]
        torch.cuda.synchronize()
        db.find_idle_slots(slot_query(0, n, K, mask, S.WHICH_NOTES, float(S.SETTLE), 512, 20), dv.data_ptr(), dc.data_ptr())
        for i in range(3):
            db.notes_on_slots(batches[i], K, vmask, dv.data_ptr(), dc.data_ptr(), 8 * i, outs[i][0].data_ptr(), outs[i][1].data_ptr())
        torch.cuda.synchronize()
        got = [o[0].cpu().numpy()[:8] for o in outs]
        for i in range(3):
            want = M.place(8, K, lst, 20, 8 * i, n)
            assert np.array_equal(got[i], want), (i, got[i], want)
            M.store_notes((truth,), truth, batches[i], K, vmask, want, gl.synth_sample_count)
        assert [o[1].cpu().numpy().tolist() for o in outs] == [[8, 0], [8, 0], [4, 4]]
        block(db, truth, gl, tables, 128, bank, "after three batches on one query")
    finally:
        db.close()


@pytest.mark.gpu
def test_entries_that_are_no_slot_and_unmasked_voices(dev):
    """A hand-made list: negative, misaligned and past-the-bank entries are dropped whole and their neighbourhood keeps every word;
    voices without a bit in voice_mask keep every word although their records are not even finite; SET_PHASE clears voice_finished
    on masked voices only."""
    import torch
    n, K, mask = 320, 8, 0x55
    vmask = 0x55
    db, bank, tables, truth, gl = reach(dev, n, K, mask, False)
    try:
        fin = truth["voice_finished"].reshape(-1, K) != 0
        both = [s * K for s in range(n // K) if fin[s][[0, 2, 4, 6]].any() and fin[s][[1, 3, 5, 7]].any()]
        assert len(both) >= 2, "no slot holds a finished voice at a masked and at an unmasked position"
        entries = np.array([both[0], -8, 12, 100, n, n - 4, both[1], 2**31 - 8, -2**31, 312, 16], np.int32)
        count = len(entries) - 1                                                   # the last entry lies past the count
        notes = slot_notes(len(entries), K, vmask, 3, M.SET_PHASE | M.SET_PAN)
        assert device.slot_notes_check(notes, K, vmask) == 0 and device.notes_check(notes) == BAD
        dv, dc = torch.from_numpy(entries).cuda(), torch.tensor([count, 99], dtype=torch.int32, device="cuda")
        da, dr = buffers(len(entries))
        torch.cuda.synchronize()
        db.notes_on_slots(notes, K, vmask, dv.data_ptr(), dc.data_ptr(), 0, da.data_ptr(), dr.data_ptr())
        torch.cuda.synchronize()
        want = M.place(len(entries), K, entries, count, 0, n)
        assert want.tolist() == [both[0], -1, -1, -1, -1, -1, both[1], -1, -1, 312, -1]
        assert np.array_equal(da.cpu().numpy()[:len(entries)], want) and dr.cpu().numpy().tolist() == [3, len(entries) - 3]
        fin0 = truth["voice_finished"].copy()
        touched = M.store_notes((truth,), truth, notes, K, vmask, want, gl.synth_sample_count)
        a = state_is(db, truth, bank, "the stores")
        assert len(touched) == 12 and (a["voice_finished"][touched] == 0).all() and (fin0[touched] != 0).any()
        others = np.setdiff1d(np.arange(n), touched)
        assert (a["voice_finished"][others] == fin0[others]).all() and (fin0[[both[0] + l for l in (1, 3, 5, 7)]] != 0).any()
        block(db, truth, gl, tables, 128, bank, "a block later")
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 4. stamps

@pytest.mark.gpu
def test_stamps_through_an_earlier_assignment(dev):
    """A chord larger than the idle list leaves -1 holes in d_assigned; handed back as the note-off list it releases the placed
    slots -- with the count and without --, and a release on slots whose envelopes are not active changes nothing."""
    import torch
    n, K, mask, vmask = 320, 8, 0x80, 0xF0
    db, bank, tables, truth, gl = reach(dev, n, K, mask, False)
    try:
        lst = M.idle_slots(truth, 0, n, K, mask, S.WHICH_NOTES, S.SETTLE)
        count = len(lst) + 3
        notes = slot_notes(count, K, vmask, 9)
        da, dr = buffers(count)
        torch.cuda.synchronize()
        db.note_on_idle_slots(notes, slot_query(0, n, K, mask, S.WHICH_NOTES, float(S.SETTLE), None, 0), vmask, da.data_ptr(), dr.data_ptr())
        want = M.place(count, K, lst, len(lst), 0, n)
        M.store_notes((truth,), truth, notes, K, vmask, want, gl.synth_sample_count)
        block(db, truth, gl, tables, 192, bank, "the chord")                      # attack and decay are over: a release counts
        assert np.array_equal(da.cpu().numpy()[:count], want) and (want[-3:] == -1).all()
        # the first half through a count, then everything without one (stamping a released voice again moves its release)
        half = torch.tensor([count // 2, 0], dtype=torch.int32, device="cuda")
        db.stamp_slots(da.data_ptr(), count, K, vmask, REL, half.data_ptr())
        M.stamp(truth, M.stamp_voices(want, count, count // 2, K, vmask, n), REL, gl.synth_sample_count)
        block(db, truth, gl, tables, 64, bank, "half released")
        db.stamp_slots(da.data_ptr(), count, K, vmask, REL)
        M.stamp(truth, M.stamp_voices(want, count, None, K, vmask, n), REL, gl.synth_sample_count)
        # slots whose masked envelopes are at rest: the release must not count there
        quiet = M.idle_slots(truth, 0, n, K, vmask, M.ENV, 1.0)
        assert len(quiet) > 0
        dq = torch.from_numpy(quiet).cuda()
        db.stamp_slots(dq.data_ptr(), len(quiet), K, vmask, REL)
        M.stamp(truth, M.stamp_voices(quiet, len(quiet), None, K, vmask, n), REL, gl.synth_sample_count)
        block(db, truth, gl, tables, 256, bank, "all released")
        e = truth["voice_amp_envelope"]
        placed = M.stamp_voices(want, count, None, K, vmask, n)
        # (the scene leaves some voices a release that never ends, and some no envelope at all: nothing ever clears their is_active)
        short = placed[(e["release_time"][placed] <= 200.0) & (truth["voice_use_amp_envelope"][placed] != 0)]
        assert len(short) > 0 and (e["is_active"][short] == 0).all()               # the chord has ended
        block(db, truth, gl, tables, 64, bank, "at rest")
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 5. a tiled patch, end to end

def enveloped_patch(patch, n, members):
    """bank_patch with envelopes on the `members` of every copy, every one of them released long ago; fast smoothers there."""
    bank, tables, g = banks.bank_patch(patch, n)
    K = {"3sk": 4, "18sk": 16}[patch]
    now = int(g.synth_sample_count)
    sel = np.isin(np.arange(n) % K, members)
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel] = np.float32(20.0), np.float32(50.0)
    e["sustain_level"][sel], e["release_time"][sel] = np.float32(0.6), np.float32(100.0)
    e["velocity"][sel] = np.float32(1.0)
    e["is_active"][sel] = 1
    e["sample_start"][sel] = np.uint64(now - 40000)
    e["sample_release"][sel] = np.uint64(now - 50)
    bank["voice_smoother_smoothing"][sel] = np.float32(0.5)
    return bank, tables, g, K


@pytest.mark.gpu
@pytest.mark.parametrize("patch,members,voices,kernel", [("3sk", (0, 1, 2), (0, 1, 2, 3), None), ("18sk", (0, 10), (0, 1, 2, 10), 2)])
def test_a_tiled_patch_end_to_end(dev, patch, members, voices, kernel):
    """Everything released and rendered to rest; a chord through note_on_idle_slots; three blocks; the note-off through d_assigned;
    two blocks.  State and per-voice stems are those of the host route (find_idle_slots_host + skred_bank_update on a twin) and of
    the oracle, and both routes run the same kernels in every block."""
    import torch
    n, F, chord = 512, 64, 5
    bank, tables, g, K = enveloped_patch(patch, n, members)
    mmask, vmask = sum(1 << l for l in members), sum(1 << l for l in voices)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    truth, gl, mirror = bank.copy(), g.copy(), bank.copy()

    def blocks(count, tag):
        for i in range(count):
            x, xs = db.render_host(F, 2, 0, want_stems=True)
            y, ys = twin.render_host(F, 2, 0, want_stems=True)
            ref = cpuref.render(truth, gl, tables, F, 0, want_stems=True)
            assert xs.tobytes() == ys.tobytes() and x.tobytes() == y.tobytes(), f"{tag} {i}: the two routes differ"
            assert xs.tobytes() == ref["stems"].tobytes(), f"{tag} {i}: stems differ from the oracle"
            a, b = state_is(db, truth, bank, f"{tag} {i}"), bank.copy()
            twin.download(b)
            assert not a.rw_equal(b), a.rw_equal(b)
            assert db.last_kernel() == twin.last_kernel() and db.last_pack() == twin.last_pack(), (tag, i, db.last_kernel(), twin.last_kernel())
            if kernel is not None:
                assert db.last_kernel() == kernel, (tag, i, db.last_kernel())

    try:
        blocks(4, "to rest")
        q = slot_query(0, n, K, mmask, S.WHICH_NOTES, float(S.SETTLE), (n // K // 2) * K, chord)
        want = M.idle_slots(truth, 0, n, K, mmask, S.WHICH_NOTES, S.SETTLE, q.start)
        assert len(want) == n // K, "the bank did not come to rest"
        notes = slot_notes(chord, K, vmask, 4)
        da, dr = buffers(chord)
        torch.cuda.synchronize()
        db.note_on_idle_slots(notes, q, vmask, da.data_ptr(), dr.data_ptr())
        picks, total = twin.find_idle_slots_host(q)
        assert total == n // K and np.array_equal(picks, want[:chord])
        now = gl.synth_sample_count
        touched = M.store_notes((truth, mirror), truth, notes, K, vmask, picks, now)
        twin.update(mirror, touched, DIRTY_PARAMS | DIRTY_PHASE | TRIG)
        blocks(3, "the chord")
        assert np.array_equal(da.cpu().numpy()[:chord], picks) and dr.cpu().numpy().tolist() == [chord, 0]
        assert (truth["voice_amp_envelope"]["is_active"][picks] == 1).all()
        db.stamp_slots(da.data_ptr(), chord, K, vmask, REL)
        twin.update(mirror, touched, REL)
        M.stamp(truth, touched, REL, gl.synth_sample_count)
        blocks(2, "the release")
        assert (truth["voice_amp_envelope"]["is_active"][picks] == 0).all()
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 6. the in-place rule

@pytest.mark.gpu
def test_two_per_lane_in_place_after_a_slot_chord(dev):
    """What a slot call owes the planner.  A two-per-lane bank of 4096 voices with SKRED_OPT_IN_PLACE = 2 renders its motion list in
    place while the PROVEN bound on the list's length -- the length a launch reported plus the voices touched since -- stays at or
    below 4096 / 6 + 64 = 746 (skred_bank_plan.c: plan_inplace).  Slots of 8 voices, voice_mask 0xFE: a note touches 7 voices.

      a chord of 2 notes     14 voices: the block is rendered in place;
      a chord of 110 notes   770 voices, more than 746: the block must leave the in-place path.  110 itself is far below 746: a
                             library that counted notes instead of voices would stay in place, with more listed voices than rows;
      a chord of 2 notes     in place again (the bound has come down: the big chord's voices reached their sustain);
      the big chord's note-off through skred_bank_stamp_slots, 110 entries: 770 voices again, not in place.

    In every block last_in_place(), the kernel, the mix and the state are those of the host route (skred_bank_update names every
    voice), and the state is the oracle's."""
    import torch
    n, K, F, BIG, SMALL = 4096, 8, 256, 110, 2
    mmask = vmask = 0xFE                                        # voice 0 of every slot sounds on (traffic_bank: every eighth voice)
    per_note = bin(vmask).count("1")
    limit = n // 6 + 64
    assert BIG <= limit < BIG * per_note and SMALL * per_note <= limit
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    db, twin = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    truth, gl, mirror = bank.copy(), g.copy(), bank.copy()
    chords = {3: (SMALL, 0, True), 6: (BIG, 1024, False), 9: (SMALL, 3072, True)}      # block: notes, `from`, in place?
    release_at, expect_release = 11, False
    taken, kept = [], {}
    try:
        for k in range(13):
            tag = f"block {k}"
            expect = None
            if k in chords:
                count, start, expect = chords[k]
                q = slot_query(0, n, K, mmask, S.WHICH_NOTES, float(S.SETTLE), start, count)
                want = M.idle_slots(truth, 0, n, K, mmask, S.WHICH_NOTES, S.SETTLE, start)[:count]
                assert len(want) == count, tag
                notes = slot_notes(count, K, vmask, k)
                da, dr = buffers(count)
                torch.cuda.synchronize()
                db.note_on_idle_slots(notes, q, vmask, da.data_ptr(), dr.data_ptr())
                picks, _ = twin.find_idle_slots_host(q)
                assert np.array_equal(picks, want), tag
                touched = M.store_notes((truth, mirror), truth, notes, K, vmask, picks, gl.synth_sample_count)
                assert len(touched) == count * per_note
                twin.update(mirror, touched, DIRTY_PARAMS | DIRTY_PHASE | TRIG)
                kept[k] = (da, dr, picks, touched)
            if k == release_at:
                da, dr, picks, touched = kept[6]
                expect = expect_release
                db.stamp_slots(da.data_ptr(), BIG, K, vmask, REL)
                twin.update(mirror, touched, REL)
                M.stamp(truth, touched, REL, gl.synth_sample_count)
            x, y = render_blocks(db, (F,))[0], render_blocks(twin, (F,))[0]
            cpuref.render(truth, gl, tables, F, 0)
            taken.append((db.last_in_place(), twin.last_in_place()))
            print(tag, "in place (device route, host route):", taken[-1])
            assert db.last_kernel() == twin.last_kernel() == 3, (tag, db.last_kernel(), twin.last_kernel())
            assert taken[-1][0] == taken[-1][1], f"{tag}: in place on one route only: {taken}"
            if expect is not None:
                assert taken[-1][0] is expect, f"{tag}: in place {taken[-1][0]}, expected {expect}: {taken}"
            assert x.tobytes() == y.tobytes(), f"{tag}: the mixes differ"
            state_is(db, truth, bank, tag)
            assert db.list_violations() == twin.list_violations() == 0, tag
            if k in kept and k == max(kept):
                da, dr, picks, _ = kept[k]
                assert np.array_equal(da.cpu().numpy()[:len(picks)], picks) and dr.cpu().numpy().tolist() == [len(picks), 0], tag
        assert {t[0] for t in taken} == {True, False}, taken     # both ways of rendering the list ran
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 7. refusals

@pytest.mark.gpu
def test_refusals_write_nothing(dev):
    import torch
    n, K, mask = 320, 8, 0x55
    db, bank, tables, truth, gl = reach(dev, n, K, mask, False)
    try:
        L = db.L
        count = 4
        notes = device.note_array(slot_notes(count, K, mask, 1, junk=False))
        p = C.cast(notes, C.c_void_p)
        dv = torch.tensor([8, 16, 24, 32], dtype=torch.int32, device="cuda")
        dc = torch.tensor([4, 4], dtype=torch.int32, device="cuda")
        da, dr = buffers(count)
        sv, sc = buffers(n // K)
        torch.cuda.synchronize()

        def find(h=db.h, sl=sv.data_ptr(), cn=sc.data_ptr(), **kw):
            args = dict(first=0, count=n, slot_voices=K, member_mask=mask, which=S.WHICH_NOTES, settle_level=0.0, start=None, max_out=n // K)
            args.update(kw)
            q = slot_query(**args)
            return L.skred_bank_find_idle_slots(h, C.byref(q), sl or None, cn or None, None)

        def on_slots(h=db.h, nt=p, cnt=count, k=K, vm=mask, sl=dv.data_ptr(), cn=dc.data_ptr(), first=0, res=dr.data_ptr()):
            return L.skred_bank_notes_on_slots(h, nt, cnt, k, vm, sl or None, cn or None, first, da.data_ptr(), res or None, None)

        def on_idle(h=db.h, nt=p, cnt=count, vm=mask, res=dr.data_ptr(), **kw):
            args = dict(first=0, count=n, slot_voices=K, member_mask=mask, which=S.WHICH_NOTES, settle_level=0.0, start=None, max_out=-5)
            args.update(kw)
            q = slot_query(**args)
            return L.skred_bank_note_on_idle_slots(h, C.byref(q), nt, cnt, vm, da.data_ptr(), res or None, None)

        def stamp(h=db.h, sl=dv.data_ptr(), cnt=count, k=K, vm=mask, st=REL):
            return L.skred_bank_stamp_slots(h, sl or None, cnt, None, k, vm, st, None)

        assert find(h=None) == BAD and find(cn=0) == BAD and find(sl=0) == BAD and find(max_out=-1) == BAD
        assert find(which=0) == BAD and find(which=M.ENV | M.UNNAMED) == BAD and find(member_mask=0) == BAD and find(member_mask=0x100) == BAD
        assert find(settle_level=-1.0) == BAD
        assert find(slot_voices=3) == RANGE and find(first=4) == RANGE and find(count=n + 8) == RANGE and find(start=12) == RANGE
        assert find(count=316) == RANGE and find(start=n) == RANGE
        assert on_slots(h=None) == BAD and on_slots(nt=None) == BAD and on_slots(sl=0) == BAD and on_slots(cn=0) == BAD
        assert on_slots(res=0) == BAD and on_slots(cnt=-1) == BAD and on_slots(first=-1) == BAD
        assert on_slots(k=5) == RANGE and on_slots(vm=0) == BAD and on_slots(vm=0x1FF) == BAD
        bad = slot_notes(count, K, mask, 1, junk=False)
        bad[K + 2] = device.NoteC(NAN, 1.0, 0.0, 0.5, 0.5, 0)                      # a masked position (bit 2)
        bp = C.cast(device.note_array(bad), C.c_void_p)
        assert on_slots(nt=bp) == BAD and on_idle(nt=bp) == BAD
        assert on_idle(h=None) == BAD and on_idle(nt=None) == BAD and on_idle(res=0) == BAD and on_idle(cnt=-1) == BAD
        assert on_idle(which=S.WHICH_ALL) == BAD and on_idle(which=M.AMP) == BAD and on_idle(vm=0) == BAD
        assert on_idle(first=4) == RANGE and on_idle(slot_voices=128) == RANGE
        assert stamp(h=None) == BAD and stamp(sl=0) == BAD and stamp(cnt=-1) == BAD and stamp(st=0) == BAD and stamp(st=REL | 1) == BAD
        assert stamp(k=12) == RANGE and stamp(vm=0) == BAD and stamp(vm=0x100) == BAD
        assert on_slots(cnt=0) == 0 and on_idle(cnt=0) == 0 and stamp(cnt=0) == 0
        torch.cuda.synchronize()
        for t in (da, dr, sv, sc):
            assert (t.cpu().numpy() == FILL).all()                                 # nothing reached the device
        state_is(db, truth, bank, "after the refusals")
        check_query(db, truth, 0, n, K, mask, S.WHICH_NOTES, S.SETTLE, None, n // K)   # ... and the bank still answers
        block(db, truth, gl, tables, 64, bank, "a block after the refusals")
    finally:
        db.close()
