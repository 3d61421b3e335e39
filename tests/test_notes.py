"""Device-side note-ons (skred_bank_notes_on_list / _note_on_idle / _stamp_list): notes placed on a voice list the device holds.

Every comparison is bit for bit.  The truth is the ORACLE's bank (cpuref.render of the same blocks, with the note-ons and releases
stored into it the way the reference's `l` command stores them); beside it runs a TWIN bank that takes the host path the calls
replace -- find_idle_host, the host view, skred_bank_update -- and must end every block with the same mix, the same state and the
same kernel choice.  DeviceBank.download returns the read-write fields only; the increment, the velocity and the envelope clock a
note stores show in the state they produce a block later (the running phase, the amp smoother's gain, is_active).
Banks, the idle-list truth and the trigger / release stores on the oracle's side come from tests/test_idle.py.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import cpuref
from skred_amd import device
from test_idle import (DIRTY_PARAMS, DIRTY_PHASE, ENV, FIN, AMP, SETTLE, STAMP_RELEASE, STAMP_TRIGGER, do_release, expected,
                       open_bank, render_blocks, traffic_bank)

DIRTY_PAN = 8
SET_PHASE, SET_PAN = device.NOTE_SET_PHASE, device.NOTE_SET_PAN
BAD = -2
WHICH = FIN | ENV
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def make_notes(K, seed, flags=SET_PHASE):
    """K notes with distinct pitches and velocities; `flags`: one value or one per note.  The fields a note does not set hold NaN:
    the library must not look at them."""
    flags = [flags] * K if isinstance(flags, int) else list(flags)
    out = []
    for k in range(K):
        f = flags[k]
        out.append(device.NoteC(np.float32(0.37 + 0.011 * k + 0.003 * seed), np.float32(0.25 + 0.04 * k + 0.001 * seed),
                                np.float32(0.25 * (k % 3)) if f & SET_PHASE else NAN,
                                np.float32(0.1 + 0.01 * k) if f & SET_PAN else NAN,
                                np.float32(0.9 - 0.02 * k) if f & SET_PAN else NAN, f))
    return out


def store_notes(hosts, truth, notes, voices, now):
    """What the placement stores, on host views: `hosts` get the values (a twin's update carries them), `truth` the stamp too."""
    for t, v in zip(notes, voices):
        if v < 0:
            continue
        for h in hosts:
            h["voice_phase_inc"][v] = t.phase_inc
            h["voice_amp_envelope"]["velocity"][v] = t.velocity
            if t.flags & SET_PHASE:
                h["voice_phase"][v] = t.phase
                h["voice_finished"][v] = 0
            if t.flags & SET_PAN:
                h["voice_pan_left"][v] = t.pan_left
                h["voice_pan_right"][v] = t.pan_right
        e = truth["voice_amp_envelope"]
        e["sample_start"][v] = now
        e["sample_release"][v] = 0
        e["is_active"][v] = 1


def outputs(K, fill=-7):
    import torch
    return (torch.full((K + 8,), fill, dtype=torch.int32, device="cuda"), torch.full((2,), fill, dtype=torch.int32, device="cuda"))


def same_state(db, twin, truth, like, tag):
    a, b = like.copy(), like.copy()
    db.download(a)
    twin.download(b)
    assert not a.rw_equal(b), f"{tag}: device-side path and host path differ: {a.rw_equal(b)}"
    assert not a.rw_equal(truth), f"{tag}: state differs from the oracle: {a.rw_equal(truth)}"


def same_mix(db, twin, frames, tag):
    x, y = render_blocks(db, (frames,))[0], render_blocks(twin, (frames,))[0]
    assert (x.view(np.uint32) == y.view(np.uint32)).all(), f"{tag}: the mixes differ"


# ---------------------------------------------------------------------------------------------- CPU: the checks, without a device

def test_notes_check_accepts_a_valid_batch():
    L = device.load()
    assert device.notes_check(make_notes(16, 0, [k % 4 for k in range(16)])) == 0
    one = device.note_array([device.NoteC(0.5, 1.0, 0.0, 0.5, 0.5, SET_PHASE | SET_PAN)])
    assert L.skred_notes_check(C.cast(one, C.c_void_p), 1) == 0
    assert L.skred_notes_check(C.cast(one, C.c_void_p), 0) == 0
    # values a note does not set are not looked at
    assert device.notes_check([device.NoteC(0.5, 1.0, NAN, float("inf"), NAN, 0)]) == 0
    assert device.notes_check([device.NoteC(-0.5, -0.0, -3.0, -1.0, 2.0, SET_PHASE | SET_PAN)]) == 0


BAD_NOTES = {
    "unknown_flag": device.NoteC(0.5, 1.0, 0.0, 0.5, 0.5, 4),
    "high_flag": device.NoteC(0.5, 1.0, 0.0, 0.5, 0.5, SET_PHASE | (1 << 31)),
    "reserved0": device.NoteC(0.5, 1.0, 0.0, 0.5, 0.5, 0, (C.c_uint32 * 2)(1, 0)),
    "reserved1": device.NoteC(0.5, 1.0, 0.0, 0.5, 0.5, 0, (C.c_uint32 * 2)(0, 9)),
    "inc_nan": device.NoteC(NAN, 1.0, 0.0, 0.5, 0.5, 0),
    "inc_inf": device.NoteC(float("inf"), 1.0, 0.0, 0.5, 0.5, 0),
    "velocity_nan": device.NoteC(0.5, NAN, 0.0, 0.5, 0.5, 0),
    "velocity_inf": device.NoteC(0.5, -float("inf"), 0.0, 0.5, 0.5, 0),
    "phase_nan": device.NoteC(0.5, 1.0, NAN, 0.5, 0.5, SET_PHASE),
    "phase_inf": device.NoteC(0.5, 1.0, float("inf"), 0.5, 0.5, SET_PHASE | SET_PAN),
    "pan_left_nan": device.NoteC(0.5, 1.0, 0.0, NAN, 0.5, SET_PAN),
    "pan_right_inf": device.NoteC(0.5, 1.0, 0.0, 0.5, float("inf"), SET_PAN | SET_PHASE),
}


@pytest.mark.parametrize("case", list(BAD_NOTES))
def test_notes_check_refuses(case):
    good = make_notes(5, 1)
    assert device.notes_check(good) == 0
    for at in (0, 2, 4):                                  # the bad note anywhere in the batch
        batch = list(good)
        batch[at] = BAD_NOTES[case]
        assert device.notes_check(batch) == BAD, (case, at)


def test_refusals_without_a_device():
    L = device.load()
    notes = device.note_array(make_notes(4, 2))
    p = C.cast(notes, C.c_void_p)
    assert L.skred_notes_check(None, 4) == BAD and L.skred_notes_check(p, -1) == BAD
    word = (C.c_uint32 * 8)()                             # stands in for device memory: a refusal never reads it
    q = device.IdleQueryC(0, 1, ENV, 0.0, 0, 0)
    assert L.skred_bank_notes_on_list(None, p, 4, word, word, 0, word, word, None) == BAD
    assert L.skred_bank_note_on_idle(None, C.byref(q), p, 4, word, word, None) == BAD
    assert L.skred_bank_stamp_list(None, word, 4, None, STAMP_RELEASE, None) == BAD
    assert b"stamp_list" in L.skred_amd_last_error()


# ---------------------------------------------------------------------------------------------- 1. the same as the host path

@pytest.mark.gpu
@pytest.mark.parametrize("n,family", [(1000, 1), (4096, 3)])
def test_same_as_the_host_path(dev, n, family):
    """Six blocks of an allocator: `db` places K notes per block with note_on_idle and releases the voices of two blocks ago by
    handing that block's d_assigned to stamp_list; `twin` asks find_idle_host, writes the host view and updates."""
    import torch
    K, F = 16, 256
    bank, tables, g = traffic_bank(n)
    setup = (lambda d: d.fast2_min_voices(0)) if family == 3 else None
    db, twin = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    truth, gl, mirror = bank.copy(), g.copy(), bank.copy()
    assigned, history, last = [], [], n - 1
    try:
        for k in range(6):
            tag = f"n {n} block {k}"
            notes = make_notes(K, k)
            start = (last + 1) % n
            now = gl.synth_sample_count
            picks, _ = twin.find_idle_host(0, n, WHICH, float(SETTLE), start, K)
            assert np.array_equal(picks, expected(truth, 0, n, WHICH, SETTLE, start)[:K]) and len(picks) == K, tag
            da, dr = outputs(K)
            torch.cuda.synchronize()
            db.note_on_idle(notes, 0, n, WHICH, float(SETTLE), start, da.data_ptr(), dr.data_ptr())
            store_notes((truth, mirror), truth, notes, picks, now)
            twin.update(mirror, picks, DIRTY_PARAMS | DIRTY_PHASE | STAMP_TRIGGER)
            if k >= 2:
                older = history[k - 2]
                db.stamp_list(assigned[k - 2].data_ptr(), K, STAMP_RELEASE)
                twin.update(mirror, older, STAMP_RELEASE)
                do_release(truth, older, now)
            assigned.append(da)
            history.append(picks)
            last = int(picks[-1])
            same_mix(db, twin, F, tag)
            cpuref.render(truth, gl, tables, F, 0)
            got, res = da.cpu().numpy(), dr.cpu().numpy()
            assert np.array_equal(got[:K], picks) and (got[K:] == -7).all(), f"{tag}: d_assigned {got.tolist()}, the twin picked {picks.tolist()}"
            assert res.tolist() == [K, 0], f"{tag}: d_result {res.tolist()}"
            same_state(db, twin, truth, bank, tag)
            assert db.last_kernel() == twin.last_kernel() == family, (tag, db.last_kernel(), twin.last_kernel())
            assert db.last_pack() == twin.last_pack(), tag
            assert db.list_violations() == twin.list_violations() == 0, tag
        e = truth["voice_amp_envelope"]
        assert (e["is_active"][history[0]] == 0).all() and (e["is_active"][history[5]] == 1).all()   # released notes ended, fresh ones sound
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 2. scarce and empty lists, no notes

@pytest.mark.gpu
def test_scarce_and_empty_lists(dev):
    import torch
    n, K, F = 1000, 16, 256
    bank, tables, g = traffic_bank(n)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    truth, gl, mirror = bank.copy(), g.copy(), bank.copy()
    try:
        render_blocks(db, (F,)); render_blocks(twin, (F,))
        cpuref.render(truth, gl, tables, F, 0)
        notes = make_notes(K, 3, SET_PHASE | SET_PAN)
        # fewer idle voices than notes
        want = expected(truth, 3, 10, WHICH, SETTLE)
        assert 0 < len(want) < K, len(want)
        da, dr = outputs(K)
        torch.cuda.synchronize()
        db.note_on_idle(notes, 3, 10, WHICH, float(SETTLE), None, da.data_ptr(), dr.data_ptr())
        torch.cuda.synchronize()
        got, res = da.cpu().numpy(), dr.cpu().numpy()
        assert res.tolist() == [len(want), K - len(want)] and res[1] > 0, res.tolist()
        assert np.array_equal(got[:len(want)], want) and (got[len(want):K] == -1).all() and (got[K:] == -7).all(), got.tolist()
        store_notes((truth, mirror), truth, notes, want, gl.synth_sample_count)
        twin.update(mirror, want, DIRTY_PARAMS | DIRTY_PHASE | DIRTY_PAN | STAMP_TRIGGER)
        # a range without an idle voice: every note is dropped, nothing is stored
        busy = expected(truth, 8, 1, WHICH, SETTLE)
        assert len(busy) == 0
        before = bank.copy()
        db.download(before)
        da, dr = outputs(K)
        torch.cuda.synchronize()
        db.note_on_idle(notes, 8, 1, WHICH, float(SETTLE), None, da.data_ptr(), dr.data_ptr())
        torch.cuda.synchronize()
        assert dr.cpu().numpy().tolist() == [0, K] and (da.cpu().numpy()[:K] == -1).all()
        after = bank.copy()
        db.download(after)
        assert not before.rw_equal(after), before.rw_equal(after)
        # no notes: nothing happens, whatever the list holds
        da, dr = outputs(K)
        torch.cuda.synchronize()
        db.note_on_idle([], 0, n, WHICH, float(SETTLE), None, da.data_ptr(), dr.data_ptr())
        db.notes_on_list([], da.data_ptr(), dr.data_ptr(), 0, da.data_ptr(), dr.data_ptr())
        db.stamp_list(da.data_ptr(), 0, STAMP_RELEASE)
        torch.cuda.synchronize()
        assert (dr.cpu().numpy() == -7).all() and (da.cpu().numpy() == -7).all()
        # ... and the parameters the dropped notes carried went nowhere: the next block is the twin's and the oracle's
        same_mix(db, twin, F, "after the empty lists")
        cpuref.render(truth, gl, tables, F, 0)
        same_state(db, twin, truth, bank, "after the empty lists")
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 3. the cursor

@pytest.mark.gpu
def test_cursor_shares_one_query(dev):
    import torch
    n, K, F = 1000, 16, 256
    bank, tables, g = traffic_bank(n)
    db = open_bank(dev, bank, tables, g)
    truth, gl = bank.copy(), g.copy()
    try:
        lst = expected(truth, 0, n, WHICH, SETTLE, 500)[:2 * K]
        assert len(lst) == 2 * K
        dv = torch.full((2 * K + 8,), -1, dtype=torch.int32, device="cuda")
        dc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        batches = [make_notes(K, 10 + i) for i in range(3)]
        outs = [outputs(K) for _ in range(3)]
        torch.cuda.synchronize()
        db.find_idle(0, n, WHICH, float(SETTLE), 500, 2 * K, dv.data_ptr(), dc.data_ptr())
        for i in range(3):
            db.notes_on_list(batches[i], dv.data_ptr(), dc.data_ptr(), i * K, outs[i][0].data_ptr(), outs[i][1].data_ptr())
        torch.cuda.synchronize()
        assert dc.cpu().numpy()[0] == 2 * K and np.array_equal(dv.cpu().numpy()[:2 * K], lst)
        got = [o[0].cpu().numpy()[:K] for o in outs]
        assert np.array_equal(got[0], lst[:K]) and np.array_equal(got[1], lst[K:]), (got, lst)
        assert not set(got[0]) & set(got[1])
        assert (got[2] == -1).all()
        assert [o[1].cpu().numpy().tolist() for o in outs] == [[K, 0], [K, 0], [0, K]]
        now = gl.synth_sample_count
        store_notes((truth,), truth, batches[0], lst[:K], now)
        store_notes((truth,), truth, batches[1], lst[K:], now)
        render_blocks(db, (F,))
        cpuref.render(truth, gl, tables, F, 0)
        a = bank.copy()
        db.download(a)
        assert not a.rw_equal(truth), a.rw_equal(truth)
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 4. stream order, no host wait

@pytest.mark.gpu
def test_stream_order_without_a_host_wait(dev):
    """Releases stamped, a block long enough for them to end, the note-ons on the voices that block set free, a block -- on one
    stream of the caller's, nothing waited for until the end."""
    import torch
    n, K, F = 1000, 16, 512
    bank, tables, g = traffic_bank(n)
    db = open_bank(dev, bank, tables, g)
    try:
        s = torch.cuda.Stream()
        o1, o2 = torch.zeros(F, 2, device="cuda"), torch.zeros(F, 2, device="cuda")
        da, dr = outputs(K)
        released = np.arange(0, n, 16, dtype=np.int32)
        notes = make_notes(K, 4)
        truth, gl = bank.copy(), g.copy()
        assert not set(released) & set(expected(truth, 0, n, WHICH, SETTLE))
        torch.cuda.synchronize()
        db.update(bank, released, STAMP_RELEASE, s.cuda_stream)
        db.render_mix(F, o1.data_ptr(), 2, 0, 0, s.cuda_stream)
        db.note_on_idle(notes, 0, n, WHICH, float(SETTLE), None, da.data_ptr(), dr.data_ptr(), s.cuda_stream)
        db.render_mix(F, o2.data_ptr(), 2, 0, 0, s.cuda_stream)
        s.synchronize()
        do_release(truth, released, gl.synth_sample_count)
        cpuref.render(truth, gl, tables, F, 0)
        want = expected(truth, 0, n, WHICH, SETTLE)[:K]
        assert len(want) == K and set(released) & set(want), "no voice of the list was set free by the block in front of it"
        store_notes((truth,), truth, notes, want, gl.synth_sample_count)
        cpuref.render(truth, gl, tables, F, 0)
        assert np.array_equal(da.cpu().numpy()[:K], want) and dr.cpu().numpy().tolist() == [K, 0]
        a = bank.copy()
        db.download(a)
        assert not a.rw_equal(truth), a.rw_equal(truth)
        assert db.list_violations() == 0
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 5. the flags

@pytest.mark.gpu
def test_flags(dev):
    """Without SET_PHASE the running phase and voice_finished stay; without SET_PAN the pans stay (the notes hold NaN there)."""
    import torch
    n, K, F = 1000, 16, 256
    bank, tables, g = traffic_bank(n)
    bank["voice_finished"][[2, 5, 7, 13]] = 1
    db = open_bank(dev, bank, tables, g)
    truth, gl = bank.copy(), g.copy()
    try:
        render_blocks(db, (F,))
        cpuref.render(truth, gl, tables, F, 0)
        flags = [k % 4 for k in range(K)]
        notes = make_notes(K, 5, flags)
        want = expected(truth, 0, n, WHICH, SETTLE)[:K]
        fin, fl = truth["voice_finished"][want] != 0, np.array(flags)
        for f in range(4):                                 # every combination meets a finished voice and a running one
            assert (fin & (fl == f)).any() and (~fin & (fl == f)).any(), f
        phase0, pan0, fin0 = truth["voice_phase"].copy(), truth["voice_pan_left"].copy(), truth["voice_finished"].copy()
        da, dr = outputs(K)
        torch.cuda.synchronize()
        db.note_on_idle(notes, 0, n, WHICH, float(SETTLE), None, da.data_ptr(), dr.data_ptr())
        a = bank.copy()
        db.download(a)                                     # the stores themselves, before any block
        store_notes((truth,), truth, notes, want, gl.synth_sample_count)
        assert np.array_equal(da.cpu().numpy()[:K], want)
        assert not a.rw_equal(truth), a.rw_equal(truth)
        keep, move = want[(fl & SET_PHASE) == 0], want[(fl & SET_PHASE) != 0]
        assert (a["voice_phase"][keep].view(np.uint32) == phase0[keep].view(np.uint32)).all() and (phase0[keep] != 0).any()
        assert (a["voice_finished"][keep] == fin0[keep]).all() and (a["voice_finished"][move] == 0).all()
        assert (a["voice_pan_left"][want[(fl & SET_PAN) == 0]] == pan0[want[(fl & SET_PAN) == 0]]).all()
        assert (a["voice_pan_left"][want[(fl & SET_PAN) != 0]] != pan0[want[(fl & SET_PAN) != 0]]).all()
        render_blocks(db, (F,))
        cpuref.render(truth, gl, tables, F, 0)
        db.download(a)
        assert not a.rw_equal(truth), a.rw_equal(truth)
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 6. stamp_list's guards

@pytest.mark.gpu
def test_stamp_list_guards(dev):
    import torch
    n, F = 1000, 512
    bank, tables, g = traffic_bank(n)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    truth, gl = bank.copy(), g.copy()
    try:
        # sounding voices (every eighth) among holes, a voice past the bank and the largest int; the count ends the list early
        lst = np.array([-1, 8, 16, -1, n, 24, 2**31 - 1, -2**31, 32, 40], np.int32)
        inside = 8
        valid = np.array([8, 16, 24], np.int32)
        assert (truth["voice_amp_envelope"]["is_active"][[8, 16, 24, 32, 40]] == 1).all()
        dv, dc = torch.from_numpy(lst).cuda(), torch.tensor([inside, 99], dtype=torch.int32, device="cuda")
        on = np.array([1, -1, 2, n + 5, 3], np.int32)      # no count: all n entries; a trigger and a release in one call
        dv2 = torch.from_numpy(on).cuda()
        torch.cuda.synchronize()
        db.stamp_list(dv.data_ptr(), len(lst), STAMP_RELEASE, dc.data_ptr())
        db.stamp_list(dv2.data_ptr(), len(on), STAMP_TRIGGER | STAMP_RELEASE)
        twin.update(bank, valid, STAMP_RELEASE)
        twin.update(bank, on[[0, 2, 4]], STAMP_TRIGGER | STAMP_RELEASE)
        now = gl.synth_sample_count
        do_release(truth, valid, now)
        e = truth["voice_amp_envelope"]
        e["sample_start"][on[[0, 2, 4]]], e["is_active"][on[[0, 2, 4]]] = now, 1
        e["sample_release"][on[[0, 2, 4]]] = now
        same_mix(db, twin, F, "stamp_list")
        cpuref.render(truth, gl, tables, F, 0)
        same_state(db, twin, truth, bank, "stamp_list")
        assert (e["is_active"][valid] == 0).all() and (e["is_active"][[32, 40]] == 1).all()   # past the count: still held
        assert db.list_violations() == twin.list_violations() == 0
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 7. refusals

@pytest.mark.gpu
def test_refusals_leave_the_bank_usable(dev):
    import torch
    n, K, F = 1000, 8, 256
    bank, tables, g = traffic_bank(n)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    truth, gl, mirror = bank.copy(), g.copy(), bank.copy()
    try:
        L = db.L
        good = device.note_array(make_notes(K, 6))
        gp = C.cast(good, C.c_void_p)
        dv = torch.arange(1, K + 1, dtype=torch.int32, device="cuda")
        dc = torch.tensor([K, K], dtype=torch.int32, device="cuda")
        da, dr = outputs(K)
        torch.cuda.synchronize()

        def on_list(bank_h=db.h, notes=gp, count=K, voices=dv.data_ptr(), counts=dc.data_ptr(), first=0, res=dr.data_ptr()):
            return L.skred_bank_notes_on_list(bank_h, notes, count, voices or None, counts or None, first, da.data_ptr(), res or None, None)

        def on_idle(bank_h=db.h, notes=gp, count=K, which=WHICH, q=True, res=dr.data_ptr(), qfirst=0, qcount=n):
            qq = dev.IdleQueryC(qfirst, qcount, which, float(SETTLE), qfirst, -5)      # (max_out is ignored)
            return L.skred_bank_note_on_idle(bank_h, C.byref(qq) if q else None, notes, count, da.data_ptr(), res or None, None)

        def stamp(bank_h=db.h, voices=dv.data_ptr(), count=K, stamps=STAMP_RELEASE):
            return L.skred_bank_stamp_list(bank_h, voices or None, count, None, stamps, None)

        assert on_list(bank_h=None) == BAD and on_list(notes=None) == BAD and on_list(voices=0) == BAD
        assert on_list(counts=0) == BAD and on_list(res=0) == BAD
        assert on_list(count=-1) == BAD and on_list(first=-1) == BAD
        assert on_idle(bank_h=None) == BAD and on_idle(notes=None) == BAD and on_idle(q=False) == BAD and on_idle(res=0) == BAD
        assert on_idle(count=-1) == BAD
        assert on_idle(which=WHICH | AMP) == BAD and on_idle(which=AMP) == BAD
        assert on_idle(which=0) == BAD and on_idle(qcount=n + 1) == -4                 # the query's own refusals
        for name, note in BAD_NOTES.items():
            batch = list(make_notes(K, 6))
            batch[K - 1] = note
            arr = device.note_array(batch)
            p = C.cast(arr, C.c_void_p)
            assert on_list(notes=p) == BAD and on_idle(notes=p) == BAD, name
        assert stamp(bank_h=None) == BAD and stamp(voices=0) == BAD and stamp(count=-1) == BAD
        assert stamp(stamps=0) == BAD and stamp(stamps=STAMP_RELEASE | DIRTY_PARAMS) == BAD and stamp(stamps=1 << 10) == BAD
        assert on_list(count=0) == 0 and on_idle(count=0) == 0 and stamp(count=0) == 0
        torch.cuda.synchronize()
        assert (da.cpu().numpy() == -7).all() and (dr.cpu().numpy() == -7).all()       # nothing reached the device
        # the bank still takes notes and renders, like its twin
        notes = make_notes(K, 6)
        want = expected(truth, 0, n, WHICH, SETTLE)[:K]
        db.note_on_idle(notes, 0, n, WHICH, float(SETTLE), None, da.data_ptr(), dr.data_ptr())
        store_notes((truth, mirror), truth, notes, want, gl.synth_sample_count)
        twin.update(mirror, want, DIRTY_PARAMS | DIRTY_PHASE | STAMP_TRIGGER)
        same_mix(db, twin, F, "after the refusals")
        cpuref.render(truth, gl, tables, F, 0)
        assert np.array_equal(da.cpu().numpy()[:K], want) and dr.cpu().numpy().tolist() == [K, 0]
        same_state(db, twin, truth, bank, "after the refusals")
    finally:
        db.close()
        twin.close()
