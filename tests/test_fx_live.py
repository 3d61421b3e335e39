"""Live control of the fixed-point bank on the GPU: skred_fxbank_update, _find_idle / _find_idle_host, _notes_on_list /
_note_on_idle / _stamp_list, and skred_fxbank_stamp through the staging ring.

Every comparison is exact -- these are integers.  The same action is applied to the ORACLE's bank through tests/fx_live_model.py,
oracle.cpuref.fx_render renders the block, and the downloaded read-write fields, the mix and the device lists / counts must be
equal bit for bit.  DeviceFxBank.download returns the read-write fields only: a parameter an action stored shows in the block
rendered after it (the mix, the running phase, the smoother's gain, is_active).

One host view holds one value per voice, so a voice listed three times in ONE call carries three equal records (the result must
be that of one application); "different values, the last one wins" is checked with three calls back to back on one stream.
"""
import ctypes as C

import numpy as np
import pytest

import fx_live_model as model
from oracle import cpuref
from skred_amd import device, fxbank as fxb

pytestmark = pytest.mark.gpu

FIN, ENV, AMP = fxb.IDLE_FINISHED, fxb.IDLE_ENV_DONE, fxb.IDLE_AMP_ZERO
ALL_BITS = model.ALL_VALUE_BITS | fxb.STAMP_TRIGGER | fxb.STAMP_RELEASE
BLOCKS = [(1, 0), (64, 1), (100, 0), (1, 1), (64, 0), (100, 1)]        # frames, interp: around every update


@pytest.fixture(scope="module")
def base():
    """1 000 voices (not a multiple of 256) of the bank_fx recipe, with muted, silent, unsmoothed, unfiltered and one-shot voices."""
    n = 1000
    b, pool, c0 = fxb.bank_fx(n)
    b["disconnect"][::7] = 1
    b["amp_q15"][::11] = 0
    b["smoother_enable"][::13] = 0
    b["filter_mode"][::5] = 0
    one = np.arange(3, n, 17)
    b["one_shot"][one] = 1
    b["phase_inc"][one] = ((1 << 32) // (50 + (one * 37) % 1450)).astype(np.uint32)
    return b, pool, c0


def open_fx(b, pool, c0):
    db = fxb.DeviceFxBank(b.n)
    db.set_tables(pool)
    db.upload(b)
    db.set_sample_count(c0)
    return db


def block(db, ref, pool, cnt, frames, interp, tag):
    """One block on both sides: the mixes and then the whole read-write state must be equal."""
    mix, _ = db.render_host(frames, interp)
    want, _, cnt = cpuref.fx_render(ref, pool, cnt, frames, interp)
    assert (mix == want).all(), f"{tag}: the mix differs from the oracle's"
    got = ref.copy()
    db.download(got)
    assert not got.rw_mismatch(ref), f"{tag}: state differs from the oracle's: {got.rw_mismatch(ref)}"
    assert db.sample_count() == cnt
    return cnt


def scramble(h, rng, now):
    """New values in EVERY field of the host view (inside the definition's promised range): an update must move only what it names."""
    n = h.n
    perm = rng.permutation(n)
    for k in ("table_offset", "log2_size"):                # a table window stays a table window
        h[k] = h[k][perm]
    perm = rng.permutation(n)
    for k in ("filter_mode", "b0_q30", "b1_q30", "b2_q30", "a1_q30", "a2_q30"):
        h[k] = h[k][perm]
    h["phase_inc"] = rng.integers(1 << 18, 1 << 27, n)
    h["amp_q15"] = rng.integers(0, 32769, n) * (rng.integers(0, 9, n) != 0)
    h["disconnect"] = rng.integers(0, 12, n) == 0
    h["use_envelope"] = rng.integers(0, 6, n) != 0
    h["smoother_enable"] = rng.integers(0, 4, n) != 0
    h["one_shot"] = rng.integers(0, 10, n) == 0
    h["attack_frames"] = rng.integers(0, 3000, n)
    h["decay_frames"] = rng.integers(0, 3000, n)
    h["release_frames"] = rng.integers(0, 3000, n)
    h["sustain_q15"] = rng.integers(0, 32769, n)
    h["smoother_k_q15"] = rng.integers(1, 3000, n)
    h["velocity_q15"] = rng.integers(0, 32769, n)
    h["pan_left_q15"] = rng.integers(0, 32769, n)
    h["pan_right_q15"] = rng.integers(0, 32769, n)
    h["phase"] = rng.integers(0, 1 << 32, n)
    h["finished"] = rng.integers(0, 15, n) == 0
    h["is_active"] = rng.integers(0, 3, n) * 5             # any non-zero value means active
    for k in ("x1", "x2", "y1", "y2"):
        h[k] = rng.integers(-(1 << 22), 1 << 22, n)
    h["smoother_gain_q15"] = rng.integers(0, 30000, n)
    h["voice_sample"] = rng.integers(-20000, 20000, n)
    h["sample_start"] = now - rng.integers(0, 20000, n)
    h["sample_release"] = (now - rng.integers(0, 3000, n)) * (rng.integers(0, 3, n) == 0)


def dev_i32(k, fill=-7):
    import torch
    return torch.full((k,), fill, dtype=torch.int32, device="cuda")


def host_of(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. updates

BIT_CASES = {"params": fxb.DIRTY_PARAMS, "pan": fxb.DIRTY_PAN, "phase": fxb.DIRTY_PHASE, "env_state": fxb.DIRTY_ENV_STATE,
             "filter_state": fxb.DIRTY_FILTER_STATE, "smoother": fxb.DIRTY_SMOOTHER, "sample": fxb.DIRTY_SAMPLE,
             "env_clock": fxb.DIRTY_ENV_CLOCK, "trigger": fxb.STAMP_TRIGGER, "release": fxb.STAMP_RELEASE,
             "clock_then_stamps": fxb.DIRTY_ENV_CLOCK | fxb.STAMP_RELEASE, "all": ALL_BITS}


@pytest.mark.parametrize("case", list(BIT_CASES))
def test_fx_update_moves_what_it_names_and_nothing_else(base, case):
    b, pool, c0 = base
    dirty = BIT_CASES[case]
    ref, cnt = b.copy(), c0
    db = open_fx(b, pool, c0)
    rng = np.random.default_rng(list(BIT_CASES).index(case))
    h = b.copy()
    cnt = block(db, ref, pool, cnt, 37, 1, "before")       # the voices are sounding: the host's copies are stale from here on
    for frames, interp in BLOCKS:
        scramble(h, rng, cnt)
        voices = rng.choice(b.n, 1 + int(rng.integers(0, 200)), replace=False).astype(np.int32)
        db.update(h, voices, dirty)
        model.apply_update(ref, h, voices, dirty, cnt)
        cnt = block(db, ref, pool, cnt, frames, interp, f"{case} {frames}x{interp}")
    db.close()


@pytest.mark.parametrize("size", [1, 63, 64, 65, 300])
def test_fx_update_batch_sizes_and_repeated_voices(base, size):
    b, pool, c0 = base
    ref, cnt = b.copy(), c0
    db = open_fx(b, pool, c0)
    rng = np.random.default_rng(100 + size)
    h = b.copy()
    cnt = block(db, ref, pool, cnt, 64, 1, "before")
    scramble(h, rng, cnt)
    voices = rng.choice(b.n, size, replace=False).astype(np.int32)
    if size == 300:                                        # one voice three times in the batch: three launches, one result
        voices[150] = voices[7]
        voices[299] = voices[7]
    db.update(h, voices, ALL_BITS)
    model.apply_update(ref, h, voices, ALL_BITS, cnt)
    cnt = block(db, ref, pool, cnt, 100, 1, f"batch of {size}")
    # the same voice in three calls back to back with different values: order kept, the last one wins
    v = voices[:1]
    for k in range(3):
        h["phase_inc"][v] = 1000003 * (k + 1)
        h["pan_left_q15"][v] = 5000 * (k + 1)
        h["phase"][v] = 77 * (k + 1)
        db.update(h, v, fxb.DIRTY_PARAMS | fxb.DIRTY_PAN | fxb.DIRTY_PHASE)
        model.apply_update(ref, h, v, fxb.DIRTY_PARAMS | fxb.DIRTY_PAN | fxb.DIRTY_PHASE, cnt)
    assert ref["phase_inc"][v[0]] == 3000009
    cnt = block(db, ref, pool, cnt, 64, 0, "three calls")
    db.close()


def test_fx_update_ring_wraps_without_a_wait_for_the_device(base):
    """Three times as many batches as the ring has slots, back to back on one stream, then ONE render."""
    b, pool, c0 = base
    ref, cnt = b.copy(), c0
    db = open_fx(b, pool, c0)
    rng = np.random.default_rng(9)
    h = b.copy()
    cnt = block(db, ref, pool, cnt, 64, 1, "before")
    for k in range(3 * fxb.FX_RING_SLOTS):
        scramble(h, rng, cnt)
        voices = rng.choice(b.n, 1 + 13 * k, replace=False).astype(np.int32)
        dirty = [fxb.DIRTY_PARAMS | fxb.DIRTY_PAN, ALL_BITS, fxb.STAMP_RELEASE, fxb.DIRTY_PHASE | fxb.DIRTY_SMOOTHER][k % 4]
        db.update(h, voices, dirty)
        model.apply_update(ref, h, voices, dirty, cnt)
    cnt = block(db, ref, pool, cnt, 100, 1, "after 3 x ring batches")
    db.close()


def test_fx_update_params_with_a_filter_grow_n_filter():
    """A bank WITHOUT any filter voice; one voice gets a biquad through PARAMS: the next block must run the biquad instantiation."""
    b, pool, c0 = fxb.bank_fx(1000, with_filter=False)
    donor, _, _ = fxb.bank_fx(1000)
    ref, cnt = b.copy(), c0
    db = open_fx(b, pool, c0)
    cnt = block(db, ref, pool, cnt, 64, 1, "before")
    h = b.copy()
    for k in ("filter_mode", "b0_q30", "b1_q30", "b2_q30", "a1_q30", "a2_q30"):
        h[k][17] = donor[k][17]
    assert h["filter_mode"][17] != 0
    db.update(h, [17], fxb.DIRTY_PARAMS)
    model.apply_update(ref, h, [17], fxb.DIRTY_PARAMS, cnt)
    cnt = block(db, ref, pool, cnt, 64, 1, "first filtered block")
    assert (ref["y1"][17] != 0) and (np.delete(ref["y1"], 17) == 0).all()
    db.close()


def test_fx_stamp_goes_through_the_ring(base):
    b, pool, c0 = base
    ref, cnt = b.copy(), c0
    db = open_fx(b, pool, c0)
    cnt = block(db, ref, pool, cnt, 64, 1, "before")
    rng = np.random.default_rng(4)
    for k in range(2 * fxb.FX_RING_SLOTS + 1):             # pairs of stamp calls back to back, past the ring's length
        off = rng.choice(b.n, 40, replace=False).astype(np.int32)
        on = rng.choice(b.n, 70, replace=False).astype(np.int32)
        db.stamp(off, fxb.FX_STAMP_RELEASE)
        db.stamp(on, fxb.FX_STAMP_TRIGGER)
        model.stamp(ref, off, fxb.STAMP_RELEASE, cnt)
        model.stamp(ref, on, fxb.STAMP_TRIGGER, cnt)
        if k % 6 == 5:
            cnt = block(db, ref, pool, cnt, 64, 1, f"stamps {k}")
    cnt = block(db, ref, pool, cnt, 100, 0, "stamps")
    db.close()


def test_fx_staging_ring_serves_every_call_family_back_to_back():
    """The batch path (skred_fx_stage.c) is the one way a host-written batch reaches a kernel of this bank, whatever the call: 3 x
    FX_RING_SLOTS = 24 staged calls of twelve kinds go to bank A back to back on one stream -- every slot of the ring is reused twice,
    by a call of another family, under nothing but its event -- and to bank B with a device synchronise after each.  Everything the
    calls write must be the same, byte for byte.  This ring always reads the slot's device twin behind a copy: there is no size
    threshold to cross, so 4096 voices do.  Voice i carries the tag i + 1 for i < 1024.  Every device buffer exists before the first
    call, so nothing but the calls themselves is issued in between."""
    import torch
    n, E, calls = 4096, 8, 3 * fxb.FX_RING_SLOTS
    bank, pool, c0 = fxb.bank_fx(n)
    REL = fxb.STAMP_RELEASE

    def i32(values):
        return torch.tensor(np.asarray(values, np.int64).astype(np.int32), dtype=torch.int32, device="cuda")

    def ids_of(k):
        return np.arange(E) * 97 + 13 * k                     # eight voices below 1024: voice v carries the tag v + 1

    def run(sync_each):
        db = open_fx(bank, pool, c0)
        host = bank.copy()
        db.render_host(64, 1)                                 # the voices are sounding, the clock has moved
        first = i32(np.arange(1024))
        db.tag_list(first.data_ptr(), np.arange(1, 1025))
        lists = [i32(ids_of(k)) for k in range(calls)]
        high = [i32(3100 + ids_of(k)) for k in range(calls)]
        cnt = i32([E])
        results = [torch.zeros(3, dtype=torch.int32, device="cuda") for _ in range(calls)]
        found = [torch.full((E,), -7, dtype=torch.int32, device="cuda") for _ in range(calls)]
        torch.cuda.synchronize()
        for k in range(calls):
            ids, lst, res, val = ids_of(k), lists[k].data_ptr(), results[k].data_ptr(), 100 + 7 * k
            pan = fxb.fx_ctl(fxb.CTL_PAN, pan_left_q15=val, pan_right_q15=2 * val)
            kind = k % 12
            if kind == 0:
                vs = (2048 + ids).astype(np.int32)
                host["phase_inc"][vs] = 1000003 * (k + 1)
                db.update(host, vs, fxb.DIRTY_PARAMS)
            elif kind == 1:
                if k < 12:
                    db.update(host, (2048 + ids).astype(np.int32), REL)
                else:
                    db.stamp(2048 + ids, fxb.FX_STAMP_TRIGGER)
            elif kind == 2:
                notes = [fxb.FxNoteC(3000017 + val, 9000 + val, 77 * val, val, 32000 - val, fxb.NOTE_SET_PHASE | fxb.NOTE_SET_PAN)
                         for _ in range(E)]
                db.notes_on_list(notes, lst, cnt.data_ptr(), 0, 0, res)
            elif kind == 3:
                db.tag_list(high[k].data_ptr(), 5000 + ids, 0, res)
            elif kind == 4:
                db.find_owned(0, n, np.concatenate([ids[:6] + 1, [5000 + 13 * 3, 77777]]), found[k].data_ptr())
            elif kind == 5:
                db.stamp_owned(lst, ids + 1, REL, res)
            elif kind == 6:
                db.release_tags(0, n, ids + 1, REL, res)
            elif kind == 7:
                db.ctl_range(pan, 0, n, res)
            elif kind == 8:
                db.ctl_list(pan, lst, E, 0, res)
            elif kind == 9:
                db.ctl_owned(pan, lst, ids + 1, 0, res)
            elif kind == 10:
                db.ctl_match(fxb.fx_ctl(fxb.CTL_VELOCITY, velocity_q15=val), 0, n, k & 3, 3, res)
            else:
                each = [fxb.fx_each(fxb.EACH_VELOCITY, velocity_q15=val + j) for j in range(E)]
                db.ctl_owned_each(pan, each, lst, ids + 1, 0, res)
            if sync_each:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        got, params = bank.copy(), bank.copy()
        db.download(got)
        owners, recips = db.download_owners(), db.download_params(params)
        mix, _ = db.render_host(64, 1)
        db.close()
        return dict(bank=got, params=params, owners=owners, recips=recips, mix=mix, results=[host_of(r) for r in results],
                    found=[host_of(found[k]) for k in range(calls) if k % 12 == 4])

    a, b = run(False), run(True)
    for view in ("bank", "params"):
        differ = [name for name in a[view].a if a[view].a[name].tobytes() != b[view].a[name].tobytes()]
        assert not differ, (view, differ)
    assert a["owners"].tobytes() == b["owners"].tobytes() and a["recips"].tobytes() == b["recips"].tobytes()
    for k, (ra, rb) in enumerate(zip(a["results"], b["results"])):
        assert ra.tobytes() == rb.tobytes(), (k, ra, rb)
    assert len(a["found"]) == 2 and all(fa.tobytes() == fb.tobytes() for fa, fb in zip(a["found"], b["found"]))
    assert a["mix"].tobytes() == b["mix"].tobytes()
    # the calls did what they say: nothing above compares two banks that both stood still
    assert int(a["owners"][3100 + 13 * 3]) == 5000 + 13 * 3 and a["found"][0].tolist()[:6] == ids_of(4)[:6].tolist()
    assert a["found"][0].tolist()[6:] == [3100 + 13 * 3, -1] and a["results"][2].tolist()[:2] == [E, 0]
    assert int(a["params"]["pan_left_q15"][n - 1]) == 100 + 7 * 19 and a["results"][7].tolist()[:2] == [n, 0]
    assert int(a["params"]["phase_inc"][2048 + 13 * 12]) == 1000003 * 13 and a["results"][5].tolist() == [E, 0, 0]


# ---------------------------------------------------------------------------------------------- 2. the idle list

def idle_state(n, seed):
    """A bank whose idle state is written on the host and uploaded: every combination of the predicate's inputs occurs."""
    b, pool, c0 = fxb.bank_fx(n, with_filter=False)
    rng = np.random.default_rng(seed)
    b["use_envelope"] = rng.integers(0, 5, n) != 0
    b["is_active"] = rng.integers(0, 3, n) != 0
    b["smoother_enable"] = rng.integers(0, 3, n) != 0
    b["smoother_gain_q15"] = rng.integers(-2, 3, n) * rng.integers(0, 2, n) * 3
    b["smoother_gain_q15"][::101] = -(1 << 31)             # |g| needs 64 bits
    b["finished"] = rng.integers(0, 9, n) == 0
    b["amp_q15"] = 20000 * (rng.integers(0, 7, n) != 0)
    return b, pool, c0


@pytest.fixture(scope="module")
def big():
    n = 70000                                              # 274 workgroups: the last arriver's scan owns more than one count per thread
    b, pool, c0 = idle_state(n, 1)
    db = open_fx(b, pool, c0)
    yield b, pool, c0, db
    db.close()


def run_query(db, b, first, count, which, settle, start, max_out, room=None):
    room = max(max_out, 0) + 8 if room is None else room
    d_voices, d_count = dev_i32(room), dev_i32(2)
    db.find_idle(first, count, which, settle, start, max_out, d_voices.data_ptr() if max_out > 0 else 0, d_count.data_ptr())
    got_v, got_c = host_of(d_voices), host_of(d_count)
    want, total = model.idle_list(b, first, count, which, settle, start, max_out)
    assert list(got_c) == [want.size, total], (list(got_c), want.size, total)
    assert (got_v[:want.size] == want).all(), "the list differs from the model's"
    assert (got_v[want.size:] == -7).all(), "entries past `written` were touched"
    return got_v, got_c, total


@pytest.mark.parametrize("which,settle", [(FIN, 0), (ENV, 0), (ENV, 3), (AMP, 0), (FIN | ENV | AMP, 3), (FIN | ENV, 0x7FFFFFFF)])
def test_fx_find_idle_on_70000_voices(big, which, settle):
    b, pool, c0, db = big
    first, count, start = 37, 69990 - 37, 35011
    v1, c1, total = run_query(db, b, first, count, which, settle, start, count)
    assert total > 1000
    v2, c2, _ = run_query(db, b, first, count, which, settle, start, count)
    assert v1.tobytes() == v2.tobytes() and c1.tobytes() == c2.tobytes(), "the same query wrote other bytes"
    run_query(db, b, first, count, which, settle, start, 0)                     # count only
    run_query(db, b, first, count, which, settle, first, 1000)                  # max_out < total: the guard words stay
    run_query(db, b, first, count, which, settle, first + count - 1, 257)       # from = the last voice: wraps at once
    host, host_total = db.find_idle_host(first, count, which, settle, start, count)
    assert host_total == total and (host == v1[:total]).all(), "the host form differs from the device form"


def test_fx_find_idle_reads_the_bank_only():
    """Queries between blocks change nothing: two blocks after them equal the oracle's, which never saw a query."""
    n = 70000
    b, pool, c0 = idle_state(n, 2)
    b["smoother_gain_q15"] = np.abs(np.maximum(b["smoother_gain_q15"], -100))    # (rendered: inside the promised range)
    ref, cnt = b.copy(), c0
    db = open_fx(b, pool, c0)
    run_query(db, b, 0, n, FIN | ENV | AMP, 0, 12345, n)
    cnt = block(db, ref, pool, cnt, 64, 1, "first block after the query")
    run_query(db, ref, 37, 60000, ENV, 0, 50000, 500)                          # the state the device computed
    cnt = block(db, ref, pool, cnt, 64, 1, "second block")
    db.close()


def test_fx_find_idle_small_ranges_and_empty_lists():
    n = 300
    b, pool, c0 = idle_state(n, 3)
    db = open_fx(b, pool, c0)
    for which in (FIN, ENV, AMP, FIN | AMP):
        run_query(db, b, 70, 40, which, 0, 90, 40)                             # inside one wave of the second span
        run_query(db, b, 0, n, which, 0, 299, n)
        run_query(db, b, 63, 2, which, 0, 64, 2)                               # across a wave edge
        run_query(db, b, 299, 1, which, 0, 299, 1)
    b2 = b.copy()
    b2["finished"], b2["amp_q15"], b2["is_active"] = 0, 100, 1                  # no idle voice at all
    db.upload(b2)
    _, c, total = run_query(db, b2, 0, n, FIN | ENV | AMP, 0x7FFFFFFF, 150, n)
    assert total == 0 and list(c) == [0, 0]
    host, host_total = db.find_idle_host(0, n, FIN | ENV | AMP, 0, 0)
    assert host.size == 0 and host_total == 0
    db.close()


# ---------------------------------------------------------------------------------------------- 3. note-ons

def note_bank():
    """1 000 voices, about half of them free: ended envelopes with a settled smoother, and finished one-shots."""
    n = 1000
    b, pool, c0 = fxb.bank_fx(n)
    rng = np.random.default_rng(21)
    free = rng.integers(0, 2, n) == 0
    b["is_active"][free] = 0
    b["smoother_gain_q15"][free] = 0
    one = np.arange(5, n, 9)
    b["one_shot"][one] = 1
    b["finished"][one] = 1
    b["phase"][one] = 0xFFFFFFFF
    b["phase_inc"][one] = ((1 << 32) // (300 + one)).astype(np.uint32)
    return b, pool, c0


def make_notes(k, seed, flags):
    flags = [flags] * k if isinstance(flags, int) else list(flags)
    return [fxb.FxNoteC(3000017 + 40009 * i + seed, 9000 + 23 * i, (0x01234567 * (i + 1)) & 0xFFFFFFFF, 700 + 31 * i, 32000 - 29 * i,
                        flags[i]) for i in range(k)]


def place(db, ref, notes, d_voices, d_count, listed, count0, first_entry, cnt):
    d_assigned, d_result = dev_i32(len(notes) + 8), dev_i32(2)
    db.notes_on_list(notes, d_voices.data_ptr(), d_count.data_ptr(), first_entry, d_assigned.data_ptr(), d_result.data_ptr())
    want, counts = model.place_notes(ref, notes, listed, count0, first_entry, cnt)
    got = host_of(d_assigned)
    assert (got[:len(notes)] == want).all() and (got[len(notes):] == -7).all(), "d_assigned differs from the model's"
    assert tuple(host_of(d_result)) == counts, (host_of(d_result), counts)
    return d_assigned, want


@pytest.mark.parametrize("k", [1, 64, fxb.FX_NOTE_SPAN + 1])
def test_fx_notes_on_list(k):
    b, pool, c0 = note_bank()
    ref, cnt = b.copy(), c0
    db = open_fx(b, pool, c0)
    cnt = block(db, ref, pool, cnt, 64, 1, "before")
    d_voices, d_count, _ = None, None, None
    room = k + 40
    d_voices, d_count = dev_i32(room + 8), dev_i32(2)
    db.find_idle(0, b.n, FIN | ENV, 0, 500, room, d_voices.data_ptr(), d_count.data_ptr())
    listed, total = model.idle_list(ref, 0, b.n, FIN | ENV, 0, 500, room)
    assert total >= room and list(host_of(d_count)) == [room, total]
    flags = [(i % 4) for i in range(k)]                    # nothing, SET_PHASE, SET_PAN, both
    notes = make_notes(k, 1, flags)
    _, first = place(db, ref, notes, d_voices, d_count, listed, room, 0, cnt)
    assert (first >= 0).all()
    # a second call shares the query through first_entry; the list is shorter than the two batches: its tail is dropped
    notes2 = make_notes(60, 2, fxb.NOTE_SET_PHASE)
    _, second = place(db, ref, notes2, d_voices, d_count, listed, room, k, cnt)
    assert (second[:40] >= 0).all() and (second[40:] == -1).all()
    cnt = block(db, ref, pool, cnt, 64, 1, "first block of the notes")
    cnt = block(db, ref, pool, cnt, 100, 0, "second block of the notes")
    db.close()


def test_fx_note_revives_a_finished_one_shot_and_sets_pans():
    b, pool, c0 = note_bank()
    ref, cnt = b.copy(), c0
    db = open_fx(b, pool, c0)
    d_voices, d_count = dev_i32(48), dev_i32(2)
    db.find_idle(0, b.n, FIN, 0, 0, 40, d_voices.data_ptr(), d_count.data_ptr())
    listed, total = model.idle_list(ref, 0, b.n, FIN, 0, 0, 40)
    assert total > 40 and (ref["finished"][listed] == 1).all()
    notes = make_notes(40, 3, [fxb.NOTE_SET_PHASE | fxb.NOTE_SET_PAN] * 20 + [fxb.NOTE_SET_PAN] * 20)
    for t, v in zip(notes, listed):
        t.phase_inc = int(ref["phase_inc"][v])             # one cycle of the table again
        t.phase = 0
    _, got = place(db, ref, notes, d_voices, d_count, listed, 40, 0, cnt)
    assert (ref["finished"][listed[:20]] == 0).all() and (ref["finished"][listed[20:]] == 1).all()
    mix0 = ref["voice_sample"][listed[:20]].copy()
    cnt = block(db, ref, pool, cnt, 100, 1, "revived")
    assert (ref["voice_sample"][listed[:20]] != mix0).any(), "no revived voice sounded"
    assert (ref["pan_left_q15"][listed] == [t.pan_left_q15 for t in notes]).all()
    db.close()


def test_fx_note_on_idle_equals_the_host_path_and_stamp_list_ends_the_notes():
    """note_on_idle on one bank; find_idle_host + update(PARAMS | PAN | PHASE | STAMP_TRIGGER) of the same voices on a twin: the same
    state and the same two blocks, and both equal the oracle's.  Then d_assigned, -1 holes included, is the note-off list."""
    b, pool, c0 = note_bank()
    ref, cnt = b.copy(), c0
    db, twin = open_fx(b, pool, c0), open_fx(b, pool, c0)
    first, count, start = 100, 120, 160
    listed, total = model.idle_list(ref, first, count, ENV | FIN, 0, start, count)
    k = total + 9                                          # more notes than free voices: the last nine are dropped
    notes = make_notes(k, 5, fxb.NOTE_SET_PHASE | fxb.NOTE_SET_PAN)
    d_assigned, d_result = dev_i32(k + 8), dev_i32(2)
    db.note_on_idle(notes, first, count, ENV | FIN, 0, start, d_assigned.data_ptr(), d_result.data_ptr())
    want, counts = model.place_notes(ref, notes, listed, total, 0, cnt)
    assert tuple(host_of(d_result)) == counts == (total, 9)
    assert (host_of(d_assigned)[:k] == want).all() and (want[total:] == -1).all()
    # the twin: the list on the host, the notes' values in the host view, an update
    voices, t_total = twin.find_idle_host(first, count, ENV | FIN, 0, start, k)
    assert t_total == total and (voices == listed).all()
    h = b.copy()                                           # parameters the device still holds; phase and pans come from the notes
    for t, v in zip(notes, voices):
        h["phase_inc"][v], h["velocity_q15"][v], h["phase"][v], h["finished"][v] = t.phase_inc, t.velocity_q15, t.phase, 0
        h["pan_left_q15"][v], h["pan_right_q15"][v] = t.pan_left_q15, t.pan_right_q15
    twin.update(h, voices, fxb.DIRTY_PARAMS | fxb.DIRTY_PAN | fxb.DIRTY_PHASE | fxb.STAMP_TRIGGER)
    a, c = ref.copy(), ref.copy()
    db.download(a)
    twin.download(c)
    assert not a.rw_mismatch(c) and not a.rw_mismatch(ref), (a.rw_mismatch(c), a.rw_mismatch(ref))
    for frames, interp in ((64, 1), (100, 0)):
        m_twin, _ = twin.render_host(frames, interp)
        mix, _ = db.render_host(frames, interp)
        assert (mix == m_twin).all(), "device-side path and host path differ"
        want_mix, _, cnt = cpuref.fx_render(ref, pool, cnt, frames, interp)
        assert (mix == want_mix).all()
    # note-offs through the list the placement left
    db.stamp_list(d_assigned.data_ptr(), k, fxb.STAMP_RELEASE)
    model.stamp(ref, want[want >= 0], fxb.STAMP_RELEASE, cnt)
    cnt = block(db, ref, pool, cnt, 64, 1, "released through stamp_list")
    # ... and with a count in device memory: only the first d_count[0] entries
    d_count = dev_i32(2, 5)
    db.stamp_list(d_assigned.data_ptr(), k, fxb.STAMP_TRIGGER | fxb.STAMP_RELEASE, d_count.data_ptr())
    model.stamp(ref, want[:5], fxb.STAMP_TRIGGER | fxb.STAMP_RELEASE, cnt)
    cnt = block(db, ref, pool, cnt, 64, 0, "stamp_list with a device count")
    db.close()
    twin.close()


# ---------------------------------------------------------------------------------------------- 4. refusals

def test_fx_refusals_leave_the_bank_usable(base):
    b, pool, c0 = base
    ref, cnt = b.copy(), c0
    db = open_fx(b, pool, c0)
    cnt = block(db, ref, pool, cnt, 64, 1, "before")
    h = b.copy()
    h["phase_inc"][:] = 12345                              # must never arrive
    d, note = dev_i32(16), make_notes(1, 0, 0)
    bad_table = h.copy()
    bad_table["table_offset"][3] = len(pool) - 4
    bad_amp = h.copy()
    bad_amp["amp_q15"][2] = 65536
    bad_line = h.copy()
    bad_line["y1"][1] = 1 << 29
    refused = [
        lambda: db.update(h, [0, 1], fxb.DIRTY_PARAMS | fxb.DIRTY_HOLD),
        lambda: db.update(h, [0, b.n], fxb.DIRTY_PARAMS),
        lambda: db.update(h, [-1], fxb.STAMP_TRIGGER),
        lambda: db.update(h, [0], 0),
        lambda: db.update(h, [0], 1 << 11),
        lambda: db.update(bad_table, [0, 3], fxb.DIRTY_PARAMS),
        lambda: db.update(bad_amp, [2], fxb.DIRTY_PARAMS),
        lambda: db.update(bad_line, [0, 1], fxb.DIRTY_FILTER_STATE),
        lambda: db.find_idle(0, b.n, ENV | fxb.IDLE_UNNAMED, 0, 0, 8, d.data_ptr(), d.data_ptr()),
        lambda: db.find_idle(0, b.n, ENV, -1, 0, 8, d.data_ptr(), d.data_ptr()),
        lambda: db.find_idle(0, b.n + 1, ENV, 0, 0, 8, d.data_ptr(), d.data_ptr()),
        lambda: db.find_idle(0, b.n, ENV, 0, 0, 8, 0, d.data_ptr()),
        lambda: db.note_on_idle(note, 0, b.n, ENV | AMP, 0, 0, d.data_ptr(), d.data_ptr()),
        lambda: db.notes_on_list(make_notes(1, 0, 4), d.data_ptr(), d.data_ptr(), 0, d.data_ptr(), d.data_ptr()),
        lambda: db.notes_on_list(note, d.data_ptr(), d.data_ptr(), -1, d.data_ptr(), d.data_ptr()),
        lambda: db.stamp_list(d.data_ptr(), 4, fxb.DIRTY_PARAMS),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(device.SkredAmdError):
            call()
        assert (host_of(d) == -7).all(), k
    # the kinds NOT named are not checked: the bad delay line does not stop a pan update
    db.update(bad_line, [0, 1], fxb.DIRTY_PAN)
    model.apply_update(ref, bad_line, [0, 1], fxb.DIRTY_PAN, cnt)
    db.update(h, [], fxb.DIRTY_PARAMS)                     # an empty batch is fine
    cnt = block(db, ref, pool, cnt, 100, 1, "after the refusals")
    db.close()
