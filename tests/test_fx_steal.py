"""Voice stealing on the fixed-point bank on the GPU: skred_fxbank_find_steal / _find_steal_host / _note_on_steal.

The expectation is tests/fx_steal_model.py -- the definition of include/skred_amd_fxpt.h in numpy, exact -- evaluated on the ORACLE's
bank: oracle.cpuref.fx_render renders the blocks, tests/fx_live_model.py applies the stamps, updates and notes, and after every
block the device's downloaded state must equal the oracle's before a list is compared.  Lists and counts are compared byte for
byte; d_voices is pre-filled with -7 and entries past `written` must keep it.  Scenes and queries: tests/fx_steal_scenes.py
(tests/test_fx_steal_cpu.py shows that none is vacuous).
"""
import ctypes as C

import numpy as np
import pytest

import fx_live_model as live
import fx_steal_model as sm
import fx_steal_scenes as sc
from fx_steal_model import AMP, ENV, FIN, OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, STEAL_MAX, Query
from oracle import cpuref
from skred_amd import device, fxbank as fxb
from test_fx_live import block, dev_i32, host_of, make_notes, open_fx

pytestmark = pytest.mark.gpu

WHICH, SETTLE = FIN | ENV, 3


def reach(name):
    """(queried bank, oracle's bank, now) after the scene's blocks, the device's state checked against the oracle's on the way"""
    n, variant, make = sc.SCENES[name]
    b, pool, c0, truth, now, role, special = sc.scene(n, variant)
    db = open_fx(b, pool, c0)
    ref, cnt = b.copy(), c0
    for frames, interp in sc.FRAMES:
        cnt = block(db, ref, pool, cnt, frames, interp, name)
    assert cnt == now and not ref.rw_mismatch(truth)
    return db, ref, pool, cnt


def query(db, q, stream=0):
    import torch
    dv, dc = dev_i32(q.max_out + 8), dev_i32(2)
    torch.cuda.synchronize()
    db.find_steal(q.c(), dv.data_ptr() if q.max_out > 0 else 0, dc.data_ptr(), stream)
    torch.cuda.synchronize()
    return host_of(dv), host_of(dc)


def check(db, ref, now, q):
    want, total = sm.victims(ref, now, q)
    dv, dc = query(db, q)
    print(f"{q}: total {total}, written {want.size}")
    assert (int(dc[0]), int(dc[1])) == (want.size, total), f"{q}: d_count {dc.tolist()}, expected ({want.size}, {total})"
    assert np.array_equal(dv[:want.size], want), f"{q}: first mismatch at {int(np.flatnonzero(dv[:want.size] != want)[0])}"
    assert (dv[want.size:] == -7).all(), f"{q}: entries past `written` were touched"
    return dv, dc


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_fx_steal_scenes(name):
    db, ref, pool, now = reach(name)
    try:
        queries = sc.scene_queries(name)
        for q, _ in queries:
            check(db, ref, now, q)
        q = queries[0][0]
        a, b = query(db, q), query(db, q)                       # the same state gives the same bytes
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        for q, _ in queries[:4]:                                # the host form gives the same list as the device form
            want, total = sm.victims(ref, now, q)
            voices, tot = db.find_steal_host(q.c())
            assert tot == total and np.array_equal(voices, want), q
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- purity, stream order

def test_fx_query_reads_the_bank_only():
    """A bank queried between its blocks against an unqueried twin under note-offs: state, mix and master gain bit for bit."""
    import torch
    b, pool, c0, role, _ = sc.steal_bank(4096)
    db, twin = open_fx(b, pool, c0), open_fx(b, pool, c0)
    ref, cnt = b.copy(), c0
    rng = np.random.default_rng(5)
    outs = [torch.zeros((128, 2), dtype=torch.int64, device="cuda") for _ in range(2)]
    try:
        for k in range(4):
            off = np.sort(rng.choice(b.n, 40, replace=False)).astype(np.int32)
            for d in (db, twin):
                d.stamp(off, fxb.FX_STAMP_RELEASE)
            live.stamp(ref, off, fxb.STAMP_RELEASE, cnt)
            query(db, Query(0, b.n, OLDEST, RELEASED_FIRST, 10, FIN | ENV | AMP, SETTLE, STEAL_MAX))
            frames = (128, 100, 64, 1)[k]
            for d, o in zip((db, twin), outs):
                d.render_mix(frames, o.data_ptr(), k & 1)
            torch.cuda.synchronize()
            assert torch.equal(outs[0][:frames], outs[1][:frames]), f"block {k}: the query changed the mix"
            _, _, cnt = cpuref.fx_render(ref, pool, cnt, frames, k & 1)
            dv, dc = check(db, ref, cnt, Query(37, 3000, QUIETEST, RELEASED_ONLY, 0, FIN, 0, 50))
            assert dc[1] > 0
            query(db, Query(70, 40, max_out=0))
        a, c = b.copy(), b.copy()
        db.download(a)
        twin.download(c)
        assert not a.rw_mismatch(c) and not a.rw_mismatch(ref), (a.rw_mismatch(c), a.rw_mismatch(ref))
        assert db.master_gain() == twin.master_gain() and db.sample_count() == twin.sample_count() == cnt
    finally:
        db.close()
        twin.close()


def test_fx_stream_order_without_a_host_wait():
    """A release stamp, a query, a render and a second query on one stream, ONE synchronise at the end: the first list sees the
    release, the second one the block -- the short releases have run out, the long ones are 64 frames on."""
    import torch
    n, frames = 1000, 64
    b, pool, c0, role, _ = sc.steal_bank(n)
    b["sample_release"] = 0
    b["release_frames"][::32] = 32                           # these end inside the block
    db = open_fx(b, pool, c0)
    ref = b.copy()
    try:
        s = torch.cuda.Stream()
        q = Query(0, n, flags=RELEASED_ONLY, max_out=n)
        assert sm.victims(ref, c0, q)[1] == 0
        released = np.arange(0, n, 16, dtype=np.int32)
        dv = [dev_i32(n + 8) for _ in range(2)]
        dc = [dev_i32(2) for _ in range(2)]
        mix = torch.zeros((frames, 2), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        db.stamp(released, fxb.FX_STAMP_RELEASE, s.cuda_stream)
        db.find_steal(q.c(), dv[0].data_ptr(), dc[0].data_ptr(), s.cuda_stream)
        db.render(frames, mix.data_ptr(), 1, 0, s.cuda_stream)
        db.find_steal(q.c(), dv[1].data_ptr(), dc[1].data_ptr(), s.cuda_stream)
        s.synchronize()
        live.stamp(ref, released, fxb.STAMP_RELEASE, c0)
        first, t1 = sm.victims(ref, c0, q)
        want_mix, _, cnt = cpuref.fx_render(ref, pool, c0, frames, 1)
        second, t2 = sm.victims(ref, cnt, q)
        assert 0 < t2 < t1 and set(second) < set(first)
        assert (host_of(mix) == want_mix).all()
        for want, total, v, c in ((first, t1, dv[0], dc[0]), (second, t2, dv[1], dc[1])):
            got = host_of(v)
            assert host_of(c).tolist() == [want.size, total]
            assert np.array_equal(got[:want.size], want) and (got[want.size:] == -7).all()
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- note_on_steal

def idle_c(first, count, start, which=WHICH, settle=SETTLE):
    return fxb.FxIdleQueryC(first, count, which, settle, start, 0)


def joined_list(ref, now, idle, sq, k):
    """what note_on_steal places on: the idle list (room for k), then the victims as far as the batch reaches"""
    first, count, start = idle
    listed, _ = live.idle_list(ref, first, count, WHICH, SETTLE, start, k)
    victims, _ = sm.victims(ref, now, sq.but(exclude_idle=WHICH, settle_q15=SETTLE, max_out=min(k, STEAL_MAX)))
    joined = np.concatenate([listed, victims])[:k].astype(np.int32)
    return joined, listed, victims


@pytest.mark.parametrize("n", [1000, 4096])
def test_fx_note_on_steal_equals_the_host_path(n):
    """A batch larger than the idle list: `db` places it with note_on_steal; `twin` asks find_idle_host and find_steal_host, writes the
    notes into a host view and sends an update.  State, d_assigned, d_result and the following blocks are equal, and equal the model
    run through the oracle.  Then d_assigned ends the notes through stamp_list."""
    b, pool, c0, role, _ = sc.steal_bank(n)
    db, twin = open_fx(b, pool, c0), open_fx(b, pool, c0)
    ref, cnt = b.copy(), c0
    try:
        m_twin, _ = twin.render_host(65, 1)
        cnt = block(db, ref, pool, cnt, 65, 1, "before")
        idle, sq = (100, 120, 160), Query(3, n - 7, OLDEST, RELEASED_FIRST, 64)
        total_idle = live.idle_list(ref, *idle[:2], WHICH, SETTLE, idle[2])[1]
        k = total_idle + 37
        joined, listed, victims = joined_list(ref, cnt, idle, sq, k)
        assert 0 < listed.size == total_idle and joined.size == k and len(set(joined.tolist())) == k
        notes = make_notes(k, 5, fxb.NOTE_SET_PHASE | fxb.NOTE_SET_PAN)
        d_assigned, d_result = dev_i32(k + 8), dev_i32(3)
        db.note_on_steal(notes, idle_c(*idle), sq.but(exclude_idle=AMP, settle_q15=0, max_out=1).c(),      # those three are overridden
                         d_assigned.data_ptr(), d_result.data_ptr())
        want, counts = live.place_notes(ref, notes, joined, k, 0, cnt)
        assert host_of(d_result).tolist() == [k, 0, 37] and counts == (k, 0)
        got = host_of(d_assigned)
        assert np.array_equal(got[:k], want) and np.array_equal(want, joined) and (got[k:] == -7).all()
        assert np.array_equal(want[:total_idle], listed) and np.array_equal(want[total_idle:], victims[:37]), "idle first, then victims in victim order"
        # the twin: both lists on the host, the notes' values in the host view, an update
        t_idle, _ = twin.find_idle_host(idle[0], idle[1], WHICH, SETTLE, idle[2], k)
        t_victims, _ = twin.find_steal_host(sq.but(exclude_idle=WHICH, settle_q15=SETTLE, max_out=min(k, STEAL_MAX)).c())
        voices = np.concatenate([t_idle, t_victims])[:k].astype(np.int32)
        assert np.array_equal(voices, joined)
        h = b.copy()
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
        db.stamp_list(d_assigned.data_ptr(), k, fxb.STAMP_RELEASE)
        live.stamp(ref, want, fxb.STAMP_RELEASE, cnt)
        cnt = block(db, ref, pool, cnt, 64, 1, "released through stamp_list")
    finally:
        db.close()
        twin.close()


def test_fx_note_on_steal_counts_and_drops():
    """More notes than idle voices and victims together: the rest is dropped, d_assigned holds -1 for it, d_result is exact; a batch
    the idle list alone can hold steals nothing; an empty batch does nothing."""
    n = 1000
    b, pool, c0, role, _ = sc.steal_bank(n)
    db = open_fx(b, pool, c0)
    ref, cnt = b.copy(), c0
    try:
        cnt = block(db, ref, pool, cnt, 65, 1, "before")
        idle, sq = (100, 120, 160), Query(300, 40, QUIETEST, RELEASED_ONLY)
        d0a, d0r = dev_i32(8), dev_i32(3)
        db.note_on_steal([], idle_c(*idle), sq.c(), d0a.data_ptr(), d0r.data_ptr())
        assert (host_of(d0a) == -7).all() and (host_of(d0r) == -7).all(), "an empty batch wrote something"
        for idle, extra in (((100, 120, 160), 9), ((400, 120, 430), -5)):    # (the first burst uses its range's idle voices up)
            total_idle = live.idle_list(ref, *idle[:2], WHICH, SETTLE, idle[2])[1]
            n_victims = sm.victims(ref, cnt, sq.but(exclude_idle=WHICH, settle_q15=SETTLE, max_out=STEAL_MAX))[1]
            assert total_idle > 5 and (0 < n_victims < 40 or extra < 0)
            k = total_idle + n_victims + extra if extra > 0 else total_idle + extra
            joined, listed, victims = joined_list(ref, cnt, idle, sq, k)
            notes = make_notes(k, 7 + extra, fxb.NOTE_SET_PHASE)
            d_assigned, d_result = dev_i32(k + 8), dev_i32(3)
            db.note_on_steal(notes, idle_c(*idle), sq.c(), d_assigned.data_ptr(), d_result.data_ptr())
            want, counts = live.place_notes(ref, notes, joined, joined.size, 0, cnt)
            stolen = max(0, joined.size - listed.size)
            assert host_of(d_result).tolist() == [counts[0], counts[1], stolen]
            assert counts == ((k - extra, extra) if extra > 0 else (k, 0)) and stolen == (n_victims if extra > 0 else 0)
            got = host_of(d_assigned)
            assert np.array_equal(got[:k], want) and (got[k:] == -7).all()
            assert (want[joined.size:] == -1).all() and (want[:joined.size] == joined).all()
            cnt = block(db, ref, pool, cnt, 64, 1, f"after the batch of {k}")
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- refusals

def test_fx_steal_refusals_leave_the_bank_usable():
    n = 1000
    b, pool, c0, role, _ = sc.steal_bank(n)
    db = open_fx(b, pool, c0)
    ref, cnt = b.copy(), c0
    try:
        cnt = block(db, ref, pool, cnt, 65, 1, "before")
        d, note = dev_i32(16), make_notes(1, 0, 0)
        p = d.data_ptr()
        good, iq = Query(0, n, max_out=8), idle_c(0, n, 0)
        refused = [
            lambda: db.find_steal(good.but(policy=2).c(), p, p),
            lambda: db.find_steal(good.but(flags=fxb.STEAL_UNNAMED).c(), p, p),
            lambda: db.find_steal(good.but(exclude_idle=fxb.IDLE_UNNAMED).c(), p, p),
            lambda: db.find_steal(good.but(settle_q15=-1).c(), p, p),
            lambda: db.find_steal(good.but(max_out=STEAL_MAX + 1).c(), p, p),
            lambda: db.find_steal(good.but(count=n + 1).c(), p, p),
            lambda: db.find_steal(good.c(), 0, p),
            lambda: db.find_steal(good.c(), p, 0),
            lambda: db.find_steal_host(good.but(first=-1).c()),
            lambda: db.note_on_steal(note, idle_c(0, n, 0, which=ENV | AMP), good.c(), p, p),
            lambda: db.note_on_steal(note, idle_c(0, n, n), good.c(), p, p),
            lambda: db.note_on_steal(note, iq, good.but(policy=7).c(), p, p),
            lambda: db.note_on_steal(note, iq, good.but(flags=4).c(), p, p),
            lambda: db.note_on_steal(make_notes(1, 0, 4), iq, good.c(), p, p),
            lambda: db.note_on_steal(note, iq, good.c(), p, 0),
        ]
        for k, call in enumerate(refused):
            with pytest.raises(device.SkredAmdError):
                call()
            assert (host_of(d) == -7).all(), k
        reserved = good.c()
        reserved.reserved = 1
        with pytest.raises(device.SkredAmdError):
            db.find_steal(reserved, p, p)
        cnt = block(db, ref, pool, cnt, 100, 1, "after the refusals")
        check(db, ref, cnt, good)
    finally:
        db.close()
