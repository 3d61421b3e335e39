"""Slot stealing on the device (skred_bank_find_steal_slots / _find_steal_slots_host / _note_on_steal_slots).

Every list is compared byte for byte with tests/slot_steal_model.py, computed twice: on the ORACLE's bank after cpuref.render of the
same blocks, and on the download of a TWIN bank that was never queried (DeviceBank.download returns the read-write fields; the
envelope clocks, which only stamps change, are the oracle's).  d_slots is pre-filled with -1; entries past `written` must stay -1.
The scenes are tests/slot_steal_scenes.py's; tests/test_slot_steal_cpu.py asserts on the oracle's state that none is vacuous, and
that the hand-made scenes below (wide keys, ties, ages) do what they are for.
"""
import ctypes as C

import numpy as np
import pytest

import slot_model as SM
import slot_steal_model as M
import slot_steal_scenes as S
import steal_model as sm
from oracle import cpuref
from skred_amd import banks, device
from skred_amd.bank import slot_query
from slot_scenes import masks
from steal_model import OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, STEAL_MAX, FIN, ENV, AMP, UNNAMED
from test_idle import open_bank, render_blocks, traffic_bank

DIRTY_PARAMS, DIRTY_PHASE = 1, 2
REL, TRIG = SM.STAMP_RELEASE, SM.STAMP_TRIGGER
BAD, RANGE = -2, -4
WHICH = FIN | ENV


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


# ---------------------------------------------------------------------------------------------- hand-made scenes (no block needed)

def plain_bank(n, now=None):
    """bank_c2, every voice enveloped and sustaining since long ago."""
    bank, tables, g = banks.bank_c2(n)
    if now is not None:
        g.synth_sample_count = now
    now = int(g.synth_sample_count)
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][:] = 1
    e["is_active"] = 1
    e["sample_start"] = np.uint64(now - 3000)
    e["sample_release"] = np.uint64(0)
    return bank, tables, g, now


def wide_scene():
    """Starts that differ only above bit 32, only in bit 0, and two at or above 2^62 -- every one of them held by a member that is NOT
    its slot's first voice, the other members of those slots started at 5.  Slot 10 holds one member at (high word 1, low word 5) and
    one at (0, 777): a butterfly that took the maximum of the two words independently would make it 2^32 + 777 and rank it behind
    slot 11 (2^32 + 400)."""
    n, K = 320, 8
    bank, tables, g, now = plain_bank(n, (1 << 33) + 12345)
    st = bank["voice_amp_envelope"]["sample_start"]
    special = {0: 777, 3: 777, 1: 777 + (1 << 32), 4: 777 + (1 << 32), 2: 777 + (2 << 32), 5: 777 + (2 << 32), 6: 4001, 7: 4000,
               8: (1 << 62) + 9, 9: 1 << 62}
    for s, value in special.items():
        st[s * K:(s + 1) * K] = np.uint64(5)
        st[s * K + 1 + s % 7] = np.uint64(value)
    st[10 * K:12 * K] = np.uint64(5)
    st[10 * K + 3], st[10 * K + 5], st[11 * K + 6] = np.uint64((1 << 32) + 5), np.uint64(777), np.uint64((1 << 32) + 400)
    facts = dict(expect_head=[s * K for s in (0, 3, 7, 6, 10, 11, 1, 4, 2, 5)], saturated=[8 * K, 9 * K], tables=tables, g=g)
    return bank, now, M.SlotQuery(0, n, K, 0xFF, max_out=n // K), facts


def ties_scene():
    """Every slot of seventeen workgroups has the same key: the list is the first voices in index order, however short."""
    n, K = 4160, 2
    bank, tables, g, now = plain_bank(n)
    ties_scene.rest = (tables, g)
    return bank, now, M.SlotQuery(0, n, K, 3, max_out=STEAL_MAX)


def age_scene():
    n, K, mask = 320, 8, 0x55
    bank, tables, g, now = plain_bank(n)
    e = bank["voice_amp_envelope"]
    e["sample_start"][:] = np.uint64(now - 5000)
    a, b = 3 * K, 5 * K
    e["sample_start"][a + 2] = np.uint64(now + 100000)        # a member stamped ahead of the clock: age 0
    e["sample_start"][b + 6] = np.uint64(now - 700)           # the youngest LIVE member of slot b
    e["sample_start"][b + 7] = np.uint64(now - 3)             # outside the mask
    e["sample_start"][b + 4] = np.uint64(now - 1)             # a member, but not live
    e["is_active"][b + 4] = 0
    return bank, now, M.SlotQuery(0, n, K, mask, max_out=n // K), dict(ahead_slot=a, slot=b, age=700, tables=tables, g=g)


# ---------------------------------------------------------------------------------------------- the list

def run_query(db, q, stream=0):
    import torch
    dv = torch.full((q.max_out + 8,), -1, dtype=torch.int32, device="cuda")
    dc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    db.find_steal_slots(q.c(), dv.data_ptr(), dc.data_ptr(), stream)
    torch.cuda.synchronize()
    return dv.cpu().numpy(), dc.cpu().numpy()


def check(db, truth, got, now, q):
    want = M.victim_slots(truth, now, q)
    if got is not None:
        assert np.array_equal(want, M.victim_slots(got, now, q)), "the oracle's state and the twin's downloaded state disagree"
    dv, dc = run_query(db, q)
    total, written = len(want), min(len(want), q.max_out)
    print(f"{q}: total {total}, written {written}")
    assert (int(dc[0]), int(dc[1])) == (written, total), f"{q}: d_count {dc.tolist()}, expected ({written}, {total})"
    assert np.array_equal(dv[:written], want[:written]), f"{q}: first mismatch at {int(np.flatnonzero(dv[:written] != want[:written])[0])}"
    assert (dv[written:] == -1).all(), f"{q}: entries past `written` were touched"
    return want


def reach(dev, n, K, mask):
    bank, tables, g, truth, now, kind = S.scene(n, K, mask)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    render_blocks(db, S.FRAMES)
    render_blocks(twin, S.FRAMES)
    got = truth.copy()
    twin.download(got)
    twin.close()
    assert not got.rw_equal(truth), got.rw_equal(truth)
    return db, truth, got, now


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,name", S.FULL_CASES + S.SMALL_CASES)
def test_scenes(dev, n, K, name):
    mask = masks(K)[name]
    db, truth, got, now = reach(dev, n, K, mask)
    try:
        qs = S.queries(n, K, mask) + S.threshold_queries(truth, now, n, K, mask)
        for q in qs:
            check(db, truth, got, now, q)
        a, b = run_query(db, qs[1]), run_query(db, qs[1])             # the same state gives the same bytes
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        q = qs[0].but(max_out=3)
        slots, total = db.find_steal_slots_host(q.c())                # the host form waits for the stream only
        want = M.victim_slots(truth, now, q)
        assert total == len(want) and np.array_equal(slots, want[:3])
    finally:
        db.close()


@pytest.mark.gpu
def test_a_range_off_the_64_boundaries(dev):
    n, K, mask, first, count = S.UNALIGNED
    db, truth, got, now = reach(dev, n, K, mask)
    try:
        for q in S.queries(n, K, mask, first, count) + S.threshold_queries(truth, now, n, K, mask, first, count):
            want = check(db, truth, got, now, q)
            assert all(first <= h < first + count for h in want)
        check(db, truth, got, now, M.SlotQuery(312, 8, K, mask, max_out=4))          # one slot
    finally:
        db.close()


def upload(dev, bank, tables, g):
    return open_bank(dev, bank, tables, g)


@pytest.mark.gpu
def test_ties_across_workgroups(dev):
    bank, now, q = ties_scene()
    db = upload(dev, bank, *ties_scene.rest)
    try:
        for mo in (STEAL_MAX, 1):
            want = check(db, bank, None, now, q.but(max_out=mo))
            assert len(want) == 4160 // 2
        check(db, bank, None, now, q.but(flags=RELEASED_FIRST, policy=QUIETEST, max_out=700))
    finally:
        db.close()


@pytest.mark.gpu
def test_keys_are_64_bits_wide(dev):
    bank, now, q, facts = wide_scene()
    db = upload(dev, bank, facts["tables"], facts["g"])
    try:
        want = check(db, bank, None, now, q)
        assert want[:len(facts["expect_head"])].tolist() == facts["expect_head"] and want[-2:].tolist() == facts["saturated"]
        for mo in (1, 2, 3, 5, 7, 9):                                     # thresholds inside the runs that differ in high words only
            check(db, bank, None, now, q.but(max_out=mo))
        check(db, bank, None, now, q.but(flags=RELEASED_FIRST))
    finally:
        db.close()


@pytest.mark.gpu
def test_ages(dev):
    bank, now, q, facts = age_scene()
    db = upload(dev, bank, facts["tables"], facts["g"])
    try:
        assert check(db, bank, None, now, q)[-1] == facts["ahead_slot"]
        assert facts["ahead_slot"] not in check(db, bank, None, now, q.but(min_age=1))
        for d, inside in ((0, True), (-1, True), (1, False)):
            assert (facts["slot"] in check(db, bank, None, now, q.but(min_age=facts["age"] + d))) == inside
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- K = 1: the voice calls

@pytest.mark.gpu
def test_one_voice_slots_are_the_voice_calls(dev):
    """With K = 1, mask 1: find_steal_slots writes the bytes of find_steal, note_on_steal_slots those of note_on_steal -- lists,
    counts, d_assigned, d_result, the state and the mix of the next blocks -- on twin banks."""
    import torch
    import test_steal as TS
    from test_notes import make_notes, same_mix, same_state, store_notes
    n, F, count = 1000, 256, 16
    bank, tables, g = TS.varied_traffic_bank(n)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    truth, gl = bank.copy(), g.copy()
    try:
        for d in (db, twin):
            render_blocks(d, (F,))
        cpuref.render(truth, gl, tables, F, 0)
        now = int(gl.synth_sample_count)
        ran = 0
        for policy in (OLDEST, QUIETEST):
            for flags in (0, RELEASED_FIRST, RELEASED_ONLY):
                for ex in (0, WHICH):
                    for first, cnt, mo in ((0, n, STEAL_MAX), (37, 300, 40), (0, n, 1), (5, 900, 0)):
                        q = M.SlotQuery(first, cnt, 1, 1, policy, flags, 10, ex, 1e-3, mo)
                        sv, sc = run_query(db, q)
                        vv = torch.full((mo + 8,), -1, dtype=torch.int32, device="cuda")
                        vc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
                        torch.cuda.synchronize()
                        twin.find_steal(q.voice().c(), vv.data_ptr(), vc.data_ptr())
                        torch.cuda.synchronize()
                        assert sv.tobytes() == vv.cpu().numpy().tobytes() and sc.tobytes() == vc.cpu().numpy().tobytes(), q
                        assert np.array_equal(sv[:sc[0]], sm.victim_order(truth, now, q.voice())[:mo])
                        ran += sc[1] > 0
        assert ran > 20
        notes = make_notes(count, 4)
        vq = sm.Query(0, n, OLDEST, RELEASED_FIRST, min_age=1)
        sq = M.SlotQuery(0, n, 1, 1, OLDEST, RELEASED_FIRST, min_age=1)
        outs = []
        for d, call in ((db, lambda a, r: db.note_on_steal_slots(notes, slot_query(3, 7, 1, 1, WHICH, 1e-3, 3, 0), sq.c(), 1, a, r)),
                        (twin, lambda a, r: twin.note_on_steal(notes, device.IdleQueryC(3, 7, WHICH, 1e-3, 3, 0), vq.c(), a, r))):
            da = torch.full((count + 8,), -7, dtype=torch.int32, device="cuda")
            dr = torch.full((3,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            call(da.data_ptr(), dr.data_ptr())
            torch.cuda.synchronize()
            outs.append((da.cpu().numpy(), dr.cpu().numpy()))
        assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes(), outs
        picks, res = outs[0][0][:count], outs[0][1]
        assert res[0] == count and 0 < res[2] < count, res
        store_notes((truth,), truth, notes, picks, now)
        for k in range(2):
            same_mix(db, twin, F, f"block {k}")
            cpuref.render(truth, gl, tables, F, 0)
        same_state(db, twin, truth, bank, "K = 1")
        assert db.last_kernel() == twin.last_kernel()
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- purity, stream order

@pytest.mark.gpu
def test_query_reads_the_bank_only(dev):
    n, K, mask, F = 1088, 8, 0x55, 128
    bank, tables, g, truth, now, kind = S.scene(n, K, mask)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    try:
        for k in range(4):
            x, y = render_blocks(db, (F,))[0], render_blocks(twin, (F,))[0]
            assert x.tobytes() == y.tobytes(), f"block {k}: the query changed the mix"
            assert db.last_kernel() == twin.last_kernel() and db.last_pack() == twin.last_pack()
            dv, dc = run_query(db, M.SlotQuery(0, n, K, mask, QUIETEST, RELEASED_FIRST, 10, WHICH, 1e-3, STEAL_MAX))
            assert dc[1] > 0
            run_query(db, M.SlotQuery(24, 296, K, mask, max_out=0))
        a, b = bank.copy(), bank.copy()
        db.download(a)
        twin.download(b)
        assert not a.rw_equal(b), a.rw_equal(b)
        ga, gb = db.get_globals(), twin.get_globals()
        assert ga.synth_sample_count == gb.synth_sample_count and ga.noise_rng == gb.noise_rng
    finally:
        db.close()
        twin.close()


@pytest.mark.gpu
def test_stream_order_without_a_host_wait(dev):
    """A release through skred_bank_stamp_slots and the query behind it on one stream, nothing waited for in between."""
    import torch
    bank, now, q, facts = age_scene()
    n, K, mask = bank.n, q.K, q.mask
    db = upload(dev, bank, facts["tables"], facts["g"])
    try:
        q = q.but(flags=RELEASED_ONLY)
        assert len(M.victim_slots(bank, now, q)) == 0
        released = np.array([8, 5 * K, 128, 312], np.int32)
        s = torch.cuda.Stream()
        dl = torch.from_numpy(released).cuda()
        dv = torch.full((q.max_out + 8,), -1, dtype=torch.int32, device="cuda")
        dc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        db.stamp_slots(dl.data_ptr(), len(released), K, mask, REL, 0, s.cuda_stream)
        db.find_steal_slots(q.c(), dv.data_ptr(), dc.data_ptr(), s.cuda_stream)
        s.synchronize()
        truth = bank.copy()
        SM.stamp(truth, SM.stamp_voices(released, len(released), None, K, mask, n), REL, now)
        want = M.victim_slots(truth, now, q)
        assert sorted(want.tolist()) == sorted(released.tolist())
        got, cnt = dv.cpu().numpy(), dc.cpu().numpy()
        assert cnt.tolist() == [len(want), len(want)] and np.array_equal(got[:len(want)], want) and (got[len(want):] == -1).all()
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- note_on_steal_slots

def playing_patch(patch, n, members):
    """bank_patch with envelopes on the `members` of every copy: every fourth copy released so that it comes to rest inside the
    first blocks, the others sounding -- held since staggered times, every third of them in a release that does not end."""
    bank, tables, g = banks.bank_patch(patch, n)
    K = {"3sk": 4, "18sk": 16}[patch]
    now = int(g.synth_sample_count)
    v = np.arange(n)
    copy = v // K
    sel = np.isin(v % K, members)
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel] = np.float32(20.0), np.float32(50.0)
    e["sustain_level"][sel], e["release_time"][sel] = np.float32(0.6), np.float32(1e6)
    e["velocity"][sel] = np.float32(1.0)
    e["is_active"][sel] = 1
    e["sample_start"][sel] = (now - 40000 - (copy[sel] * 37) % 1000 - (v[sel] % K)).astype(np.uint64)
    e["sample_release"][sel] = np.uint64(0)
    lingering = sel & (copy % 4 != 0) & (copy % 3 == 0)
    e["sample_release"][lingering] = (now - 2000 + (copy[lingering] * 11) % 500).astype(np.uint64)
    ending = sel & (copy % 4 == 0)
    e["sample_release"][ending] = np.uint64(now - 50)
    e["release_time"][ending] = np.float32(100.0)
    bank["voice_smoother_smoothing"][sel] = np.float32(0.5)
    return bank, tables, g, K


def patch_notes(count, K, vmask, seed):
    from test_slots import slot_notes
    return slot_notes(count, K, vmask, seed, [SM.SET_PHASE, SM.SET_PHASE | SM.SET_PAN])


def model_burst(truth, now, iq, sq, count):
    """(d_assigned, (placed, dropped, stolen)) of a burst, from the two models."""
    idle = SM.idle_slots(truth, iq.first, iq.count, iq.slot_voices, iq.member_mask, iq.which, iq.settle_level, iq.start)[:count]
    q = sq.but(exclude_idle=iq.which, settle_level=float(iq.settle_level), max_out=min(count, STEAL_MAX))
    victims = M.victim_slots(truth, now, q)[:q.max_out]
    assert not set(idle.tolist()) & set(victims.tolist())
    joined = np.concatenate([idle, victims]).astype(np.int32)[:count]
    out = np.full(count, -1, np.int32)
    out[:len(joined)] = joined
    return out, (len(joined), count - len(joined), len(joined) - len(idle)), len(idle), len(victims)


@pytest.mark.gpu
@pytest.mark.parametrize("patch,members,voices", [("3sk", (0, 1, 2), (0, 1, 2, 3)), ("18sk", (0, 10), (0, 1, 2, 10))])
def test_bursts_on_a_tiled_patch(dev, patch, members, voices):
    """Bursts below, at and above the idle count, above idle + candidates (notes are dropped) and with no idle slot at all.  d_result
    and d_assigned are the model's; state, stems and mix after every burst's blocks are those of the host route on a twin
    (find_idle_slots_host + find_steal_slots_host + skred_bank_update) and of the oracle."""
    import torch
    n, F = 512, 64
    bank, tables, g, K = playing_patch(patch, n, members)
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
            a, b = bank.copy(), bank.copy()
            db.download(a)
            twin.download(b)
            assert not a.rw_equal(truth), f"{tag} {i}: state differs from the oracle: {a.rw_equal(truth)}"
            assert not a.rw_equal(b), a.rw_equal(b)
            assert db.last_kernel() == twin.last_kernel() and db.last_pack() == twin.last_pack()

    try:
        blocks(4, "to rest")
        # every range of 8 copies holds 2 idle ones (every fourth copy); the steal range holds 6 sounding ones -- and what earlier
        # bursts placed there
        r0, r1, r2, one, narrow = (0, 8 * K), (8 * K, 8 * K), (16 * K, 8 * K), (K, K), (0, 8 * K)
        seen = set()
        for i, (irange, srange, count, policy, flags) in enumerate(((r0, narrow, 1, OLDEST, RELEASED_FIRST), (r0, narrow, None, QUIETEST, 0),
                                                                   (r1, narrow, "+3", OLDEST, RELEASED_FIRST), (r2, narrow, "all+2", OLDEST, 0),
                                                                   (one, narrow, 3, OLDEST, RELEASED_FIRST))):
            now = int(gl.synth_sample_count)
            iq = slot_query(irange[0], irange[1], K, mmask, WHICH, 1e-3, irange[0], 0)
            sq = M.SlotQuery(srange[0], srange[1], K, mmask, policy, flags, max_out=5)
            n_idle = len(SM.idle_slots(truth, irange[0], irange[1], K, mmask, WHICH, 1e-3))
            n_cand = len(M.victim_slots(truth, now, sq.but(exclude_idle=WHICH, settle_level=1e-3)))
            count = n_idle if count is None else n_idle + 3 if count == "+3" else n_idle + n_cand + 2 if count == "all+2" else count
            want, counts, got_idle, got_victims = model_burst(truth, now, iq, sq, count)
            kind = ("below" if count < n_idle else "at" if count == n_idle else "dropped" if counts[1] else "stolen") if n_idle else "no idle"
            seen.add(kind)
            print(f"burst {i}: {count} notes, {n_idle} idle, {n_cand} candidates -> {counts} ({kind})")
            notes = patch_notes(count, K, vmask, i)
            da = torch.full((count + 8,), -7, dtype=torch.int32, device="cuda")
            dr = torch.full((3,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            db.note_on_steal_slots(notes, iq, sq.c(), vmask, da.data_ptr(), dr.data_ptr())
            iq.max_out = count
            idle, _ = twin.find_idle_slots_host(iq)
            victims, _ = twin.find_steal_slots_host(sq.but(exclude_idle=WHICH, settle_level=1e-3, max_out=min(count, STEAL_MAX)).c())
            picks = np.full(count, -1, np.int32)
            joined = np.concatenate([idle, victims]).astype(np.int32)[:count]
            picks[:len(joined)] = joined
            assert np.array_equal(picks, want), (picks, want)
            touched = SM.store_notes((truth, mirror), truth, notes, K, vmask, picks, now)
            twin.update(mirror, touched, DIRTY_PARAMS | DIRTY_PHASE | 8 | TRIG)
            blocks(2, f"burst {i}")
            got, res = da.cpu().numpy(), dr.cpu().numpy()
            assert np.array_equal(got[:count], want) and (got[count:] == -7).all(), (got.tolist(), want.tolist())
            assert tuple(res.tolist()) == counts, (res.tolist(), counts)
        assert seen == {"below", "at", "stolen", "dropped", "no idle"}, seen
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- the in-place rule

@pytest.mark.gpu
def test_two_per_lane_in_place_after_a_stolen_chord(dev):
    """tests/test_slots.py's bank and bound (4096 voices, two per lane, SKRED_OPT_IN_PLACE = 2: the list is rendered in place while
    the proven bound stays at or below 4096 / 6 + 64 = 746 voices).  member_mask 0x01 is the voice of every slot that sounds on, so
    no slot is idle and every note is stolen; voice_mask 0xFE: a note touches 7 voices.  A chord of 2 (14 voices) stays in place, a
    chord of 110 (770 voices; 110 itself is far below 746) must leave it; both as the host route decides."""
    import torch
    from test_slots import slot_notes
    n, K, F, BIG, SMALL = 4096, 8, 256, 110, 2
    mmask, vmask = 0x01, 0xFE
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    db, twin = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    truth, gl, mirror = bank.copy(), g.copy(), bank.copy()
    chords = {3: (SMALL, True), 6: (BIG, False)}
    taken = []
    try:
        for k in range(8):
            expect = None
            if k in chords:
                count, expect = chords[k]
                now = int(gl.synth_sample_count)
                iq = slot_query(0, n, K, mmask, WHICH, 1e-3, 0, 0)
                sq = M.SlotQuery(0, n, K, mmask, OLDEST, 0)
                want, counts, n_idle, _ = model_burst(truth, now, iq, sq, count)
                assert n_idle == 0 and counts == (count, 0, count)
                notes = slot_notes(count, K, vmask, k)
                da = torch.full((count + 8,), -7, dtype=torch.int32, device="cuda")
                dr = torch.full((3,), -7, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                db.note_on_steal_slots(notes, iq, sq.c(), vmask, da.data_ptr(), dr.data_ptr())
                picks, _ = twin.find_steal_slots_host(sq.but(exclude_idle=WHICH, settle_level=1e-3, max_out=count).c())
                assert np.array_equal(picks, want)
                touched = SM.store_notes((truth, mirror), truth, notes, K, vmask, picks, now)
                assert len(touched) == count * 7
                twin.update(mirror, touched, DIRTY_PARAMS | DIRTY_PHASE | TRIG)
            x, y = render_blocks(db, (F,))[0], render_blocks(twin, (F,))[0]
            cpuref.render(truth, gl, tables, F, 0)
            taken.append((db.last_in_place(), twin.last_in_place()))
            assert db.last_kernel() == twin.last_kernel() == 3
            assert taken[-1][0] == taken[-1][1], f"block {k}: in place on one route only: {taken}"
            if expect is not None:
                assert taken[-1][0] is expect, f"block {k}: in place {taken[-1][0]}, expected {expect}: {taken}"
                assert np.array_equal(da.cpu().numpy()[:count], want) and dr.cpu().numpy().tolist() == [count, 0, count]
            assert x.tobytes() == y.tobytes(), f"block {k}: the mixes differ"
            a = bank.copy()
            db.download(a)
            assert not a.rw_equal(truth), a.rw_equal(truth)
            assert db.list_violations() == twin.list_violations() == 0
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_write_nothing(dev):
    import torch
    import test_slot_steal_cpu as CPU
    from test_slots import slot_notes
    n, K, mask = 1024, 8, 0x55
    bank, tables, g, now = plain_bank(n)
    db = upload(dev, bank, tables, g)
    try:
        L = db.L
        dv = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        dc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        da = torch.full((16,), -1, dtype=torch.int32, device="cuda")
        dr = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        count = 4
        p = C.cast(device.note_array(slot_notes(count, K, mask, 1, junk=False)), C.c_void_p)
        torch.cuda.synchronize()

        def on(h=db.h, nt=p, cnt=count, vm=mask, res=dr.data_ptr(), sq=None, **kw):
            args = dict(first=0, count=n, slot_voices=K, member_mask=mask, which=WHICH, settle_level=0.0, start=None, max_out=-5)
            args.update(kw)
            iq = slot_query(**args)
            sq = CPU.good() if sq is None else sq
            return L.skred_bank_note_on_steal_slots(h, C.byref(iq), C.byref(sq), nt, cnt, vm, da.data_ptr(), res or None, None)

        for case, (_, code) in CPU.REFUSED.items():
            q = CPU.refused_query(case)
            assert L.skred_bank_find_steal_slots(db.h, C.byref(q), dv.data_ptr(), dc.data_ptr(), None) == code, case
            host = np.full(STEAL_MAX, -1, np.int32)
            assert L.skred_bank_find_steal_slots_host(db.h, C.byref(q), host.ctypes.data, None, None) == code, case
            if not case.startswith(("exclude", "max_out", "settle")):              # (the library overrides those three fields)
                assert on(sq=q) == code, case
        gq = CPU.good()
        assert L.skred_bank_find_steal_slots(db.h, C.byref(gq), None, dc.data_ptr(), None) == BAD      # max_out > 0 and no list
        assert L.skred_bank_find_steal_slots(db.h, C.byref(gq), dv.data_ptr(), None, None) == BAD
        assert L.skred_bank_find_steal_slots(None, C.byref(gq), dv.data_ptr(), dc.data_ptr(), None) == BAD
        # the two queries must agree on K and on the mask
        assert on(sq=CPU.good(slot_voices=4, member_mask=0x5)) == BAD and on(sq=CPU.good(member_mask=0x15)) == BAD
        assert on(slot_voices=16) == BAD and on(member_mask=0xFF) == BAD
        assert on(sq=CPU.good(first=8, count=64)) == 0                               # ranges may differ
        torch.cuda.synchronize()
        assert (dr.cpu().numpy() != -1).all()
        dr.fill_(-1)
        da.fill_(-1)
        torch.cuda.synchronize()
        assert on(which=WHICH | AMP) == BAD and on(which=AMP) == BAD and on(which=ENV | UNNAMED) == BAD and on(which=0) == BAD
        assert on(h=None) == BAD and on(nt=None) == BAD and on(res=0) == BAD and on(cnt=-1) == BAD
        assert on(vm=0) == BAD and on(vm=0x100) == BAD and on(first=4) == RANGE and on(count=n + 8) == RANGE
        bad = slot_notes(count, K, mask, 1, junk=False)
        bad[K + 2] = device.NoteC(float("nan"), 1.0, 0.0, 0.5, 0.5, 0)             # a masked position (bit 2)
        assert on(nt=C.cast(device.note_array(bad), C.c_void_p)) == BAD
        assert on(cnt=0) == 0
        torch.cuda.synchronize()
        for t in (dv, dc, da, dr):
            assert (t.cpu().numpy() == -1).all()                                   # nothing reached the device
        truth = bank.copy()
        SM.store_notes((), truth, slot_notes(count, K, mask, 1, junk=False), K, mask, M.victim_slots(bank, now, M.SlotQuery(8, 64, K, mask))[:count], now)
        check(db, truth, None, now, M.SlotQuery(0, n, K, mask, max_out=40))         # ... and the bank still answers
    finally:
        db.close()
