"""Channel polyphony on the device (skred_bank_find_steal_slots_match / _match_host / _note_on_channel).

Every list and count is compared byte for byte with tests/chan_model.py on the ORACLE's state plus a numpy owner array (the device's
owner words are put there with skred_bank_tag_slots and read back with download_owners).  d_slots is pre-filled with -1; entries past
`written` must stay -1.  The scenes are tests/chan_scenes.py's on the banks of tests/slot_steal_scenes.py; tests/test_chan_cpu.py
asserts on the oracle's state that none is vacuous and that the burst script shows every kind.
"""
import ctypes as C

import numpy as np
import pytest

import chan_model as CM
import chan_scenes as CS
import slot_model as SM
import slot_steal_model as M
import slot_steal_scenes as S
from oracle import cpuref
from skred_amd import device
from skred_amd.bank import slot_query
from steal_model import OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, STEAL_MAX, FIN, ENV, AMP
from test_idle import open_bank, render_blocks, traffic_bank

DIRTY_PARAMS, DIRTY_PHASE = 1, 2
TRIG = SM.STAMP_TRIGGER
BAD, RANGE = -2, -4
WHICH = FIN | ENV


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def set_owners(db, own, K):
    """The device's owner words := own's words at the first voices (zero tags included), through skred_bank_tag_slots."""
    import torch
    heads = np.arange(0, len(own) - len(own) % K, K).astype(np.int32)
    dl = torch.from_numpy(heads).cuda()
    torch.cuda.synchronize()
    db.tag_slots(dl.data_ptr(), own[heads], K)
    torch.cuda.synchronize()
    got = db.download_owners()
    assert np.array_equal(got[heads], own[heads])


def run_query(db, q, match, stream=0):
    import torch
    dv = torch.full((q.max_out + 8,), -1, dtype=torch.int32, device="cuda")
    dc = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    db.find_steal_slots_match(q.c(), device.owner_match(*match), dv.data_ptr(), dc.data_ptr(), stream)
    torch.cuda.synchronize()
    return dv.cpu().numpy(), dc.cpu().numpy()


def check(db, truth, now, q, own, match):
    want, counts = CM.query(truth, now, q, own, match)
    dv, dc = run_query(db, q, match)
    written = counts[0]
    print(f"{q} {match}: {counts}")
    assert dc[:3].tolist() == counts and dc[3] == -1, f"{q} {match}: d_count {dc.tolist()}, expected {counts}"
    assert np.array_equal(dv[:written], want), f"{q} {match}: first mismatch at {int(np.flatnonzero(dv[:written] != want)[0])}"
    assert (dv[written:] == -1).all(), f"{q} {match}: entries past `written` were touched"
    return want, counts


def reach(dev, n, K, mask):
    bank, tables, g, truth, now, kind = S.scene(n, K, mask)
    db = open_bank(dev, bank, tables, g)
    render_blocks(db, S.FRAMES)
    got = truth.copy()
    db.download(got)
    assert not got.rw_equal(truth), got.rw_equal(truth)
    return db, truth, now


def scene_queries(first, count, K, mask):
    base = M.SlotQuery(first, count, K, mask, max_out=STEAL_MAX)
    ex = dict(exclude_idle=S.EXCLUDE, settle_level=float(S.SETTLE))
    return [base, base.but(policy=QUIETEST, flags=RELEASED_FIRST, **ex), base.but(flags=RELEASED_ONLY, min_age=S.MIN_AGE, **ex),
            base.but(flags=RELEASED_FIRST | RELEASED_ONLY, policy=QUIETEST), base.but(min_age=S.MIN_AGE, max_out=1, **ex),
            base.but(max_out=0, **ex), base.but(max_out=0, flags=RELEASED_ONLY), base.but(max_out=1, flags=RELEASED_FIRST)]


# ---------------------------------------------------------------------------------------------- the query

@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 8, 64])
def test_query_scenes(dev, K):
    """Banks of 1 500 voices: the whole bank, a range off the 64-voice boundaries, a range that starts at 256 - K and spans two
    workgroups; every match of the scene; max_out 0, 1 and 1 024; mask 0 with everything tagged against find_steal_slots."""
    import torch
    n, mask = 1500, (1 << K) - 1
    whole = n - n % K
    db, truth, now = reach(dev, n, K, mask)
    try:
        own = CS.owners(n, K)
        set_owners(db, own, K)
        off = ((24 + K - 1) // K * K, 296 // K * K) if K < 64 else (64, 320)
        ranges = [(0, whole), off, (256 - K, 2 * K), (256 - K, 256 + K)]     # (the last: 256 - K .. 512, across the span edge at 448)
        ran = 0
        for first, count in ranges:
            for q in scene_queries(first, count, K, mask):
                for match in CS.matches(own, K):
                    want, counts = check(db, truth, now, q, own, match)
                    assert all(first <= h < first + count for h in want)
                    ran += counts[2] > counts[1]
        assert ran > 10, "no query told the sounding count from the candidates"
        q = scene_queries(0, whole, K, mask)[1]
        a, b = run_query(db, q, CM.channel(CS.A)), run_query(db, q, CM.channel(CS.A))    # the same state gives the same bytes
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        nobody, counts = check(db, truth, now, q, own, CM.channel(77))
        assert len(nobody) == 0 and counts == [0, 0, 0]
        slots, total, sounding = db.find_steal_slots_match_host(q.but(max_out=3).c(), device.owner_match(*CM.channel(CS.B)))
        want, counts = CM.query(truth, now, q.but(max_out=3), own, CM.channel(CS.B))
        assert np.array_equal(slots, want) and [len(slots), total, sounding] == counts
        # mask 0, every slot tagged: the bytes of find_steal_slots
        set_owners(db, np.full(n, 5, np.uint32), K)
        for q in scene_queries(0, whole, K, mask) + scene_queries(*off, K, mask):
            dv, dc = run_query(db, q, (0, 0))
            pv = torch.full((q.max_out + 8,), -1, dtype=torch.int32, device="cuda")
            pc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            db.find_steal_slots(q.c(), pv.data_ptr(), pc.data_ptr())
            torch.cuda.synchronize()
            assert dv.tobytes() == pv.cpu().numpy().tobytes() and dc[:2].tobytes() == pc.cpu().numpy().tobytes(), q
            assert dc[2] >= dc[1]
    finally:
        db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 4, 64])
def test_matched_key_pass_with_mask_zero_is_the_plain_one(dev, K):
    """The two instantiations of the slot key pass on one bank of 600 voices, every slot tagged, match (0, 0): the list and the first
    two count words are find_steal_slots's bytes.  The range starts off a 64-voice boundary (K = 64, whose slots are 64-aligned:
    at voice 64, which moves the span edge to 320) and crosses a 256-voice workgroup span with sounding slots on both sides, so two workgroups add to
    the sounding word and the last arriver publishes it; each matched query runs twice in a row on one stream with no host wait
    between the two: the second starts from a re-armed word."""
    import torch
    n, mask = 600, (1 << K) - 1
    first = {1: 37, 4: 36, 64: 64}[K]
    count = (n - n % K) - first
    edge = (first & ~63) + 256                                                   # where the second workgroup's span begins
    db, truth, now = reach(dev, n, K, mask)
    try:
        own = np.full(n, 5, np.uint32)
        set_owners(db, own, K)
        for policy, flags in ((OLDEST, 0), (QUIETEST, RELEASED_ONLY)):           # (RELEASED_ONLY: fewer candidates than sounding slots)
            for max_out in (0, 5):
                q = M.SlotQuery(first, count, K, mask, policy=policy, flags=flags, max_out=max_out, exclude_idle=S.EXCLUDE,
                                settle_level=float(S.SETTLE))
                want, counts = CM.query(truth, now, q, own, (0, 0))
                left = CM.query(truth, now, q.but(count=edge - first), own, (0, 0))[1][2]
                assert 0 < left < counts[2], "both workgroups must have sounding slots to add"
                pv = torch.full((max_out + 8,), -1, dtype=torch.int32, device="cuda")
                pc = torch.full((4,), -1, dtype=torch.int32, device="cuda")
                dv = [torch.full((max_out + 8,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
                dc = [torch.full((4,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
                torch.cuda.synchronize()
                db.find_steal_slots(q.c(), pv.data_ptr(), pc.data_ptr())
                for i in range(2):
                    db.find_steal_slots_match(q.c(), device.owner_match(0, 0), dv[i].data_ptr(), dc[i].data_ptr())
                torch.cuda.synchronize()
                pv, pc = pv.cpu().numpy(), pc.cpu().numpy()
                assert pc[:2].tolist() == counts[:2] and (pc[2:] == -1).all() and np.array_equal(pv[:counts[0]], want), (q, pc)
                for i in range(2):
                    gv, gc = dv[i].cpu().numpy(), dc[i].cpu().numpy()
                    print(f"K {K} policy {policy} max_out {max_out} run {i}: plain {pc[:2].tolist()} matched {gc.tolist()}")
                    assert gv.tobytes() == pv.tobytes() and gc[:2].tobytes() == pc[:2].tobytes(), (q, i)
                    assert gc[2] == counts[2] and gc[3] == -1, (q, i, gc.tolist(), counts)
    finally:
        db.close()


@pytest.mark.gpu
def test_ties_at_the_threshold_inside_one_channel(dev):
    """70 000 voices, every slot with the same key, the two channels interleaved: the list is the channel's first voices in index
    order, however short; the other channel's slots lie between them."""
    from test_slot_steal import plain_bank
    n, K = 70000, 2
    bank, tables, g, now = plain_bank(n)
    own = np.zeros(n, np.uint32)
    heads = np.arange(0, n, K)
    own[heads] = np.where((heads // K) % 3 == 1, CS.tag_of(CS.B, 7), CS.tag_of(CS.A, 7)).astype(np.uint32)
    db = open_bank(dev, bank, tables, g)
    try:
        set_owners(db, own, K)
        q = M.SlotQuery(0, n, K, 3, max_out=STEAL_MAX)
        total_b = int(((heads // K) % 3 == 1).sum())
        for match, total in ((CM.channel(CS.A), n // K - total_b), (CM.channel(CS.B), total_b)):
            for mo in (STEAL_MAX, 1, 0):
                want, counts = check(db, bank, now, q.but(max_out=mo), own, match)
                assert counts == [min(mo, total), total, total] and want.tolist() == sorted(want.tolist())
        check(db, bank, now, q.but(flags=RELEASED_FIRST, policy=QUIETEST, max_out=700, first=4096 - 2, count=30000), own, CM.channel(CS.B))
    finally:
        db.close()


@pytest.mark.gpu
def test_query_reads_the_bank_only(dev):
    n, K, mask, F = 1088, 8, 0x55, 128
    bank, tables, g, truth, now, kind = S.scene(n, K, mask)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    try:
        own = CS.owners(n, K)
        set_owners(db, own, K)
        for k in range(4):
            x, y = render_blocks(db, (F,))[0], render_blocks(twin, (F,))[0]
            assert x.tobytes() == y.tobytes(), f"block {k}: the query changed the mix"
            assert db.last_kernel() == twin.last_kernel() and db.last_pack() == twin.last_pack()
            dv, dc = run_query(db, M.SlotQuery(0, n, K, mask, QUIETEST, RELEASED_FIRST, 10, WHICH, 1e-3, STEAL_MAX), CM.channel(CS.A))
            assert dc[1] > 0 and dc[2] >= dc[1]
            run_query(db, M.SlotQuery(24, 296, K, mask, max_out=0), CM.channel(CS.B))
        a, b = bank.copy(), bank.copy()
        db.download(a)
        twin.download(b)
        assert not a.rw_equal(b), a.rw_equal(b)
        ga, gb = db.get_globals(), twin.get_globals()
        assert ga.synth_sample_count == gb.synth_sample_count and ga.noise_rng == gb.noise_rng
        heads = np.arange(0, n, K)
        assert np.array_equal(db.download_owners()[heads], own[heads])
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- note_on_channel

def burst_on_device(db, args, vmask):
    import torch
    iq, sq, match, cap, n, tags, notes = args
    da = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")
    dr = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    db.note_on_channel(notes, tags, iq, sq.c(), device.owner_match(*match), cap, vmask, da.data_ptr(), dr.data_ptr())
    return da, dr


def burst_on_twin(twin, mirror, args, vmask, K, now, truth_for_values):
    """The host route: find_idle_slots_host, find_steal_slots_match_host, the a / b rule in numpy, skred_bank_update, tag_slots."""
    import torch
    iq, sq, match, cap, n, tags, notes = args
    hq = slot_query(iq.first, iq.count, K, iq.member_mask, iq.which, iq.settle_level, iq.start, n)
    idle, _ = twin.find_idle_slots_host(hq)
    victims, total, sounding = twin.find_steal_slots_match_host(sq.but(exclude_idle=iq.which, settle_level=float(iq.settle_level),
                                                                        max_out=min(n, STEAL_MAX)).c(), device.owner_match(*match))
    a, b = CM.split(n, len(idle), sounding, len(victims), cap)
    picks = np.full(n, -1, np.int32)
    picks[:a], picks[a:a + b] = idle[:a], victims[:b]
    touched = SM.store_notes((mirror,), truth_for_values, notes, K, vmask, picks, now)
    if len(touched):
        twin.update(mirror, touched, DIRTY_PARAMS | DIRTY_PHASE | 8 | TRIG)
    placed = picks[:a + b]
    if len(placed):
        dl = torch.from_numpy(placed.copy()).cuda()
        torch.cuda.synchronize()
        twin.tag_slots(dl.data_ptr(), tags[:a + b], K)
        torch.cuda.synchronize()
    return picks, [a + b, n - a - b, b, sounding]


@pytest.mark.gpu
@pytest.mark.parametrize("patch,members,voices", [("3sk", (0, 1, 2), (0, 1, 2, 3)), ("18sk", (0, 10), (0, 1, 2, 10))])
def test_bursts_on_two_channels(dev, patch, members, voices):
    """The burst script of tests/chan_scenes.py -- under the cap, at it, above a lowered one, dropped, no idle slot, mono -- on a
    device bank, on a twin driven by the host route, and on the oracle: d_assigned, the four result words, the owner words, and state,
    stems and mix over two blocks after every burst."""
    from test_chan_cpu import run_burst_script
    box = {}

    def on_burst(step, st, args, want, now):
        bank, tables, g, K = st["bank"], st["tables"], st["g"], st["K"]
        if step == -1:
            box["db"], box["twin"] = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
            box["mirror"], box["scratch"] = bank.copy(), bank.copy()
            for d in (box["db"], box["twin"]):
                set_owners(d, st["own"], K)
                for _ in range(4):
                    d.render_host(CS.F, 2, 0, want_stems=True)
            return
        db, twin = box["db"], box["twin"]
        if args == "block":
            x, xs = db.render_host(CS.F, 2, 0, want_stems=True)
            y, ys = twin.render_host(CS.F, 2, 0, want_stems=True)
            assert xs.tobytes() == ys.tobytes() and x.tobytes() == y.tobytes(), f"burst {step}: the two routes differ"
            assert xs.tobytes() == want["stems"].tobytes(), f"burst {step}: stems differ from the oracle"
            a, b = bank.copy(), bank.copy()
            db.download(a)
            twin.download(b)
            assert not a.rw_equal(st["truth"]), f"burst {step}: state differs from the oracle: {a.rw_equal(st['truth'])}"
            assert not a.rw_equal(b), a.rw_equal(b)
            assert db.last_kernel() == twin.last_kernel() and db.last_pack() == twin.last_pack()
            return
        picks, res = want
        n, tags = args[4], args[5]
        da, dr = burst_on_device(db, args, st["vmask"])
        tpicks, tres = burst_on_twin(twin, box["mirror"], args, st["vmask"], K, now, box["scratch"])
        import torch
        torch.cuda.synchronize()
        got, gres = da.cpu().numpy(), dr.cpu().numpy()
        print(f"burst {step} {CS.BURSTS[step][0]}: n {n}, cap {args[3]} -> {gres.tolist()} {got[:n].tolist()}")
        assert np.array_equal(got[:n], picks) and (got[n:] == -7).all(), (got.tolist(), picks.tolist())
        assert gres[:4].tolist() == res and gres[4] == -7, (gres.tolist(), res)
        assert np.array_equal(tpicks, picks) and tres == res
        own = st["own"].copy()
        CM.tag(own, picks, tags, K)
        heads = np.arange(0, bank.n, K)
        assert np.array_equal(db.download_owners()[heads], own[heads]), "owner words differ from the model"
        assert np.array_equal(twin.download_owners()[heads], own[heads])

    try:
        seen, log = run_burst_script(patch, members, voices, on_burst)
        assert seen >= CS.KINDS, (seen, log)
    finally:
        for k in ("db", "twin"):
            if k in box:
                box[k].close()


@pytest.mark.gpu
def test_no_cap_no_match_is_note_on_steal_slots(dev):
    """cap = SKRED_CHAN_NO_CAP, mask 0, everything tagged: the bytes of note_on_steal_slots followed by tag_slots on a twin."""
    import torch
    from test_slot_steal import patch_notes, playing_patch
    n, members, voices = 512, (0, 1, 2), (0, 1, 2, 3)
    bank, tables, g, K = playing_patch("3sk", n, members)
    mmask, vmask = sum(1 << l for l in members), sum(1 << l for l in voices)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    try:
        for d in (db, twin):
            set_owners(d, np.full(n, 9, np.uint32), K)
            render_blocks(d, (CS.F,) * 4)
        for i, (irange, count) in enumerate((((0, 8 * K), 1), ((8 * K, 8 * K), 5), ((K, K), 3), ((16 * K, 8 * K), 12))):
            iq = slot_query(irange[0], irange[1], K, mmask, WHICH, 1e-3, irange[0], 0)
            sq = M.SlotQuery(0, 8 * K, K, mmask, OLDEST, RELEASED_FIRST)
            notes = patch_notes(count, K, vmask, i)
            tags = np.arange(1, count + 1, dtype=np.uint32) + np.uint32(100 * i)
            outs = []
            for d, chan in ((db, True), (twin, False)):
                da = torch.full((count + 8,), -7, dtype=torch.int32, device="cuda")
                dr = torch.full((4,), -7, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                if chan:
                    d.note_on_channel(notes, tags, iq, sq.c(), device.owner_match(0, 0), CM.NO_CAP, vmask, da.data_ptr(), dr.data_ptr())
                else:
                    d.note_on_steal_slots(notes, iq, sq.c(), vmask, da.data_ptr(), dr.data_ptr())
                    d.tag_slots(da.data_ptr(), tags, K)
                torch.cuda.synchronize()
                outs.append((da.cpu().numpy(), dr.cpu().numpy()))
            assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1][:3].tobytes() == outs[1][1][:3].tobytes(), (i, outs)
            assert outs[1][1][3] == -7 and outs[0][1][3] >= 0
            assert np.array_equal(db.download_owners(), twin.download_owners())
            for k in range(2):
                x, y = render_blocks(db, (CS.F,))[0], render_blocks(twin, (CS.F,))[0]
                assert x.tobytes() == y.tobytes(), f"burst {i} block {k}"
            a, b = bank.copy(), bank.copy()
            db.download(a)
            twin.download(b)
            assert not a.rw_equal(b), a.rw_equal(b)
        assert outs[0][1][1] > 0, "the last burst drops nothing"
    finally:
        db.close()
        twin.close()


@pytest.mark.gpu
def test_a_burst_never_touches_the_other_channel(dev):
    """A bank with no idle slot: a burst on channel A, larger than channel A, re-triggers and re-tags slots of channel A only."""
    import torch
    from test_slot_steal import patch_notes, playing_patch
    n, members, voices = 512, (0, 10), (0, 1, 2, 10)
    bank, tables, g, K = playing_patch("18sk", n, members)
    e = bank["voice_amp_envelope"]
    e["sample_release"][:] = np.uint64(0)                                        # nobody ends: no slot comes to rest
    e["release_time"][:] = np.float32(1e6)
    mmask, vmask = sum(1 << l for l in members), sum(1 << l for l in voices)
    slots = n // K
    own = np.zeros(n, np.uint32)
    heads = np.arange(0, n, K)
    own[heads] = np.where(np.arange(slots) % 2 == 0, CS.tag_of(CS.A, 1), CS.tag_of(CS.B, 1)).astype(np.uint32) + np.arange(slots, dtype=np.uint32)
    db = open_bank(dev, bank, tables, g)
    try:
        set_owners(db, own, K)
        render_blocks(db, (CS.F,))
        start0, rel0 = db.download_env_clocks()
        count = slots // 2 + 3                                                   # three more notes than channel A has slots
        iq = slot_query(0, n, K, mmask, WHICH, 1e-3, 0, 0)
        sq = M.SlotQuery(0, n, K, mmask, OLDEST, 0)
        tags = np.array([CS.tag_of(CS.A, 5000 + k) for k in range(count)], np.uint32)
        da = torch.full((count,), -7, dtype=torch.int32, device="cuda")
        dr = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        db.note_on_channel(patch_notes(count, K, vmask, 3), tags, iq, sq.c(), device.owner_match(*CM.channel(CS.A)), CM.NO_CAP, vmask,
                           da.data_ptr(), dr.data_ptr())
        torch.cuda.synchronize()
        assert dr.cpu().numpy().tolist() == [slots // 2, 3, slots // 2, slots // 2]
        got = da.cpu().numpy()
        assert sorted(got[:slots // 2].tolist()) == heads[::2].tolist() and (got[slots // 2:] == -1).all()
        start1, rel1 = db.download_env_clocks()
        owners = db.download_owners()
        b_voices = ((np.arange(n) // K) % 2 == 1)
        assert np.array_equal(start0[b_voices], start1[b_voices]) and np.array_equal(rel0[b_voices], rel1[b_voices]), "a slot of channel B was re-triggered"
        assert np.array_equal(owners[heads[1::2]], own[heads[1::2]]), "a slot of channel B was re-tagged"
        assert (owners[heads[::2]] >> 24 == CS.A).all() and set(owners[heads[::2]].tolist()) == set(tags[:slots // 2].tolist())
        a_masked = ~b_voices & np.isin(np.arange(n) % K, voices)
        assert (start1[a_masked] != start0[a_masked]).all()
    finally:
        db.close()


@pytest.mark.gpu
def test_two_per_lane_in_place_after_a_channel_burst(dev):
    """tests/test_slot_steal.py's in-place shape: 4 096 voices, two per lane, SKRED_OPT_IN_PLACE = 2.  A chord of 2 stays in place, a
    chord of 110 (770 voices) must leave it -- on the channel call as on note_on_steal_slots on a twin."""
    import torch
    from test_slots import slot_notes
    n, K, F, BIG, SMALL = 4096, 8, 256, 110, 2
    mmask, vmask = 0x01, 0xFE
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(2))   # noqa: E731
    db, twin = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    chords = {3: (SMALL, True), 6: (BIG, False)}
    taken = []
    try:
        for d in (db, twin):
            set_owners(d, np.full(n, CS.tag_of(CS.A, 1), np.uint32), K)
        for k in range(8):
            expect = None
            if k in chords:
                count, expect = chords[k]
                iq = slot_query(0, n, K, mmask, WHICH, 1e-3, 0, 0)
                sq = M.SlotQuery(0, n, K, mmask, OLDEST, 0)
                notes = slot_notes(count, K, vmask, k)
                tags = np.full(count, CS.tag_of(CS.A, 2 + k), np.uint32)
                da = [torch.full((count,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
                dr = [torch.full((4,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
                torch.cuda.synchronize()
                db.note_on_channel(notes, tags, iq, sq.c(), device.owner_match(*CM.channel(CS.A)), CM.NO_CAP, vmask, da[0].data_ptr(), dr[0].data_ptr())
                twin.note_on_steal_slots(notes, iq, sq.c(), vmask, da[1].data_ptr(), dr[1].data_ptr())
            x, y = render_blocks(db, (F,))[0], render_blocks(twin, (F,))[0]
            taken.append((db.last_in_place(), twin.last_in_place()))
            assert db.last_kernel() == twin.last_kernel() == 3
            assert taken[-1][0] == taken[-1][1], f"block {k}: in place on one route only: {taken}"
            if expect is not None:
                assert taken[-1][0] is expect, f"block {k}: in place {taken[-1][0]}, expected {expect}: {taken}"
                assert np.array_equal(da[0].cpu().numpy(), da[1].cpu().numpy())
                assert dr[0].cpu().numpy().tolist() == [count, 0, count, n // K] and dr[1].cpu().numpy()[:3].tolist() == [count, 0, count]
            assert x.tobytes() == y.tobytes(), f"block {k}: the mixes differ"
            assert db.list_violations() == twin.list_violations() == 0
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_write_nothing(dev):
    import torch
    import test_slot_steal_cpu as CPU
    from test_slot_steal import plain_bank
    from test_slots import slot_notes
    n, K, mask = 1024, 8, 0x55
    bank, tables, g, now = plain_bank(n)
    db = open_bank(dev, bank, tables, g)
    try:
        L = db.L
        own = np.full(n, CS.tag_of(CS.A, 1), np.uint32)
        set_owners(db, own, K)
        dv = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        dc = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        da = torch.full((16,), -1, dtype=torch.int32, device="cuda")
        dr = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        count = 4
        p = C.cast(device.note_array(slot_notes(count, K, mask, 1, junk=False)), C.c_void_p)
        good_tags = np.array([CS.tag_of(CS.A, 10 + k) for k in range(count)], np.uint32)
        chan = device.owner_match(*CM.channel(CS.A))
        torch.cuda.synchronize()

        def on(h=db.h, nt=p, cnt=count, vm=mask, res=dr.data_ptr(), sq=None, m=chan, tags=good_tags, cap=8, **kw):
            args = dict(first=0, count=n, slot_voices=K, member_mask=mask, which=WHICH, settle_level=0.0, start=None, max_out=-5)
            args.update(kw)
            iq = slot_query(**args)
            sq = CPU.good() if sq is None else sq
            t = None if tags is None else np.ascontiguousarray(tags, np.uint32)
            return L.skred_bank_note_on_channel(h, C.byref(iq), C.byref(sq), C.byref(m) if m is not None else None, cap, nt,
                                                t.ctypes.data if t is not None else None, cnt, vm, da.data_ptr(), res or None, None)

        for case, (_, code) in CPU.REFUSED.items():
            q = CPU.refused_query(case)
            assert L.skred_bank_find_steal_slots_match(db.h, C.byref(q), C.byref(chan), dv.data_ptr(), dc.data_ptr(), None) == code, case
            host = np.full(STEAL_MAX, -1, np.int32)
            assert L.skred_bank_find_steal_slots_match_host(db.h, C.byref(q), C.byref(chan), host.ctypes.data, None, None, None) == code, case
            if not case.startswith(("exclude", "max_out", "settle")):              # (the library overrides those three fields)
                assert on(sq=q) == code, case
        gq = CPU.good()
        bad_m = device.owner_match(0x03000001, 0xFF000000)
        F3 = L.skred_bank_find_steal_slots_match
        assert F3(db.h, C.byref(gq), C.byref(chan), None, dc.data_ptr(), None) == BAD      # max_out > 0 and no list
        assert F3(db.h, C.byref(gq), C.byref(chan), dv.data_ptr(), None, None) == BAD
        assert F3(None, C.byref(gq), C.byref(chan), dv.data_ptr(), dc.data_ptr(), None) == BAD
        assert F3(db.h, C.byref(gq), None, dv.data_ptr(), dc.data_ptr(), None) == BAD
        assert F3(db.h, C.byref(gq), C.byref(bad_m), dv.data_ptr(), dc.data_ptr(), None) == BAD
        assert on(sq=CPU.good(slot_voices=4, member_mask=0x5)) == BAD and on(sq=CPU.good(member_mask=0x15)) == BAD
        assert on(slot_voices=16) == BAD and on(member_mask=0xFF) == BAD
        assert on(which=WHICH | AMP) == BAD and on(which=AMP) == BAD and on(which=0) == BAD
        assert on(h=None) == BAD and on(nt=None) == BAD and on(res=0) == BAD and on(cnt=-1) == BAD
        assert on(m=None) == BAD and on(m=bad_m) == BAD and on(tags=None) == BAD
        assert on(tags=[CS.tag_of(CS.A, 1), 0, CS.tag_of(CS.A, 2), CS.tag_of(CS.A, 3)]) == BAD
        assert on(tags=[CS.tag_of(CS.A, 1), CS.tag_of(CS.B, 1), CS.tag_of(CS.A, 2), CS.tag_of(CS.A, 3)]) == BAD
        assert on(vm=0) == BAD and on(vm=0x100) == BAD and on(first=4) == RANGE and on(count=n + 8) == RANGE
        bad = slot_notes(count, K, mask, 1, junk=False)
        bad[K + 2] = device.NoteC(float("nan"), 1.0, 0.0, 0.5, 0.5, 0)             # a masked position (bit 2)
        assert on(nt=C.cast(device.note_array(bad), C.c_void_p)) == BAD
        assert on(cnt=0) == 0
        torch.cuda.synchronize()
        for t in (dv, dc, da, dr):
            assert (t.cpu().numpy() == -1).all()                                   # nothing reached the device
        assert np.array_equal(db.download_owners(), np.where(np.arange(n) % K == 0, own, 0))
        check(db, bank, now, M.SlotQuery(0, n, K, mask, max_out=40), own, CM.channel(CS.A))   # ... and the bank still answers
        assert on(sq=CPU.good(first=8, count=64)) == 0                               # ranges may differ
        torch.cuda.synchronize()
        assert dr.cpu().numpy().tolist() == [4, 0, 4, 8]
    finally:
        db.close()
