"""Channel polyphony on the fixed-point bank on the GPU: skred_fxbank_find_steal_match / _find_steal_match_host / _note_on_channel.

The expectation is tests/fx_chan_model.py -- the definition of include/skred_amd_fxpt.h in numpy, exact -- evaluated on the ORACLE's
bank: oracle.cpuref.fx_render renders the blocks, tests/fx_live_model.py places the notes, tests/fx_owner_model.py writes the tags.
Lists, counts, owner words and every word of the bank are compared byte for byte; d_voices is pre-filled with -7 and entries past
`written` must keep it.  Scenes: tests/fx_chan_scenes.py (tests/test_fx_chan_cpu.py shows that none is vacuous).
"""
import ctypes as C

import numpy as np
import pytest

import fx_chan_model as CM
import fx_chan_scenes as CS
import fx_live_model as live
import fx_steal_model as sm
import fx_steal_scenes as sc
from fx_steal_model import ENV, FIN, OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, STEAL_MAX, Query
from oracle import cpuref
from skred_amd import device, fxbank as fxb
from test_fx_live import block, dev_i32, host_of, open_fx

pytestmark = pytest.mark.gpu

FLAGS = ("disconnect", "use_envelope", "smoother_enable", "one_shot", "filter_mode", "finished", "is_active")   # one bit on the device


def tag_all(db, own):
    """The owner array onto the device: one tag_list over every voice (0 clears)."""
    import torch
    voices = torch.arange(len(own), dtype=torch.int32, device="cuda")
    db.tag_list(voices.data_ptr(), own)
    torch.cuda.synchronize()


def reach(n, variant, own):
    """(queried bank, oracle's bank, now) after the scene's blocks, tagged; the device's state checked against the oracle's on the way"""
    b, pool, c0, truth, now, role, special = sc.scene(n, variant)
    db = open_fx(b, pool, c0)
    ref, cnt = b.copy(), c0
    for frames, interp in sc.FRAMES:
        cnt = block(db, ref, pool, cnt, frames, interp, variant)
    assert cnt == now and not ref.rw_mismatch(truth)
    if own is not None:
        tag_all(db, own)
        assert np.array_equal(db.download_owners(), own)
    return db, ref, pool, cnt


def mquery(db, q, match, stream=0):
    import torch
    dv, dc = dev_i32(q.max_out + 8), dev_i32(5)
    torch.cuda.synchronize()
    db.find_steal_match(q.c(), match[0], match[1], dv.data_ptr() if q.max_out > 0 else 0, dc.data_ptr(), stream)
    torch.cuda.synchronize()
    return host_of(dv), host_of(dc)


def check(db, ref, now, q, own, match):
    want, counts = CM.query(ref, now, q, own, match)
    dv, dc = mquery(db, q, match)
    assert dc[:3].tolist() == counts and (dc[3:] == -7).all(), f"{q} {match}: d_count {dc.tolist()}, expected {counts}"
    assert np.array_equal(dv[:want.size], want), f"{q} {match}: first mismatch at {int(np.flatnonzero(dv[:want.size] != want)[0])}"
    assert (dv[want.size:] == -7).all(), f"{q} {match}: entries past `written` were touched"
    return dv, dc


def whole_bank(db, like):
    """Every word of the bank as the device holds it: the read-write fields and the parameters, the envelope clocks among them."""
    got = like.copy()
    db.download(got)
    db.download_params(got)
    return got


def assert_same_bank(got, ref, tag):
    for name, _, _ in fxb.FX_FIELDS:
        a, b = (got[name] != 0, ref[name] != 0) if name in FLAGS else (got[name], ref[name])
        assert np.array_equal(a, b), f"{tag}: {name} differs at {np.flatnonzero(a != b)[:8].tolist()}"


# ---------------------------------------------------------------------------------------------- the query

def test_fx_chan_query_scenes():
    """1 500 voices: 6 workgroups, the last one partial.  Every query of the scene under every match."""
    b, pool, c0, truth, now, own = CS.query_scene()
    db, ref, pool, cnt = reach(CS.N_QUERY, "plain", own)
    try:
        ms = CS.matches(own, ref)
        for match in ms:
            for q in CS.queries():
                check(db, ref, cnt, q, own, match)
        for match in ms[:4]:                                          # the host form gives the same list and counts
            for q in CS.queries()[:5]:
                want, counts = CM.query(ref, cnt, q, own, match)
                voices, total, sounding = db.find_steal_match_host(q.c(), *match)
                assert np.array_equal(voices, want) and [len(voices), total, sounding] == counts, (q, match)
    finally:
        db.close()


def test_fx_chan_ties_at_the_threshold():
    """70 000 voices, more than SKRED_STEAL_MAX equal keys at the threshold inside one channel, interleaved with the other channel's
    voices that carry the same keys: index order decides, and the other channel is never listed."""
    own = CS.ties_owners()
    db, ref, pool, cnt = reach(CS.N_TIES, "ties", own)
    try:
        for q in CS.ties_queries():
            for ch in (CS.A, CS.B):
                dv, dc = check(db, ref, cnt, q, own, CM.channel(ch))
                assert (own[dv[:dc[0]]] >> np.uint32(24) == ch).all()
    finally:
        db.close()


def test_fx_chan_mask_zero_with_everything_tagged_is_find_steal():
    import torch
    own = np.full(CS.N_QUERY, 5, np.uint32)
    db, ref, pool, cnt = reach(CS.N_QUERY, "plain", own)
    twin, _, _, _ = reach(CS.N_QUERY, "plain", None)
    try:
        for q in CS.queries():
            dv, dc = mquery(db, q, (0, 0))
            tv, tc = dev_i32(q.max_out + 8), dev_i32(5)
            twin.find_steal(q.c(), tv.data_ptr() if q.max_out > 0 else 0, tc.data_ptr())
            torch.cuda.synchronize()
            assert dv.tobytes() == host_of(tv).tobytes() and dc[:2].tobytes() == host_of(tc)[:2].tobytes(), q
            assert dc[2] >= dc[1]
    finally:
        db.close()
        twin.close()


def test_fx_matched_key_pass_with_mask_zero_is_the_plain_one():
    """The two instantiations of the fixed-point key pass on one bank of 600 voices, every voice tagged, match (0, 0): the list and
    the first two count words are find_steal's bytes.  The range starts off a 64-voice boundary and crosses a 256-voice workgroup
    span with sounding voices on both sides, so two workgroups add to the sounding word and the last arriver publishes it; each
    matched query runs twice in a row on one stream with no host wait between the two: the second starts from a re-armed word."""
    import torch
    n, first = 600, 37
    count, edge = n - first, 256
    own = np.full(n, 5, np.uint32)
    db, ref, pool, cnt = reach(n, "plain", own)
    try:
        for policy, flags in ((OLDEST, 0), (QUIETEST, RELEASED_ONLY)):           # (RELEASED_ONLY: fewer candidates than sounding voices)
            for max_out in (0, 5):
                q = Query(first, count, policy, flags, 0, FIN | ENV, 3, max_out)
                want, counts = CM.query(ref, cnt, q, own, (0, 0))
                left = CM.query(ref, cnt, q.but(count=edge - first), own, (0, 0))[1][2]
                assert 0 < left < counts[2], "both workgroups must have sounding voices to add"
                pv, pc = dev_i32(max_out + 8), dev_i32(5)
                dv, dc = [dev_i32(max_out + 8) for _ in range(2)], [dev_i32(5) for _ in range(2)]
                torch.cuda.synchronize()
                db.find_steal(q.c(), pv.data_ptr() if max_out > 0 else 0, pc.data_ptr())
                for i in range(2):
                    db.find_steal_match(q.c(), 0, 0, dv[i].data_ptr() if max_out > 0 else 0, dc[i].data_ptr())
                torch.cuda.synchronize()
                pv, pc = host_of(pv), host_of(pc)
                assert pc[:2].tolist() == counts[:2] and (pc[2:] == -7).all() and np.array_equal(pv[:counts[0]], want), (q, pc)
                for i in range(2):
                    gv, gc = host_of(dv[i]), host_of(dc[i])
                    print(f"policy {policy} flags {flags} max_out {max_out} run {i}: plain {pc[:2].tolist()} matched {gc.tolist()}")
                    assert gv.tobytes() == pv.tobytes() and gc[:2].tobytes() == pc[:2].tobytes(), (q, i)
                    assert gc[2] == counts[2] and (gc[3:] == -7).all(), (q, i, gc.tolist(), counts)
    finally:
        db.close()


def test_fx_chan_query_reads_the_bank_only():
    """A bank queried between its blocks against a twin that is never queried (and never tagged): state, parameters, mix and master
    gain bit for bit.  Two queries in a row give the same counts (the count word was re-armed), and skred_fxbank_find_steal behind a
    matched query still gives its own bytes (they share the scratch)."""
    import torch
    b, pool, c0, truth, now, own = CS.query_scene()
    db, twin = open_fx(b, pool, c0), open_fx(b, pool, c0)
    tag_all(db, own)
    ref, cnt = b.copy(), c0
    outs = [torch.zeros((128, 2), dtype=torch.int64, device="cuda") for _ in range(2)]
    plain = Query(37, 1300, QUIETEST, RELEASED_ONLY, 0, FIN, 0, 50)
    try:
        for k, frames in enumerate((128, 100, 64, 1)):
            q = Query(0, b.n, OLDEST, RELEASED_FIRST, 10, FIN | ENV, CS.SETTLE, STEAL_MAX)
            first = check(db, ref, cnt, q, own, CM.channel(CS.A))
            second = mquery(db, q, CM.channel(CS.A))
            assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
            assert first[1][2] > 0
            check(db, ref, cnt, q.but(max_out=0), own, CM.channel(CS.B))
            want, total = sm.victims(ref, cnt, plain)                  # the plain query behind the matched one
            dv, dc = dev_i32(plain.max_out + 8), dev_i32(5)
            db.find_steal(plain.c(), dv.data_ptr(), dc.data_ptr())
            torch.cuda.synchronize()
            assert host_of(dc).tolist() == [want.size, total, -7, -7, -7] and np.array_equal(host_of(dv)[:want.size], want)
            check(db, ref, cnt, q.but(max_out=16), own, CM.channel(CS.B))   # ... and the matched one behind the plain one
            for d, o in zip((db, twin), outs):
                d.render_mix(frames, o.data_ptr(), k & 1)
            torch.cuda.synchronize()
            assert torch.equal(outs[0][:frames], outs[1][:frames]), f"block {k}: the query changed the mix"
            _, _, cnt = cpuref.fx_render(ref, pool, cnt, frames, k & 1)
        a, c = whole_bank(db, b), whole_bank(twin, b)
        for name, _, _ in fxb.FX_FIELDS:
            assert a[name].tobytes() == c[name].tobytes(), name
        assert not a.rw_mismatch(ref)
        assert db.master_gain() == twin.master_gain() and db.sample_count() == twin.sample_count() == cnt
        assert np.array_equal(db.download_owners(), own)
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- the burst

def host_route(twin, h_like, own_host, iq, sq, match, cap, n, tags, notes, now):
    """The burst made only of entry points that need no matched query: owners and bank downloaded behind a device wait, the pick in
    numpy, the notes written into a host view and sent as an update, the tags through tag_list."""
    import torch
    own_now = twin.download_owners()
    h = whole_bank(twin, h_like)
    want, res, _ = CM.burst(h, now, own_now, iq, sq, match, cap, n)
    voices = want[:res[0]]
    if res[0]:
        for t, v in zip(notes, voices):
            h["phase_inc"][v], h["velocity_q15"][v] = t.phase_inc, t.velocity_q15
            if t.flags & fxb.NOTE_SET_PHASE:
                h["phase"][v], h["finished"][v] = t.phase, 0
            if t.flags & fxb.NOTE_SET_PAN:
                h["pan_left_q15"][v], h["pan_right_q15"][v] = t.pan_left_q15, t.pan_right_q15
        twin.update(h, voices, fxb.DIRTY_PARAMS | fxb.DIRTY_PAN | fxb.DIRTY_PHASE | fxb.STAMP_TRIGGER)
        d = torch.from_numpy(voices.copy()).cuda()
        twin.tag_list(d.data_ptr(), tags[:res[0]])
        torch.cuda.synchronize()
    return want, res


def test_fx_chan_bursts_on_two_channels():
    """The script of tests/fx_chan_scenes.py on 1 024 voices and 64-frame blocks: after every burst d_assigned, the four result words,
    the owner words and every word of the bank equal the model's; mixes and stems equal the oracle's bit for bit.  A twin makes the
    same bursts on the host route and ends byte-equal.  (That victims come from the channel only and that the other channel's
    owners and clocks never change is asserted by the script on the model, which the device equals word for word.)"""
    dev = {}

    def on_burst(step, state, args, want, now):
        if step == -1:
            b, pool, c0 = state["bank"], state["pool"], state["c0"]
            dev["db"], dev["twin"] = open_fx(b, pool, c0), open_fx(b, pool, c0)
            for d in (dev["db"], dev["twin"]):
                tag_all(d, state["own"])
                for _ in range(2):
                    d.render_host(CS.F, 1)
            assert_same_bank(whole_bank(dev["db"], b), state["truth"], "before the first burst")
            return
        db, twin, truth = dev["db"], dev["twin"], state["truth"]
        if args == "block":
            mix, stems, _ = want
            for d, who in ((db, "device route"), (twin, "host route")):
                got_mix, got_stems = d.render_host(CS.F, 1, want_stems=True)
                assert (got_mix == mix).all() and (got_stems == stems).all(), f"burst {step}, {who}: the block differs from the oracle's"
                assert_same_bank(whole_bank(d, truth), truth, f"after a block behind burst {step}, {who}")
            return
        iq, sq, match, cap, n, tags, notes = args
        assigned, res = want
        d_assigned, d_result = dev_i32(n + 8), dev_i32(6)
        db.note_on_channel(notes, iq, sq.but(exclude_idle=fxb.IDLE_AMP_ZERO, settle_q15=0, max_out=1).c(), match[0], match[1], cap, tags,
                           d_assigned.data_ptr(), d_result.data_ptr())                                   # (those three are overridden)
        got_a, got_r = host_of(d_assigned), host_of(d_result)
        name = CS.BURSTS[step][0]
        assert got_r.tolist() == res + [-7, -7], f"{name}: d_result {got_r.tolist()}, expected {res}"
        assert np.array_equal(got_a[:n], assigned) and (got_a[n:] == -7).all(), f"{name}: d_assigned {got_a[:n].tolist()}, expected {assigned.tolist()}"
        expect, own = truth.copy(), state["own"].copy()
        live.place_notes(expect, notes, assigned, res[0], 0, now)
        CM.tag(own, assigned, tags)
        assert np.array_equal(db.download_owners(), own), f"{name}: owner words differ at {np.flatnonzero(db.download_owners() != own)[:8].tolist()}"
        assert_same_bank(whole_bank(db, truth), expect, name)
        t_assigned, t_res = host_route(twin, truth, None, iq, sq, match, cap, n, tags, notes, now)
        assert np.array_equal(t_assigned, assigned) and t_res == res
        assert np.array_equal(twin.download_owners(), own)
        assert_same_bank(whole_bank(twin, truth), expect, name + ", host route")

    try:
        seen, log = CS.run_burst_script(on_burst)
        assert seen >= CS.KINDS, (seen, log)
    finally:
        for d in dev.values():
            d.close()


def test_fx_chan_through_a_shard():
    """One rank, local indices: a census and a burst through skred_fxshard_bank()."""
    from skred_amd.sharded import _lib
    b, pool, c0, own = CS.burst_bank()
    L = fxb._bind(_lib())
    L.skred_shard_destroy.argtypes = [C.c_void_p]
    L.skred_shard_destroy.restype = None
    h = C.c_void_p()
    assert L.skred_fxshard_create(0, 0, 1, 0, b.n, C.byref(h)) == 0
    try:
        fx = fxb.DeviceFxBank.borrowed(L.skred_fxshard_bank(h), b.n)
        fx.set_tables(pool)
        cb = b.as_c()
        assert L.skred_fxshard_upload(h, C.byref(cb)) == 0
        fx.set_sample_count(c0)
        tag_all(fx, own)
        ref, cnt = b.copy(), c0
        cnt = block(fx, ref, pool, cnt, CS.F, 1, "shard, before")
        q = Query(0, b.n, exclude_idle=CS.WHICH, settle_q15=CS.SETTLE, max_out=0)
        check(fx, ref, cnt, q, own, CM.channel(CS.A))                                # the census
        iq, sq, match, cap, n, tags = CS.burst_args(1, ref, cnt, own)                # "mixed": idle voices and victims
        notes = CS.burst_notes(n, 1)
        want, res, _ = CM.burst(ref, cnt, own, iq, sq, match, cap, n)
        assert res[0] == n and 0 < res[2] < n
        d_assigned, d_result = dev_i32(n + 8), dev_i32(6)
        fx.note_on_channel(notes, iq, sq.c(), match[0], match[1], cap, tags, d_assigned.data_ptr(), d_result.data_ptr())
        assert host_of(d_result).tolist() == res + [-7, -7] and np.array_equal(host_of(d_assigned)[:n], want)
        live.place_notes(ref, notes, want, res[0], 0, cnt)
        CM.tag(own, want, tags)
        assert np.array_equal(fx.download_owners(), own)
        cnt = block(fx, ref, pool, cnt, CS.F, 1, "shard, after the burst")
        check(fx, ref, cnt, q, own, CM.channel(CS.A))
    finally:
        L.skred_shard_destroy(h)


# ---------------------------------------------------------------------------------------------- refusals

def test_fx_chan_refusals_leave_the_bank_usable():
    b, pool, c0, own = CS.burst_bank()
    db = open_fx(b, pool, c0)
    tag_all(db, own)
    ref, cnt = b.copy(), c0
    try:
        cnt = block(db, ref, pool, cnt, CS.F, 1, "before")
        before = whole_bank(db, ref)
        d = dev_i32(16)
        p = d.data_ptr()
        n = b.n
        good, iq = Query(0, n, max_out=8), fxb.FxIdleQueryC(0, n, CS.WHICH, CS.SETTLE, 0, 0)
        a, mask = CM.channel(CS.A)
        note, tag = CS.burst_notes(1, 0), [CS.tag_of(CS.A, 5)]
        bad_note = CS.burst_notes(1, 0)
        bad_note[0].flags = 4
        refused = [
            lambda: db.find_steal_match(good.but(policy=2).c(), a, mask, p, p),
            lambda: db.find_steal_match(good.but(flags=fxb.STEAL_UNNAMED).c(), a, mask, p, p),
            lambda: db.find_steal_match(good.but(exclude_idle=fxb.IDLE_UNNAMED).c(), a, mask, p, p),
            lambda: db.find_steal_match(good.but(settle_q15=-1).c(), a, mask, p, p),
            lambda: db.find_steal_match(good.but(max_out=STEAL_MAX + 1).c(), a, mask, p, p),
            lambda: db.find_steal_match(good.but(count=n + 1).c(), a, mask, p, p),
            lambda: db.find_steal_match(good.c(), a | 1, mask, p, p),                       # value has bits outside the mask
            lambda: db.find_steal_match(good.c(), a, mask, 0, p),
            lambda: db.find_steal_match(good.c(), a, mask, p, 0),
            lambda: db.find_steal_match_host(good.but(first=-1).c(), a, mask),
            lambda: db.note_on_channel(note, fxb.FxIdleQueryC(0, n, ENV | fxb.IDLE_AMP_ZERO, 3, 0, 0), good.c(), a, mask, 4, tag, p, p),
            lambda: db.note_on_channel(note, fxb.FxIdleQueryC(0, n, CS.WHICH, 3, n, 0), good.c(), a, mask, 4, tag, p, p),
            lambda: db.note_on_channel(note, iq, good.but(policy=7).c(), a, mask, 4, tag, p, p),
            lambda: db.note_on_channel(note, iq, good.but(flags=4).c(), a, mask, 4, tag, p, p),
            lambda: db.note_on_channel(note, iq, good.c(), a | 1, mask, 4, tag, p, p),
            lambda: db.note_on_channel(note, iq, good.c(), a, mask, 4, [0], p, p),
            lambda: db.note_on_channel(note, iq, good.c(), a, mask, 4, [CS.tag_of(CS.B, 5)], p, p),
            lambda: db.note_on_channel(bad_note, iq, good.c(), a, mask, 4, tag, p, p),
            lambda: db.note_on_channel(note, iq, good.c(), a, mask, 4, tag, p, 0),
        ]
        for k, call in enumerate(refused):
            with pytest.raises(device.SkredAmdError):
                call()
            assert (host_of(d) == -7).all(), k
        db.note_on_channel([], iq, good.c(), a, mask, 4, np.zeros(0, np.uint32), p, p)        # an empty burst does nothing
        assert (host_of(d) == -7).all()
        assert_same_bank(whole_bank(db, ref), before, "after the refusals")
        assert np.array_equal(db.download_owners(), own)
        cnt = block(db, ref, pool, cnt, 100, 1, "after the refusals")
        check(db, ref, cnt, good, own, (a, mask))
    finally:
        db.close()
