"""Note owners of the fixed-point bank on the GPU: skred_fxbank_tag_list / _find_owned / _stamp_owned / _release_tags / _owner_clear /
_download_owners.

The expectation is tests/fx_owner_model.py applied to the ORACLE's bank (oracle.cpuref.fx_render renders the blocks): after every
call the device's whole state -- read-write fields, parameter fields, owner words -- the lists and every result word must equal
the model's byte for byte, and the blocks around the calls equal the oracle's mix and stems bit for bit.  Shapes: banks of 300 and
1 088 voices (no multiple of 64 or 256: a last partly filled workgroup), ranges that start off 0 and end inside a workgroup, 1, 2,
3, 1 023 and 1 024 tags (the power-of-two padding of the find pass's table on both sides), a tag of 0xFFFFFFFF (the padding's own
value), one tag on two voices, lists with -1 holes, a d_count shorter than n, a voice listed twice."""
import numpy as np
import pytest

import fx_owner_model as om
import fx_owner_scenes as sc
from oracle import cpuref
from fx_ctl_gpu import assert_state, block, ctl_bank, dev_fill, dev_i32, host_of, open_fx, u32
from skred_amd import device, fxbank as fxb

pytestmark = pytest.mark.gpu

REL, TRIG = fxb.STAMP_RELEASE, fxb.STAMP_TRIGGER


def distinct_tags(k, seed):
    rng = np.random.default_rng(seed)
    t = rng.choice(np.arange(1, 2**32 - 1, 4099, dtype=np.uint64), k, replace=False).astype(np.uint32)
    t[k // 2] = 0xFFFFFFFF
    return t


@pytest.mark.parametrize("n", [300, 1088])
def test_fx_owner_calls_equal_the_model(n):
    import torch
    b, pool, c0 = ctl_bank(n)
    db, twin = open_fx(b, pool, c0), open_fx(b, pool, c0)
    ref, cnt, owner = b.copy(), c0, om.new(n)
    try:
        assert (db.download_owners() == 0).all(), "a bank that was never tagged"
        db.owner_clear(0, n)                                               # nothing to do, and no array yet
        cnt = block(db, ref, pool, cnt, 65, 1, "before")
        twin.render_host(65, 1)
        # ---- tag_list: -1 holes, entries past the bank, a d_count shorter than n, tag 0 clears
        k = min(n, 1024)
        voices = np.random.default_rng(n).permutation(n)[:k].astype(np.int32)
        tags = distinct_tags(k, n)
        entries = voices.copy()
        entries[[3, 77]] = [-1, n]
        d_entries, d_res = dev_i32(entries), dev_fill(4)
        db.tag_list(d_entries.data_ptr(), tags, 0, d_res.data_ptr())
        assert u32(d_res)[:2] == om.tag_list(owner, entries, tags) == [k - 2, 2] and host_of(d_res)[2:].tolist() == [-7, -7]
        assert_state(db, ref, "tag_list", owner)
        d_cnt = dev_i32([5, 99])
        db.tag_list(d_entries.data_ptr(), [0, 0, 7, 0, 0, 9, 9, 9], d_cnt.data_ptr(), d_res.data_ptr())
        assert u32(d_res)[:2] == om.tag_list(owner, entries, [0, 0, 7, 0, 0, 9, 9, 9], 5) == [4, 1]
        # one tag on two voices: the lower one wins the find
        lo, hi = sorted(voices[10:12].tolist())
        twice = 0x7777
        d_pair = dev_i32([hi, lo])
        db.tag_list(d_pair.data_ptr(), [twice, twice])
        om.tag_list(owner, [hi, lo], [twice, twice])
        assert_state(db, ref, "tagged twice", owner)
        # ---- find_owned: 1, 2, 3, 1023, 1024 tags; ranges off 0 that end inside a workgroup
        carried = [int(t) for t in owner[voices[20:]] if t not in (0, twice, 0xFFFFFFFF)]
        for m in (1, 2, 3, 1023, 1024):
            ask = ([twice, 0xFFFFFFFF] + carried)[:m]
            nobody = [t for t in range(0x10, 0x10 + 2 * m) if t not in set(owner.tolist())]
            ask = np.array((ask + nobody)[:m], np.uint32)
            ask = ask[np.random.default_rng(m).permutation(m)]
            for first, count in ((0, n), (37, n - 37 - 70), (lo + 1, n - lo - 1), (hi, 1)):
                want = om.find_owned(owner, first, count, ask)
                d_out = dev_fill(m + 4)
                db.find_owned(first, count, ask, d_out.data_ptr())
                got = host_of(d_out)
                assert np.array_equal(got[:m], want) and (got[m:] == -7).all(), (m, first, count)
            if m >= 2:
                assert om.find_owned(owner, 0, n, ask)[list(ask).index(twice)] == lo
                assert om.find_owned(owner, lo + 1, n - lo - 1, ask)[list(ask).index(twice)] == hi
        # a twin that made no owner call renders the same block: the calls above touched no plane
        mix_twin, st_twin = twin.render_host(100, 0, want_stems=True)
        mix, st = db.render_host(100, 0, want_stems=True)
        assert (mix == mix_twin).all() and (st == st_twin).all() and db.master_gain() == twin.master_gain()
        _, _, cnt = cpuref.fx_render(ref, pool, cnt, 100, 0)
        assert_state(db, ref, "after the owner-only calls", owner)
        # ---- stamp_owned: right and wrong tags, holes, a short d_count, a voice listed twice
        lst = np.concatenate([voices[20:60], [-1, n + 5], voices[20:22]]).astype(np.int32)
        ltags = owner[np.clip(lst, 0, n - 1)].copy()
        ltags[ltags == 0] = 5
        ltags[[1, 7, 30]] ^= 0x100                                         # the guard's misses
        d_lst, d_res3 = dev_i32(lst), dev_fill(5)
        for d_count, stamps in ((None, REL), (9, TRIG | REL), (None, TRIG)):
            d_c = dev_i32([d_count, 0]) if d_count is not None else None
            db.stamp_owned(d_lst.data_ptr(), ltags, stamps, d_res3.data_ptr(), d_c.data_ptr() if d_c is not None else 0)
            want, _ = om.stamp_owned(owner, ref, lst, ltags, d_count, stamps, cnt)
            assert u32(d_res3)[:3] == want and host_of(d_res3)[3:].tolist() == [-7, -7], (d_count, stamps)
            assert want[1] > 0 and (d_count is not None or want[2] == 2)
            assert_state(db, ref, f"stamp_owned {d_count} {stamps}", owner)
        cnt = block(db, ref, pool, cnt, 64, 1, "after stamp_owned")
        # ---- release_tags over a range off 0: carried inside, carried only outside, carried by nobody, the tag on two voices
        ask = np.array([twice, 0xFFFFFFFF] + carried[:40] + [0x0BAD0BAD], np.uint32)
        first, count = 37, n - 37 - 70
        db.release_tags(first, count, ask, REL, d_res3.data_ptr())
        want, stamped, found = om.release_tags(owner, ref, first, count, ask, REL, cnt)
        assert u32(d_res3)[:3] == want and want[0] > 0 and want[1] == 0 and want[2] > 0
        assert_state(db, ref, "release_tags", owner)
        cnt = block(db, ref, pool, cnt, 100, 0, "after release_tags")
        # ---- owner_clear, then the released tags are nobody's
        db.owner_clear(37, 100)
        om.clear(owner, 37, 100)
        assert_state(db, ref, "owner_clear", owner)
        torch.cuda.synchronize()
    finally:
        db.close()
        twin.close()


def test_fx_theft_scene_end_to_end():
    """note_on_idle, tag_list, a block, note_on_steal, tag_list, a block, release_tags of the first tags, a block: chord B stole chord
    A's voices, so A's note-off by id -- and the guarded stamp on A's old d_assigned -- release nobody; B's own note-off releases B."""
    st = sc.Story()
    db = open_fx(st.start, st.pool, st.c0)
    try:
        mix, _ = db.render_host(sc.WARM, 1)
        assert (mix == st.block(sc.WARM)).all()
        d_a, d_b, d_res, d_tag = dev_fill(sc.CHORD), dev_fill(sc.CHORD), dev_fill(3), dev_fill(2)
        db.note_on_idle(sc.notes(sc.CHORD, 1), 0, sc.N, sc.WHICH, sc.SETTLE, 0, d_a.data_ptr(), d_res.data_ptr())
        db.tag_list(d_a.data_ptr(), sc.A_TAGS, 0, d_tag.data_ptr())
        a_assigned, counts, tagged = st.chord_a()
        assert np.array_equal(host_of(d_a), a_assigned) and tuple(u32(d_res)[:2]) == counts and u32(d_tag) == tagged
        assert_state(db, st.truth, "chord A", st.owner)
        mix, _ = db.render_host(64, 1)
        assert (mix == st.block()).all()
        idle_q = fxb.FxIdleQueryC(0, sc.N, sc.WHICH, sc.SETTLE, 0, 0)
        db.note_on_steal(sc.notes(sc.CHORD, 2), idle_q, sc.steal_query().c(), d_b.data_ptr(), d_res.data_ptr())
        db.tag_list(d_b.data_ptr(), sc.B_TAGS, 0, d_tag.data_ptr())
        b_assigned, counts, tagged = st.chord_b()
        assert np.array_equal(host_of(d_b), b_assigned) and tuple(u32(d_res)) == counts == (sc.CHORD, 0, sc.CHORD) and u32(d_tag) == tagged
        assert set(b_assigned.tolist()) == set(a_assigned.tolist()), "the scene does not steal"
        assert_state(db, st.truth, "chord B", st.owner)
        mix, _ = db.render_host(64, 1)
        assert (mix == st.block()).all()
        db.release_tags(0, sc.N, sc.A_TAGS, sc.REL, d_res.data_ptr())
        want, _, _ = st.a_off_by_tag()
        assert u32(d_res) == want == [0, 0, sc.CHORD]
        db.stamp_owned(d_a.data_ptr(), sc.A_TAGS, sc.REL, d_res.data_ptr())
        want, _ = st.a_off_guarded(a_assigned)
        assert u32(d_res) == want == [0, sc.CHORD, 0]
        assert_state(db, st.truth, "A's note-offs", st.owner)
        assert (st.truth["sample_release"] == 0).all(), "somebody was released"
        mix, stems = db.render_host(64, 1, want_stems=True)
        want_mix = st.block()
        assert (mix == want_mix).all()
        db.release_tags(0, sc.N, sc.B_TAGS, sc.REL, d_res.data_ptr())
        want, voices, _ = om.release_tags(st.owner, st.truth, 0, sc.N, sc.B_TAGS, sc.REL, st.cnt)
        assert u32(d_res) == want == [sc.CHORD, 0, 0] and np.array_equal(voices, b_assigned)
        assert_state(db, st.truth, "B's note-off", st.owner)
        mix, _ = db.render_host(100, 0)
        assert (mix == st.block(100, 0)).all()
    finally:
        db.close()


def test_fx_owner_refusals_leave_the_bank_usable():
    n = 300
    b, pool, c0 = ctl_bank(n)
    db = open_fx(b, pool, c0)
    ref, cnt, owner = b.copy(), c0, om.new(n)
    try:
        d = dev_fill(16)
        p = d.data_ptr()
        d_two = dev_i32([4, 5])
        db.tag_list(d_two.data_ptr(), [1, 2])
        om.tag_list(owner, [4, 5], [1, 2])
        refused = [
            lambda: db.tag_list(0, [1, 2]),
            lambda: db.find_owned(0, n, [1, 0], p),
            lambda: db.find_owned(0, n, [1, 1], p),
            lambda: db.find_owned(0, n + 1, [1, 2], p),
            lambda: db.find_owned(n, 1, [1, 2], p),
            lambda: db.find_owned(0, 0, [1, 2], p),
            lambda: db.find_owned(0, n, list(range(1, 1026)), p),
            lambda: db.find_owned(0, n, [1, 2], 0),
            lambda: db.stamp_owned(p, [1, 0], REL, p),
            lambda: db.stamp_owned(p, [1, 2], 0, p),
            lambda: db.stamp_owned(p, [1, 2], REL | 1, p),
            lambda: db.stamp_owned(p, [1, 2], REL, 0),
            lambda: db.release_tags(0, n, [1, 1], REL, p),
            lambda: db.release_tags(0, n, [1, 2], REL, 0),
            lambda: db.release_tags(-1, n, [1, 2], REL, p),
            lambda: db.owner_clear(0, n + 1),
            lambda: db.download_owners(1, n),
        ]
        for k, call in enumerate(refused):
            with pytest.raises(device.SkredAmdError):
                call()
            assert (host_of(d) == -7).all(), k
        db.find_owned(0, n, [], p)
        db.stamp_owned(p, [], REL, p)
        db.release_tags(0, n, [], REL, p)
        db.tag_list(p, [])
        assert (host_of(d) == -7).all(), "an empty call wrote something"
        cnt = block(db, ref, pool, cnt, 100, 1, "after the refusals")
        assert_state(db, ref, "after the refusals", owner)
    finally:
        db.close()
