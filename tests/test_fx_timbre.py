"""Per-note timbre on the fixed-point bank on the GPU: skred_fxbank_ctl_owned_each_filter / _ctl_tags_each_filter.

The expectation is tests/fx_timbre_model.py applied to the ORACLE's bank: every result word must equal the model's, after every call
EVERY word the device holds (read-write fields -- the delay line with them --, parameter fields, reciprocals, owner words) must equal
the model's byte for byte, and the blocks after the calls equal oracle.cpuref.fx_render's mix and stems bit for bit.  Banks of 600
voices tagged over 16 channels; lists of 1, 2, 1023 and 1024 entries with -1 holes, entries outside the bank and stale tags; a count
word shorter than the list; the range [37, 537).  A twin driven by n single skred_fxbank_ctl_owned calls must hold the same bytes;
with entries given, every word but the five coefficient words must be what skred_fxbank_ctl_owned_each alone leaves on another twin."""
import numpy as np
import pytest

import fx_chan_model as CM
import fx_chan_scenes as CS
import fx_expr_model as em
import fx_live_model as live
import fx_owner_model as om
import fx_timbre_model as tm
from fx_ctl_gpu import assert_state, block, ctl_bank, dev_fill, dev_i32, host_of, open_fx, u32
from oracle import cpuref
from skred_amd import device, fxbank as fxb
from skred_amd.fxbank import fx_ctl, fx_each, fx_filter_each

pytestmark = pytest.mark.gpu

N = 600
DELAY = ("x1", "x2", "y1", "y2")


def open_tagged(n, twins=0):
    b, pool, c0 = ctl_bank(n)
    v = np.arange(n)
    tags = (((v % 16) << 24) | (v + 1)).astype(np.uint32)
    tags[(v >= 300) & (v % 13 == 5)] = 0                                                          # nobody's
    owner = om.new(n)
    om.tag_list(owner, v, tags)
    dbs = [open_fx(b, pool, c0) for _ in range(1 + twins)]
    d_all = dev_i32(v)
    for db in dbs:
        db.tag_list(d_all.data_ptr(), tags)
    return dbs, b.copy(), pool, c0, owner


def coeffs(k):
    """the k-th of a ladder of cutoffs: skred_filter_coeffs' fp32 words as Q2.30, with the int32 extremes mixed in"""
    if k % 97 == 11:
        return fx_filter_each(-(1 << 31), (1 << 31) - 1, 0, -1, 1)
    c = device.filter_coeffs(1 + k % 5, 110.0 * 2.0 ** ((k % 72) / 12.0), 0.7 + 0.01 * (k % 50), 48000.0)
    return fx_filter_each(*[tm.q30(x) for x in c])


def delay_lines(b):
    return [b[k].copy() for k in DELAY if k in b.a]


BASE = fx_ctl(fxb.CTL_AMP | fxb.CTL_SMOOTHING, amp_q15=20000, smoother_k_q15=3000)


def entry(k):
    return fx_each((fxb.EACH_INC_SCALE, fxb.EACH_AMP_SCALE, fxb.EACH_VELOCITY, fxb.EACH_PAN, fxb.EACH_ALL)[k % 5], inc_scale_q16=60000 + 97 * k,
                   amp_scale_q16=1 + 3001 * k, velocity_q15=(k * 131) % 65536, pan_left_q15=(k * 257) % 65536, pan_right_q15=65535 - (k * 257) % 65536)


@pytest.mark.parametrize("n_entries", [1, 2, 1023, 1024])
def test_fx_per_entry_coefficients_equal_the_model_and_the_twins(n_entries):
    (db, singles, plain_each), ref, pool, c0, owner = open_tagged(N, twins=2)
    cnt = c0
    try:
        for t in (singles, plain_each):
            t.render_host(65, 1)
        cnt = block(db, ref, pool, cnt, 65, 1, "before")
        rng = np.random.default_rng(n_entries)
        voices = np.full(n_entries, -1, np.int32)
        pick = rng.permutation(N)[:min(n_entries, N)].astype(np.int32)
        voices[:len(pick)] = pick                                                                # (more entries than voices: -1 holes)
        tags = np.array([owner[v] if v >= 0 and owner[v] else 0x7F000001 + k for k, v in enumerate(voices)], np.uint32)
        if n_entries > 2:
            tags[[7, 70, 170]] ^= 1                                                              # stale tags: counted, the voices untouched
            voices[[5, 100, 279, 280]] = [-1, N, -2**31, N + 5]                                  # holes and out-of-bank entries: skipped
        filt = [coeffs(k) for k in range(n_entries)]
        entries = [entry(k) for k in range(n_entries)]
        d_voices = dev_i32(voices)
        delay = delay_lines(ref)
        assert delay, "the bank has a delay line to leave alone"
        steps = [("a record, entries, coefficients", BASE, entries, None), ("coefficients only", None, None, None),
                 ("entries without a record", None, [fx_each(fxb.EACH_VELOCITY, velocity_q15=k % 65536) for k in range(n_entries)], None),
                 ("a count word", BASE, entries, max(n_entries // 2, 1))]
        for name, c, ee, count in steps:
            before = ref.copy()
            d_res, d_cnt = dev_fill(5), dev_i32([count or 0, 0])
            db.ctl_owned_each_filter(c, ee, filt, d_voices.data_ptr(), tags, d_cnt.data_ptr() if count else 0, d_res.data_ptr())
            want = tm.ctl_owned_each_filter(owner, ref, c, ee, filt, voices, tags, count)
            assert u32(d_res)[:3] == want and host_of(d_res)[3:].tolist() == [-7, -7], (name, u32(d_res), want)
            assert n_entries <= 2 or (want[0] > 200 and want[2] >= 1), want
            assert_state(db, ref, name, owner)
            assert all(np.array_equal(x, y) for x, y in zip(delay, delay_lines(ref))), "the model moved the delay line"
            if c is None and ee is None:
                changed = sorted(k for k in ref.a if not np.array_equal(ref[k], before[k]))
                assert set(changed) <= set(tm.COEFFS), changed
            for k in range(n_entries if count is None else min(count, n_entries)):                # the parent's only route
                if 0 <= voices[k] < N:
                    singles.ctl_owned(tm.single_record(c, ee[k] if ee is not None else None, filt[k]), d_voices.data_ptr() + 4 * k, [tags[k]])
            assert_state(singles, ref, name + ": the twin of single ctl_owned calls", owner)
            if name.startswith("a record"):
                plain_each.ctl_owned_each(c, ee, d_voices.data_ptr(), tags)
                twin_ref = before.copy()
                em.ctl_owned_each(owner, twin_ref, c, ee, voices, tags)
                for k in tm.COEFFS:
                    twin_ref[k][...] = before[k]
                    assert not np.array_equal(ref[k], before[k]) or want[0] == 0
                assert_state(plain_each, twin_ref, name + ": ctl_owned_each alone", owner)
                others = [k for k in ref.a if k not in tm.COEFFS]
                assert all(np.array_equal(ref[k], twin_ref[k]) for k in others), "a word other than the five coefficients differs"
        cnt = block(db, ref, pool, cnt, 64, 1, "the block after")
        # by note id over [37, 537): the tags travel sorted, every set of coefficients stays beside its tag
        uniq = tags.copy()
        for name, c, ee in (("tags", BASE, entries), ("tags, coefficients only", None, None)):
            d_res = dev_fill(4)
            db.ctl_tags_each_filter(c, ee, filt, 37, 500, uniq, d_res.data_ptr())
            want, lst = tm.ctl_tags_each_filter(owner, ref, c, ee, filt, 37, 500, uniq)
            assert u32(d_res)[:3] == want and want[2] == 0 and host_of(d_res)[3] == -7, (name, u32(d_res), want)
            assert all(37 <= v < 537 for v in lst if v >= 0)
            assert_state(db, ref, name, owner)
        for frames, interp in ((64, 1), (100, 0)):
            cnt = block(db, ref, pool, cnt, frames, interp, "at the end")
        assert_state(db, ref, "at the end", owner)
    finally:
        for d in (db, singles, plain_each):
            d.close()


def test_fx_a_chord_with_one_cutoff_per_note():
    """tests/fx_chan_scenes.py's burst bank (the bank_fx recipe): a chord through skred_fxbank_note_on_channel, held to
    tests/fx_chan_model.py, then one cutoff per note by note id.  Two blocks of 64 frames: mix and stems bit for bit against
    oracle.cpuref.fx_render."""
    b, pool, c0, own = CS.burst_bank()
    db = open_fx(b, pool, c0)
    try:
        import torch
        db.tag_list(torch.arange(b.n, dtype=torch.int32, device="cuda").data_ptr(), own)
        ref, cnt = b.copy(), c0
        cnt = block(db, ref, pool, cnt, CS.F, 1, "before")
        iq, sq, match, cap, n, tags = CS.burst_args(1, ref, cnt, own)
        notes = CS.burst_notes(n, 1)
        want, res, _ = CM.burst(ref, cnt, own, iq, sq, match, cap, n)
        d_assigned, d_result = dev_fill(n + 8), dev_fill(6)
        db.note_on_channel(notes, iq, sq.c(), match[0], match[1], cap, tags, d_assigned.data_ptr(), d_result.data_ptr())
        assert host_of(d_result).tolist() == res + [-7, -7] and np.array_equal(host_of(d_assigned)[:n], want)
        live.place_notes(ref, notes, want, res[0], 0, cnt)
        CM.tag(own, want, tags)
        placed = [k for k in range(n) if want[k] >= 0]
        assert len(placed) >= 3
        filt = [fx_filter_each(*[tm.q30(x) for x in device.filter_coeffs(1, 150.0 + 37.0 * k, 0.9, 48000.0)]) for k in range(n)]
        d_res = dev_fill(4)
        order = np.argsort(-tags.astype(np.int64))                                               # the tags descending: the sort has work to do
        db.ctl_tags_each_filter(None, None, [filt[k] for k in order], 0, b.n, tags[order], d_res.data_ptr())
        got, lst = tm.ctl_tags_each_filter(own, ref, None, None, [filt[k] for k in order], 0, b.n, tags[order])
        assert u32(d_res)[:3] == got == [len(placed), 0, 0] and host_of(d_res)[3] == -7
        for k in placed:
            assert ref["b0_q30"][want[k]] == filt[k].b0_q30 and ref["a2_q30"][want[k]] == filt[k].a2_q30
        assert len({int(ref["a1_q30"][want[k]]) for k in placed}) == len(placed)
        assert_state(db, ref, "one cutoff per note", own)
        for k in range(2):
            mix, st = db.render_host(CS.F, 1, want_stems=True)
            want_mix, want_st, cnt = cpuref.fx_render(ref, pool, cnt, CS.F, 1, want_stems=True)
            assert (mix == want_mix).all() and (st == want_st).all(), f"block {k}"
            assert np.abs(want_st[:, [want[j] for j in placed]]).sum() > 0
        assert_state(db, ref, "after the blocks", own)
    finally:
        db.close()


def test_fx_timbre_refusals_leave_the_bank_usable():
    (db,), ref, pool, c0, owner = open_tagged(N)
    try:
        d = dev_fill(16)
        p = d.data_ptr()
        pan, names = fx_ctl(fxb.CTL_PAN, pan_left_q15=1, pan_right_q15=2), fx_ctl(fxb.CTL_FILTER)
        good = [coeffs(0), coeffs(1)]
        resv = [coeffs(0), coeffs(1)]
        resv[1].reserved[0] = 1
        refused = [
            lambda: db.ctl_owned_each_filter(pan, None, good, 0, [1, 2], 0, p),
            lambda: db.ctl_owned_each_filter(pan, None, good, p, [1, 0], 0, p),
            lambda: db.ctl_owned_each_filter(pan, None, resv, p, [1, 2], 0, p),
            lambda: db.ctl_owned_each_filter(names, None, good, p, [1, 2], 0, p),
            lambda: db.ctl_owned_each_filter(pan, [fx_each(0), fx_each(fxb.EACH_PAN)], good, p, [1, 2], 0, p),
            lambda: db.ctl_tags_each_filter(pan, None, good, 0, N, [5, 5], p),
            lambda: db.ctl_tags_each_filter(pan, None, good, 0, N + 1, [5, 6], p),
            lambda: db.ctl_tags_each_filter(names, None, good, 0, N, [5, 6], p),
            lambda: db.ctl_tags_each_filter(None, None, resv, 0, N, [5, 6], p),
        ]
        for k, call in enumerate(refused):
            with pytest.raises(device.SkredAmdError):
                call()
            assert (host_of(d) == -7).all(), k
        L = fxb._bind(device.load())
        t = np.array([1, 2], np.uint32)
        assert L.skred_fxbank_ctl_owned_each_filter(db.h, None, None, None, p, t.ctypes.data, 2, None, None, None) == -2   # no coefficients
        db.ctl_owned_each_filter(pan, None, [], p, [], 0, p)
        db.ctl_tags_each_filter(None, None, [], 0, N, [], p)
        assert (host_of(d) == -7).all(), "an empty call wrote something"
        block(db, ref, pool, c0, 100, 1, "after the refusals")
        assert_state(db, ref, "after the refusals", owner)
    finally:
        db.close()
