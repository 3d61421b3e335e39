"""Controllers of the fixed-point bank on the GPU: skred_fxbank_ctl_range / _ctl_list / _ctl_owned.

The expectation is tests/fx_ctl_model.py applied to the ORACLE's bank: after every call EVERY word the device holds (read-write
fields, parameter fields, reciprocals, owner words) and every result word must equal the model's byte for byte, and the blocks
around the calls equal oracle.cpuref.fx_render's mix and stems bit for bit.  Banks of 300 and 1 088 voices (no multiple of 64 or
256), ranges that start off 0 and end inside a workgroup, lists with -1 holes, a d_count shorter than n, a voice listed twice;
voices with and without filter, envelope and smoother, muted, released and silent (amp 0) ones."""
import numpy as np
import pytest

import fx_ctl_model as cm
import fx_owner_model as om
from fx_ctl_gpu import assert_state, block, ctl_bank, dev_fill, dev_i32, host_of, open_fx, u32
from oracle import cpuref
from skred_amd import device, fxbank as fxb
from skred_amd.fxbank import fx_ctl

pytestmark = pytest.mark.gpu

COEFFS = dict(b0_q30=123456789, b1_q30=-246913578, b2_q30=123456789, a1_q30=-1900000000, a2_q30=900000000)
FIELDS = {
    "phase_inc": fx_ctl(fxb.CTL_PHASE_INC, phase_inc=0x01234567),
    "inc_scale": fx_ctl(fxb.CTL_INC_SCALE, inc_scale_q16=69433),                              # a semitone up
    "inc_and_scale": fx_ctl(fxb.CTL_PHASE_INC | fxb.CTL_INC_SCALE, phase_inc=0x00800000, inc_scale_q16=32768),
    "amp": fx_ctl(fxb.CTL_AMP, amp_q15=20000),
    "pan": fx_ctl(fxb.CTL_PAN, pan_left_q15=30000, pan_right_q15=2768),
    "filter": fx_ctl(fxb.CTL_FILTER, **COEFFS),
    "env_times": fx_ctl(fxb.CTL_ENV_TIMES, attack_frames=100, decay_frames=0, release_frames=700, sustain_q15=20000),
    "velocity": fx_ctl(fxb.CTL_VELOCITY, velocity_q15=12345),
    "smoothing": fx_ctl(fxb.CTL_SMOOTHING, smoother_k_q15=3000),
    "all": fx_ctl(fxb.CTL_ALL, phase_inc=0x00765432, inc_scale_q16=61858, amp_q15=30000, pan_left_q15=1000, pan_right_q15=31000,
                  attack_frames=1, decay_frames=300, release_frames=0, sustain_q15=32768, velocity_q15=30000, smoother_k_q15=32768, **COEFFS),
}


@pytest.mark.parametrize("n", [300, 1088])
@pytest.mark.parametrize("field", list(FIELDS))
def test_fx_ctl_range_stores_what_it_names_and_nothing_else(field, n):
    b, pool, c0 = ctl_bank(n)
    c = FIELDS[field]
    db = open_fx(b, pool, c0)
    ref, cnt = b.copy(), c0
    try:
        cnt = block(db, ref, pool, cnt, 65, 1, "before")
        d_res = dev_fill(4)
        for first, count in ((37, n - 37 - 70), (n - 1, 1), (0, n)):                            # off 0 and ending inside a workgroup; the last voice; everyone
            db.ctl_range(c, first, count, d_res.data_ptr())
            want = cm.ctl_range(ref, c, first, count)
            assert u32(d_res)[:2] == want and host_of(d_res)[2:].tolist() == [-7, -7], (first, count)
            assert count == 1 or (want[1] > 0) == bool(c.which & fxb.CTL_AMP), "silent voices are in every range of more than 11"
            assert_state(db, ref, f"{field} [{first},+{count})")
            cnt = block(db, ref, pool, cnt, 64, 1, f"{field} after [{first},+{count})")
        cnt = block(db, ref, pool, cnt, 100, 0, f"{field}: a second block")
        assert_state(db, ref, f"{field} at the end")
    finally:
        db.close()


def test_fx_ctl_inc_scale_overflow_boundary_on_the_device():
    n = 300
    b, pool, c0 = ctl_bank(n)
    b["phase_inc"][[0, 1, 2, 3, 299]] = [0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 1, 0x80000000]
    db = open_fx(b, pool, c0)
    ref = b.copy()
    try:
        d_res = dev_fill(2)
        for c, want in ((fx_ctl(fxb.CTL_INC_SCALE, inc_scale_q16=131072), None),
                        (fx_ctl(fxb.CTL_INC_SCALE | fxb.CTL_PHASE_INC, phase_inc=0x10001, inc_scale_q16=0xFFFFFFFF), [n, n]),
                        (fx_ctl(fxb.CTL_INC_SCALE | fxb.CTL_PHASE_INC, phase_inc=0x10000, inc_scale_q16=0xFFFFFFFF), [n, 0])):
            db.ctl_range(c, 0, n, d_res.data_ptr())
            res = cm.ctl_range(ref, c, 0, n)
            assert u32(d_res) == res and (want is None or res == want)
            assert_state(db, ref, f"scale {c.inc_scale_q16:#x}")
            if want is None:
                assert res[1] >= 3 and ref["phase_inc"][:4].tolist() == [0xFFFFFFFE, 0x80000000, 0xFFFFFFFF, 2]
        assert (ref["phase_inc"] == 0xFFFFFFFF).all()
        block(db, ref, pool, c0, 64, 1, "every increment at its ceiling")
    finally:
        db.close()


@pytest.mark.parametrize("n", [300, 1088])
def test_fx_ctl_list_and_owned_equal_the_model(n):
    b, pool, c0 = ctl_bank(n)
    db = open_fx(b, pool, c0)
    ref, cnt, owner = b.copy(), c0, om.new(n)
    try:
        cnt = block(db, ref, pool, cnt, 65, 1, "before")
        rng = np.random.default_rng(n)
        voices = rng.permutation(n)[:280].astype(np.int32)
        lst = np.concatenate([voices, voices[:3]]).astype(np.int32)                             # three voices listed twice
        lst[[5, 100, 279]] = [-1, n, -2**31]
        d_lst, d_res, d_cnt = dev_i32(lst), dev_fill(5), dev_i32([260, 0])
        absolute = fx_ctl(fxb.CTL_ALL & ~fxb.CTL_INC_SCALE, phase_inc=0x00765432, amp_q15=30000, pan_left_q15=1000, pan_right_q15=31000,
                          attack_frames=10, decay_frames=300, release_frames=50, sustain_q15=9000, velocity_q15=30000,
                          smoother_k_q15=700, **COEFFS)
        for c, count in ((absolute, None), (FIELDS["inc_scale"], 260), (FIELDS["pan"], 260)):
            db.ctl_list(c, d_lst.data_ptr(), len(lst), d_cnt.data_ptr() if count else 0, d_res.data_ptr())
            want = cm.ctl_list(ref, c, lst, len(lst), count)
            assert u32(d_res)[:2] == want and host_of(d_res)[2:].tolist() == [-7, -7, -7]
            assert want[0] == (len(lst) - 3 if count is None else 258)
            assert_state(db, ref, f"ctl_list {c.which:#x}")
            cnt = block(db, ref, pool, cnt, 64, 1, f"after ctl_list {c.which:#x}")
        # ---- the guarded form: tag half of the list, ask with some wrong tags
        tags = (0x80000000 + np.arange(len(lst))).astype(np.uint32)
        tags[280:] = tags[:3]                                                                    # (the voices listed twice carry one tag)
        db.tag_list(d_lst.data_ptr(), tags[:140], 0, 0)
        om.tag_list(owner, lst, tags[:140])
        ask = tags.copy()
        ask[[1, 50, 139]] ^= 1
        for c, count in ((FIELDS["all"], None), (FIELDS["filter"], 260)):
            if c.which & fxb.CTL_INC_SCALE:
                ask[280:] ^= 2                                                                   # the second listing of a voice misses the guard
            db.ctl_owned(c, d_lst.data_ptr(), ask, d_cnt.data_ptr() if count else 0, d_res.data_ptr())
            want = cm.ctl_list(ref, c, lst, len(lst), count, owner, ask)
            assert u32(d_res)[:3] == want and host_of(d_res)[3:].tolist() == [-7, -7]
            assert want[0] > 100 and want[2] > 100
            assert_state(db, ref, f"ctl_owned {c.which:#x}", owner)
            cnt = block(db, ref, pool, cnt, 64, 1, f"after ctl_owned {c.which:#x}")
        # ---- a controller whose guard misses everywhere stores nothing
        db.ctl_owned(FIELDS["all"], d_lst.data_ptr(), np.full(len(lst), 0x42, np.uint32), 0, d_res.data_ptr())
        assert u32(d_res)[:3] == [0, 0, len(lst) - 3]
        assert_state(db, ref, "a guard that misses everywhere", owner)
    finally:
        db.close()


def test_fx_ctl_owned_equals_a_twin_driven_by_update():
    """`db` moves a chord's controls with ctl_owned; `twin` gets the same values through host-view writes and skred_fxbank_update of
    exactly the voices the guard lets through.  Same download, same blocks; a third bank that makes no owner or controller call at
    all renders what the oracle renders without them."""
    n = 300
    b, pool, c0 = ctl_bank(n)
    db, twin, idle = open_fx(b, pool, c0), open_fx(b, pool, c0), open_fx(b, pool, c0)
    ref, cnt, owner = b.copy(), c0, om.new(n)
    plain, plain_cnt = b.copy(), c0
    try:
        for d in (twin, idle):
            d.render_host(65, 1)
        cnt = block(db, ref, pool, cnt, 65, 1, "before")
        _, _, plain_cnt = cpuref.fx_render(plain, pool, plain_cnt, 65, 1)
        chord = np.arange(7, n, 9).astype(np.int32)
        tags = (100 + np.arange(len(chord))).astype(np.uint32)
        d_chord = dev_i32(chord)
        db.tag_list(d_chord.data_ptr(), tags)
        om.tag_list(owner, chord, tags)
        stolen = chord[::4]
        d_stolen = dev_i32(stolen)
        db.tag_list(d_stolen.data_ptr(), tags[::4] + 5000)
        om.tag_list(owner, stolen, tags[::4] + 5000)
        c = fx_ctl(fxb.CTL_ALL & ~(fxb.CTL_INC_SCALE | fxb.CTL_AMP), phase_inc=0x00654321, pan_left_q15=5000, pan_right_q15=27768,
                   attack_frames=200, decay_frames=100, release_frames=4000, sustain_q15=15000, velocity_q15=25000, smoother_k_q15=1500,
                   **COEFFS)
        d_res = dev_fill(3)
        db.ctl_owned(c, d_chord.data_ptr(), tags, 0, d_res.data_ptr())
        want = cm.ctl_list(ref, c, chord, len(chord), None, owner, tags)
        assert u32(d_res) == want == [len(chord) - len(stolen), 0, len(stolen)]
        kept = np.setdiff1d(chord, stolen).astype(np.int32)
        h = b.copy()
        for name in cm.STORED:
            if name != "amp_q15":
                h[name][kept] = getattr(c, name)
        twin.update(h, kept, fxb.DIRTY_PARAMS | fxb.DIRTY_PAN)
        got_db, got_twin = ref.copy(), ref.copy()
        db.download(got_db)
        twin.download(got_twin)
        r_db, r_twin = db.download_params(got_db), twin.download_params(got_twin)
        assert all(got_db[k].tobytes() == got_twin[k].tobytes() for k in got_db.a) and r_db.tobytes() == r_twin.tobytes()
        assert_state(db, ref, "ctl_owned", owner)
        for frames, interp in ((64, 1), (100, 0)):
            m_twin, s_twin = twin.render_host(frames, interp, want_stems=True)
            m_db, s_db = db.render_host(frames, interp, want_stems=True)
            assert (m_db == m_twin).all() and (s_db == s_twin).all(), "the device-side path and the update path differ"
            want_mix, want_st, cnt = cpuref.fx_render(ref, pool, cnt, frames, interp, want_stems=True)
            assert (m_db == want_mix).all() and (s_db == want_st).all()
            m_idle, _ = idle.render_host(frames, interp)
            want_plain, _, plain_cnt = cpuref.fx_render(plain, pool, plain_cnt, frames, interp)
            assert (m_idle == want_plain).all() and not (m_idle == m_db).all()
    finally:
        for d in (db, twin, idle):
            d.close()


def test_fx_ctl_stream_order_without_a_host_wait():
    """A block, a bank-wide controller, a guarded controller, a note-off by id and a second block on ONE stream with ONE synchronise at
    the end: the first block renders the old values, the second the new ones."""
    import torch
    n, frames = 1088, 64
    b, pool, c0 = ctl_bank(n)
    db = open_fx(b, pool, c0)
    ref, owner = b.copy(), om.new(n)
    try:
        chord = np.arange(3, n, 5).astype(np.int32)
        tags = (7 + np.arange(len(chord))).astype(np.uint32)
        ask = tags.copy()
        ask[::2] += 100000                                                                       # every other tag is wrong
        d_chord, d_res = dev_i32(chord), [dev_fill(3) for _ in range(4)]
        mixes = [torch.zeros((frames, 2), dtype=torch.int64, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        q = s.cuda_stream
        db.tag_list(d_chord.data_ptr(), tags, 0, d_res[0].data_ptr(), q)
        db.render(frames, mixes[0].data_ptr(), 1, 0, q)
        db.ctl_range(FIELDS["filter"], 0, n, d_res[1].data_ptr(), q)
        db.ctl_owned(FIELDS["amp"], d_chord.data_ptr(), ask, 0, d_res[2].data_ptr(), q)
        db.release_tags(0, n, tags[:100], fxb.STAMP_RELEASE, d_res[3].data_ptr(), q)
        db.render(frames, mixes[1].data_ptr(), 1, 0, q)
        s.synchronize()
        want = [om.tag_list(owner, chord, tags)]
        mix0, _, cnt = cpuref.fx_render(ref, pool, c0, frames, 1)
        want.append(cm.ctl_range(ref, FIELDS["filter"], 0, n))
        want.append(cm.ctl_list(ref, FIELDS["amp"], chord, len(chord), None, owner, ask))
        want.append(om.release_tags(owner, ref, 0, n, tags[:100], fxb.STAMP_RELEASE, cnt)[0])
        mix1, _, cnt = cpuref.fx_render(ref, pool, cnt, frames, 1)
        assert (host_of(mixes[0]) == mix0).all() and (host_of(mixes[1]) == mix1).all() and not (mix0 == mix1).all()
        for got, w in zip(d_res, want):
            assert u32(got)[:len(w)] == w
        assert want[2][0] > 0 and want[2][2] > 0 and want[3][0] == 100
        assert_state(db, ref, "at the end of the stream", owner)
    finally:
        db.close()


def test_fx_ctl_refusals_leave_the_bank_usable():
    n = 300
    b, pool, c0 = ctl_bank(n)
    db = open_fx(b, pool, c0)
    ref, cnt = b.copy(), c0
    try:
        d = dev_fill(16)
        p = d.data_ptr()
        pan = FIELDS["pan"]
        refused = [
            lambda: db.ctl_range(fx_ctl(0), 0, n, p),
            lambda: db.ctl_range(fx_ctl(fxb.CTL_PAN | 1 << 8, pan_left_q15=1), 0, n, p),
            lambda: db.ctl_range(fx_ctl(fxb.CTL_PAN | 1 << 13, pan_left_q15=1), 0, n, p),
            lambda: db.ctl_range(fx_ctl(fxb.CTL_AMP, amp_q15=0), 0, n, p),
            lambda: db.ctl_range(fx_ctl(fxb.CTL_VELOCITY, velocity_q15=65536), 0, n, p),
            lambda: db.ctl_range(pan, 0, n + 1, p),
            lambda: db.ctl_range(pan, -1, 2, p),
            lambda: db.ctl_range(pan, 0, -1, p),
            lambda: db.ctl_list(pan, 0, 4, 0, p),
            lambda: db.ctl_list(pan, p, -1, 0, p),
            lambda: db.ctl_list(fx_ctl(fxb.CTL_SMOOTHING, smoother_k_q15=32769), p, 4, 0, p),
            lambda: db.ctl_owned(pan, p, [1, 0], 0, p),
            lambda: db.ctl_owned(pan, 0, [1, 2], 0, p),
            lambda: db.ctl_owned(fx_ctl(fxb.CTL_ENV_TIMES, sustain_q15=-1), p, [1, 2], 0, p),
        ]
        for k, call in enumerate(refused):
            with pytest.raises(device.SkredAmdError):
                call()
            assert (host_of(d) == -7).all(), k
        reserved = fx_ctl(fxb.CTL_PAN)
        reserved.reserved[2] = 1
        with pytest.raises(device.SkredAmdError):
            db.ctl_range(reserved, 0, n, p)
        db.ctl_range(pan, 17, 0, p)
        db.ctl_list(pan, p, 0, 0, p)
        db.ctl_owned(pan, p, [], 0, p)
        assert (host_of(d) == -7).all(), "an empty call wrote something"
        assert (db.download_owners() == 0).all()
        cnt = block(db, ref, pool, cnt, 100, 1, "after the refusals")
        assert_state(db, ref, "after the refusals")
    finally:
        db.close()
