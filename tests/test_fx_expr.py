"""Channels and per-note expression on the fixed-point bank on the GPU: skred_fxbank_find_match / _find_match_host / _stamp_match /
_ctl_match / _ctl_owned_each / _ctl_tags_each.

The expectation is tests/fx_expr_model.py applied to the ORACLE's bank: every list, total and result word must equal the model's,
after every writing call EVERY word the device holds (read-write fields, parameter fields, reciprocals, owner words) must equal the
model's byte for byte, and the blocks after the calls equal oracle.cpuref.fx_render's mix and stems bit for bit.  Banks of 1 500
voices tagged over 16 channels (channel << 24 | note id) with untagged voices mixed in, one of 70 000 so the ordered compaction
crosses many workgroups; ranges that start off a multiple of 64 and end inside a wavefront and a workgroup."""
import numpy as np
import pytest

import fx_expr_model as em
import fx_owner_model as om
from fx_ctl_gpu import assert_state, block, ctl_bank, dev_fill, dev_i32, host_of, open_fx, u32
from oracle import cpuref
from skred_amd import device, fxbank as fxb
from skred_amd.fxbank import fx_ctl, fx_each

pytestmark = pytest.mark.gpu

N = 1500
CHANNEL, NOTE, EVERYONE = 0xFF000000, 0xFFFFFFFF, 0
FULL = 600                                                                                     # voices below it are all tagged
COEFFS = dict(b0_q30=123456789, b1_q30=-246913578, b2_q30=123456789, a1_q30=-1900000000, a2_q30=900000000)


def channel_tags(n):
    """channel << 24 | note id over 16 channels; from voice FULL on every thirteenth voice is nobody's"""
    v = np.arange(n)
    tags = (((v % 16) << 24) | (v + 1)).astype(np.uint32)
    tags[(v >= FULL) & (v % 13 == 5)] = 0
    return tags


def open_tagged(n, twins=0):
    """(banks, the oracle's bank, the pool, the clock, the owner words): the banks hold the same voices and the same tags"""
    b, pool, c0 = ctl_bank(n)
    tags = channel_tags(n)
    owner = om.new(n)
    om.tag_list(owner, np.arange(n), tags)
    dbs = [open_fx(b, pool, c0) for _ in range(1 + twins)]
    d_all = dev_i32(np.arange(n))
    for db in dbs:
        db.tag_list(d_all.data_ptr(), tags)                                                      # (a zero tag clears: nobody's)
    return dbs, b.copy(), pool, c0, owner


def close_all(dbs):
    for d in dbs:
        d.close()


# ---------------------------------------------------------------------------------------------- A. masked matches

MATCHES = [(0, EVERYONE), (3 << 24, CHANNEL), (0, CHANNEL), ((7 << 24) | 8, NOTE), (200 << 24, CHANNEL)]
RANGES = [(37, 1), (37, 63), (37, 64), (37, 65), (37, 255), (37, 256), (37, 257), (1243, 257), (0, N)]


def test_fx_find_match_equals_the_model():
    (db,), ref, pool, c0, owner = open_tagged(N)
    try:
        assert db.download_owners().tobytes() == owner.tobytes()
        nobody = 0
        for value, mask in MATCHES:
            for first, count in RANGES:
                want, total = em.find_match(owner, first, count, value, mask)
                nobody += total == 0
                for max_out in sorted({0, max(total // 2, 1), total + 3, count}):
                    d_voices, d_count = dev_fill(count + 8), dev_fill(2)
                    db.find_match(first, count, value, mask, max_out, d_voices.data_ptr() if max_out else 0, d_count.data_ptr())
                    got, cnt = host_of(d_voices), host_of(d_count)
                    tag = (hex(value), hex(mask), first, count, max_out)
                    written = min(total, max_out)
                    assert cnt.view(np.uint32)[0] == total and cnt[1] == -7, tag
                    assert got[:written].tolist() == want[:written].tolist(), tag
                    assert (got[written:] == -7).all(), ("entries past the written part were touched", tag)   # the canary
                    lst, tot = db.find_match_host(first, count, value, mask, max_out)
                    assert tot == total and lst.tolist() == want[:written].tolist(), tag
                    again = dev_fill(count + 8)
                    db.find_match(first, count, value, mask, max_out, again.data_ptr() if max_out else 0, d_count.data_ptr())
                    assert host_of(again).tobytes() == got.tobytes(), ("two queries on the same state differ", tag)
        assert nobody >= len(RANGES), "a value nobody carries: total 0, the list untouched"
        lst, tot = db.find_match_host(0, N, 3 << 24, CHANNEL)
        assert tot == len(lst) > 80 and (owner[lst] >> 24 == 3).all()
    finally:
        db.close()


def test_fx_find_match_over_many_workgroups():
    n = 70000
    (db,), ref, pool, c0, owner = open_tagged(n)
    try:
        for (value, mask), (first, count) in (((5 << 24, CHANNEL), (0, n)), ((0, EVERYONE), (333, n - 400)), ((11 << 24, CHANNEL), (65, 66000))):
            want, total = em.find_match(owner, first, count, value, mask)
            assert total > 3000
            lst, tot = db.find_match_host(first, count, value, mask)
            assert tot == total and lst.tobytes() == want.tobytes()
            cut = total - 1000
            d_voices, d_count = dev_fill(total + 8), dev_fill(2)
            db.find_match(first, count, value, mask, cut, d_voices.data_ptr(), d_count.data_ptr())
            got = host_of(d_voices)
            assert u32(d_count)[0] == total and got[:cut].tobytes() == want[:cut].tobytes() and (got[cut:] == -7).all()
        d_res = dev_fill(4)
        c = fx_ctl(fxb.CTL_PAN | fxb.CTL_AMP, pan_left_q15=111, pan_right_q15=222, amp_q15=4321)
        db.ctl_match(c, 129, n - 130, 9 << 24, CHANNEL, d_res.data_ptr())
        want = em.ctl_match(owner, ref, c, 129, n - 130, 9 << 24, CHANNEL)
        assert u32(d_res)[:3] == want and want[0] > 3000 and want[1] > 0 and host_of(d_res)[3] == -7
        db.stamp_match(129, n - 130, 9 << 24, CHANNEL, fxb.STAMP_RELEASE, d_res.data_ptr())
        want, _ = em.stamp_match(owner, ref, 129, n - 130, 9 << 24, CHANNEL, fxb.STAMP_RELEASE, c0)
        assert u32(d_res)[:2] == want
        assert_state(db, ref, "70 000 voices", owner)
    finally:
        db.close()


def test_fx_stamp_match_and_ctl_match_equal_the_model_and_a_list_driven_twin():
    (db, twin), ref, pool, c0, owner = open_tagged(N, twins=1)
    cnt = c0
    try:
        twin.render_host(65, 1)
        cnt = block(db, ref, pool, cnt, 65, 1, "before")
        pan_amp = fx_ctl(fxb.CTL_PAN | fxb.CTL_AMP, pan_left_q15=30000, pan_right_q15=2768, amp_q15=20000)
        everything = fx_ctl(fxb.CTL_ALL, phase_inc=0x00765432, inc_scale_q16=61858, amp_q15=30000, pan_left_q15=1000, pan_right_q15=31000,
                            attack_frames=1, decay_frames=300, release_frames=0, sustain_q15=32768, velocity_q15=30000, smoother_k_q15=32768,
                            **COEFFS)
        steps = [("stamp", fxb.STAMP_RELEASE, (37, N - 37 - 70), (3 << 24, CHANNEL)),            # most voices miss
                 ("ctl", pan_amp, (37, N - 37 - 70), (4 << 24, CHANNEL)),
                 ("ctl", fx_ctl(fxb.CTL_INC_SCALE, inc_scale_q16=69433), (N - 257, 257), (5 << 24, CHANNEL)),
                 ("stamp", fxb.STAMP_TRIGGER, (37, FULL - 37), (0, EVERYONE)),                    # nobody misses
                 ("ctl", everything, (37, FULL - 37), (0, EVERYONE)),
                 ("stamp", fxb.STAMP_TRIGGER | fxb.STAMP_RELEASE, (0, N), ((6 << 24) | 7, NOTE)),  # one note
                 ("ctl", fx_ctl(fxb.CTL_FILTER, **COEFFS), (0, N), (0, EVERYONE)),
                 ("ctl", pan_amp, (1, 64), (200 << 24, CHANNEL))]                                  # nobody matches
        for k, (kind, what, (first, count), (value, mask)) in enumerate(steps):
            tag = f"step {k}: {kind} [{first},+{count}) {value:#x}/{mask:#x}"
            lst, total = em.find_match(owner, first, count, value, mask)
            d_lst, d_res = dev_i32(lst if total else [-1]), dev_fill(5)
            if kind == "stamp":
                db.stamp_match(first, count, value, mask, what, d_res.data_ptr())
                want, _ = em.stamp_match(owner, ref, first, count, value, mask, what, cnt)
                assert u32(d_res)[:2] == want == [total, count - total] and host_of(d_res)[2:].tolist() == [-7] * 3, tag
                twin.stamp_list(d_lst.data_ptr(), max(total, 1), what)
            else:
                db.ctl_match(what, first, count, value, mask, d_res.data_ptr())
                want = em.ctl_match(owner, ref, what, first, count, value, mask)
                assert u32(d_res)[:3] == want and want[0] == total and want[2] == count - total and host_of(d_res)[3:].tolist() == [-7] * 2, tag
                twin.ctl_list(what, d_lst.data_ptr(), max(total, 1))
            assert_state(db, ref, tag, owner)
            assert_state(twin, ref, tag + " (the twin, driven by the model's list)", owner)
        assert [s for s in steps if s[0] == "ctl"] and want == [0, 0, 64]
        db.ctl_match(pan_amp, 0, N, 7 << 24, CHANNEL)                                             # no result wanted
        em.ctl_match(owner, ref, pan_amp, 0, N, 7 << 24, CHANNEL)
        twin.ctl_list(pan_amp, dev_i32(em.find_match(owner, 0, N, 7 << 24, CHANNEL)[0]).data_ptr(), em.find_match(owner, 0, N, 7 << 24, CHANNEL)[1])
        for frames, interp in ((64, 1), (100, 0)):
            m_twin, s_twin = twin.render_host(frames, interp, want_stems=True)
            m_db, s_db = db.render_host(frames, interp, want_stems=True)
            want_mix, want_st, cnt = cpuref.fx_render(ref, pool, cnt, frames, interp, want_stems=True)
            assert (m_db == want_mix).all() and (s_db == want_st).all() and (m_twin == want_mix).all() and (s_twin == want_st).all()
        assert_state(db, ref, "at the end", owner)
    finally:
        close_all((db, twin))


# ---------------------------------------------------------------------------------------------- B. per-entry values

BASE = fx_ctl(fxb.CTL_AMP | fxb.CTL_SMOOTHING | fxb.CTL_FILTER, amp_q15=20000, smoother_k_q15=3000, **COEFFS)
EACH_CASES = {
    "inc_scale": (BASE, lambda k: fx_each(fxb.EACH_INC_SCALE, inc_scale_q16=60000 + 97 * k)),
    "amp_scale": (BASE, lambda k: fx_each(fxb.EACH_AMP_SCALE, amp_scale_q16=1 + 3001 * k)),
    "velocity": (BASE, lambda k: fx_each(fxb.EACH_VELOCITY, velocity_q15=(k * 131) % 65536)),
    "pan": (BASE, lambda k: fx_each(fxb.EACH_PAN, pan_left_q15=(k * 257) % 65536, pan_right_q15=65535 - (k * 257) % 65536)),
    "all_four": (BASE, lambda k: fx_each(fxb.EACH_ALL, inc_scale_q16=65536 + 11 * k, amp_scale_q16=30000 + 701 * k, velocity_q15=k,
                                         pan_left_q15=65535 - k, pan_right_q15=k)),
    "velocity_replaces": (fx_ctl(fxb.CTL_VELOCITY | fxb.CTL_PAN, velocity_q15=5, pan_left_q15=6, pan_right_q15=7),
                          lambda k: fx_each(fxb.EACH_VELOCITY if k % 2 else fxb.EACH_PAN, velocity_q15=1000 + k, pan_left_q15=k, pan_right_q15=2 * k)),
    "no_record": (None, lambda k: fx_each(fxb.EACH_INC_SCALE | fxb.EACH_VELOCITY | fxb.EACH_PAN, inc_scale_q16=70000 - 13 * k, velocity_q15=40000 + k,
                                          pan_left_q15=k, pan_right_q15=3 * k)),
}


def drive_twin(twin, c, entries, voices, tags, count=None):
    """n single skred_fxbank_ctl_owned calls with the equivalent records (fx_expr_model.single_record)"""
    for k in range(len(tags) if count is None else min(count, len(tags))):
        r = em.single_record(c, entries[k])
        if r is not None:
            twin.ctl_owned(r, dev_i32([voices[k]]).data_ptr(), [tags[k]])


@pytest.mark.parametrize("case", list(EACH_CASES))
def test_fx_ctl_owned_each_equals_the_model_and_n_single_calls(case):
    (db, twin), ref, pool, c0, owner = open_tagged(N, twins=1)
    c, make = EACH_CASES[case]
    cnt = c0
    try:
        twin.render_host(65, 1)
        cnt = block(db, ref, pool, cnt, 65, 1, "before")
        rng = np.random.default_rng(len(case))
        voices = rng.permutation(N)[:300].astype(np.int32)
        tags = np.where(owner[voices] != 0, owner[voices], 0x7F000001).astype(np.uint32)          # untagged voices: a tag nobody carries
        tags[[7, 70, 170]] ^= 1                                                                    # stale tags: counted, the voices untouched
        voices[[5, 100, 279, 280]] = [-1, N, -2**31, N + 5]                                        # holes and out-of-bank entries: skipped
        entries = [make(k) for k in range(len(voices))]
        d_voices, d_res, d_cnt = dev_i32(voices), dev_fill(5), dev_i32([260, 0])
        for count in (None, 260):
            db.ctl_owned_each(c, entries, d_voices.data_ptr(), tags, d_cnt.data_ptr() if count else 0, d_res.data_ptr())
            want = em.ctl_owned_each(owner, ref, c, entries, voices, tags, count)
            assert u32(d_res)[:3] == want and host_of(d_res)[3:].tolist() == [-7, -7], (case, count)
            assert want[0] > 200 and want[2] >= 3, want
            assert_state(db, ref, f"{case} count {count}", owner)
            drive_twin(twin, c, entries, voices, tags, count)
            assert_state(twin, ref, f"{case} count {count}: the twin of single calls", owner)
            cnt = block(db, ref, pool, cnt, 64, 1, f"{case} count {count}: the block after")
            twin.render_host(64, 1)
        if "amp" in case or "all" in case:
            assert want[1] > 0, "silent voices are on the list: their amp is withheld"
        m_twin, s_twin = twin.render_host(100, 0, want_stems=True)
        m_db, s_db = db.render_host(100, 0, want_stems=True)
        want_mix, want_st, cnt = cpuref.fx_render(ref, pool, cnt, 100, 0, want_stems=True)
        assert (m_db == want_mix).all() and (s_db == want_st).all() and (m_twin == m_db).all() and (s_twin == s_db).all()
    finally:
        close_all((db, twin))


def test_fx_ctl_owned_each_edge_products_on_the_device():
    (db,), ref, pool, c0, owner = open_tagged(N)
    try:
        b = ref.copy()
        b["phase_inc"][[10, 11, 12, 13]] = [0x10000, 0x10001, 0x80000000, 0xFFFFFFFF]
        b["amp_q15"][[20, 21]] = 0
        db.upload(b)
        ref = b.copy()
        d_res = dev_fill(3)
        one, full = fx_ctl(fxb.CTL_AMP, amp_q15=1), fx_ctl(fxb.CTL_AMP, amp_q15=65535)
        inc = [fx_each(fxb.EACH_INC_SCALE, inc_scale_q16=s) for s in (0xFFFFFFFF, 0xFFFFFFFF, 131072, 65536)]
        amp = lambda *scales: [fx_each(fxb.EACH_AMP_SCALE, amp_scale_q16=s) for s in scales]
        both = fx_each(fxb.EACH_AMP_SCALE | fxb.EACH_INC_SCALE | fxb.EACH_VELOCITY, amp_scale_q16=1, inc_scale_q16=65537, velocity_q15=777)
        steps = [(None, inc, [10, 11, 12, 13], [4, 2, 0]),                                        # 0xFFFFFFFF stored, 0x100000000 withheld
                 (one, amp(65536, 0x7FFF, 0xFFFF, 0xFFFFFFFF), [30, 31, 32, 33], [4, 2, 0]),       # 1 stored; 0 withheld twice; 65535 stored
                 (full, amp(65536, 65538, 1, 2), [38, 39, 40, 41], [4, 2, 0]),                     # 65535 stored; 65536 and 0 withheld; 1 stored
                 (full, amp(32768, 1), [20, 21], [2, 2, 0]),                                       # device amp 0: withheld once, not twice
                 (full, [both], [13], [1, 2, 0])]                                                  # the increment and the amp: 2 at the most
        for c, entries, voices, result in steps:
            assert (ref["amp_q15"][[v for v in voices if v >= 30]] != 0).all()
            db.ctl_owned_each(c, entries, dev_i32(voices).data_ptr(), owner[voices], 0, d_res.data_ptr())
            want = em.ctl_owned_each(owner, ref, c, entries, voices, owner[voices])
            assert u32(d_res) == want == result, (voices, u32(d_res), want)
            assert_state(db, ref, f"edge products on {voices}", owner)
        assert ref["phase_inc"][[10, 11, 12, 13]].tolist() == [0xFFFFFFFF, 0x10001, 0x80000000, 0xFFFFFFFF]
        assert ref["amp_q15"][[30, 33, 38, 41]].tolist() == [1, 65535, 65535, 1] and ref["amp_q15"][[20, 21]].tolist() == [0, 0]
        assert ref["velocity_q15"][13] == 777
        block(db, ref, pool, c0, 64, 1, "after the edge products")
    finally:
        db.close()


@pytest.mark.parametrize("n_tags", [1, 2, 1023, 1024])
def test_fx_ctl_tags_each_reaches_the_lowest_voice_of_each_tag(n_tags):
    (db,), ref, pool, c0, owner = open_tagged(N)
    cnt = c0
    try:
        # two voices carry one tag (the lower one is reached), and some asked tags are carried by nobody
        dup = np.array([900, 1400], np.int32)
        db.tag_list(dev_i32(dup).data_ptr(), [0x0A0000AA, 0x0A0000AA])
        om.tag_list(owner, dup, [0x0A0000AA, 0x0A0000AA])
        rng = np.random.default_rng(n_tags)
        candidates = np.concatenate([np.unique(owner[owner != 0]), 0x7E000000 + np.arange(40, dtype=np.uint32)]).astype(np.uint32)
        tags = rng.permutation(candidates)[:n_tags].astype(np.uint32)                               # unsorted: the host sorts and permutes
        if n_tags > 2 and 0x0A0000AA not in tags:
            tags[0] = 0x0A0000AA
        assert len(np.unique(tags)) == n_tags
        c = fx_ctl(fxb.CTL_AMP | fxb.CTL_SMOOTHING, amp_q15=25000, smoother_k_q15=2000)
        entries = [fx_each(fxb.EACH_ALL, inc_scale_q16=65000 + k, amp_scale_q16=20000 + 40 * k, velocity_q15=k, pan_left_q15=2 * k,
                           pan_right_q15=65535 - k) for k in range(n_tags)]
        d_res = dev_fill(4)
        for first, count in ((0, N), (37, 1243)):
            db.ctl_tags_each(c, entries, first, count, tags, d_res.data_ptr())
            want, lst = em.ctl_tags_each(owner, ref, c, entries, first, count, tags)
            assert u32(d_res)[:3] == want and want[2] == 0 and host_of(d_res)[3] == -7, (n_tags, first, count)
            assert want[0] == int((lst >= 0).sum()) and (n_tags <= 2 or 1400 not in lst.tolist())
            assert_state(db, ref, f"{n_tags} tags over [{first},+{count})", owner)
            cnt = block(db, ref, pool, cnt, 64, 1, f"{n_tags} tags: the block after")
        db.ctl_tags_each(None, [fx_each(fxb.EACH_VELOCITY, velocity_q15=k) for k in range(n_tags)], 0, N, tags)      # no record, no result
        em.ctl_tags_each(owner, ref, None, [fx_each(fxb.EACH_VELOCITY, velocity_q15=k) for k in range(n_tags)], 0, N, tags)
        assert_state(db, ref, f"{n_tags} tags without a record", owner)
    finally:
        db.close()


def test_fx_match_queries_leave_the_render_alone():
    """A bank that makes only match queries renders the blocks of a twin that makes none, bit for bit."""
    (db, twin), ref, pool, c0, owner = open_tagged(N, twins=1)
    cnt = c0
    try:
        d_voices, d_count = dev_fill(N), dev_fill(2)
        for frames, interp in ((65, 1), (64, 1), (100, 0)):
            db.find_match(0, N, 3 << 24, CHANNEL, N, d_voices.data_ptr(), d_count.data_ptr())
            db.find_match_host(37, 1000, 0, EVERYONE, 10)
            db.find_match(5, 700, 0, EVERYONE, 0, 0, d_count.data_ptr())
            m_db, s_db = db.render_host(frames, interp, want_stems=True)
            m_twin, s_twin = twin.render_host(frames, interp, want_stems=True)
            want_mix, want_st, cnt = cpuref.fx_render(ref, pool, cnt, frames, interp, want_stems=True)
            assert (m_db == m_twin).all() and (s_db == s_twin).all() and (m_db == want_mix).all() and (s_db == want_st).all()
        assert_state(db, ref, "after the queries", owner)
    finally:
        close_all((db, twin))


def test_fx_expr_refusals_leave_the_bank_usable():
    (db,), ref, pool, c0, owner = open_tagged(N)
    try:
        d = dev_fill(16)
        p = d.data_ptr()
        pan, e = fx_ctl(fxb.CTL_PAN, pan_left_q15=1, pan_right_q15=2), [fx_each(fxb.EACH_PAN), fx_each(fxb.EACH_VELOCITY)]
        refused = [
            lambda: db.find_match(0, N, 0x03000001, CHANNEL, 4, p, p),
            lambda: db.find_match(0, N, 3 << 24, CHANNEL, -1, p, p),
            lambda: db.find_match(0, N, 3 << 24, CHANNEL, 4, 0, p),
            lambda: db.find_match(0, N, 3 << 24, CHANNEL, 4, p, 0),
            lambda: db.find_match(0, N + 1, 3 << 24, CHANNEL, 4, p, p),
            lambda: db.find_match(0, 0, 3 << 24, CHANNEL, 4, p, p),
            lambda: db.find_match_host(-1, 8, 3 << 24, CHANNEL, 4),
            lambda: db.stamp_match(0, N, 3 << 24, CHANNEL, 0, p),
            lambda: db.stamp_match(0, N, 3 << 24, CHANNEL, fxb.STAMP_RELEASE, 0),
            lambda: db.stamp_match(0, N, 1, 0, fxb.STAMP_RELEASE, p),
            lambda: db.ctl_match(fx_ctl(0), 0, N, 3 << 24, CHANNEL, p),
            lambda: db.ctl_match(pan, 0, 0, 3 << 24, CHANNEL, p),
            lambda: db.ctl_match(pan, 0, N, 1 << 24, 0x00FFFFFF, p),
            lambda: db.ctl_owned_each(pan, e, 0, [1, 2], 0, p),
            lambda: db.ctl_owned_each(pan, e, p, [1, 0], 0, p),
            lambda: db.ctl_owned_each(pan, [fx_each(0), fx_each(fxb.EACH_PAN)], p, [1, 2], 0, p),
            lambda: db.ctl_owned_each(None, [fx_each(fxb.EACH_AMP_SCALE, amp_scale_q16=65536)], p, [1], 0, p),
            lambda: db.ctl_owned_each(fx_ctl(fxb.CTL_PHASE_INC, phase_inc=5), [fx_each(fxb.EACH_INC_SCALE, inc_scale_q16=65536)], p, [1], 0, p),
            lambda: db.ctl_tags_each(pan, e, 0, N, [5, 5], p),
            lambda: db.ctl_tags_each(pan, e, 0, N + 1, [5, 6], p),
            lambda: db.ctl_tags_each(pan, [fx_each(fxb.EACH_VELOCITY, velocity_q15=65536)], 0, N, [5], p),
        ]
        for k, call in enumerate(refused):
            with pytest.raises(device.SkredAmdError):
                call()
            assert (host_of(d) == -7).all(), k
        db.ctl_owned_each(pan, [], p, [], 0, p)
        db.ctl_tags_each(pan, [], 0, N, [], p)
        assert (host_of(d) == -7).all(), "an empty call wrote something"
        block(db, ref, pool, c0, 100, 1, "after the refusals")
        assert_state(db, ref, "after the refusals", owner)
    finally:
        db.close()
