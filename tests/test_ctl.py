"""Patch controllers on the device (skred_bank_ctl_range / skred_bank_ctl_slots / skred_bank_download_ctl), bit for bit.

Every call is held to three things:
  1. DeviceBank.download + download_ctl right after it == tests/ctl_model.py on the uploaded view: every word a controller can store
     and every state word, on every voice (those outside the range, the list and the mask included), and d_result == the model's counts;
  2. a twin bank driven by the host route -- the model's stores written into the host view, skred_bank_update with
     DIRTY_PARAMS | DIRTY_PAN on exactly the voices the model wrote -- downloads the same bytes, and gives the same state and the same
     mix after each of 5 further blocks of 64 frames (checked after every block: 1, 2 and 5 among them);
  3. oracle.cpuref with the model's stores: stems bit for bit (where the family writes stems), state bit for bit, mix within the
     project's 1e-5 relative RMS.
INC_SCALE: every increment and ratio used here gives a NORMAL fp32 product (increments 1e-3 .. 1e2, ratios 0.5 .. 2), or overflows on
purpose; no product is subnormal, so the build's denormal mode does not enter.
"""
import ctypes as C
import types

import numpy as np
import pytest

import ctl_model as M
import slot_model as SM
from oracle import cpuref
from skred_amd import banks, device
from skred_amd.bank import slot_query
from skred_amd.device import ctl
from test_idle import open_bank, render_blocks, traffic_bank
from test_patch_banks import rel_rms
from test_slots import enveloped_patch, slot_notes

DIRTY_PARAMS, DIRTY_PHASE, DIRTY_PAN, TRIG, REL = 1, 2, 8, 256, 512
BAD, RANGE = -2, -4
FILL = -7
F = 64
SEMITONE = 1.0594631


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def rig(dev, bank, tables, g, setup=None):
    return types.SimpleNamespace(db=open_bank(dev, bank, tables, g, setup), twin=open_bank(dev, bank, tables, g, setup), bank=bank,
                                 tables=tables, truth=bank.copy(), gl=g.copy(), mirror=bank.copy(), n=bank.n)


def close(r):
    r.db.close()
    r.twin.close()


def record(bits, l=0, seed=0, **over):
    """A record with distinct finite values per voice of the slot."""
    co = banks.biquad_coeffs(np.array([1]), np.array([700.0 + 90.0 * l + 10.0 * seed], np.float32), np.array([1.2], np.float32), 48000)
    v = dict(phase_inc=0.21 + 0.013 * l + 0.001 * seed, inc_scale=SEMITONE, amp=0.4 + 0.01 * l, pan_left=0.15 + 0.01 * l, pan_right=0.8 - 0.01 * l,
             b0=float(co["b0"][0]), b1=float(co["b1"][0]), b2=float(co["b2"][0]), a1=float(co["a1"][0]), a2=float(co["a2"][0]),
             attack_time=30.0, decay_time=60.0 + l, sustain_level=0.5, release_time=400.0, velocity=0.7 + 0.004 * l, smoothing=0.25,
             fm_depth=0.05, freq_scale=1.0, am_depth=0.1, pan_depth=0.1, cz_depth=0.2, cz_dist=0.3)
    v.update(over)
    return ctl(bits, **v)


def junk():
    c = ctl(0xFFFFFFFF, **{k: float("nan") for k in ("phase_inc", "inc_scale", "amp", "b0", "a2", "velocity", "cz_dist")})
    c.reserved = 9
    return c


def records(K, mask, bits, seed=0, **over):
    """K records: `bits` where the mask has a bit, junk skred_ctl_check would refuse elsewhere."""
    return [record(bits, l, seed, **over) if (mask >> l) & 1 else junk() for l in range(K)]


def downloaded(db, like):
    a = like.copy()
    db.download(a)
    db.download_ctl(a)
    return a


def call(r, ctls, mask, first=None, count=None, entries=None, n=None, d_count=None, tag=""):
    """One controller call on the device route, the model on the oracle's bank and the host view, the host route on the twin."""
    import torch
    res = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if entries is None:
        r.db.ctl_range(ctls, first, count, mask, res.data_ptr())
        want, touched = M.ctl_range((r.truth, r.mirror), ctls, first, count, mask)
    else:
        entries = np.array(entries, np.int32)               # (a copy: a reversed view has a negative stride)
        n = len(entries) if n is None else n
        dl = torch.from_numpy(entries).cuda()
        dc = None if d_count is None else torch.tensor([d_count, 12345], dtype=torch.int32, device="cuda")
        r.db.ctl_slots(ctls, mask, dl.data_ptr(), n, dc.data_ptr() if dc is not None else 0, res.data_ptr())
        want, touched = M.ctl_slots((r.truth, r.mirror), ctls, mask, entries, n, d_count, r.n)
    torch.cuda.synchronize()
    got = res.cpu().numpy().view(np.uint32).tolist()
    print(f"{tag}: d_result {got}, the model {want}, {len(touched)} voices")
    assert got == want, f"{tag}: d_result {got}, the model says {want}"
    a = downloaded(r.db, r.bank)
    assert not M.words_differ(a, r.mirror), f"{tag}: controller words differ from the model: {M.words_differ(a, r.mirror)}"
    assert not a.rw_equal(r.truth), f"{tag}: state differs from the model: {a.rw_equal(r.truth)}"
    if len(touched):
        r.twin.update(r.mirror, touched, DIRTY_PARAMS | DIRTY_PAN)
    b = downloaded(r.twin, r.bank)
    assert not M.words_differ(a, b) and not a.rw_equal(b), f"{tag}: the host route downloads other bytes: {M.words_differ(a, b)} {a.rw_equal(b)}"
    return want, touched


def blocks(r, count=5, stems=True, tag="", twin_mix=True):
    """`count` blocks of F frames on both routes and the oracle, everything compared after every block."""
    for k in range(1, count + 1):
        if stems:
            x, xs = r.db.render_host(F, 2, 0, want_stems=True)
            y, ys = r.twin.render_host(F, 2, 0, want_stems=True)
        else:
            x, y = render_blocks(r.db, (F,))[0], render_blocks(r.twin, (F,))[0]
        ref = cpuref.render(r.truth, r.gl, r.tables, F, 0, want_stems=stems)
        ref_mix = cpuref.master(r.gl, ref["sum64"].astype(np.float32))
        err = rel_rms(x, ref_mix)
        print(f"{tag} block {k}: mix rel rms vs the oracle {err:.3g}, equal to the host route: {x.tobytes() == y.tobytes()}")
        if stems:
            assert xs.tobytes() == ys.tobytes(), f"{tag} block {k}: the two routes' stems differ"
            assert xs.tobytes() == ref["stems"].tobytes(), f"{tag} block {k}: stems differ from the oracle"
        if twin_mix:
            assert x.tobytes() == y.tobytes(), f"{tag} block {k}: the two routes' mixes differ"
        assert err <= 1e-5, f"{tag} block {k}: mix rel rms {err}"
        a, b = r.bank.copy(), r.bank.copy()
        r.db.download(a)
        r.twin.download(b)
        assert not a.rw_equal(r.truth), f"{tag} block {k}: state differs from the oracle: {a.rw_equal(r.truth)}"
        assert not a.rw_equal(b), f"{tag} block {k}: state differs from the host route: {a.rw_equal(b)}"
        assert r.db.last_kernel() == r.twin.last_kernel(), (tag, k, r.db.last_kernel(), r.twin.last_kernel())
    a = downloaded(r.db, r.bank)
    assert not M.words_differ(a, r.mirror), f"{tag}: a block changed a controller word: {M.words_differ(a, r.mirror)}"


# ---------------------------------------------------------------------------------------------- 1. every bit, every shape

@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 4, 64])
def test_every_bit_alone_and_all_together(dev, K):
    """Every SKRED_CTL_* bit on its own and all of them together, over: the whole bank; one slot; a range that starts and ends inside
    a 64-voice group (K <= 16); 832 voices from voice 64 (four workgroups of the range kernel, the last one partial) with the single
    high bit K - 1 as the mask; the same shapes through a list.  K = 1, mask 1: per-voice calls."""
    n = 1088
    bank, tables, g = banks.bank_c2(n)
    bank["voice_amp"][5::8] = 0.0                     # voices the AMP guard must leave alone
    bank["voice_amp"][6::16] = np.float32(-0.0)
    full, high = (1 << K) - 1 if K < 64 else (1 << 64) - 1, 1 << (K - 1)
    alt = full if K == 1 else sum(1 << l for l in range(0, K, 2)) | high
    shapes = [(0, n - n % K, full), (K, K, full), (64, 832, high), (64 * (n // 64 - 1), 64, alt)]
    if K <= 16:
        shapes.append((64 + K, 32, alt))
    r = rig(dev, bank, tables, g)
    try:
        blocks(r, 1, tag="before")
        for i, bit in enumerate(M.BITS):
            first, count, mask = shapes[i % len(shapes)]
            call(r, records(K, mask, bit, i), mask, first, count, tag=f"K {K} bit {bit:#x} range [{first},+{count}) mask {mask:#x}")
            first, count, mask = shapes[(i + 2) % len(shapes)]
            entries = np.arange(first, first + count, K, dtype=np.int32)[::-1][:300]
            call(r, records(K, mask, bit, i + 20), mask, entries=entries, tag=f"K {K} bit {bit:#x} list of {len(entries)} mask {mask:#x}")
        assert (r.truth["voice_amp"][5::8] == 0).all() and (r.mirror["voice_amp"][5::8] == 0).all()
        blocks(r, 2, tag="after the single bits")
        for bits in (M.ALL & ~M.INC_SCALE, M.ALL & ~M.PHASE_INC):
            for first, count, mask in shapes[:3]:
                call(r, records(K, mask, bits, 7), mask, first, count, tag=f"K {K} all bits {bits:#x} [{first},+{count})")
        blocks(r, 5, tag="after all bits together")
    finally:
        close(r)


# ---------------------------------------------------------------------------------------------- 2. padding voices, list rules

@pytest.mark.gpu
def test_a_bank_of_200_voices_with_padding_behind_the_range(dev):
    n, K = 200, 8
    bank, tables, g = banks.bank_c2(n)
    r = rig(dev, bank, tables, g)
    try:
        call(r, records(K, 0xFF, M.FILTER | M.PAN | M.AMP, 1), 0xFF, 0, n, tag="the whole bank")
        call(r, records(K, 0x80, M.ENV_TIMES | M.VELOCITY, 2), 0x80, 192, 8, tag="the last slot, high bit")
        call(r, records(K, 0x81, M.SMOOTHING | M.INC_SCALE, 3), 0x81, entries=[192, 200, 196, 0, 208], tag="a list at the end of the bank")
        blocks(r, 5, tag="200 voices")
    finally:
        close(r)


@pytest.mark.gpu
def test_list_holes_duplicates_and_counts(dev):
    """-1 holes, entries that are not a multiple of K or lie past the bank, a slot named twice (absolute stores: the same as once,
    counted twice), *d_count smaller than n, and no count at all."""
    n, K, mask = 320, 8, 0x55
    bank, tables, g = banks.bank_c2(n)
    bank["voice_amp"][2::16] = 0.0
    entries = np.array([8, -1, 12, 320, 8, 312, -8, 2**31 - 8, -2**31, 16, 24, 32], np.int32)
    r = rig(dev, bank, tables, g)
    try:
        blocks(r, 1, tag="before")
        ctls = records(K, mask, M.AMP | M.FILTER | M.PAN | M.PHASE_INC, 4)
        want, touched = call(r, ctls, mask, entries=entries, d_count=10, tag="with a count of 10")
        assert want[0] == 4 * 4 and want[1] > 0 and set(touched) == {e + l for e in (8, 312, 16) for l in (0, 2, 4, 6)}
        want, touched = call(r, records(K, mask, M.VELOCITY | M.ENV_TIMES, 5), mask, entries=entries, tag="without a count")
        assert want[0] == 6 * 4
        want, touched = call(r, records(K, mask, M.PAN, 6), mask, entries=entries, n=3, d_count=10, tag="n smaller than the count")
        assert want[0] == 1 * 4                                 # (8, -1, 12: one slot)
        want, touched = call(r, records(K, mask, M.PAN, 6), mask, entries=entries, d_count=0, tag="a count of 0")
        assert want == [0, 0] and len(touched) == 0
        blocks(r, 5, tag="after the lists")
    finally:
        close(r)


# ---------------------------------------------------------------------------------------------- 3. the two guards

@pytest.mark.gpu
def test_amp_and_depths_on_a_modulated_patch(dev):
    """18.sk tiled (the modulated kernel): its unused voices have amp 0 and stay there under a bank-wide AMP, counted in
    d_result[1]; every modulation depth, the frequency scale and the CZ words at values of the patch's own size."""
    n, K = 512, 16
    bank, tables, g = banks.bank_patch("18sk", n)
    zero = int((bank["voice_amp"] == 0).sum())
    assert 0 < zero < n
    r = rig(dev, bank, tables, g)
    try:
        blocks(r, 1, tag="18sk before")
        ctls = [record(M.AMP, l, amp=float(np.float32(0.8) * bank["voice_amp"][l]) if bank["voice_amp"][l] != 0 else 0.5) for l in range(K)]
        want, _ = call(r, ctls, 0xFFFF, 0, n, tag="18sk amp")
        assert want == [n, zero] and int((r.truth["voice_amp"] == 0).sum()) == zero
        depth = M.FM_DEPTH | M.FREQ_SCALE | M.AM_DEPTH | M.PAN_DEPTH | M.CZ_DEPTH | M.CZ_DIST
        ctls = [record(depth, l, fm_depth=float(np.float32(0.5) * bank["voice_freq_mod_depth"][l]), freq_scale=float(bank["voice_freq_scale"][l]),
                       am_depth=float(np.float32(0.5) * bank["voice_amp_mod_depth"][l]), pan_depth=float(np.float32(0.5) * bank["voice_pan_mod_depth"][l]),
                       cz_depth=float(np.float32(0.5) * bank["voice_cz_mod_depth"][l]), cz_dist=float(np.float32(0.5) * bank["voice_cz_distortion"][l]))
                for l in range(K)]
        call(r, ctls, 0xFFFF, 0, n // 2, tag="18sk depths")
        blocks(r, 5, tag="18sk")
        assert r.db.last_kernel() == 2, r.db.last_kernel()
    finally:
        close(r)


@pytest.mark.gpu
def test_inc_scale_keeps_an_increment_whose_product_overflows(dev):
    n = 256
    bank, tables, g = banks.bank_c2(n)
    bank["voice_phase_inc"][7], bank["voice_amp"][7] = np.float32(3e38), 0.0      # (amp 0: the voice is skipped, its increment never runs)
    bank["voice_phase_inc"][200], bank["voice_amp"][200] = np.float32(-3e38), 0.0
    inc0 = bank["voice_phase_inc"].copy()
    with np.errstate(over="ignore"):
        products = inc0.astype(np.float32) * np.float32(2.0)
    fin = np.isfinite(products)
    assert (np.abs(products[fin]) >= np.finfo(np.float32).tiny).all(), "a subnormal product"
    r = rig(dev, bank, tables, g)
    try:
        want, _ = call(r, [record(M.INC_SCALE, inc_scale=2.0)], 1, 0, n, tag="scale by 2")
        assert want == [n, 2]
        a = downloaded(r.db, bank)
        assert a["voice_phase_inc"][7] == np.float32(3e38) and a["voice_phase_inc"][200] == np.float32(-3e38)
        assert a["voice_phase_inc"][fin].tobytes() == products[fin].tobytes()
        call(r, [record(M.INC_SCALE, inc_scale=0.5 * SEMITONE)], 1, 0, n, tag="back down, a semitone up")
        blocks(r, 5, tag="after the bends")
    finally:
        close(r)


# ---------------------------------------------------------------------------------------------- 4. a controller inside a note

@pytest.mark.gpu
@pytest.mark.parametrize("patch,members,voices", [("3sk", (0, 1, 2), (0, 1, 2, 3)), ("18sk", (0, 10), (0, 1, 2, 10))])
def test_a_controller_between_a_note_on_and_its_note_off(dev, patch, members, voices):
    """note_on_idle_slots, two blocks, a controller on the chord's d_assigned (a bend, a louder and wider voice, a longer release),
    two blocks, stamp_slots, blocks to the end of the old release time: the host route and the oracle throughout."""
    import torch
    n, chord = 512, 5
    bank, tables, g, K = enveloped_patch(patch, n, members)
    mmask, vmask = sum(1 << l for l in members), sum(1 << l for l in voices)
    r = rig(dev, bank, tables, g)
    try:
        blocks(r, 4, tag="to rest")
        q = slot_query(0, n, K, mmask, SM.FIN | SM.ENV, 1e-3, (n // K // 2) * K, chord + 2)
        notes = slot_notes(chord + 2, K, vmask, 4)
        da = torch.full((chord + 2 + 8,), FILL, dtype=torch.int32, device="cuda")
        dr = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.db.note_on_idle_slots(notes, q, vmask, da.data_ptr(), dr.data_ptr())
        picks, total = r.twin.find_idle_slots_host(q)
        assert len(picks) == chord + 2
        touched = SM.store_notes((r.truth, r.mirror), r.truth, notes, K, vmask, picks, r.gl.synth_sample_count)
        r.twin.update(r.mirror, touched, DIRTY_PARAMS | DIRTY_PHASE | TRIG)
        blocks(r, 2, tag="the chord")
        assigned = da.cpu().numpy()[:chord + 2]
        assert np.array_equal(assigned, picks)
        # the controller on "this chord only": the device route reads d_assigned itself
        bits = M.INC_SCALE | M.AMP | M.PAN | M.VELOCITY | M.ENV_TIMES | M.SMOOTHING
        ctls = records(K, vmask, bits, 2, attack_time=20.0, decay_time=50.0, sustain_level=0.7, release_time=250.0)
        res = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
        r.db.ctl_slots(ctls, vmask, da.data_ptr(), chord + 2, 0, res.data_ptr())
        want, ctouched = M.ctl_slots((r.truth, r.mirror), ctls, vmask, picks, chord + 2, None, n)
        r.twin.update(r.mirror, ctouched, DIRTY_PARAMS | DIRTY_PAN)
        torch.cuda.synchronize()
        assert res.cpu().numpy().view(np.uint32).tolist() == want and set(ctouched) == set(touched)
        a = downloaded(r.db, bank)
        assert not M.words_differ(a, r.mirror), M.words_differ(a, r.mirror)
        blocks(r, 2, tag="the controller")
        r.db.stamp_slots(da.data_ptr(), chord + 2, K, vmask, REL)
        r.twin.update(r.mirror, touched, REL)
        SM.stamp(r.truth, touched, REL, r.gl.synth_sample_count)
        blocks(r, 2, tag="the release")
        e = r.truth["voice_amp_envelope"]
        env = touched[r.truth["voice_use_amp_envelope"][touched] != 0]
        assert len(env) and (e["is_active"][env] == 1).all(), "the longer release (250 frames, not 100) must still run after 128 frames"
        blocks(r, 3, tag="the end")
        assert (e["is_active"][env] == 0).all()
    finally:
        close(r)


# ---------------------------------------------------------------------------------------------- 5. the two-per-lane family

@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
def test_two_per_lane_bank_wide_controllers(dev, mode):
    """traffic_bank(4096) with SKRED_OPT_FAST2_MIN_VOICES = 0 (the option then admits every size; 4096 voices is the bank the project's
    other two-per-lane control tests run) and SKRED_OPT_IN_PLACE = `mode`.  A bank-wide FILTER + PAN + depth controller lists nobody
    and leaves the planner's view of the (empty) list alone: no list violation, last_kernel and last_in_place as on the twin, state
    bit for bit; the host route lists every voice, so its mix is another summation and is held to the oracle's 1e-5 here.  A bank-wide AMP controller lists every voice on both routes: mixes
    bit for bit."""
    n, K = 4096, 8
    bank, tables, g = traffic_bank(n)
    setup = lambda d: (d.fast2_min_voices(0), d.in_place(mode))   # noqa: E731
    r = rig(dev, bank, tables, g, setup)
    try:
        blocks(r, 3, stems=False, tag=f"mode {mode} steady")
        assert r.db.last_kernel() == 3
        sweep = M.FILTER | M.PAN | M.FM_DEPTH | M.AM_DEPTH | M.PAN_DEPTH | M.CZ_DEPTH | M.CZ_DIST | M.PHASE_INC
        call(r, records(K, 0xFF, sweep, 1), 0xFF, 0, n, tag=f"mode {mode} sweep")
        for k in range(3):
            blocks(r, 1, stems=False, tag=f"mode {mode} after the sweep {k}", twin_mix=False)
            got = (r.db.last_kernel(), r.db.last_in_place(), r.db.list_violations())
            ref = (r.twin.last_kernel(), r.twin.last_in_place(), r.twin.list_violations())
            print(f"mode {mode} block {k} after the sweep: (kernel, in place, violations) device route {got}, host route {ref}")
            assert got[2] == 0 and ref[2] == 0
            assert got[0] == ref[0] == 3
            assert got[1] == ref[1], f"last_in_place: device route {got[1]}, host route {ref[1]}"
        call(r, records(K, 0xFF, M.AMP | M.VELOCITY, 2), 0xFF, 0, n, tag=f"mode {mode} amp")
        blocks(r, 4, stems=False, tag=f"mode {mode} after the amp")
        assert r.db.last_kernel() == 3 and r.db.list_violations() == r.twin.list_violations() == 0
        assert r.db.last_in_place() == r.twin.last_in_place()
    finally:
        close(r)


# ---------------------------------------------------------------------------------------------- 6. no host wait

@pytest.mark.gpu
def test_stream_order_without_a_host_wait(dev):
    """Other work, three blocks, a controller, a block -- on one stream of the caller's, nothing waited for until the end: the call
    returns while the stream is still busy, and the caller's array is scribbled over as soon as it does."""
    import torch
    n, K, FR = 4096, 4, 512
    bank, tables, g = banks.bank_c2(n)
    db = open_bank(dev, bank, tables, g)
    truth, gl = bank.copy(), g.copy()
    try:
        s = torch.cuda.Stream()
        outs = [torch.zeros(FR, 2, device="cuda") for _ in range(4)]
        res = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
        ctls = records(K, 0xF, M.FILTER | M.AMP | M.INC_SCALE, 3)
        kept = [ctl(c.set, **{f: getattr(c, f) for f, _ in c._fields_[1:-1]}) for c in ctls]
        arr = device.ctl_array(ctls)
        x = torch.randn(8192, 8192, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):                           # tens of milliseconds of work ahead of the bank's on the same stream
            for _ in range(8):
                y = x @ x
        for o in outs[:3]:
            db.render_mix(FR, o.data_ptr(), 2, 0, 0, s.cuda_stream)
        db.ctl_range(arr, 0, n, 0xF, res.data_ptr(), s.cuda_stream)
        busy = not s.query()
        C.memset(arr, 0xFF, C.sizeof(arr))                   # the array is the caller's again
        db.render_mix(FR, outs[3].data_ptr(), 2, 0, 0, s.cuda_stream)
        s.synchronize()
        print("the stream was still busy when ctl_range returned:", busy)
        for _ in range(3):
            cpuref.render(truth, gl, tables, FR, 0)
        want, _ = M.ctl_range((truth,), kept, 0, n, 0xF)
        ref = cpuref.render(truth, gl, tables, FR, 0)
        assert res.cpu().numpy().view(np.uint32).tolist() == want
        a = downloaded(db, bank)
        assert not M.words_differ(a, truth) and not a.rw_equal(truth), (M.words_differ(a, truth), a.rw_equal(truth))
        assert busy, "the stream had already run dry when the call returned"
        del y
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 7. refusals

@pytest.mark.gpu
def test_refusals_write_nothing(dev):
    import torch
    n, K = 200, 8
    bank, tables, g = banks.bank_c2(n)
    db = open_bank(dev, bank, tables, g)
    try:
        L = db.L
        good = device.ctl_array(records(K, 0xFF, M.FILTER | M.AMP, 1))
        p = C.cast(good, C.c_void_p)
        res = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
        dl = torch.tensor([0, 8, 16], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def rng(h=db.h, c=p, first=0, count=n, k=K, m=0xFF):
            return L.skred_bank_ctl_range(h, c, first, count, k, m, res.data_ptr(), None)

        def lst(h=db.h, c=p, k=K, m=0xFF, sl=dl.data_ptr(), cnt=3):
            return L.skred_bank_ctl_slots(h, c, k, m, sl or None, cnt, None, res.data_ptr(), None)

        assert rng(h=None) == BAD and rng(c=None) == BAD and rng(m=0) == BAD and rng(m=0x1FF) == BAD
        assert rng(k=3) == RANGE and rng(k=128) == RANGE and rng(first=4) == RANGE and rng(count=196) == RANGE
        assert rng(first=-8) == RANGE and rng(count=-8) == RANGE and rng(count=208) == RANGE and rng(first=200, count=8) == RANGE
        assert lst(h=None) == BAD and lst(c=None) == BAD and lst(sl=0) == BAD and lst(cnt=-1) == BAD and lst(k=5) == RANGE and lst(m=0) == BAD
        for bad in (ctl(0), ctl(M.PHASE_INC | M.INC_SCALE, phase_inc=0.1, inc_scale=1.0), ctl(M.AMP, amp=0.0), ctl(M.PAN, pan_left=float("inf")),
                    ctl(1 << 20), junk()):
            recs = records(K, 0xFF, M.FILTER, 1)
            recs[5] = bad
            bp = C.cast(device.ctl_array(recs), C.c_void_p)
            assert rng(c=bp) == BAD and lst(c=bp) == BAD
            assert rng(c=bp, m=0xDF) == 0 and rng(c=bp, m=0xDF, count=0) == 0      # ... and accepted where voice 5 has no bit
        assert rng(count=0) == 0 and rng(first=200, count=0) == 0 and lst(cnt=0) == 0
        torch.cuda.synchronize()
    finally:
        db.close()


@pytest.mark.gpu
def test_refused_calls_leave_the_result_and_the_bank_alone(dev):
    import torch
    n, K = 200, 8
    bank, tables, g = banks.bank_c2(n)
    db = open_bank(dev, bank, tables, g)
    try:
        res = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
        p = C.cast(device.ctl_array(records(K, 0xFF, M.FILTER, 1)), C.c_void_p)
        torch.cuda.synchronize()
        assert db.L.skred_bank_ctl_range(db.h, p, 0, 208, K, 0xFF, res.data_ptr(), None) == RANGE
        assert db.L.skred_bank_ctl_range(db.h, p, 0, 0, K, 0xFF, res.data_ptr(), None) == 0
        assert db.L.skred_bank_ctl_slots(db.h, p, K, 0xFF, res.data_ptr(), -1, None, res.data_ptr(), None) == BAD
        torch.cuda.synchronize()
        assert (res.cpu().numpy() == FILL).all()
        a = downloaded(db, bank)
        assert not M.words_differ(a, bank) and not a.rw_equal(bank)
    finally:
        db.close()
