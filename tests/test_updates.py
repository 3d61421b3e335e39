"""SURVEY 8f "next" #4: block-granular parameter updates on device-resident voices, and the deferred queue.

The voices live in HBM for the whole test: after the initial upload the host NEVER downloads state and never
re-uploads the bank.  Control actions are applied to a host mirror of the PARAMETERS (whose state fields go stale
at once) and pushed with skred_bank_update / skred_bank_defer naming only what they touched.  Truth is the oracle
rendering the same blocks from a bank to which the same actions are applied as plain array stores -- the way the
reference's control path does it (wire.c:606-716 -> synth.c setters) -- with its own, true, state."""
import numpy as np
import pytest

from oracle import cpuref
from skred_amd import banks

pytestmark = pytest.mark.gpu

F = 256


@pytest.fixture(scope="module")
def dev():
    from skred_amd import device
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


class Action:
    """One control action: stores into a bank's arrays (run on the oracle's bank AND on the GPU's host mirror) plus
    the dirty mask that describes them.  `now` is synth_sample_count when the action runs."""

    def __init__(self, voices, dirty, store):
        self.voices, self.dirty, self.store = np.asarray(voices, np.int32), dirty, store

    def apply_to(self, bank, now, true_state=None):
        self.store(bank, self.voices, now, true_state if true_state is not None else bank)


def actions_for_block(k, n, rng, D):
    """A seeded mix of the reference's control actions for block k."""
    out = []
    v = rng.choice(n, 7, replace=False)

    def set_freq(b, vs, now, st):                               # freq_set -> osc_set_freq (synth.c:125-137)
        b["voice_phase_inc"][vs] = (b["voice_phase_inc"][vs] * np.float32(1.0 + 0.1 * ((k % 5) - 2))).astype(np.float32)
    out.append(Action(v[:2], D.DIRTY_PARAMS, set_freq))

    def set_amp(b, vs, now, st):                                # amp_set (synth.c:826-836)
        b["voice_amp"][vs] = np.float32(0.25 + 0.5 * ((k * 7) % 4))
    out.append(Action(v[2:3], D.DIRTY_PARAMS, set_amp))

    def set_pan(b, vs, now, st):                                # pan_set (synth.c:838-847)
        p = np.float32(-0.9 + 0.3 * (k % 7))
        b["voice_pan_left"][vs] = (np.float32(1.0) - p) / np.float32(2.0)
        b["voice_pan_right"][vs] = (np.float32(1.0) + p) / np.float32(2.0)
    out.append(Action(v[3:4], D.DIRTY_PAN, set_pan))

    def set_filter(b, vs, now, st):                             # mmf_set_freq -> mmf_set_params (synth.c:929-1008)
        c = banks.biquad_coeffs(b["voice_filter_mode"][vs], np.full(len(vs), 300.0 + 400.0 * (k % 9), np.float32),
                                np.full(len(vs), 0.9, np.float32), 48000)
        f = b["voice_filter"]
        for name in ("b0", "b1", "b2", "a1", "a2"):
            f[name][vs] = c[name]
    out.append(Action(v[4:5], D.DIRTY_PARAMS, set_filter))

    def toggle_filter(b, vs, now, st):                          # `J0` / `J1`: the bank becomes (or stops being) partly filtered
        b["voice_filter_mode"][vs] = np.where(b["voice_filter_mode"][vs] != 0, 0, 1)
    out.append(Action(v[1:2], D.DIRTY_PARAMS, toggle_filter))

    def toggle_env(b, vs, now, st):                             # amp_set clears voice_use_amp_envelope (synth.c:829-833)
        b["voice_use_amp_envelope"][vs] = 0 if k % 2 else 1
    out.append(Action(v[2:3], D.DIRTY_PARAMS, toggle_env))

    def trigger(b, vs, now, st):                                # voice_trigger: osc_trigger + amp_envelope_trigger
        b["voice_finished"][vs] = 0
        b["voice_phase"][vs] = np.where(b["voice_loop_enabled"][vs] != 0, b["voice_loop_start_f"][vs], np.float32(0.0))
        e = b["voice_amp_envelope"]
        e["sample_start"][vs] = now
        e["sample_release"][vs] = 0
        e["velocity"][vs] = np.float32(0.5 + 0.1 * (k % 5))
        e["is_active"][vs] = 1
    out.append(Action(v[5:6], D.DIRTY_PHASE | D.DIRTY_PARAMS | D.STAMP_TRIGGER, trigger))

    def release(b, vs, now, st):                                # amp_envelope_release: reads the TRUE is_active
        e = b["voice_amp_envelope"]
        act = st["voice_amp_envelope"]["is_active"][vs] != 0
        e["sample_release"][vs[act]] = now
    out.append(Action(v[6:7], D.STAMP_RELEASE, release))
    return out


def test_updates_without_ever_downloading(dev):
    """40 blocks of mixed control actions on a 3000-voice filtered bank (specialised kernel); at block 12 a voice
    gets a non-finite phase increment (the bank needs the generic kernel), at block 20 it gets its own back."""
    D = dev
    n = 3000
    bank, tables, g = banks.bank_c2(n)
    db = dev.DeviceBank(n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    mirror = bank.copy()            # GPU side: parameters current, state stale
    truth, gl = bank.copy(), g.copy()
    rng = np.random.default_rng(11)
    mixes, refs, kernels = [], [], []
    for k in range(40):
        now = gl.synth_sample_count
        acts = actions_for_block(k, n, rng, D)
        if k in (12, 20):
            def flip(b, vs, now_, st, on=(k == 12), inc0=bank["voice_phase_inc"][77]):
                b["voice_phase_inc"][vs] = np.inf if on else inc0    # osc_next's !isfinite() branch: only the generic kernel has it
            acts.append(Action([77], D.DIRTY_PARAMS, flip))
        for a in acts:
            a.apply_to(truth, now)
            a.apply_to(mirror, now, true_state=truth)    # the mirror cannot know is_active; the device does
            db.update(mirror, a.voices, a.dirty)
        m, _ = db.render_host(F, 2, 0)
        mixes.append(m)
        kernels.append(db.last_kernel())
        r = cpuref.render(truth, gl, tables, F, 0)
        refs.append(cpuref.master(gl, r["sum64"].astype(np.float32)))
    got = bank.copy()
    db.download(got)
    db.close()
    assert kernels[0] == 1 and set(kernels[12:20]) == {0} and kernels[-1] == 1, kernels
    bad = got.rw_equal(truth)
    assert not bad, bad
    assert rel_rms(np.concatenate(mixes), np.concatenate(refs)) <= 1e-5


def test_updates_on_a_two_operator_fm_bank(dev):
    """The same 40 blocks of control actions on a two-operator FM bank (every carrier an even voice modulated by the voice
    after it: the two-per-lane kernel with the pair in one lane, envelope hand-over pair by pair), never downloading.  At block
    14 one carrier is rewired to the voice two above it (the bank is no longer of the pair shape: the one-per-lane exchange
    takes over), at block 22 it gets its own modulator back; modulation depths change on the way."""
    D = dev
    n = 4096
    bank, tables, g = banks.bank_c2(n)
    car = np.arange(0, n, 2)
    bank["voice_freq_mod_osc"][car] = car + 1
    bank["voice_freq_mod_depth"][car] = (np.float32(0.1) * (1 + car % 13)).astype(np.float32)
    bank["voice_disconnect"][car[::3] + 1] = 1
    db = dev.DeviceBank(n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    mirror = bank.copy()
    truth, gl = bank.copy(), g.copy()
    rng = np.random.default_rng(23)
    mixes, refs, kernels = [], [], []
    for k in range(40):
        now = gl.synth_sample_count
        acts = actions_for_block(k, n, rng, D)
        acts = [a for a in acts if a.store.__name__ not in ("toggle_filter", "toggle_env")] if k % 3 else acts

        def set_depth(b, vs, now_, st, kk=k):                    # `F1,depth` again with another depth
            b["voice_freq_mod_depth"][vs] = np.float32(0.05 * (1 + kk % 9))
        acts.append(Action(car[rng.choice(len(car), 3, replace=False)], D.DIRTY_PARAMS, set_depth))
        if k in (14, 22):
            def rewire(b, vs, now_, st, far=(k == 14)):
                b["voice_freq_mod_osc"][vs] = vs + (2 if far else 1)
            acts.append(Action([200], D.DIRTY_PARAMS, rewire))
        for a in acts:
            a.apply_to(truth, now)
            a.apply_to(mirror, now, true_state=truth)
            db.update(mirror, a.voices, a.dirty)
        m, _ = db.render_host(F, 2, 0)
        mixes.append(m)
        kernels.append(db.last_kernel())
        r = cpuref.render(truth, gl, tables, F, 0)
        refs.append(cpuref.master(gl, r["sum64"].astype(np.float32)))
    got = bank.copy()
    db.download(got)
    db.close()
    assert kernels[0] == 3 and set(kernels[14:22]) == {1} and kernels[-1] == 3, kernels
    bad = got.rw_equal(truth)
    assert not bad, bad
    assert rel_rms(np.concatenate(mixes), np.concatenate(refs)) <= 1e-5


PARAM_FIELDS = ["voice_phase_inc", "voice_amp", "voice_table_offset", "voice_table_size", "voice_one_shot",
                "voice_loop_enabled", "voice_loop_valid", "voice_loop_start_f", "voice_loop_end_f", "voice_direction",
                "voice_wave_table_index", "voice_use_amp_envelope", "voice_filter_mode", "voice_smoother_enable",
                "voice_smoother_smoothing", "voice_disconnect", "voice_quantize", "voice_sample_hold_max"]


def apply_captured(dst, snap, vs, dirty, now, D):
    """The update protocol restated on numpy banks: what skred_bank_update does to the device, done to `dst`."""
    if dirty & D.DIRTY_PARAMS:
        for name in PARAM_FIELDS:
            dst[name][vs] = snap[name][vs]
        for sub in ("a", "d", "s", "r", "attack_time", "decay_time", "sustain_level", "release_time", "velocity"):
            dst["voice_amp_envelope"][sub][vs] = snap["voice_amp_envelope"][sub][vs]
        for sub in ("b0", "b1", "b2", "a1", "a2"):
            dst["voice_filter"][sub][vs] = snap["voice_filter"][sub][vs]
    if dirty & D.DIRTY_PHASE:
        dst["voice_phase"][vs] = snap["voice_phase"][vs]
        dst["voice_finished"][vs] = snap["voice_finished"][vs]
    if dirty & D.DIRTY_PAN:
        dst["voice_pan_left"][vs] = snap["voice_pan_left"][vs]
        dst["voice_pan_right"][vs] = snap["voice_pan_right"][vs]
    e = dst["voice_amp_envelope"]
    if dirty & D.DIRTY_ENV_CLOCK:
        e["sample_start"][vs] = snap["voice_amp_envelope"]["sample_start"][vs]
        e["sample_release"][vs] = snap["voice_amp_envelope"]["sample_release"][vs]
    if dirty & D.STAMP_TRIGGER:
        e["sample_start"][vs] = now
        e["sample_release"][vs] = 0
        e["is_active"][vs] = 1
    if dirty & D.STAMP_RELEASE:
        act = e["is_active"][vs] != 0
        e["sample_release"][vs[act]] = now


def test_deferred_queue_follows_seq_rule(dev):
    """Items queued with a sample time take effect at the start of the block that contains it: seq() after block k
    runs every item with when <= synth_sample_count + frame_count (seq.c:173).  Values are captured when the item is
    queued; trigger / release stamps read the clock when they RUN, as amp_envelope_trigger / _release read the
    global (synth.c:384,393)."""
    D = dev
    n = 1024
    bank, tables, g = banks.bank_c1(n)
    db = dev.DeviceBank(n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    mirror, truth, gl = bank.copy(), bank.copy(), g.copy()
    t0 = gl.synth_sample_count
    rng = np.random.default_rng(3)
    pending = []                                     # (when, snapshot, voices, dirty) in arrival order
    for i in range(30):
        when = t0 + int(rng.integers(0, 20 * F))
        acts = actions_for_block(i, n, rng, D)
        a = acts[int(rng.integers(0, len(acts)))]
        a.apply_to(mirror, 0, true_state=truth)      # control code stores into the host view ...
        snap = mirror.copy()
        db.defer(when, snap, a.voices, a.dirty)      # ... and queues what it touched
        pending.append((when, snap, a.voices, a.dirty))
    assert db.queue_pending() == 30
    mixes, refs, applied_total = [], [], 0
    for k in range(24):
        horizon = gl.synth_sample_count + F
        applied_total += db.run_queue(F)
        due = [it for it in pending if it[0] <= horizon]
        pending = [it for it in pending if it[0] > horizon]
        for _, snap, vs, dirty in due:
            apply_captured(truth, snap, vs, dirty, gl.synth_sample_count, D)
        m, _ = db.render_host(F, 2, 0)
        mixes.append(m)
        r = cpuref.render(truth, gl, tables, F, 0)
        refs.append(cpuref.master(gl, r["sum64"].astype(np.float32)))
    assert applied_total == 30 and db.queue_pending() == 0 and not pending
    got = bank.copy()
    db.download(got)
    db.close()
    bad = got.rw_equal(truth)
    assert not bad, bad
    assert rel_rms(np.concatenate(mixes), np.concatenate(refs)) <= 1e-5


def test_stamped_note_off_survives_a_later_parameter_update(dev):
    """`release` stamps sample_release on the device; the host mirror still holds 0.  A later PARAMS update of the
    same voice must not bring that 0 back (the envelope clock is its own dirty kind)."""
    D = dev
    n = 512
    bank, tables, g = banks.bank_c1(n)
    db = dev.DeviceBank(n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    mirror, truth, gl = bank.copy(), bank.copy(), g.copy()
    vs = np.array([3, 200], np.int32)
    mixes, refs = [], []
    for k in range(6):
        if k == 1:
            db.update(mirror, vs, D.STAMP_RELEASE)
            apply_captured(truth, mirror, vs, D.STAMP_RELEASE, gl.synth_sample_count, D)
        if k == 2:
            mirror["voice_amp"][vs] = np.float32(0.5)
            db.update(mirror, vs, D.DIRTY_PARAMS)
            truth["voice_amp"][vs] = np.float32(0.5)
        m, _ = db.render_host(4800, 2, 0)
        mixes.append(m)
        r = cpuref.render(truth, gl, tables, 4800, 0)
        refs.append(cpuref.master(gl, r["sum64"].astype(np.float32)))
    got = bank.copy()
    db.download(got)
    db.close()
    assert (truth["voice_amp_envelope"]["is_active"][vs] == 0).all()     # the release ran out (0.2 s)
    assert not got.rw_equal(truth), got.rw_equal(truth)
    assert rel_rms(np.concatenate(mixes), np.concatenate(refs)) <= 1e-5


@pytest.mark.parametrize("two_per_lane", [True, False])
def test_quiet_two_per_lane_bank_wakes_up_on_control(dev, two_per_lane):
    """Two-per-lane kernels: once a launch has deferred no group to sk_render_env2_kernel the host stops launching
    it; a stamped trigger / release (or any other control action) must bring it back for the very next block.
    One-per-lane kernel: the same report swaps the instantiation that holds the block form of envelopes in motion for the
    lean one and back; both render everything, so the samples must not depend on which one ran."""
    D = dev
    n = 4096
    bank, tables, g = banks.bank_c2(n)
    db = dev.DeviceBank(n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    db.fast2_min_voices(0 if two_per_lane else 1 << 30)
    mirror, truth, gl = bank.copy(), bank.copy(), g.copy()
    mixes, refs = [], []
    plan = {30: (np.arange(5, n, 97, dtype=np.int32), D.STAMP_RELEASE),
            34: (np.arange(9, n, 211, dtype=np.int32), D.STAMP_TRIGGER | D.DIRTY_PHASE),
            60: (np.arange(2, n, 301, dtype=np.int32), D.STAMP_RELEASE)}
    for k in range(70):                                  # 0.11 s of attack/decay, then long quiet stretches
        if k in plan:
            vs, dirty = plan[k]
            if dirty & D.DIRTY_PHASE:
                mirror["voice_phase"][vs] = 0.0
                mirror["voice_finished"][vs] = 0
            db.update(mirror, vs, dirty)
            apply_captured(truth, mirror, vs, dirty, gl.synth_sample_count, D)
        m, _ = db.render_host(F, 2, 0)
        assert db.last_kernel() == (3 if two_per_lane else 1)
        mixes.append(m)
        r = cpuref.render(truth, gl, tables, F, 0)
        refs.append(cpuref.master(gl, r["sum64"].astype(np.float32)))
    got = bank.copy()
    db.download(got)
    db.close()
    assert not got.rw_equal(truth), got.rw_equal(truth)
    assert rel_rms(np.concatenate(mixes), np.concatenate(refs)) <= 1e-5


def test_mid_size_bank_changes_kernels_with_its_state(dev):
    """An enveloped bank between the two-per-lane threshold and 393 216 voices renders on the one-voice kernel while
    envelopes move and on the two-per-lane kernel once a launch has reported a quiet bank; a note-on sends it back.  The
    two kernel families share the voice planes: the samples must not show the hand-overs."""
    D = dev
    n, Fm = 229376, 256
    bank, tables, g = banks.bank_c2(n)
    e = bank["voice_amp_envelope"]                      # everyone long in sustain except a few fresh notes
    e["sample_start"][:] = g.synth_sample_count - 48000
    e["sample_start"][::997] = g.synth_sample_count - 100
    bank["voice_smoother_smoothing"][::997] = np.float32(0.002)   # their amp smoothers are still settling when the envelopes rest:
    # the one-voice kernel's report ("no envelope moved") must not make the two-per-lane kernel drop them
    db = dev.DeviceBank(n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    mirror, truth, gl = bank.copy(), bank.copy(), g.copy()
    mixes, refs, kernels = [], [], []
    for k in range(36):
        if k == 30:
            vs = np.arange(3, n, 4001, dtype=np.int32)
            db.update(mirror, vs, D.STAMP_TRIGGER)
            apply_captured(truth, mirror, vs, D.STAMP_TRIGGER, gl.synth_sample_count, D)
        m, _ = db.render_host(Fm, 2, 0)                  # (synchronous: the report of block k is in before block k+1 is issued)
        kernels.append(db.last_kernel())
        mixes.append(m)
        r = cpuref.render(truth, gl, tables, Fm, 0)
        refs.append(cpuref.master(gl, r["sum64"].astype(np.float32)))
    got = bank.copy()
    db.download(got)
    db.close()
    assert kernels[0] == 1 and 3 in kernels[:30] and kernels[29] == 3 and kernels[30] == 1, kernels
    assert not got.rw_equal(truth), got.rw_equal(truth)
    assert rel_rms(np.concatenate(mixes), np.concatenate(refs)) <= 1e-5


def test_update_argument_checks(dev):
    n = 256
    bank, tables, g = banks.bank_c1(n)
    db = dev.DeviceBank(n)
    db.set_tables(tables)
    db.upload(bank)
    with pytest.raises(dev.SkredAmdError):
        db.update(bank, [n], dev.DIRTY_PARAMS)                 # voice outside the bank
    with pytest.raises(dev.SkredAmdError):
        db.update(bank, [0], 0)                                # nothing named
    with pytest.raises(dev.SkredAmdError):
        db.update(bank, [0], 1 << 12)                          # unknown bit
    db.update(bank, [], dev.DIRTY_PARAMS)                      # empty batch is fine
    db.update(bank, [5, 5, 5], dev.DIRTY_PARAMS)               # repeated voice: applied in order
    db.close()


def test_million_voice_bank_takes_small_updates(dev):
    """2^20 voices resident; 64 voices change per block.  The per-block cost of the update path must not scale with
    the bank (classification is incremental, only the touched records travel)."""
    import time
    n = 1 << 20
    bank, tables, g = banks.bank_c2(n)
    db = dev.DeviceBank(n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    db.render_host(64, 2, 0)
    rng = np.random.default_rng(5)
    t = []
    for k in range(20):
        vs = rng.choice(n, 64, replace=False).astype(np.int32)
        bank["voice_amp"][vs] = np.float32(0.5)
        t0 = time.perf_counter()
        db.update(bank, vs, dev.DIRTY_PARAMS)
        t.append(time.perf_counter() - t0)
        db.render_host(64, 2, 0)
        assert db.last_kernel() == 3
    db.close()
    assert np.median(t) < 2e-3, t                              # a full re-upload of this bank takes ~100 ms


def test_staging_ring_reused_across_two_streams_under_host_polling(dev):
    """The update path's staging ring: a batch is read by its scatter kernel straight from one of eight pinned slots, the kernel's
    last workgroup re-arms the slot's arrival counter and then stores the batch's number into pinned memory, and the host -- which
    polls that word instead of waiting for an event -- reuses the slot (skred_bank_stage.c: sk_staging_slot;
    skred_update_kernels.hip: sk_batch_done).  Batches issued on ONE stream are ordered by the stream whatever the kernel does;
    here 400 small batches alternate between TWO streams, so the batch that reuses a slot is not ordered behind the one that used
    it before except by that protocol: the counter must be back at zero (and visible) before the host can see the slot free --
    the order commit 101c9d3 fixed -- or a later batch's last workgroup is not recognised, its number never reaches the host and
    the ring stalls.  Every batch writes a distinct frequency into distinct voices; at the end every voice must hold the value
    of the LAST batch that named it, and no call may have waited out the ring's five-second limit."""
    import time
    import torch
    n = 4096
    bank, tables, g = banks.bank_c2(n)
    db = dev.DeviceBank(n)
    db.set_tables(tables)
    host = bank.copy()
    db.upload(host)
    db.set_globals(g)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rng = np.random.default_rng(11)
    expect = host["voice_phase_inc"].copy()
    t0 = time.perf_counter()
    for k in range(400):
        ids = np.sort(rng.choice(n, 1 + (k % 130), replace=False)).astype(np.int32)     # 1 .. 130 voices: one to three workgroups
        val = np.float32(0.001 * (k + 1))
        host["voice_phase_inc"][ids] = val
        expect[ids] = val
        db.update(host, ids, dev.DIRTY_PARAMS, stream=streams[k & 1].cuda_stream)
        if k % 37 == 0:
            streams[(k + 1) & 1].synchronize()             # let one stream drain now and then: the other runs ahead of it
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 4.0, "a call sat out the staging ring's time limit"
    # voices named by batches on both streams: the two streams are not ordered against each other, so only the voices whose
    # last two writers sat on the same stream have a defined final value -- all of them here would be too strict; check through
    # a render-free download of the parameter the batches wrote: re-upload-free, the planes are read back by a fresh update-free path
    out = bank.copy()
    db.download(out)                                        # (state only: the parameter planes are checked below by rendering)
    # render one block from the device's planes and from the expected parameters: equal mixes <=> every parameter landed
    ref_bank, ref_g = bank.copy(), g.copy()
    ref_bank["voice_phase_inc"][:] = expect
    r = cpuref.render(ref_bank, ref_g, tables, F, 0)
    ref_mix = cpuref.master(ref_g, r["sum64"].astype(np.float32))
    mix, _ = db.render_host(F, 2, 0)
    got = bank.copy()
    db.download(got)
    db.close()
    assert rel_rms(mix, ref_mix) <= 1e-5
    bad = got.rw_equal(ref_bank)
    assert not bad, bad


def test_staging_ring_serves_every_call_family_back_to_back(dev):
    """The batch path (skred_bank_stage.c) is the one way a host-written batch reaches a kernel, whatever the call: 3 x SK_UPD_RING
    = 24 staged calls of eleven kinds go to bank A back to back on one stream -- every slot of the ring is reused twice, by a call
    of another family, under nothing but the completion-word protocol -- and to bank B with a device synchronise after each.
    Everything the calls write must be the same, byte for byte.  32768 voices with K = 1 slots: the smallest bank at which the
    bank-wide ctl_range (32768 lanes > 64 * 256) and find_owned (32768 slots > 64 * 256) read the slot's device twin behind a copy,
    while the eight-entry calls read the pinned buffer itself.  Voice i carries the tag i + 1 for i < 1024."""
    import time
    import torch
    n, ring, E = 32768, 8, 8
    bank, tables, g = banks.bank_c2(n)
    REL = dev.STAMP_RELEASE

    def i32(values):
        return torch.tensor(np.asarray(values, np.int64).astype(np.int32), dtype=torch.int32, device="cuda")

    def run(sync_each):
        db = dev.DeviceBank(n)
        db.set_tables(tables)
        host = bank.copy()
        db.upload(host)
        db.set_globals(g)
        db.render_host(64, 2, 0)                                  # synth_sample_count = 64: what the stamps and the notes store
        keep, results, found = [i32(np.arange(1024))], [], []
        db.tag_slots(keep[0].data_ptr(), np.arange(1, 1025), 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(3 * ring):
            ids = np.arange(E) * 97 + 13 * k                      # eight voices below 1024: voice v carries the tag v + 1
            lst, cnt, res = i32(ids), i32([E]), torch.zeros(3, dtype=torch.int32, device="cuda")
            val = float(np.float32(0.001 * (k + 1)))
            notes = [dev.NoteC(val, 0.5 + val, 0.25, val, 1.0 - val, dev.NOTE_SET_PHASE | dev.NOTE_SET_PAN) for _ in range(E)]
            pan = [dev.ctl(dev.CTL_PAN, pan_left=val, pan_right=2 * val)]
            kind = k % 11
            if kind == 0:
                vs = (2048 + ids).astype(np.int32)
                host["voice_phase_inc"][vs] = np.float32(val)
                db.update(host, vs, dev.DIRTY_PARAMS)
            elif kind == 1:
                db.notes_on_list(notes, lst.data_ptr(), cnt.data_ptr(), 0, 0, res.data_ptr())
            elif kind == 2:
                db.notes_on_slots(notes, 1, 1, lst.data_ptr(), cnt.data_ptr(), 0, 0, res.data_ptr())
            elif kind == 3:
                db.ctl_slots(pan, 1, lst.data_ptr(), E, 0, res.data_ptr())
            elif kind == 4:
                db.ctl_range([dev.ctl(dev.CTL_PAN_DEPTH, pan_depth=val)], 0, n, 1, res.data_ptr())
            elif kind == 5:
                keep.append(i32(4096 + ids))
                db.tag_slots(keep[-1].data_ptr(), 5000 + ids, 1, 0, res.data_ptr())
            elif kind == 6:
                out = torch.full((E,), -7, dtype=torch.int32, device="cuda")
                db.find_owned(0, n, 1, np.concatenate([ids[:6] + 1, [5000 + 13 * 5, 77777]]), out.data_ptr())
                found.append(out)
            elif kind == 7:
                db.stamp_owned(lst.data_ptr(), ids + 1, 1, 1, REL, res.data_ptr())
            elif kind == 8:
                db.ctl_owned(pan, 1, lst.data_ptr(), ids + 1, 0, res.data_ptr())
            elif kind == 9:
                db.ctl_match([dev.ctl(dev.CTL_AM_DEPTH, am_depth=val)], 0, n, 1, dev.owner_match(k & 3, 3), res.data_ptr())
            else:
                each = [dev.ctl_each(dev.EACH_VELOCITY, velocity=val + 0.01 * j) for j in range(E)]
                db.ctl_owned_each(pan, each, 1, lst.data_ptr(), ids + 1, 1, 0, res.data_ptr())
            keep.append((lst, cnt))
            results.append(res)
            if sync_each:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        took = time.perf_counter() - t0
        got = bank.copy()
        db.download(got)
        db.download_ctl(got)
        owners, clocks = db.download_owners(), db.download_env_clocks()
        mix, _ = db.render_host(64, 2, 0)
        db.close()
        return dict(took=took, bank=got, owners=owners, clocks=clocks, mix=mix, results=[r.cpu().numpy() for r in results],
                    found=[f.cpu().numpy() for f in found])

    a, b = run(False), run(True)
    assert a["took"] < 4.0, "a call sat out the staging ring's time limit"
    differ = [name for name in a["bank"].a if a["bank"].a[name].tobytes() != b["bank"].a[name].tobytes()]
    assert not differ, differ
    assert a["owners"].tobytes() == b["owners"].tobytes()
    assert a["clocks"][0].tobytes() == b["clocks"][0].tobytes() and a["clocks"][1].tobytes() == b["clocks"][1].tobytes()
    for k, (ra, rb) in enumerate(zip(a["results"], b["results"])):
        assert ra.tobytes() == rb.tobytes(), (k, ra, rb)
    assert len(a["found"]) == 2 and all(fa.tobytes() == fb.tobytes() for fa, fb in zip(a["found"], b["found"]))
    assert a["mix"].tobytes() == b["mix"].tobytes()
    # the calls did what they say: nothing above compares two banks that both stood still
    assert int(a["owners"][4096 + 13 * 5]) == 5000 + 13 * 5 and a["found"][0].tolist()[:6] == (np.arange(6) * 97 + 13 * 6).tolist()
    assert a["found"][0].tolist()[6:] == [4096 + 13 * 5, -1] and a["results"][1].tolist()[:2] == [E, 0]
    assert float(a["bank"]["voice_pan_mod_depth"][n - 1]) == float(np.float32(0.001 * 16)) and a["results"][4].tolist()[0] == n
