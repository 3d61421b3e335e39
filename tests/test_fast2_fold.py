"""The folded frames of the two-voices-per-lane kernel (skred_render_fast2.hip: fast2_fold_pan, EM 7).

Once the amp smoother of every lane of a tame wave has stalled, sk_render_fast2_kernel forms the lane's (L, R) straight from the
filtered samples with the folded gains pan x sgain -- one packed multiply and one packed FMA where gain, two pan products and
their sum took four instructions -- and multiplies voice_sample = y * sgain out once per eight frames.  Nothing that is state
changes by a bit; the mix differs from the oracle's by roundings of 1e-7 relative per voice.

Every case here runs small banks of the C2/C3 recipe (or, for the two-operator FM bank, of C1) forced onto the two-per-lane kernel,
launch by launch against oracle.cpuref: after EVERY launch all read-write state (voice_sample among it) and the globals bit for
bit, and the mix within the project's 1e-5 relative RMS.  The oracle's side of a plan is computed once and shared by the CPU test
that checks the plan's premises (finite samples, sounding voices, the stall in the middle of a launch) and the GPU tests.

What this file does NOT show: that a wave took the folded path.  The kernel has no counter for it, and every assertion here
(state bit for bit, mix within 1e-5) holds of the unfolded frames as well.  The CPU tests pin down that the banks put the
kernel where the fold starts (the stall inside the second launch, muted and dead lanes in one wave, tame waves in an FM bank);
that the folded instructions then run is read from the ISA and the VALU counters, not from these tests.
"""
import functools

import numpy as np
import pytest

from oracle import cpuref
from skred_amd import banks

N = 2048                                                         # two workgroup passes of 1024 voices: 16 waves


@pytest.fixture(scope="module")
def dev():
    from skred_amd import device
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


# ---------------------------------------------------------------------------------------------- the banks

def plain_c2(n=N):
    """The C2/C3 recipe without envelopes: gain = amp from the first frame, the smoothers start at 0 and stall about 860 frames in
    (k = 0.02: 0.98^n below half an ulp) -- in the MIDDLE of a launch.  Amplitudes differ per voice, so do the stall frames."""
    bank, tables, g = banks.bank_c2(n)
    bank["voice_use_amp_envelope"][:] = 0
    bank["voice_amp"] = (np.float32(0.25) + np.float32(0.75) * banks.lcg_uniform(n, 77)).astype(np.float32)
    return bank, tables, g


def muted_c2(n=N):
    """Muted live lanes (voice_disconnect: rendered, not heard) and dead voices (amp 0) in the same waves, waves with dead voices
    only, and waves with neither."""
    bank, tables, g = plain_c2(n)
    bank["voice_disconnect"][np.arange(3, 512, 17)] = 1          # slices 0 .. 3: muted live lanes ...
    bank["voice_amp"][np.arange(5, 512, 23)] = 0.0               # ... beside dead voices
    bank["voice_disconnect"][64 + 9] = 1
    bank["voice_amp"][9] = 0.0                                   # a lane with one muted and one dead voice
    bank["voice_amp"][np.arange(1024, 1280, 5)] = 0.0            # slices 8, 9: dead voices only
    return bank, tables, g


def mixed_c2(n=N):
    bank, tables, g = plain_c2(n)
    bank["voice_filter_mode"][::3] = 0                           # filter_mode 0: the sample passes, the delay line rests
    return bank, tables, g


def muted_mixed_c2(n=N):
    bank, tables, g = muted_c2(n)
    bank["voice_filter_mode"][::3] = 0
    return bank, tables, g


def env_c2(n=N):
    return banks.bank_c2(n)


def fm_pairs(n=N):
    """A two-operator FM bank on the C1 recipe: carriers (even voices, modulated by the voice after them) in every other
    128-voice slice only, so that the bank has waves of general frames AND tame waves, which fold."""
    bank, tables, g = banks.bank_c1(n)
    bank["voice_use_amp_envelope"][:] = 0
    bank["voice_amp"] = (np.float32(0.25) + np.float32(0.75) * banks.lcg_uniform(n, 78)).astype(np.float32)
    car = np.arange(0, n - 1, 2)
    car = car[(car // 128) % 2 == 0]
    bank["voice_freq_mod_osc"][car] = car + 1
    bank["voice_freq_mod_depth"][car] = (np.float32(0.05) * (1 + (car % 37))).astype(np.float32)
    bank["voice_freq_scale"][car] = (np.float32(0.5) + np.float32(0.01) * (car % 50)).astype(np.float32)
    bank["voice_disconnect"][car[::2] + 1] = 1
    return bank, tables, g


def note_traffic(n, D):
    """A few releases and note-ons ahead of most blocks: a short motion list beside a bank at rest."""
    plan = {}
    for k in range(1, 12, 2):
        plan.setdefault(k, []).append((np.arange(5 + k, n, 401), D.STAMP_RELEASE))
        plan.setdefault(k + 1, []).append((np.arange(9 + 3 * k, n, 331), D.STAMP_TRIGGER | D.DIRTY_PHASE))
    return plan


class _Names:                                                    # (the device module's flag names, for plans made without a GPU)
    STAMP_RELEASE, STAMP_TRIGGER, DIRTY_PHASE = 1, 2, 4


def stamp(truth, vs, flags, now):
    """amp_envelope_trigger / amp_envelope_release (synth.c:383-395) as plain stores, on the oracle's bank."""
    e = truth["voice_amp_envelope"]
    if flags & _Names.DIRTY_PHASE:
        truth["voice_phase"][vs] = 0.0
        truth["voice_finished"][vs] = 0
    if flags & _Names.STAMP_TRIGGER:
        e["sample_start"][vs] = now
        e["sample_release"][vs] = 0
        e["is_active"][vs] = 1
    if flags & _Names.STAMP_RELEASE:
        act = e["is_active"][vs] != 0
        e["sample_release"][vs[act]] = now


# name: (bank, block lengths, interp, note traffic, in_place mode | None, fm pairs)
CASES = {
    "a_stall_mid_launch": (plain_c2, [512, 512, 512, 512], 0, False, None, False),
    "b_lengths": (plain_c2, [512, 512, 5, 8, 64 + 3, 200, 5, 64 + 3], 0, False, None, False),
    "b_lengths_before_the_stall": (plain_c2, [5, 8, 64 + 3, 200, 512, 200, 64 + 3, 5], 0, False, None, False),
    "c_muted_and_dead": (muted_c2, [512, 512, 200, 64 + 3, 5], 0, False, None, False),
    "d_mixed": (mixed_c2, [512, 512, 200, 64 + 3, 5], 0, False, None, False),
    "e_linear": (plain_c2, [512, 512, 200, 64 + 3, 5], 1, False, None, False),
    "e_linear_muted_mixed": (muted_mixed_c2, [512, 512, 200, 64 + 3], 1, False, None, False),
    "f_envelopes_beside": (env_c2, [512] * 6 + [200, 64 + 3, 5, 512], 0, True, 0, False),
    "f_envelopes_in_place": (env_c2, [512] * 6 + [200, 64 + 3, 5, 512], 0, True, 2, False),
    "h_fm_pairs": (fm_pairs, [512, 512, 200, 64 + 3, 5, 512], 0, False, None, True),
}


@functools.lru_cache(maxsize=None)
def plan(name):
    """The oracle's side, once: per block the master mix, the state and the globals behind it, and the stems of the whole bank
    reduced to what the tests need (64 tapped columns; whether every stem value is finite)."""
    bank_fn, blocks, interp, traffic, _, _ = CASES[name]
    bank, tables, g = bank_fn()
    n = bank.n
    events = note_traffic(n, _Names) if traffic else {}
    rng = np.random.default_rng(5)
    fixed = [0, 1, 3, 5, 9, 63, 64, 73, 127, 128, 1024, 1029, n - 65, n - 64, n - 1]     # wave edges, muted, dead, carriers, modulators
    ids = list(dict.fromkeys(fixed + [int(v) for v in rng.choice(n, 80, replace=False)]))[:64]
    ids = np.sort(np.array(ids)).astype(np.int32)
    truth, gl = bank.copy(), g.copy()
    out = []
    for k, frames in enumerate(blocks):
        for vs, flags in events.get(k, []):
            stamp(truth, np.asarray(vs, np.int32), flags, gl.synth_sample_count)
        before = np.asarray(truth["voice_smoother_gain"]).copy()
        r = cpuref.render(truth, gl, tables, frames, interp, want_stems=True)
        out.append({"mix": cpuref.master(gl, r["sum64"].astype(np.float32)), "state": truth.copy(), "g": gl.copy(),
                    "taps": np.ascontiguousarray(r["stems"][:, ids]), "finite": bool(np.isfinite(r["stems"]).all()),
                    "sounding": int((r["stems"] != 0).any((0, 2)).sum()),
                    "smoothers_moved": int((np.asarray(truth["voice_smoother_gain"]).view(np.uint32) != before.view(np.uint32)).sum())})
    return bank, tables, g, ids, events, out


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_meets_the_premises(name):
    """(CPU) The oracle alone satisfies what the GPU tests assert of it: every stem value and every state field is finite (a NaN
    would compare unequal to itself, an infinity would void the mix bar), the mixes are not silence, most voices sound."""
    bank, tables, g, ids, events, out = plan(name)
    for k, o in enumerate(out):
        assert o["finite"], f"block {k}: a stem value is not finite"
        assert np.isfinite(o["mix"]).all() and np.sqrt(np.mean(o["mix"].astype(np.float64) ** 2)) > 1e-3, f"block {k}"
        for f in ("voice_sample", "voice_smoother_gain", "voice_phase"):
            assert np.isfinite(np.asarray(o["state"][f])).all(), (k, f)
        flt = o["state"]["voice_filter"]
        for f in ("x1", "x2", "y1", "y2"):
            assert np.isfinite(np.asarray(flt[f])).all(), (k, f)
        assert o["sounding"] * 2 >= bank.n, f"block {k}: {o['sounding']} of {bank.n} voices sound"
        assert not o["state"].rw_equal(o["state"].copy())          # the comparison the GPU tests make holds of equal banks
    assert (np.asarray(out[-1]["taps"]) != 0).any((0, 2)).sum() >= 32


def test_the_smoothers_stall_in_the_middle_of_a_launch():
    """(CPU) Case (a): the un-enveloped bank's smoothers move through the first launch and stall inside the second -- every
    voice's own recurrence g += k (amp - g) in float32 comes to rest between frames 512 + 64 and 1024 - 64, so every wave starts
    to fold at a chunk boundary inside that launch -- and launches three and four find them at rest."""
    bank, tables, g, ids, events, out = plan("a_stall_mid_launch")
    amp = np.asarray(bank["voice_amp"], np.float32)
    k = np.asarray(bank["voice_smoother_smoothing"], np.float32)
    gain = np.asarray(bank["voice_smoother_gain"], np.float32).copy()
    rest = np.full(bank.n, -1)
    for f in range(2048):
        nxt = (gain + k * (amp - gain)).astype(np.float32)
        rest[(rest < 0) & (nxt.view(np.uint32) == gain.view(np.uint32))] = f
        gain = nxt
    assert (rest >= 512 + 64).all() and (rest <= 1024 - 64).all(), (rest.min(), rest.max())
    assert len(np.unique(rest)) > 1
    assert out[0]["smoothers_moved"] == bank.n and out[1]["smoothers_moved"] == bank.n
    assert out[2]["smoothers_moved"] == 0 and out[3]["smoothers_moved"] == 0
    assert (np.asarray(out[1]["state"]["voice_smoother_gain"]).view(np.uint32) == gain.view(np.uint32)).all()


def test_the_special_lanes_are_where_the_cases_say():
    """(CPU) Case (c): a wave with muted live lanes beside dead voices, a lane holding one of each, waves with dead voices only.
    Case (h): slices with carriers and slices without.  Case (f): the traffic touches voices in most blocks."""
    bank = plan("c_muted_and_dead")[0]
    muted = (np.asarray(bank["voice_disconnect"]) != 0) & (np.asarray(bank["voice_amp"]) != 0)
    dead = np.asarray(bank["voice_amp"]) == 0
    per = lambda m: m.reshape(-1, 128).any(1)
    assert (per(muted) & per(dead)).sum() >= 4 and (~per(muted) & per(dead)).sum() >= 2 and (~per(muted) & ~per(dead)).sum() >= 4
    assert muted[64 + 9] and dead[9]
    fm = np.asarray(plan("h_fm_pairs")[0]["voice_freq_mod_osc"]) >= 0
    assert per(fm).sum() == N // 256 and (~per(fm)).sum() == N // 256
    assert len(plan("f_envelopes_beside")[4]) >= 10


# ---------------------------------------------------------------------------------------------- on the GPU

def open_bank(dev, name, bank, tables, g):
    _, _, _, _, in_place, fm = CASES[name]
    db = dev.DeviceBank(bank.n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    db.fast2_min_voices(0)
    if fm:
        db.fm2_min_voices(0)
    if in_place is not None:
        db.in_place(in_place)
    return db


def dev_flags(dev, flags):
    return ((dev.STAMP_RELEASE if flags & _Names.STAMP_RELEASE else 0) | (dev.STAMP_TRIGGER if flags & _Names.STAMP_TRIGGER else 0) |
            (dev.DIRTY_PHASE if flags & _Names.DIRTY_PHASE else 0))


def run_blocks(dev, name, db, bank, taps=None):
    """The plan's blocks on `db`; after every block: state and globals bit for bit, the mix within 1e-5 relative RMS of the
    oracle's.  Returns the mixes (and fills taps = (buffer, rows) block by block)."""
    import torch
    _, blocks, interp, _, in_place, _ = CASES[name]
    _, _, _, ids, events, want = plan(name)
    mirror = bank.copy()
    mixes, taken = [], []
    for k, frames in enumerate(blocks):
        tag = f"{name} block {k} ({frames} frames)"
        for vs, flags in events.get(k, []):
            vs = np.asarray(vs, np.int32)
            if flags & _Names.DIRTY_PHASE:
                mirror["voice_phase"][vs] = 0.0
                mirror["voice_finished"][vs] = 0
            db.update(mirror, vs, dev_flags(dev, flags), 0)
        if taps is not None:
            taps[0].fill_(float("nan"))
        out = torch.zeros(frames, 2, device="cuda")
        db.render_mix(frames, out.data_ptr(), 2, 0, interp)
        assert db.last_kernel() == 3, tag
        taken.append(db.last_in_place())
        torch.cuda.synchronize()
        mix = out.cpu().numpy()
        mixes.append(mix)
        if taps is not None:
            taps[1].append(taps[0][:frames * len(ids) * 2].cpu().numpy().reshape(frames, len(ids), 2))
        got = bank.copy()
        db.download(got)
        bad = got.rw_equal(want[k]["state"])
        assert not bad, f"{tag}: voice state differs from the oracle: {bad}"
        gg, gw = db.get_globals(), want[k]["g"]
        assert gg.synth_sample_count == gw.synth_sample_count and gg.noise_rng == gw.noise_rng, tag
        assert np.float32(gg.volume_smoother_gain).tobytes() == np.float32(gw.volume_smoother_gain).tobytes(), tag
        err = rel_rms(mix, want[k]["mix"])
        print(f"{tag}: mix rel rms {err:.3e}")
        assert err <= 1e-5, f"{tag}: mix rel rms {err}"
    assert db.list_violations() == 0
    if in_place == 2:
        assert any(taken), taken                                    # the in-place instantiation did run
    elif in_place == 0:
        assert not any(taken), taken
    return mixes


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fold_against_the_oracle(dev, name):
    bank, tables, g, ids, events, want = plan(name)
    db = open_bank(dev, name, bank, tables, g)
    try:
        run_blocks(dev, name, db, bank)
    finally:
        db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a_stall_mid_launch", "c_muted_and_dead", "e_linear_muted_mixed", "f_envelopes_beside"])
def test_taps_change_nothing_and_carry_the_oracles_stems(dev, name):
    """Case (g): the same bank with and without 64 taps -- the mixes bit-equal block by block (the probe twins fold the very same
    expression), the tap rows bit-equal to the oracle's stems (they keep (y * sgain) * pan)."""
    import torch
    bank, tables, g, ids, events, want = plan(name)
    assert len(ids) == 64
    fmax = max(CASES[name][1])
    buf = torch.zeros(fmax * len(ids) * 2, device="cuda")
    tapped, plain = open_bank(dev, name, bank, tables, g), open_bank(dev, name, bank, tables, g)
    try:
        tapped.set_taps(ids, buf.data_ptr())
        rows = []
        with_taps = run_blocks(dev, name, tapped, bank, taps=(buf, rows))
        assert tapped.last_taps() == len(ids)
        without = run_blocks(dev, name, plain, bank)               # (checked as well: both banks see the same host calls)
        for k, (a, b) in enumerate(zip(with_taps, without)):
            assert (a.view(np.uint32) == b.view(np.uint32)).all(), f"{name} block {k}: a tap changed the mix"
        for k, got in enumerate(rows):
            bad = np.argwhere(got.view(np.uint32) != want[k]["taps"].view(np.uint32))
            assert len(bad) == 0, (f"{name} block {k}: {len(bad)} tap values differ from the oracle's stems; first (frame, tap, ch) "
                                   f"{bad[0]}, voice {ids[bad[0][1]]}: {got[tuple(bad[0])]!r} vs {want[k]['taps'][tuple(bad[0])]!r}")
    finally:
        tapped.set_taps([], 0)
        tapped.close()
        plain.close()
