"""The b2-reusing frames of sk_render_fast2_kernel (skred_render_fast2.hip: fast2_post_lr<.., B2R>).

A wave in which every lane's b2 is +b0 or -b0 bit for bit (tests/test_b2_identity.py: every RBJ form but the all-pass) keeps the
product P = b0 * s of the last two frames once its frames are folded, and forms the biquad's b2 term as fma(sigma, P(n-2), y)
instead of multiplying b2 by s(n-2) again.  y does not change by a bit, so nothing here has a bar of its own: every case is
compared with oracle.cpuref the way tests/test_fast2_fold.py does it -- all read-write state and the globals bit for bit after
each of two consecutive launches, the mix within that file's 1e-5 relative RMS.

The banks are the smallest that reach the code: 2 048 + 384 voices of the C2/C3 recipe (two workgroup passes of eight waves and a
ragged one of three) forced onto the two-per-lane kernel, with the smoothers at rest from the first frame so that a launch of
8 frames already runs the folded block.  Which waves take the reusing frames is decided by the kernel's vote and is not visible
from outside (as with the fold, test_fast2_fold.py); the CPU test below pins down that the banks put the yes-waves, the no-waves
and both signs of sigma where the cases say.
"""
import functools

import numpy as np
import pytest

from oracle import cpuref
from skred_amd import banks

N = 2048 + 384                                                   # 19 wave slices of 128 voices
SIGN = np.uint32(0x80000000)
LENGTHS = {"f512": [512, 512], "f77": [77, 77], "f8": [8, 8], "f75": [64 + 8 + 3, 64 + 8 + 3]}


@pytest.fixture(scope="module")
def dev():
    from skred_amd import device
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


# ---------------------------------------------------------------------------------------------- the banks

def rested(n=N):
    """The recipe (filter modes 1 + v mod 4: all four qualifying forms, both signs of sigma, in every wave) without envelopes and
    with every smoother already at its gain: g + k (amp - g) == g from the first frame, so every wave folds in its first chunk.
    A few dead voices (amp 0) carry all-pass coefficients: dead lanes do not count in the vote."""
    bank, tables, g = banks.bank_c2(n)
    bank["voice_use_amp_envelope"][:] = 0
    amp = (np.float32(0.25) + np.float32(0.75) * banks.lcg_uniform(n, 77)).astype(np.float32)
    bank["voice_amp"] = amp
    bank["voice_smoother_gain"] = amp
    dead = np.array([5, 64 + 5, 1024 + 77, n - 3])
    set_mode5(bank, dead)
    bank["voice_amp"][dead] = 0.0
    return bank, tables, g


def set_mode5(bank, vs):
    flt = bank["voice_filter"]
    co = banks.biquad_coeffs(np.full(len(vs), 5), np.asarray(flt["last_freq"])[vs], np.asarray(flt["last_resonance"])[vs], 48000)
    for k, v in co.items():
        flt[k][vs] = v
    flt["last_mode"][vs] = 5
    bank["voice_filter_mode"][vs] = 5


def one_per_wave(n=N):
    """One all-pass voice in every ODD wave slice, at a lane and a half (voice 0 / voice 1 of the lane) that move from wave to
    wave: those waves vote no and keep the plain folded frames, their neighbours vote yes."""
    bank, tables, g = rested(n)
    w = np.arange(1, n // 128, 2)
    set_mode5(bank, w * 128 + (37 * w) % 128)
    return bank, tables, g


def one_whole_wave(n=N):
    bank, tables, g = rested(n)
    set_mode5(bank, np.arange(3 * 128, 4 * 128))
    return bank, tables, g


def attack(n=N):
    """The recipe as it is: envelopes, smoothers from zero.  The voices started less than 0.11 s ago are still in attack or decay
    (the motion list: they sit in their lanes, listed, and are rendered beside); the others move their smoothers towards the
    sustain gain and stall some 900 frames in -- the waves enter the reusing frames in the middle of the first launch."""
    return banks.bank_c2(n)


BANKS = {"modes14": rested, "one5": one_per_wave, "wave5": one_whole_wave, "attack": attack}
CASES = {f"{b}-{f}-i{i}": (b, LENGTHS[f], i) for b in ("modes14", "one5", "wave5") for f in LENGTHS for i in (0, 1)}
CASES.update({f"attack-i{i}": ("attack", [1024, 512], i) for i in (0, 1)})
TAPS = np.array([3, 64 + 3, 1024 + 200, N - 2], np.int32)        # a lane's two voices, a second-pass voice, one of the ragged pass


@functools.lru_cache(maxsize=None)
def bank_of(kind):
    return BANKS[kind]()


@functools.lru_cache(maxsize=None)
def plan(name):
    """The oracle's side of a case, once: per launch the master mix, the state and the globals behind it, the tapped stems."""
    kind, blocks, interp = CASES[name]
    bank, tables, g = bank_of(kind)
    truth, gl = bank.copy(), g.copy()
    out = []
    for frames in blocks:
        before = np.asarray(truth["voice_smoother_gain"]).copy()
        r = cpuref.render(truth, gl, tables, frames, interp, want_stems=True)
        out.append({"mix": cpuref.master(gl, r["sum64"].astype(np.float32)), "state": truth.copy(), "g": gl.copy(),
                    "taps": np.ascontiguousarray(r["stems"][:, TAPS]), "finite": bool(np.isfinite(r["stems"]).all()),
                    "smoothers_moved": int((np.asarray(truth["voice_smoother_gain"]).view(np.uint32) != before.view(np.uint32)).sum())})
    return out


def votes(bank):
    """Per 128-voice wave slice: the kernel's vote (live voices only) and the signs of sigma among its live voices."""
    flt = bank["voice_filter"]
    b0, b2 = np.asarray(flt["b0"], np.float32).view(np.uint32), np.asarray(flt["b2"], np.float32).view(np.uint32)
    live = np.asarray(bank["voice_amp"]) != 0
    ok = (((b0 ^ b2) & ~SIGN) == 0) | ~live
    neg = ((b0 ^ b2) == SIGN) & live
    pos = (b0 == b2) & live
    per = lambda m, f: np.array([f(m[s:s + 128]) for s in range(0, bank.n, 128)])
    return per(ok, np.all), per(pos, np.any), per(neg, np.any)


def test_the_banks_are_what_the_cases_say():
    """(CPU) modes14: every wave votes yes and holds both signs of sigma; one5: odd waves no, even waves yes; wave5: wave 3 alone
    votes no.  The rested banks' smoothers do not move in any launch; the attack bank's move through the first launch, all of
    them rest in the second, and some voices are in attack or decay at the start.  Every oracle value is finite, no mix is
    silence."""
    yes, pos, neg = votes(bank_of("modes14")[0])
    assert yes.all() and pos.all() and neg.all() and len(yes) == 19
    yes, _, _ = votes(bank_of("one5")[0])
    assert (yes == (np.arange(19) % 2 == 0)).all()
    yes, _, _ = votes(bank_of("wave5")[0])
    assert (yes == (np.arange(19) != 3)).all()
    assert votes(bank_of("attack")[0])[0].all()
    for name in CASES:
        for k, o in enumerate(plan(name)):
            assert o["finite"], (name, k)
            assert np.isfinite(o["mix"]).all() and np.sqrt(np.mean(o["mix"].astype(np.float64) ** 2)) > 1e-3, (name, k)
            if not name.startswith("attack"):
                assert o["smoothers_moved"] == 0, (name, k)
    for i in (0, 1):
        first, second = plan(f"attack-i{i}")
        assert first["smoothers_moved"] > N // 2 and second["smoothers_moved"] < N // 4
    bank, _, g = bank_of("attack")
    e = bank["voice_amp_envelope"]
    age = g.synth_sample_count - np.asarray(e["sample_start"]).astype(np.int64)
    moving = age < np.asarray(e["attack_time"]) + np.asarray(e["decay_time"])
    assert 50 < moving.sum() < N // 4
    assert (np.asarray(plan("modes14-f8-i0")[1]["taps"]) != 0).any((0, 2)).all()     # the four tapped voices sound


# ---------------------------------------------------------------------------------------------- on the GPU

def open_bank(dev, kind):
    bank, tables, g = bank_of(kind)
    db = dev.DeviceBank(bank.n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    db.fast2_min_voices(0)
    return db


def run_blocks(name, db, taps=None):
    """The case's launches on `db`; after every one: state and globals bit for bit, the mix within 1e-5 relative RMS of the
    oracle's.  Returns the mixes (and fills taps = (buffer, rows) launch by launch)."""
    import torch
    kind, blocks, interp = CASES[name]
    bank = bank_of(kind)[0]
    want = plan(name)
    mixes = []
    for k, frames in enumerate(blocks):
        tag = f"{name} launch {k} ({frames} frames)"
        if taps is not None:
            taps[0].fill_(float("nan"))
        out = torch.zeros(frames, 2, device="cuda")
        db.render_mix(frames, out.data_ptr(), 2, 0, interp)
        assert db.last_kernel() == 3, tag
        torch.cuda.synchronize()
        mix = out.cpu().numpy()
        mixes.append(mix)
        if taps is not None:
            taps[1].append(taps[0][:frames * len(TAPS) * 2].cpu().numpy().reshape(frames, len(TAPS), 2))
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
    return mixes


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_b2reuse_against_the_oracle(dev, name):
    db = open_bank(dev, CASES[name][0])
    try:
        run_blocks(name, db)
    finally:
        db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["modes14-f77-i0", "modes14-f75-i1", "one5-f77-i0", "attack-i0"])
def test_taps_change_nothing_and_carry_the_oracles_stems(dev, name):
    """Four taps: the probe twins run the same frames, so the mix with taps is bit-equal to the mix without, launch by launch, and
    the tap rows are bit-equal to the oracle's stems."""
    import torch
    want = plan(name)
    fmax = max(CASES[name][1])
    buf = torch.zeros(fmax * len(TAPS) * 2, device="cuda")
    tapped, plain = open_bank(dev, CASES[name][0]), open_bank(dev, CASES[name][0])
    try:
        tapped.set_taps(TAPS, buf.data_ptr())
        rows = []
        with_taps = run_blocks(name, tapped, taps=(buf, rows))
        assert tapped.last_taps() == len(TAPS)
        without = run_blocks(name, plain)
        for k, (a, b) in enumerate(zip(with_taps, without)):
            assert (a.view(np.uint32) == b.view(np.uint32)).all(), f"{name} launch {k}: a tap changed the mix"
        for k, got in enumerate(rows):
            bad = np.argwhere(got.view(np.uint32) != want[k]["taps"].view(np.uint32))
            assert len(bad) == 0, (f"{name} launch {k}: {len(bad)} tap values differ from the oracle's stems; first (frame, tap, ch) "
                                   f"{bad[0]}, voice {TAPS[bad[0][1]]}: {got[tuple(bad[0])]!r} vs {want[k]['taps'][tuple(bad[0])]!r}")
    finally:
        tapped.set_taps([], 0)
        tapped.close()
        plain.close()
