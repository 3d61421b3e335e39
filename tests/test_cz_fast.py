"""SKRED_OPT_CZ_FAST: CZ phase distortion (`c<mode>,<dist>`, cz_phasor, synth.c:149-215) on the one-voice-per-lane kernel.

With the option on, a bank whose CZ voices all qualify -- mode 1..7; the CZ source absent or a higher-indexed voice of the same
aligned 64-voice group; the other modulators above the voice in its group, amplitude / pan also the voice itself -- and which
holds nothing else that needs the full-featured kernels renders on the CZ instantiations of sk_render_fast_kernel.  Checked here:

  * per-voice stems (frame-by-frame form) and voice taps (the 8-frame blocks) bit for bit against the oracle, the end-of-block
    state of every voice bit for bit, the mix within 1e-5 RMS (what tests/test_gpu_parity.py applies); option 1 == option 0 per
    voice, bit for bit;
  * ENGAGEMENT in every case: last_kernel == SKRED_KERNEL_FAST and last_cz == 1, or the opposite where the bank must not engage.
    The generated banks are checked on the CPU against the rule as restated in `qualifies` below; a bank that does not qualify
    is a failure, never a skip.
"""
import numpy as np
import pytest

import golden_io as gio
from oracle import cpuref
from skred_amd import banks

pytestmark = pytest.mark.gpu

FAST, MODULATED = 1, 2
DISTS = np.array([-1.0, -0.7, -0.3, -0.001, 0.0, 0.5, 1.0], np.float32)   # + 1.0f (no source): d = 0, interior values, the 0.999 clamp


@pytest.fixture(scope="module")
def dev():
    from skred_amd import device
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, np.float64) ** 2)))


def rel_rms(a, b):
    return rms(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(rms(b), 1e-30)


# ---------------------------------------------------------------------------------------------- the rule, restated

def qualifies(bank):
    """(every CZ voice qualifies and no other voice needs the modulated kernel, number of CZ voices): include/skred_amd.h,
    SKRED_OPT_CZ_FAST, voice by voice."""
    n = bank.n
    v = np.arange(n)
    fm = np.asarray(bank["voice_freq_mod_osc"]).copy()
    fm[fm == v] = -1                                   # (a voice as its own frequency modulator is ignored, synth.c:549)
    am, pm = np.asarray(bank["voice_amp_mod_osc"]), np.asarray(bank["voice_pan_mod_osc"])
    mode = np.asarray(bank["voice_cz_mode"])
    cz = np.where(mode != 0, np.asarray(bank["voice_cz_mod_osc"]), -1)

    def above(src):
        return (src < 0) | ((src > v) & (src < n) & (src // 64 == v // 64))

    others = above(fm) & (above(am) | (am == v)) & (above(pm) | (pm == v))
    ok = np.where(mode != 0, (mode >= 1) & (mode <= 7) & above(cz) & others, others)
    finite = np.isfinite(bank["voice_phase"]) & np.isfinite(bank["voice_phase_inc"])
    return bool((ok & finite).all()), int((mode != 0).sum())


def base_bank(n, seed=0x5EED):
    """The C2 recipe (LDS-resident pool, biquad and envelope on every voice) with the CZ fields at rest."""
    bank, tables, g = banks.bank_c2(n, seed=seed)
    bank["voice_cz_mod_osc"] = -1
    bank["voice_cz_mode"] = 0
    bank["voice_cz_distortion"] = 0.5
    bank["voice_cz_mod_depth"] = 0.0
    return bank, tables, g


def run(dev, bank, tables, g, blocks, cz_fast, interp=0, stems=False, taps=None, actions=None, pack=None, cross=False, opt_each=None):
    """Render `blocks` on a fresh device bank.  Returns (state, mixes, per-block stems or tap rows, [(last_kernel, last_cz, last_pack)])."""
    import torch
    db = dev.DeviceBank(bank.n)
    db.set_tables(tables); db.upload(bank); db.set_globals(g)
    if cz_fast is not None:
        db.set_cz_fast(cz_fast)
    if pack is not None:
        db.set_pack(pack)
    if cross:
        db.set_cross_group(True)
    host = bank.copy()
    buf = None
    if taps is not None:
        buf = torch.zeros(max(blocks) * len(taps) * 2, device="cuda")
        db.set_taps(taps, buf.data_ptr())
    mixes, rows, kinds = [], [], []
    for k, f in enumerate(blocks):
        if actions and k in actions:
            actions[k](db, host)
        if opt_each is not None:
            db.set_cz_fast(opt_each[k])
        if stems:
            mix, st = db.render_host(f, 2, interp, want_stems=True)
            mixes.append(mix); rows.append(st)
        else:
            out = torch.zeros(f, 2, device="cuda")
            db.render_mix(f, out.data_ptr(), 2, 0, interp)
            torch.cuda.synchronize()
            mixes.append(out.cpu().numpy())
            if buf is not None:
                rows.append(buf[:f * len(taps) * 2].cpu().numpy().reshape(f, len(taps), 2).copy())
        kinds.append((db.last_kernel(), int(db.last_cz()), db.last_pack()))
    got = bank.copy()
    db.download(got)
    if taps is not None:
        db.set_taps([], 0)
    db.close()
    return got, mixes, rows, kinds


def oracle(bank, tables, g, blocks, interp=0, actions=None):
    ref, ref_g = bank.copy(), g.copy()
    mixes, stems = [], []
    for k, f in enumerate(blocks):
        if actions and k in actions:
            actions[k](None, ref)
        r = cpuref.render(ref, ref_g, tables, f, interp, want_stems=True)
        mixes.append(cpuref.master(ref_g, r["sum64"].astype(np.float32)))
        stems.append(r["stems"])
    return ref, mixes, stems


def same_bits(a, b):
    return bool((np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)).all())


def check(tag, got, mixes, rows, ref, ref_mixes, ref_rows):
    bad = got.rw_equal(ref)
    assert not bad, f"{tag}: state differs from the oracle: {bad}"
    for k in range(len(mixes)):
        if rows:
            d = np.argwhere(np.ascontiguousarray(rows[k]).view(np.uint32) != np.ascontiguousarray(ref_rows[k]).view(np.uint32))
            assert len(d) == 0, f"{tag}: block {k}: {len(d)} per-voice values differ from the oracle, first (frame, voice, channel) {d[0]}"
        assert np.isfinite(ref_mixes[k]).all(), f"{tag}: the oracle's mix of block {k} is not finite"
        err = rel_rms(mixes[k], ref_mixes[k])
        print(f"{tag}: block {k} mix rel-rms {err:.3e}")
        assert err <= 1e-5, f"{tag}: block {k} mix rel-rms {err}"


def engaged(kinds):
    return all(k[0] == FAST and k[1] == 1 for k in kinds)


def not_engaged(kinds):
    return all(k[1] == 0 for k in kinds)


# ---------------------------------------------------------------------------------------------- 1: every mode, no source, stems

@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5, 6, 7])
def test_each_mode_without_a_source_with_stems(dev, mode, interp):
    bank, tables, g = base_bank(256)
    bank["voice_cz_mode"] = mode
    bank["voice_cz_distortion"] = DISTS[np.arange(256) % 7]
    ok, n_cz = qualifies(bank)
    assert ok and n_cz == 256
    for frames in (1, 7, 8, 9, 64, 67):
        blocks = [frames] * 3
        ref, ref_mixes, ref_stems = oracle(bank, tables, g, blocks, interp)
        got, mixes, stems, kinds = run(dev, bank, tables, g, blocks, 1, interp, stems=True)
        assert engaged(kinds), (mode, interp, frames, kinds)
        check(f"mode {mode} interp {interp} frames {frames}", got, mixes, stems, ref, ref_mixes, ref_stems)
        got0, _, stems0, kinds0 = run(dev, bank, tables, g, blocks, 0, interp, stems=True)
        assert all(k == (MODULATED, 0, 0) for k in kinds0), kinds0
        assert all(same_bits(a, b) for a, b in zip(stems, stems0)) and not got.rw_equal(got0)


def mixed_modes_bank(n=256):
    bank, tables, g = base_bank(n)
    v = np.arange(n)
    bank["voice_cz_mode"] = 1 + v % 7
    bank["voice_cz_distortion"] = DISTS[(v // 7) % 7]
    return bank, tables, g


# ---------------------------------------------------------------------------------------------- 2: the 8-frame blocks, through taps

@pytest.mark.parametrize("interp", [0, 1])
def test_block_paths_through_taps(dev, interp):
    bank, tables, g = mixed_modes_bank()
    assert qualifies(bank) == (True, 256)
    blocks = [64, 67, 9]
    taps = np.array([0, 1, 2, 3, 4, 5, 6, 48, 49, 63, 64, 100, 127, 128, 200, 255], np.int32)
    ref, ref_mixes, ref_stems = oracle(bank, tables, g, blocks, interp)
    want = [s[:, taps, :] for s in ref_stems]
    got, mixes, rows, kinds = run(dev, bank, tables, g, blocks, 1, interp, taps=taps)
    assert engaged(kinds), kinds
    check(f"taps interp {interp}", got, mixes, rows, ref, ref_mixes, want)
    got2, mixes2, _, kinds2 = run(dev, bank, tables, g, blocks, 1, interp)
    assert kinds2 == kinds, (kinds, kinds2)
    check(f"no taps interp {interp}", got2, mixes2, None, ref, ref_mixes, None)
    assert all(same_bits(a, b) for a, b in zip(mixes, mixes2))


# ---------------------------------------------------------------------------------------------- 3: sources above the carrier

def sourced_bank():
    """128 voices.  Group 0: CZ carriers with a CZ source above them (audible ones and `m1` ones), some with FM / AM / pan from
    above too, some with AM / pan by themselves; depths such that dist + sample * depth crosses 0 and 0.999.  Group 1: plain
    carriers frequency-modulated from above, no CZ lane (a wave without CZ beside one with)."""
    bank, tables, g = base_bank(128)
    rng = np.random.default_rng(3)
    v = np.arange(64)
    car = v[v < 48]
    src = 48 + (car % 16)
    bank["voice_cz_mode"][car] = 1 + car % 7
    bank["voice_cz_mod_osc"][car] = src
    bank["voice_cz_distortion"][car] = np.where(car % 2 == 0, 0.05, 0.9).astype(np.float32)
    bank["voice_cz_mod_depth"][car] = np.where(car % 3 == 0, 30.0, -8.0).astype(np.float32)     # sample ~ +-0.03: both clamps are crossed
    bank["voice_disconnect"][56:64] = 1                                                          # `m1` sources; 48..55 are heard
    bank["voice_freq_mod_osc"][car[car % 4 == 0]] = 60
    bank["voice_freq_mod_depth"][car] = 0.4
    bank["voice_amp_mod_osc"][car[car % 5 == 1]] = 58
    bank["voice_amp_mod_osc"][car[car % 5 == 2]] = car[car % 5 == 2]
    bank["voice_amp_mod_depth"][car] = 6.0
    bank["voice_pan_mod_osc"][car[car % 6 == 3]] = 50
    bank["voice_pan_mod_osc"][car[car % 6 == 4]] = car[car % 6 == 4]
    bank["voice_pan_mod_depth"][car] = 3.0
    bank["voice_sample"] = (rng.random(128) * 0.06 - 0.03).astype(np.float32)                    # the first frame reads these
    g1 = 64 + np.arange(0, 60)
    bank["voice_freq_mod_osc"][g1] = 64 + 60 + (g1 % 4)
    bank["voice_freq_mod_depth"][g1] = 0.7
    return bank, tables, g


@pytest.mark.parametrize("stems", [True, False])
def test_cz_source_above_the_carrier(dev, stems):
    bank, tables, g = sourced_bank()
    assert qualifies(bank) == (True, 48)
    blocks = [67, 64, 9]
    ref, ref_mixes, ref_stems = oracle(bank, tables, g, blocks)
    taps = np.concatenate([np.arange(0, 48, 2), np.arange(48, 64, 2), 64 + np.arange(0, 64, 4)]).astype(np.int32)[:64]
    got, mixes, rows, kinds = run(dev, bank, tables, g, blocks, 1, stems=stems, taps=None if stems else taps)
    assert engaged(kinds), kinds
    check(f"sources stems={stems}", got, mixes, rows, ref, ref_mixes, ref_stems if stems else [s[:, taps, :] for s in ref_stems])
    got0, _, rows0, kinds0 = run(dev, bank, tables, g, blocks, 0, stems=stems, taps=None if stems else taps)
    assert all(k[0] == MODULATED and k[1] == 0 for k in kinds0), kinds0
    assert all(same_bits(a, b) for a, b in zip(rows, rows0)) and not got.rw_equal(got0)


# ---------------------------------------------------------------------------------------------- 4 / 8: every per-lane feature

def feature_bank(seed, n, sparse=False):
    """Qualifying banks only: CZ (all modes, dist in [-1.2, 1.2], sources above with depths up to +-40) beside every per-lane feature
    of the extended instantiation -- biquad on some, envelopes in attack / decay / release, one-shots about to stop (some in mode
    4), reverse, sample & hold, bit-crush, smoother off, windowed loops with lo > 0, muted voices, voice_amp == 0, FM / AM / pan
    from above, AM / pan by the voice itself."""
    rng = np.random.default_rng(seed)
    bank, tables, g = base_bank(n, seed=0x5EED + seed)
    v = np.arange(n)
    lane = v % 64
    size = np.asarray(bank["voice_table_size"]).astype(np.float32)
    now = int(g.synth_sample_count)

    def pick(p):
        return rng.random(n) < p

    def above():
        return np.where(lane < 63, v + 1 + (rng.random(n) * (63 - lane)).astype(np.int64), -1)

    cz = pick(0.6)
    bank["voice_cz_mode"] = np.where(cz, rng.integers(1, 8, n), 0).astype(np.int32)
    bank["voice_cz_distortion"] = (rng.random(n) * 2.4 - 1.2).astype(np.float32)
    bank["voice_cz_mod_osc"] = np.where(cz & pick(0.4), above(), -1).astype(np.int32)
    bank["voice_cz_mod_depth"] = ((rng.random(n) * 2 - 1) * 40).astype(np.float32)
    bank["voice_freq_mod_osc"] = np.where(pick(0.2), above(), -1).astype(np.int32)
    bank["voice_freq_mod_depth"] = (rng.random(n) * 1.5).astype(np.float32)
    bank["voice_freq_scale"] = (0.5 + rng.random(n)).astype(np.float32)
    bank["voice_amp_mod_osc"] = np.where(pick(0.08), v, np.where(pick(0.1), above(), -1)).astype(np.int32)
    bank["voice_amp_mod_depth"] = (rng.random(n) * 8).astype(np.float32)
    bank["voice_pan_mod_osc"] = np.where(pick(0.08), v, np.where(pick(0.1), above(), -1)).astype(np.int32)
    bank["voice_pan_mod_depth"] = (rng.random(n) * 4).astype(np.float32)
    bank["voice_filter_mode"] = np.where(pick(0.5), bank["voice_filter_mode"], 0).astype(np.int32)
    bank["voice_use_amp_envelope"] = pick(0.7).astype(np.int32)
    e = bank["voice_amp_envelope"]
    e["attack_time"] = (20 + rng.random(n) * 200).astype(np.float32)
    e["decay_time"] = (20 + rng.random(n) * 200).astype(np.float32)
    e["release_time"] = (30 + rng.random(n) * 200).astype(np.float32)
    e["sample_start"] = (now - rng.integers(0, 400, n)).astype(np.uint64)         # attack / decay end inside the blocks
    e["sample_release"] = np.where(pick(0.3), now - rng.integers(0, 100, n), 0).astype(np.uint64)
    e["is_active"] = pick(0.9).astype(np.int32)
    stop = pick(0.15)
    bank["voice_one_shot"] = stop.astype(np.int32)
    bank["voice_cz_mode"] = np.where(stop & (bank["voice_cz_mode"] != 0) & pick(0.5), 4, bank["voice_cz_mode"]).astype(np.int32)
    loop = ~stop & pick(0.2)
    bank["voice_loop_enabled"] = loop.astype(np.int32)
    lo = np.floor(size * 0.25)
    bank["voice_loop_start_f"] = np.where(loop, lo, 0).astype(np.float32)
    bank["voice_loop_end_f"] = np.where(loop, np.floor(size * 0.75), size - 1).astype(np.float32)
    bank["voice_loop_valid"] = 1
    inc = (0.05 + rng.random(n) * 0.2) * size * 0.1
    bank["voice_phase_inc"] = inc.astype(np.float32)
    phase = rng.random(n) * (size - 1)
    phase = np.where(loop, lo + rng.random(n) * (size * 0.5 - 1), phase)
    phase = np.where(stop, size - inc * rng.integers(2, 90, n), phase)             # the table end is reached inside the blocks
    bank["voice_phase"] = np.maximum(phase, 0).astype(np.float32)
    bank["voice_direction"] = (~stop & pick(0.12)).astype(np.int32)
    bank["voice_sample_hold_max"] = np.where(pick(0.12), rng.integers(1, 9, n), 0).astype(np.int32)
    bank["voice_quantize"] = np.where(pick(0.12), rng.integers(1, 12, n), 0).astype(np.int32)
    bank["voice_smoother_enable"] = (~pick(0.15)).astype(np.int32)
    bank["voice_disconnect"] = pick(0.12).astype(np.int32)
    bank["voice_sample"] = (rng.random(n) * 0.1 - 0.05).astype(np.float32)
    amp = (0.2 + rng.random(n)).astype(np.float32)
    if sparse:
        keep = np.zeros(n, bool)
        for g0 in range(0, n, 64):
            c = rng.choice(60, 2, replace=False)
            keep[g0 + c] = True
            for k in c:                               # carrier + a source above it, patch-shaped
                bank["voice_cz_mode"][g0 + k] = 1 + (k % 7)
                bank["voice_cz_mod_osc"][g0 + k] = g0 + k + 1 + int(rng.integers(0, 63 - k))
                keep[bank["voice_cz_mod_osc"][g0 + k]] = True
        amp = np.where(keep, amp, 0).astype(np.float32)
    else:
        amp[pick(0.08)] = 0.0
    bank["voice_amp"] = amp
    keep_crush_in_int_range(bank, tables)
    return bank, tables, g


def keep_crush_in_int_range(bank, tables):
    """The bit-crusher (quantize_bits_int, synth.c:341-345) casts sample * levels to int.  Out of int's range that cast is undefined
    in C: the oracle's x86 build returns INT_MIN for a large positive product, the GPU's conversion saturates to INT_MAX -- in every
    kernel, they share one `crush`.  A warped position can lie far outside the table (modes 1, 2, 3 and 5 at d = 0.999 scale x by up
    to 1000: |x'| <= 501, so |pos| <= 501 * size), where the linear lookup extrapolates from the clamped index with a fraction of up
    to |pos|: |sample| <= A * (1 + 2 * 501 * size), A the largest magnitude in the voice's table.  Bit-crushed CZ voices keep as many
    bits as hold levels * that bound below 2^31, so that no case here compares undefined behaviour."""
    tab = np.asarray(tables, np.float32)
    for v in np.flatnonzero((np.asarray(bank["voice_cz_mode"]) != 0) & (np.asarray(bank["voice_quantize"]) != 0)):
        off, size = int(bank["voice_table_offset"][v]), int(bank["voice_table_size"][v])
        bound = float(np.abs(tab[off:off + size]).max()) * (1 + 2 * 501 * size)
        bits = max(b for b in range(0, 12) if ((1 << b) - 1) * bound < 2.0 ** 31)
        assert bits >= 1, (v, bound)
        bank["voice_quantize"][v] = min(int(bank["voice_quantize"][v]), bits)


def test_every_per_lane_feature_beside_cz(dev):
    bank, tables, g = feature_bank(4, 512)
    ok, n_cz = qualifies(bank)
    assert ok and n_cz > 200
    for name, want in (("voice_one_shot", 30), ("voice_direction", 20), ("voice_sample_hold_max", 20), ("voice_quantize", 20),
                       ("voice_loop_enabled", 30), ("voice_disconnect", 20)):
        assert int((np.asarray(bank[name]) != 0).sum()) >= want, name
    assert int((bank["voice_amp"] == 0).sum()) >= 10 and int((bank["voice_smoother_enable"] == 0).sum()) >= 30
    assert int(((bank["voice_cz_mode"] == 4) & (bank["voice_one_shot"] != 0)).sum()) >= 5
    blocks = [100, 64, 37]
    for interp in (0, 1):
        ref, ref_mixes, ref_stems = oracle(bank, tables, g, blocks, interp)
        assert int(np.asarray(ref["voice_finished"]).sum()) >= 20                      # the one-shots did stop inside the blocks
        got, mixes, stems, kinds = run(dev, bank, tables, g, blocks, 1, interp, stems=True)
        assert engaged(kinds), kinds
        check(f"features stems interp {interp}", got, mixes, stems, ref, ref_mixes, ref_stems)
        taps = np.arange(0, 512, 8).astype(np.int32)
        got, mixes, rows, kinds = run(dev, bank, tables, g, blocks, 1, interp, taps=taps)
        assert engaged(kinds), kinds
        check(f"features taps interp {interp}", got, mixes, rows, ref, ref_mixes, [s[:, taps, :] for s in ref_stems])


# ---------------------------------------------------------------------------------------------- 5: packed lanes

def test_packed_lanes(dev):
    bank, tables, g = feature_bank(5, 1024, sparse=True)
    ok, n_cz = qualifies(bank)
    assert ok and n_cz > 0
    assert int(((bank["voice_amp"] != 0) & (bank["voice_cz_mode"] != 0)).sum()) >= 32
    blocks = [64, 67, 9]
    ref, ref_mixes, ref_stems = oracle(bank, tables, g, blocks)
    taps = np.flatnonzero(bank["voice_amp"] != 0)[:64].astype(np.int32)
    got, mixes, rows, kinds = run(dev, bank, tables, g, blocks, 1, taps=taps, pack=2)
    assert engaged(kinds) and all(0 < k[2] < 64 for k in kinds), kinds
    check("packed", got, mixes, rows, ref, ref_mixes, [s[:, taps, :] for s in ref_stems])


# ---------------------------------------------------------------------------------------------- 6: must not engage

def _below(bank):
    bank["voice_cz_mode"][10] = 1; bank["voice_cz_mod_osc"][10] = 3; bank["voice_cz_mod_depth"][10] = 4.0


def _itself(bank):
    bank["voice_cz_mode"][10] = 2; bank["voice_cz_mod_osc"][10] = 10; bank["voice_cz_mod_depth"][10] = 4.0


def _other_group(bank):
    bank["voice_cz_mode"][10] = 3; bank["voice_cz_mod_osc"][10] = 100; bank["voice_cz_mod_depth"][10] = 4.0


def _mode9(bank):
    bank["voice_cz_mode"][10] = 9


def _same_frame_am(bank):
    bank["voice_cz_mode"][10] = 5
    bank["voice_amp_mod_osc"][20] = 4; bank["voice_amp_mod_depth"][20] = 2.0


@pytest.mark.parametrize("name", ["below", "itself", "other_group", "mode9", "same_frame_am", "global_tables"])
def test_must_not_engage(dev, name):
    if name == "global_tables":
        bank, tables, g = banks.bank_c4(256)                 # the PCM pool: not staged in LDS
        bank["voice_cz_mod_osc"] = -1
        bank["voice_cz_mode"] = 1 + np.arange(256) % 7
        bank["voice_cz_distortion"] = 0.3
        assert qualifies(bank) == (True, 256)                # the voices qualify; the pool does not
    else:
        bank, tables, g = mixed_modes_bank()
        {"below": _below, "itself": _itself, "other_group": _other_group, "mode9": _mode9, "same_frame_am": _same_frame_am}[name](bank)
        assert not qualifies(bank)[0]
    blocks = [64, 37]
    ref, ref_mixes, ref_stems = oracle(bank, tables, g, blocks)
    cross = name == "other_group"
    got1, mixes1, stems1, kinds1 = run(dev, bank, tables, g, blocks, 1, stems=True, cross=cross)
    got0, mixes0, stems0, kinds0 = run(dev, bank, tables, g, blocks, 0, stems=True, cross=cross)
    assert not_engaged(kinds1) and kinds1 == kinds0 and all(k[0] == MODULATED for k in kinds1), (kinds1, kinds0)
    check(name, got1, mixes1, stems1, ref, ref_mixes, ref_stems)
    assert all(same_bits(a, b) for a, b in zip(stems1, stems0)) and all(same_bits(a, b) for a, b in zip(mixes1, mixes0))
    assert not got1.rw_equal(got0)


# ---------------------------------------------------------------------------------------------- 7: control traffic

def test_control_traffic_moves_the_bank_between_families(dev):
    from skred_amd import device
    bank, tables, g = base_bank(256)                      # a clean bank: no CZ voice yet
    P = device.DIRTY_PARAMS

    def cz_on(db, h):                                     # block 1: `c3,0.4` on two voices, one with a source above it
        h["voice_cz_mode"][[5, 70]] = 3; h["voice_cz_distortion"][[5, 70]] = 0.4
        h["voice_cz_mod_osc"][70] = 90; h["voice_cz_mod_depth"][70] = 12.0
        if db: db.update(h, [5, 70], P)

    def repoint_below(db, h):                             # block 2: voice 70's source below it: a same-frame read
        h["voice_cz_mod_osc"][70] = 66
        if db: db.update(h, [70], P)

    def repoint_back(db, h):                              # block 3
        h["voice_cz_mod_osc"][70] = 90
        if db: db.update(h, [70], P)

    def cz_off(db, h):                                    # block 5: the last CZ voices go
        h["voice_cz_mode"][[5, 70]] = 0
        if db: db.update(h, [5, 70], P)

    actions = {1: cz_on, 2: repoint_below, 3: repoint_back, 5: cz_off}
    blocks = [64, 67, 33, 64, 9, 64]
    opt = [1, 1, 1, 1, 0, 1]                              # block 4: the option toggled off, block 5: on again
    ref, ref_mixes, ref_stems = oracle(bank, tables, g, blocks, actions=actions)
    taps = np.array([5, 66, 70, 90, 0, 255], np.int32)
    got, mixes, rows, kinds = run(dev, bank, tables, g, blocks, None, taps=taps, actions=actions, opt_each=opt)
    want = [(FAST, 0), (FAST, 1), (MODULATED, 0), (FAST, 1), (MODULATED, 0), (FAST, 0)]
    assert [k[:2] for k in kinds] == want, kinds
    check("traffic", got, mixes, rows, ref, ref_mixes, [s[:, taps, :] for s in ref_stems])


def test_a_note_lands_on_a_cz_voice(dev):
    """skred_bank_note_on_idle on a bank whose only idle voice (envelope run out) is a CZ voice: the block after the note still runs
    the CZ instantiation and equals the oracle given the same stores."""
    import torch
    from skred_amd import device
    bank, tables, g = mixed_modes_bank()
    now = int(g.synth_sample_count)
    e = bank["voice_amp_envelope"]
    e["is_active"][77] = 0                                # voice 77 (mode 1 + 77 % 7): idle
    assert qualifies(bank)[0]
    ref, ref_g = bank.copy(), g.copy()
    db = dev.DeviceBank(256)
    db.set_tables(tables); db.upload(bank); db.set_globals(g); db.set_cz_fast(True)
    note = device.NoteC(np.float32(1.75), np.float32(0.8), np.float32(3.0), 0.0, 0.0, device.NOTE_SET_PHASE)
    da = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    dr = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    for k, f in enumerate((64, 67)):
        if k == 1:
            db.note_on_idle([note], 0, 256, device.IDLE_ENV_DONE, 0.0, None, da.data_ptr(), dr.data_ptr())
            r = ref
            r["voice_phase_inc"][77] = note.phase_inc; r["voice_amp_envelope"]["velocity"][77] = note.velocity
            r["voice_phase"][77] = note.phase; r["voice_finished"][77] = 0
            r["voice_amp_envelope"]["sample_start"][77] = now + 64; r["voice_amp_envelope"]["sample_release"][77] = 0
            r["voice_amp_envelope"]["is_active"][77] = 1
        out = torch.zeros(f, 2, device="cuda")
        db.render_mix(f, out.data_ptr(), 2, 0, 0)
        torch.cuda.synchronize()
        assert (db.last_kernel(), db.last_cz()) == (FAST, True)
        rr = cpuref.render(ref, ref_g, tables, f, 0, want_stems=False)
        assert rel_rms(out.cpu().numpy(), cpuref.master(ref_g, rr["sum64"].astype(np.float32))) <= 1e-5
    assert da.cpu().numpy()[0] == 77 and dr.cpu().numpy().tolist() == [1, 0]
    got = bank.copy()
    db.download(got)
    db.close()
    assert not got.rw_equal(ref), got.rw_equal(ref)


# ---------------------------------------------------------------------------------------------- 8: seeded fuzz

@pytest.mark.parametrize("seed", range(8))
def test_fuzz_over_qualifying_banks(dev, seed):
    bank, tables, g = feature_bank(100 + seed, 192)
    ok, n_cz = qualifies(bank)
    assert ok and n_cz > 60, (ok, n_cz)
    blocks = [37, 37, 37]
    interp = seed & 1
    ref, ref_mixes, ref_stems = oracle(bank, tables, g, blocks, interp)
    got, mixes, stems, kinds = run(dev, bank, tables, g, blocks, 1, interp, stems=True)
    assert engaged(kinds), (seed, kinds)
    check(f"fuzz {seed} stems", got, mixes, stems, ref, ref_mixes, ref_stems)
    taps = np.arange(0, 192, 3).astype(np.int32)
    got, mixes, rows, kinds = run(dev, bank, tables, g, blocks, 1, interp, taps=taps)
    assert engaged(kinds), (seed, kinds)
    check(f"fuzz {seed} taps", got, mixes, rows, ref, ref_mixes, [s[:, taps, :] for s in ref_stems])
    got0, _, stems0, kinds0 = run(dev, bank, tables, g, blocks, 0, interp, stems=True)
    assert all(k[0] == MODULATED and k[1] == 0 for k in kinds0), kinds0
    assert all(same_bits(a, b) for a, b in zip(stems, stems0)) and not got.rw_equal(got0)


# ---------------------------------------------------------------------------------------------- 9: the default

def test_option_default_is_off(dev):
    bank, tables, g = mixed_modes_bank()
    blocks = [64]
    ref, ref_mixes, ref_stems = oracle(bank, tables, g, blocks)
    got, mixes, stems, kinds = run(dev, bank, tables, g, blocks, None, stems=True)      # no option set
    assert kinds == [(MODULATED, 0, 0)], kinds
    check("default", got, mixes, stems, ref, ref_mixes, ref_stems)
    db = dev.DeviceBank(64)
    assert db.L.skred_bank_set_option(db.h, 12, 1) == 0                                 # SKRED_OK
    assert db.L.skred_bank_set_option(db.h, 12, 0) == 0
    assert db.last_cz() is False
    db.close()
