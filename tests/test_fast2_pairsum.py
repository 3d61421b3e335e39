"""The packed pair tile of the two-voices-per-lane kernel (skred_render_fast2.hip: SK_FAST2_LDS_BLOCK_P).

In the 8-frame blocks of a tame wave every lane parks its (L, R) of a frame as one float2 in the wave's tile; lane (f = lane & 7,
seg = lane >> 3) then adds the eight pairs of segment seg for frame f in ascending lane order, and the eight segment sums are added
as ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)), both channels at once.  Per voice nothing changes (nothing here feeds
back): state is bit for bit the oracle's.  The mix changes in the order of its 128-term sums only, and the order is fixed.

Banks of 2 048 voices (two workgroup passes of eight waves: the second pass accumulates into the row of the first) of the C2/C3
recipe, warmed on the oracle until every envelope holds its sustain level and every amp smoother has stalled -- the state the
headline block runs in, folded frames and all -- forced onto the two-per-lane kernel and compared with oracle.cpuref: the mix
within the project's 1e-5 relative RMS, state and globals bit for bit.  The truncating cases run the pair tile; the linear
ones the folded tile the launcher keeps for them, under the same assertions.
"""
import functools

import numpy as np
import pytest

from oracle import cpuref
from skred_amd import banks

N = 2048
WARM = 14 * 512                    # 0.11 s of attack + decay, then ~900 frames until the smoothers rest: 7 168 frames cover both


@pytest.fixture(scope="module")
def dev():
    from skred_amd import device
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


# ---------------------------------------------------------------------------------------------- the banks (before the warm-up)

def full(n=N):
    return banks.bank_c2(n)


def ragged():
    return banks.bank_c2(N - 37)                                 # the last 128-voice slice holds 91 voices


MUTED = np.concatenate([np.arange(3, 512, 17), [64 + 9, 1024 + 31, 1024 + 64 + 32]])


def muted():
    """Muted live voices (voice_disconnect: rendered, state advancing, not heard) in slices 0 .. 3 and 8, every one of them
    between loud neighbours; the other waves have none."""
    bank, tables, g = banks.bank_c2(N)
    bank["voice_disconnect"][MUTED] = 1
    return bank, tables, g


def muted_twin():
    """The same bank with the muted voices heard, at pan gains of zero: what they add to the mix is an exact zero either way."""
    bank, tables, g = banks.bank_c2(N)
    bank["voice_pan_left"][MUTED] = 0.0
    bank["voice_pan_right"][MUTED] = 0.0
    return bank, tables, g


def corner_voices(n=N):
    """Per 128-voice slice the voices of lanes 0, 31 (first voice of the lane) and 32, 63 (second voice)."""
    s = np.arange(n // 128) * 128
    return s + 0, s + 31, s + 64 + 32, s + 64 + 63


def corners():
    """One loud voice in each of lanes 0, 31, 32 and 63 of every slice, silence (amp 0) elsewhere.  Lanes 0 and 32 are panned hard
    left and lanes 31 and 63 hard right in even slices, the other way round in odd ones: a wrong lane-to-segment map or a swap of
    the channels in the reduction is a channel error of order one."""
    bank, tables, g = banks.bank_c2(N)
    l0, l31, l32, l63 = corner_voices()
    amp = np.zeros(N, np.float32)
    amp[np.concatenate([l0, l31, l32, l63])] = 1.0
    bank["voice_amp"] = amp
    left, right = banks.pan_gains(np.float32(-1.0)), banks.pan_gains(np.float32(1.0))
    odd = (np.arange(N // 128) % 2) == 1
    for vs, flip in ((l0, False), (l32, False), (l31, True), (l63, True)):
        for v, o in zip(vs, odd):
            pl, pr = right if (flip != bool(o)) else left
            bank["voice_pan_left"][v], bank["voice_pan_right"][v] = pl, pr
    return bank, tables, g


BANKS = {"full": full, "ragged": ragged, "muted": muted, "muted_twin": muted_twin, "corners": corners}

# name: (bank, block lengths, interp)
CASES = {
    "f512": ("full", [512], 0),
    "f8_one_block": ("full", [8], 0),
    "f7_tail_only": ("full", [7], 0),
    "f73_blocks_and_single": ("full", [73], 0),
    "f75_blocks_pair_single": ("full", [75], 0),                 # second chunk: a block, a pair and a single frame
    "f512_linear": ("full", [512], 1),
    "f8_linear": ("full", [8], 1),
    "f7_linear": ("full", [7], 1),
    "f73_linear": ("full", [73], 1),
    "ragged": ("ragged", [512, 73], 0),
    "ragged_linear": ("ragged", [73], 1),
    "muted": ("muted", [512, 73], 0),
    "muted_linear": ("muted", [73], 1),
    "corners": ("corners", [512, 73], 0),
    "corners_linear": ("corners", [73], 1),
}


@functools.lru_cache(maxsize=None)
def warmed(bank_name):
    """The bank behind WARM frames of the oracle (truncating lookup), once."""
    bank, tables, g = BANKS[bank_name]()
    for _ in range(WARM // 512):
        cpuref.render(bank, g, tables, 512, 0, want_stems=False)
    return bank, tables, g


@functools.lru_cache(maxsize=None)
def plan(name):
    """The oracle's side of a case, once: per block the master mix, the state and the globals behind it."""
    bank_name, blocks, interp = CASES[name]
    bank, tables, g = warmed(bank_name)
    truth, gl = bank.copy(), g.copy()
    out = []
    for frames in blocks:
        r = cpuref.render(truth, gl, tables, frames, interp, want_stems=False)
        out.append({"mix": cpuref.master(gl, r["sum64"].astype(np.float32)), "state": truth.copy(), "g": gl.copy()})
    return out


@pytest.mark.parametrize("bank_name", sorted(BANKS))
def test_the_warmed_banks_are_at_rest(bank_name):
    """(CPU) After the warm-up no smoother moves any more and no envelope changes its level: 512 more frames leave every
    voice_smoother_gain as it is, bit for bit -- so every tame wave folds from its first chunk.  The mix is finite and not silence."""
    bank, tables, g = warmed(bank_name)
    truth, gl = bank.copy(), g.copy()
    before = np.asarray(truth["voice_smoother_gain"]).copy()
    r = cpuref.render(truth, gl, tables, 512, 0, want_stems=False)
    after = np.asarray(truth["voice_smoother_gain"])
    assert (after.view(np.uint32) == before.view(np.uint32)).all()
    mix = cpuref.master(gl, r["sum64"].astype(np.float32))
    assert np.isfinite(mix).all() and np.sqrt(np.mean(mix.astype(np.float64) ** 2)) > 1e-3
    for f in ("voice_sample", "voice_phase"):
        assert np.isfinite(np.asarray(truth[f])).all(), f


PAIR_POOL_BYTES = 81920 - 8 * (1024 + 4160)      # Fast2Shape::pair_tile: tables + eight waves' sums and pair tiles in half a CU's LDS
TABLE_PAD_FLOATS = 24 + 3                        # what the host appends to the pool (SK_TABLE_PAD, rounded up to four floats)


@pytest.mark.parametrize("bank_name", sorted(BANKS))
def test_the_pool_takes_the_pair_tile(bank_name):
    """(CPU) The launcher gives the packed pair tile to truncating launches of banks whose padded table pool is at most 40 448 B;
    the GPU tests cannot see which tile ran, so the premise is pinned here: the recipe's pool is well below that line (and the
    linear cases run the folded tile by the same rule)."""
    tables = warmed(bank_name)[1]
    assert PAIR_POOL_BYTES == 40448
    assert (len(tables) + TABLE_PAD_FLOATS) * 4 <= PAIR_POOL_BYTES, len(tables) * 4


def test_the_corner_bank_is_what_it_says():
    """(CPU) Four sounding voices per slice, in lanes 0, 31, 32, 63, each on one channel only; both channels carry signal."""
    bank, tables, g = warmed("corners")
    l0, l31, l32, l63 = corner_voices()
    loud = np.zeros(N, bool)
    loud[np.concatenate([l0, l31, l32, l63])] = True
    assert ((np.asarray(bank["voice_amp"]) != 0) == loud).all()
    assert (l0 % 128 == 0).all() and (l31 % 128 == 31).all() and (l32 % 128 == 64 + 32).all() and (l63 % 128 == 64 + 63).all()
    pl, pr = np.asarray(bank["voice_pan_left"])[loud], np.asarray(bank["voice_pan_right"])[loud]
    assert ((pl == 0) != (pr == 0)).all()                          # hard left or hard right
    mix = plan("corners")[0]["mix"].astype(np.float64)
    assert np.sqrt(np.mean(mix[:, 0] ** 2)) > 1e-3 and np.sqrt(np.mean(mix[:, 1] ** 2)) > 1e-3


def test_the_muted_voices_have_loud_neighbours():
    bank = warmed("muted")[0]
    dis = np.asarray(bank["voice_disconnect"]) != 0
    assert dis.sum() == len(MUTED) and (np.asarray(bank["voice_amp"]) != 0).all()
    assert not dis[MUTED - 1].any() and not dis[MUTED + 1].any()
    assert np.isfinite(np.asarray(bank["voice_sample"])).all()


# ---------------------------------------------------------------------------------------------- on the GPU

def open_bank(dev, bank, tables, g):
    db = dev.DeviceBank(bank.n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    db.fast2_min_voices(0)
    return db


def render(dev, db, frames, interp, tag):
    import torch
    out = torch.zeros(frames, 2, device="cuda")
    db.render_mix(frames, out.data_ptr(), 2, 0, interp)
    assert db.last_kernel() == 3, tag                              # the two-per-lane kernel
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_case(dev, name):
    """The case's blocks on a fresh device bank: state and globals bit for bit, the mix within 1e-5 relative RMS of the oracle's,
    overall and per channel.  Returns the mixes."""
    bank_name, blocks, interp = CASES[name]
    bank, tables, g = warmed(bank_name)
    want = plan(name)
    db = open_bank(dev, bank, tables, g)
    mixes = []
    try:
        for k, frames in enumerate(blocks):
            tag = f"{name} block {k} ({frames} frames)"
            mix = render(dev, db, frames, interp, tag)
            mixes.append(mix)
            got = bank.copy()
            db.download(got)
            bad = got.rw_equal(want[k]["state"])
            assert not bad, f"{tag}: voice state differs from the oracle: {bad}"
            gg, gw = db.get_globals(), want[k]["g"]
            assert gg.synth_sample_count == gw.synth_sample_count and gg.noise_rng == gw.noise_rng, tag
            assert np.float32(gg.volume_smoother_gain).tobytes() == np.float32(gw.volume_smoother_gain).tobytes(), tag
            errs = (rel_rms(mix, want[k]["mix"]), rel_rms(mix[:, 0], want[k]["mix"][:, 0]), rel_rms(mix[:, 1], want[k]["mix"][:, 1]))
            print(f"{tag}: mix rel rms {errs[0]:.3e} (L {errs[1]:.3e}, R {errs[2]:.3e})")
            assert max(errs) <= 1e-5, f"{tag}: mix rel rms {errs}"
        assert db.list_violations() == 0
    finally:
        db.close()
    return mixes


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_tile_against_the_oracle(dev, name):
    run_case(dev, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f512", "f73_linear", "ragged", "muted"])
def test_two_renders_give_the_same_bits(dev, name):
    """The order of the sums is fixed: the same bank rendered twice gives bit-equal mixes."""
    first, second = run_case(dev, name), run_case(dev, name)
    for k, (a, b) in enumerate(zip(first, second)):
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), f"{name} block {k}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["muted", "muted_linear"])
def test_a_muted_voice_adds_an_exact_zero(dev, name):
    """The muted bank against its twin in which the same voices are heard at pan gains of zero: the very same mix, value for
    value (-0 == +0) -- what a muted lane parks in the tile is zero, whatever its neighbours hold."""
    _, blocks, interp = CASES[name]
    muted_mix = run_case(dev, name)
    bank, tables, g = warmed("muted_twin")
    db = open_bank(dev, bank, tables, g)
    try:
        for k, frames in enumerate(blocks):
            twin = render(dev, db, frames, interp, f"{name} twin block {k}")
            assert np.array_equal(muted_mix[k], twin), f"{name} block {k}: {np.abs(muted_mix[k] - twin).max()}"
    finally:
        db.close()
