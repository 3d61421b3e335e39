"""Voice taps (skred_bank_set_taps): per-frame stems of chosen voices from every kernel family.

A tap delivers, for up to 64 named voices and every frame, what the reference stores into its stem buffer (synth.c:603-611) --
from the same launch and the same kernel paths that render the block WITHOUT taps: the modulated kernel's frame-lag form, packed
lanes and the cross-group tape included, which a launch with the full stem buffer switches off.  Every test here compares the
tap rows BIT FOR BIT (uint32, nothing masked) with the oracle's stems of the whole bank, cpuref.render(...)["stems"][:, ids], and
checks against a second device bank that runs the same blocks without taps that a tap changes nothing: voice state and globals
after each block and the mix bit for bit, the same kernel / pack / cross-group reports and form counters.  (One exception, stated
in include/skred_amd.h: a two-operator FM bank renders on the one-voice kernel while tapped; its state stays bit-equal, its mix
is another summation order and is held to the project's 1e-5 relative RMS between kernel families.)

The tap buffer is filled with NaN ahead of every block: a row the block neither zeroed nor wrote would show.
"""
import functools

import numpy as np
import pytest

import fuzz_banks
import golden_io as gio
import mod_forms
from oracle import cpuref
from skred_amd import banks

DIRTY_PARAMS = fuzz_banks.DIRTY_PARAMS


@pytest.fixture(scope="module")
def dev():
    from skred_amd import device
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


def oracle_taps(bank, tables, g, ids, blocks, interp=0):
    """The oracle's side, once per plan: per block the stems of the WHOLE bank cut down to the tapped columns.  `blocks`:
    [(frames, event | None)], event(host) -> (voices, dirty) changes the host bank ahead of the block."""
    host, gl, out = bank.copy(), g.copy(), []
    for frames, event in blocks:
        if event is not None:
            event(host)
        st = cpuref.render(host, gl, tables, frames, interp, want_stems=True)["stems"]
        out.append(np.ascontiguousarray(st[:, ids]))
    return out, host


def open_bank(dev, bank, tables, g, setup):
    db = dev.DeviceBank(bank.n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    if setup is not None:
        setup(db)
    return db


def run_tapped(dev, bank, tables, g, ids, blocks, want, setup=None, interp=0, same_mix=True, counters=False, what=""):
    """The blocks on a tapped bank and on an untapped twin.  Asserts, per block: tap rows == want[k] bit for bit; state, globals and
    mix of the two banks bit-equal; the same reports.  Returns per block (last_kernel, last_pack, last_cross_group, form counts)."""
    import torch
    ids = np.asarray(ids, np.int32)
    tapped, plain = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    fmax = max(f for f, _ in blocks)
    buf = torch.zeros(fmax * len(ids) * 2, device="cuda")
    ctr = [torch.zeros(2, dtype=torch.int32, device="cuda") for _ in range(2)]
    out = []
    try:
        tapped.set_taps(ids, buf.data_ptr())
        if counters:
            tapped.set_form_counter(ctr[0].data_ptr())
            plain.set_form_counter(ctr[1].data_ptr())
        mirror = bank.copy()
        for k, (frames, event) in enumerate(blocks):
            tag = f"{what} block {k} ({frames} frames)"
            if event is not None:
                voices, dirty = event(mirror)
                tapped.update(mirror, voices, dirty)
                plain.update(mirror, voices, dirty)
            buf.fill_(float("nan"))
            for c in ctr:
                c.zero_()
            torch.cuda.synchronize()
            mixes = []
            for db in (tapped, plain):
                o = torch.zeros(frames, 2, device="cuda")
                db.render_mix(frames, o.data_ptr(), 2, 0, interp)
                torch.cuda.synchronize()
                mixes.append(o.cpu().numpy())
            assert tapped.last_taps() == len(ids) and plain.last_taps() == 0, tag
            got = buf[:frames * len(ids) * 2].cpu().numpy().reshape(frames, len(ids), 2)
            print(f"{tag}: taps non-zero in {int((got != 0).any((0, 2)).sum())} of {len(ids)} columns")
            bad = np.argwhere(got.view(np.uint32) != want[k].view(np.uint32))
            assert len(bad) == 0, (f"{tag}: {len(bad)} tap values differ from the oracle's stems; first (frame, tap, ch) {bad[0]}, "
                                   f"voice {ids[bad[0][1]]}: {got[tuple(bad[0])]!r} vs {want[k][tuple(bad[0])]!r}")
            a, b = bank.copy(), bank.copy()
            tapped.download(a)
            plain.download(b)
            diff = a.rw_equal(b)
            assert not diff, f"{tag}: a tap changed the voice state: {diff}"
            ga, gb = tapped.get_globals(), plain.get_globals()
            assert ga.synth_sample_count == gb.synth_sample_count and ga.noise_rng == gb.noise_rng, tag
            assert np.float32(ga.volume_smoother_gain).tobytes() == np.float32(gb.volume_smoother_gain).tobytes(), tag
            if same_mix:
                assert (mixes[0].view(np.uint32) == mixes[1].view(np.uint32)).all(), f"{tag}: a tap changed the mix"
                assert tapped.last_kernel() == plain.last_kernel(), tag
            else:
                err = rel_rms(mixes[0], mixes[1])
                print(f"{tag}: mix rel rms between the kernel families {err:.3e}")
                assert err <= 1e-5, f"{tag}: mix rel rms {err}"
            assert tapped.last_pack() == plain.last_pack(), tag
            assert tapped.last_cross_group() == plain.last_cross_group(), tag
            fc = [c.cpu().numpy().tolist() for c in ctr]
            assert fc[0] == fc[1], f"{tag}: form counters {fc[0]} with taps, {fc[1]} without"
            out.append((tapped.last_kernel(), tapped.last_pack(), tapped.last_cross_group(), fc[0]))
    finally:
        for db in (tapped, plain):
            db.set_form_counter(0)
        tapped.set_taps([], 0)
        tapped.close()
        plain.close()
    return out


# ---------------------------------------------------------------------------------------------- 1. the frame-lag form, unpacked and packed

LAG_BLOCKS = [64, 1, 2, 63, 65, 513]


@functools.lru_cache(maxsize=1)
def lag_plan():
    n = 4096
    bank, tables, g = banks.bank_patch("18sk", n)
    lv = mod_forms.levels(bank)
    assert lv[0] == 0 and lv[10] == 1 and bank["voice_freq_mod_osc"][10] == 0      # `v10 ... F0,70`: a source below its reader
    K = 16                                                                         # one copy of the patch
    assert bank["voice_freq_mod_osc"][n - K + 10] == n - K
    silent = int(np.flatnonzero(np.asarray(bank["voice_amp"])[:K] == 0)[0])
    ids = np.array([0, 10, silent, 63, 64, n - K, n - K + 10, n - 1], np.int32)
    want, _ = oracle_taps(bank, tables, g, ids, [(f, None) for f in LAG_BLOCKS])
    return bank, tables, g, ids, want, silent


@pytest.mark.gpu
@pytest.mark.parametrize("pack,skew", [(0, 0), (0, 1), (2, 0), (2, 1)])
def test_lag_form_unpacked_and_packed(dev, pack, skew):
    """18.sk tiled over 4096 voices: a level-0 source and its level-1 reader (voices 0 and 10 of the first and of the last copy), a
    silent voice (exact zeros), voices 63, 64 and n - 1, over blocks of 64, 1, 2, 63, 65 and 513 frames."""
    bank, tables, g, ids, want, silent = lag_plan()
    assert all((w[:, list(ids).index(silent)] == 0).all() for w in want)
    assert all(w[:, 1].any() for w in want) and all(w[:, 0].any() for w in want)   # source and reader sound in every block

    def setup(db):
        db.set_pack(pack)
        db.set_fm_skew(skew)

    res = run_tapped(dev, bank, tables, g, ids, [(f, None) for f in LAG_BLOCKS], want, setup, counters=True, what=f"pack {pack} skew {skew}")
    for (kern, lanes, cg, fc), frames in zip(res, LAG_BLOCKS):
        assert kern == 2 and cg == (0, 0)
        assert (lanes > 0) == (pack == 2), lanes
        if skew and frames >= 2:
            assert fc[0] > 0, f"the frame-lag form did not run: {fc}"
        else:
            assert fc[0] == 0 and fc[1] > 0, fc


# ---------------------------------------------------------------------------------------------- 2. the level loop

def below_bank(n):
    """The shape tests/test_fm_skew.py::below_bank describes, on the c2 recipe: copies of eight voices.  Copies 0 mod 4: v0 F1 (from
    above), v6 F0 (same frame, from below).  Copies 1 mod 4: v5 A2 P1, v7 a noise voice A3.  Copies 2 mod 4: a two-level chain v1 F0,
    v2 F1.  Copies 3 mod 4: v4 F2 from below and v2 F4 from above, a previous-frame edge across levels.  Every wavefront holds
    copies of kinds 2 and 3, so all of them keep the level loop."""
    bank, tables, g = banks.bank_c2(n)
    v = np.arange(n)
    base = v[v % 8 == 0]
    kind = (base // 8) % 4
    bank["voice_freq_scale"][v] = (np.float32(0.5) + np.float32(0.01) * (v % 40)).astype(np.float32)

    def fm(dst, src, depth):
        bank["voice_freq_mod_osc"][dst] = src
        bank["voice_freq_mod_depth"][dst] = np.float32(depth)

    b0 = base[kind == 0]
    fm(b0, b0 + 1, 0.1); fm(b0 + 6, b0, 0.4)
    bank["voice_disconnect"][b0 + 1] = 1
    b1 = base[kind == 1]
    bank["voice_amp_mod_osc"][b1 + 5] = b1 + 2; bank["voice_amp_mod_depth"][b1 + 5] = np.float32(1.5)
    bank["voice_pan_mod_osc"][b1 + 5] = b1 + 1; bank["voice_pan_mod_depth"][b1 + 5] = np.float32(0.8)
    bank["voice_wave_table_index"][b1 + 7] = 6
    bank["voice_amp_mod_osc"][b1 + 7] = b1 + 3; bank["voice_amp_mod_depth"][b1 + 7] = np.float32(0.9)
    b2 = base[kind == 2]
    fm(b2 + 1, b2, 0.3); fm(b2 + 2, b2 + 1, 0.3)
    b3 = base[kind == 3]
    fm(b3 + 4, b3 + 2, 0.2); fm(b3 + 2, b3 + 4, 0.2)
    return bank, tables, g


@pytest.mark.gpu
def test_level_loop_two_levels(dev):
    n = 1024
    bank, tables, g = below_bank(n)
    lv = mod_forms.levels(bank)
    assert lv.max() == 2 and not mod_forms.lag_groups(bank).any()
    last = n - 32                                                # the last four copies, kinds 0 .. 3
    ids = np.array([0, 1, 6, 8 + 1, 8 + 2, 8 + 5, 8 + 7, 16, 16 + 1, 16 + 2, 24 + 2, 24 + 4, 63, 64,
                    last + 6, last + 8 + 5, last + 16 + 2, last + 24 + 4, n - 1], np.int32)
    assert set(lv[ids]) == {0, 1, 2}                             # taps on every level
    blocks = [(64, None), (1, None), (65, None), (130, None)]
    want, _ = oracle_taps(bank, tables, g, ids, blocks)
    assert (want[0][:, list(ids).index(1)] == 0).all()           # `m1`: a disconnected source writes exact zeros
    for skew in (0, 1):
        res = run_tapped(dev, bank, tables, g, ids, blocks, want, lambda db: db.set_fm_skew(skew), counters=True, what=f"skew {skew}")
        assert all(r[0] == 2 and r[3][0] == 0 and r[3][1] > 0 for r in res), res


# ---------------------------------------------------------------------------------------------- 3. block edges

@pytest.mark.gpu
@pytest.mark.parametrize("skew", [0, 1])
def test_block_edges_finish_and_silence(dev, skew):
    """Copies of kind 0 only (v0 F1 from above, v6 F0 from below) plus v3 F2 from below: one dependency level, the frame-lag form.
    v2 of copy 3 is a one-shot that finishes on the LAST frame of block 0 (a level-0 source read by v3 in its frame): its row of
    that frame is the finishing sample, frame 0 of block 1 is exactly zero.  Ahead of block 2 the level-1 voice v6 of copy 5 is
    switched off (amp = 0 through update): exact zeros from there on."""
    n, F = 256, 65
    bank, tables, g = banks.bank_c2(n)
    b0 = np.arange(0, n, 8)
    bank["voice_freq_scale"][:] = np.float32(0.75)
    for dst, src, depth in ((b0, b0 + 1, 0.1), (b0 + 6, b0, 0.4), (b0 + 3, b0 + 2, 0.2)):
        bank["voice_freq_mod_osc"][dst] = src
        bank["voice_freq_mod_depth"][dst] = np.float32(depth)
    shot, reader, off = 3 * 8 + 2, 3 * 8 + 3, 5 * 8 + 6
    size = int(bank["voice_table_size"][shot])
    bank["voice_one_shot"][shot], bank["voice_loop_enabled"][shot], bank["voice_direction"][shot] = 1, 0, 0
    bank["voice_phase_inc"][shot] = np.float32(1.0)
    bank["voice_phase"][shot] = np.float32(size - F)             # phase + F x 1.0 reaches the table's end on frame F - 1
    lv = mod_forms.levels(bank)
    assert lv.max() == 1 and mod_forms.lag_groups(bank).all() and lv[shot] == 0 and lv[reader] == 1 and lv[off] == 1
    early = bank.copy()                                          # the one-shot finishes on that frame and not before
    cpuref.render(early, g.copy(), tables, F - 1, 0)
    assert early["voice_finished"][shot] == 0
    ids = np.array([shot, reader, off, off - 6, 0, 63, 64, n - 1], np.int32)

    def silence(host):
        host["voice_amp"][off] = 0.0
        return np.array([off], np.int32), DIRTY_PARAMS

    blocks = [(F, None), (64, None), (64, silence), (2, None)]
    want, end = oracle_taps(bank, tables, g, ids, blocks)
    assert end["voice_finished"][shot] == 1
    assert want[0][:, 0].any() and (want[1][:, 0] == 0).all()    # the one-shot sounds through block 0; frame 0 of block 1 on: zeros
    print("finishing sample (L, R):", want[0][F - 1, 0])
    assert want[1][:, 2].any() and (want[2][:, 2] == 0).all() and (want[3][:, 2] == 0).all()
    res = run_tapped(dev, bank, tables, g, ids, blocks, want, lambda db: db.set_fm_skew(skew), counters=True, what=f"skew {skew}")
    assert all(r[0] == 2 for r in res)
    assert all((r[3][0] > 0) == bool(skew) for r in res), [r[3] for r in res]


# ---------------------------------------------------------------------------------------------- 4. the cross-group tape

@pytest.mark.gpu
def test_cross_group_tape(dev):
    """1024 voices with SKRED_OPT_CROSS_GROUP: voice 0 an LFO that modulates the amplitude of every voice and the pan of every
    third, and a chain of three groups (130 reads 70 reads 5).  Taps on the sources and on readers in other groups."""
    n = 1024
    bank, tables, g = banks.bank_c2(n)
    v = np.arange(n)
    bank["voice_phase_inc"][0] = np.float32(0.37)
    bank["voice_amp_mod_osc"][1:] = 0
    bank["voice_amp_mod_depth"][1:] = np.float32(0.8)
    third = (v % 3 == 0) & (v > 0)
    bank["voice_pan_mod_osc"][third] = 0
    bank["voice_pan_mod_depth"][third] = np.float32(0.5)
    bank["voice_amp_mod_osc"][130] = 70
    bank["voice_amp_mod_depth"][130] = np.float32(0.9)
    bank["voice_freq_mod_osc"][70] = 5
    bank["voice_freq_mod_depth"][70] = np.float32(0.03)
    bank["voice_freq_scale"][70] = np.float32(1.0)
    ids = np.array([0, 5, 70, 130, 1, 3, 63, 64, 66, 129, 192, 513, 960, n - 1], np.int32)
    blocks = [(64, None), (65, None), (1, None), (130, None)]
    want, _ = oracle_taps(bank, tables, g, ids, blocks)
    res = run_tapped(dev, bank, tables, g, ids, blocks, want, lambda db: db.set_cross_group(True), counters=True)
    assert all(r[0] == 2 and r[2] == (3, 2) for r in res), res   # sources 0, 5, 70; 70's group reads 5's: two pre-pass levels


# ---------------------------------------------------------------------------------------------- 5. fuzz

FUZZ = [("own_group", 4001, 1000, False), ("cross_group", 4102, 4096, False),      # (routing, seed, voices, sparse)
        ("own_group", 4203, 4096, True), ("cross_group", 4304, 1000, True)]


def fuzz_ids(bank):
    """64 taps: the group edges, then voices that can sound and have a modulator, then voices that can sound."""
    n = bank.n
    edges = [0, 63, 64, 127, 128, n - 65, n - 64, n - 1, (n - 1) & ~63, ((n - 1) & ~63) - 1]
    live = mod_forms.usable(bank) & (np.asarray(bank["voice_amp"]) != 0) & (np.asarray(bank["voice_disconnect"]) == 0)
    routed = np.zeros(n, bool)
    for key, _, _ in fuzz_banks.MOD_FIELDS:
        routed |= np.asarray(bank[key]) >= 0
    first = np.flatnonzero(live & routed)
    rest = np.flatnonzero(live & ~routed)
    step = max(1, len(first) // 36)
    order = list(edges) + list(first[::step][:36]) + list(rest[::max(1, len(rest) // 40)])
    ids = list(dict.fromkeys(int(x) for x in order if 0 <= x < n))[:64]
    assert len(ids) == 64
    return np.array(sorted(ids), np.int32)


@functools.lru_cache(maxsize=4)
def fuzz_plan(case):
    routing, seed, n, sparse = FUZZ[case]
    gold = gio.load("c4_pcm_oneshot")
    tables, cat = gold.tables, fuzz_banks.catalogue(gold.segments[0].bank_in)
    rng = np.random.default_rng(seed)
    bank, _ = fuzz_banks.wild_bank(rng, n, cat, routing, sparse=sparse)
    g = gold.segments[0].g_in.copy()
    g.synth_sample_count = fuzz_banks.COUNT0
    blocks = [(f, None) for f in fuzz_banks.block_lengths(rng)]
    ids = fuzz_ids(bank)
    want, _ = oracle_taps(bank, tables, g, ids, blocks)
    return bank, tables, g, ids, blocks, want


@pytest.mark.parametrize("case", range(len(FUZZ)))
def test_fuzz_seeds_tap_voices_that_sound(case):
    """(CPU) Through the oracle's stems: the tapped rows are finite, at least half of the 64 tapped voices are non-zero in some
    frame (the comparison cannot pass on all-zero rows), the taps include voices with modulators, and the sparse banks pack."""
    routing, seed, n, sparse = FUZZ[case]
    bank, tables, g, ids, blocks, want = fuzz_plan(case)
    assert all(np.isfinite(w).all() for w in want)
    sounding = np.zeros(len(ids), bool)
    for w in want:
        sounding |= (w != 0).any((0, 2))
    assert sounding.sum() * 2 >= len(ids), f"{sounding.sum()} of {len(ids)} tapped voices sound"
    routed = np.zeros(n, bool)
    for key, _, _ in fuzz_banks.MOD_FIELDS:
        routed |= np.asarray(bank[key]) >= 0
    assert routed[ids].sum() >= 16
    sources = mod_forms.far_sources(bank) if routing == "cross_group" else ()
    assert (routing == "cross_group") == bool(sources)
    lanes = mod_forms.pack_lanes(bank, sources)
    assert (0 < lanes <= 32) if sparse else lanes == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(FUZZ)))
def test_fuzz(dev, case):
    routing, seed, n, sparse = FUZZ[case]
    bank, tables, g, ids, blocks, want = fuzz_plan(case)

    def setup(db):
        if routing == "cross_group":
            db.set_cross_group(True)
        db.set_pack(2)

    res = run_tapped(dev, bank, tables, g, ids, blocks, want, setup, counters=True, what=f"{routing} seed {seed}")
    for kern, lanes, cg, fc in res:
        assert kern == 2
        assert (lanes > 0) == sparse
        assert (cg[0] > 0) == (routing == "cross_group")


# ---------------------------------------------------------------------------------------------- 6. the generic kernel

@pytest.mark.gpu
def test_generic_kernel(dev):
    n = 4096
    bank, tables, g = banks.bank_c2(n)
    noise, rev, held = np.array([5, 64, 2000]), np.array([6, 63, 3000]), np.array([7, 128, n - 1])
    bank["voice_wave_table_index"][noise] = 6
    bank["voice_direction"][rev] = 1
    bank["voice_sample_hold_max"][held] = 4
    bank["voice_disconnect"][9] = 1
    bank["voice_amp"][11] = 0.0
    ids = np.sort(np.concatenate([noise, rev, held, [0, 9, 11, 1023, 1024]])).astype(np.int32)
    blocks = [(64, None), (65, None), (1, None), (200, None)]
    want, _ = oracle_taps(bank, tables, g, ids, blocks)
    for interp in (0, 1):
        w = want if interp == 0 else oracle_taps(bank, tables, g, ids, blocks, 1)[0]
        res = run_tapped(dev, bank, tables, g, ids, blocks, w, lambda db: db.force_generic(True), interp=interp, what=f"interp {interp}")
        assert all(r[0] == 0 for r in res), res


# ---------------------------------------------------------------------------------------------- 7. the specialised families

@functools.lru_cache(maxsize=1)
def c2_plan():
    n = 65536
    bank, tables, g = banks.bank_c2(n)
    bank["voice_disconnect"][5005] = 1
    bank["voice_amp"][7007] = 0.0
    rng = np.random.default_rng(3)
    ids = np.unique(np.concatenate([[0, 1, 63, 64, 127, 128, 5005, 7007, n - 65, n - 64, n - 1], rng.choice(n, 53, replace=False)]))[:64]
    ids = ids.astype(np.int32)
    blocks = [(512, None), (100, None)]
    want, _ = oracle_taps(bank, tables, g, ids, blocks)
    return bank, tables, g, ids, blocks, want


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,fast2_min", [(1, 1 << 30), (3, 1)])
def test_specialised_families(dev, kernel, fast2_min):
    """bank_c2(65536) on the one-voice kernel and on the two-per-lane kernel (envelopes in motion from the first frame: the
    envelope kernel beside it writes the rows of the voices it renders), 512 and 100 frames."""
    bank, tables, g, ids, blocks, want = c2_plan()
    res = run_tapped(dev, bank, tables, g, ids, blocks, want, lambda db: db.fast2_min_voices(fast2_min), what=f"kernel {kernel}")
    assert [r[0] for r in res] == [kernel] * len(blocks), res


@pytest.mark.gpu
def test_fm_pair_bank_leaves_the_pair_form_while_tapped(dev):
    """A two-operator FM bank above SKRED_OPT_FM2_MIN_VOICES: kernel 1 while tapped (the twin without taps: kernel 3, carrier and
    modulator in one lane), state bit-equal; kernel 3 again after set_taps([], 0)."""
    import torch
    n = 4096
    bank, tables, g = banks.bank_c1(n)
    car = np.arange(0, n - 1, 2)
    bank["voice_freq_mod_osc"][car] = car + 1
    bank["voice_freq_mod_depth"][car] = (np.float32(0.05) * (1 + (car % 37))).astype(np.float32)
    bank["voice_freq_scale"][car] = (np.float32(0.5) + np.float32(0.01) * (car % 50)).astype(np.float32)
    bank["voice_disconnect"][car[::2] + 1] = 1
    ids = np.array([0, 1, 2, 3, 62, 63, 64, 65, 2048, 2049, n - 2, n - 1], np.int32)
    blocks = [(256, None), (100, None)]
    want, _ = oracle_taps(bank, tables, g, ids, blocks)
    fm2 = lambda db: db.fm2_min_voices(0)
    # (run_tapped compares last_kernel and the mix bits only with same_mix; here the two banks' families differ on purpose)
    res = run_tapped(dev, bank, tables, g, ids, blocks, want, fm2, same_mix=False, what="fm pairs")
    assert [r[0] for r in res] == [1, 1], res
    plain = open_bank(dev, bank, tables, g, fm2)
    buf = torch.zeros(64 * len(ids) * 2, device="cuda")
    out = torch.zeros(64, 2, device="cuda")
    try:
        plain.render_mix(64, out.data_ptr(), 2, 0, 0)
        assert plain.last_kernel() == 3
        plain.set_taps(ids, buf.data_ptr())
        plain.render_mix(64, out.data_ptr(), 2, 0, 0)
        assert plain.last_kernel() == 1 and plain.last_taps() == len(ids)
        plain.set_taps([], 0)
        plain.render_mix(64, out.data_ptr(), 2, 0, 0)
        torch.cuda.synchronize()
        assert plain.last_kernel() == 3 and plain.last_taps() == 0
        ref, gl = bank.copy(), g.copy()
        cpuref.render(ref, gl, tables, 192, 0)
        got = bank.copy()
        plain.download(got)
        assert not got.rw_equal(ref), got.rw_equal(ref)
    finally:
        plain.close()


# ---------------------------------------------------------------------------------------------- 8. the recorder

@pytest.mark.gpu
def test_recorder_takes_the_tap_buffer(dev):
    """8 taps of 18.sk over 1024 voices, three blocks appended to a wav.Recorder(8, ...) on the render stream: convert(all selected)
    equals the int16 the recorder gives for the oracle's eight stem columns (fed to a second recorder)."""
    import torch
    from skred_amd import wav
    n = 1024
    bank, tables, g = banks.bank_patch("18sk", n)
    ids = np.array([0, 10, 16, 26, 64, 74, n - 16, n - 6], np.int32)
    frames = [64, 100, 37]
    want, _ = oracle_taps(bank, tables, g, ids, [(f, None) for f in frames])
    assert all(w.any() for w in want)
    db = open_bank(dev, bank, tables, g, None)
    rec, ref = wav.Recorder(len(ids), 1024), wav.Recorder(len(ids), 1024)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        taps = torch.zeros(max(frames), len(ids), 2, device="cuda")
        partial = torch.zeros(max(frames), 2, device="cuda")
        db.set_taps(ids, taps.data_ptr())
        rec.start()
        ref.start()
        for f, w in zip(frames, want):
            db.render(f, partial.data_ptr(), 0, 0, stream)
            rec.append(taps.data_ptr(), f, stream)
            col = torch.from_numpy(w).cuda()
            ref.append(col.data_ptr(), f, stream)
            torch.cuda.synchronize()
        assert rec.frames == ref.frames == sum(frames)
        sel = np.ones(len(ids), np.int32)
        got, exp = rec.convert(sel), ref.convert(sel)
        assert len(got) == sum(frames) * len(ids) * 2 and got.any()
        assert got.tobytes() == exp.tobytes()
    finally:
        db.set_taps([], 0)
        rec.close()
        ref.close()
        db.close()


# ---------------------------------------------------------------------------------------------- 9. refusals

@pytest.mark.gpu
def test_refusals_leave_the_bank_usable(dev):
    import torch
    n, F = 1000, 64
    bank, tables, g = banks.bank_c2(n)
    ids = np.array([0, 63, 64, n - 1], np.int32)
    want, _ = oracle_taps(bank, tables, g, ids, [(F, None)] * 5)
    db = open_bank(dev, bank, tables, g, None)
    taps = torch.zeros(F, len(ids), 2, device="cuda")
    out = torch.zeros(F, 2, device="cuda")
    stems = torch.zeros(F, n, 2, device="cuda")
    k = 0

    def ordinary_block():                                        # ... renders correctly: the taps against the oracle, block by block
        nonlocal k
        db.set_taps(ids, taps.data_ptr())
        taps.fill_(float("nan"))
        db.render_mix(F, out.data_ptr(), 2, 0, 0)
        torch.cuda.synchronize()
        assert (taps.cpu().numpy().view(np.uint32) == want[k].view(np.uint32)).all(), f"block {k}"
        k += 1

    try:
        ordinary_block()
        with pytest.raises(dev.SkredAmdError, match="stem"):     # taps and a stem buffer
            db.render_mix(F, out.data_ptr(), 2, stems.data_ptr(), 0)
        ordinary_block()
        with pytest.raises(dev.SkredAmdError):                   # a probe while taps are set
            db.set_probe(ids, taps.data_ptr())
        ordinary_block()
        db.set_taps([], 0)
        db.set_probe(ids, taps.data_ptr())
        with pytest.raises(dev.SkredAmdError):                   # taps while a probe is set
            db.set_taps(ids, taps.data_ptr())
        db.set_probe([], 0)
        ordinary_block()
        with pytest.raises(dev.SkredAmdError, match="outside"):  # a voice out of range
            db.set_taps([0, n], taps.data_ptr())
        with pytest.raises(dev.SkredAmdError):
            db.set_taps([-1], taps.data_ptr())
        with pytest.raises(dev.SkredAmdError):                   # 65 taps
            db.set_taps(np.arange(65), taps.data_ptr())
        with pytest.raises(dev.SkredAmdError):                   # no buffer
            db.set_taps(ids, 0)
        ordinary_block()
        assert db.last_taps() == len(ids)
        ref = bank.copy()
        cpuref.render(ref, g.copy(), tables, 5 * F, 0)           # the refused launch rendered nothing
        got = bank.copy()
        db.download(got)
        assert not got.rw_equal(ref), got.rw_equal(ref)
    finally:
        db.set_probe([], 0)
        db.set_taps([], 0)
        db.close()


def test_abi_declares_taps():
    """(CPU) The header, the library and the binding agree on the two entry points."""
    import ctypes
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "skred_amd.h")).read()
    L = ctypes.CDLL(os.path.join(root, "skred_amd", "libskred_amd.so"))
    for s in ("skred_bank_set_taps", "skred_bank_last_taps"):
        assert s + "(" in hdr and hasattr(L, s)
    assert "#define SKRED_TAPS_MAX 64" in hdr
