"""Fuzz of the modulated kernel (skred_render_generic.hip: sk_render_mod_kernel and its tape forms) over blocks, forms and group edges.

Banks, control actions and block lists come from tests/fuzz_banks.py: every voice feature at random, FM / AM / pan / CZ modulators
inside the 64-voice group or (SKRED_OPT_CROSS_GROUP) in other groups, block lengths 1, 2, 63, 64, 65 and one above 512 in random
order, control actions between the blocks (pushed at once or through the deferred queue).  The oracle renders each plan once
(trajectory); every form of the kernel -- level loop / frame-lag form (SKRED_OPT_FM_SKEW 0 / 1), packed lanes or not, with the stem
buffer or without -- is then checked against it after EVERY block: read-write state and globals bit for bit, stems bit for bit
where they are taken, the mix within 1e-5 relative RMS of the oracle's f64 sum through cpuref.master.  Nothing is masked: the
seeds are chosen so that the oracle's output is finite (test_fuzz_seeds_reach_every_form, which runs without a GPU).
"""
import functools
import os

import numpy as np
import pytest

import fuzz_banks
import golden_io as gio
import mod_forms
from oracle import cpuref

SEEDS = list(range(int(os.environ.get("SKRED_FUZZ_SEEDS", "6"))))
DEFAULT_SEEDS = list(range(6))         # the seeds test_fuzz_seeds_reach_every_form settles its conditions on
SIZES = {"own_group": [64, 320, 1000, 4096], "cross_group": [1000, 4096, 65536]}
STEMS_UP_TO = 4096                     # larger banks run without the stem buffer
MIX_TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    from skred_amd import device
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, np.float64) ** 2)))


def rel_rms(a, b):
    return rms(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(rms(b), 1e-30)


# ---------------------------------------------------------------------------------------------- plans and the oracle's side

@functools.lru_cache(maxsize=1)
def pool():
    gold = gio.load("c4_pcm_oneshot")            # a sine and five one-shot tables in one pool
    return gold.tables, fuzz_banks.catalogue(gold.segments[0].bank_in), gold.segments[0].g_in


def sparse(routing, seed):
    """Which seeds draw a sparse bank (fuzz_banks.wild_bank: every group needs well under 32 lanes, so SKRED_OPT_PACK 2 packs every
    block).  The others are dense: their busiest group needs more than 32 lanes and a launch with SKRED_OPT_PACK 2 stays unpacked.
    The periods are coprime to those of the sizes, so every size comes both ways."""
    return seed % 3 != 0 if routing == "own_group" else seed % 2 == 1


def plan(routing, seed):
    """(bank, globals, [(frames, [actions], deferred?)]) of one seed."""
    tables, cat, g0 = pool()
    rng = np.random.default_rng({"own_group": 2000, "cross_group": 3000}[routing] + seed)
    n = SIZES[routing][seed % len(SIZES[routing])]
    bank, tiers = fuzz_banks.wild_bank(rng, n, cat, routing, sparse=sparse(routing, seed))
    frames = fuzz_banks.block_lengths(rng)
    acts = fuzz_banks.spread(rng, fuzz_banks.events(rng, bank, 12, tiers), len(frames))
    deferred = [bool(x) for x in rng.random(len(frames)) < 0.4]
    g = g0.copy()
    g.synth_sample_count = fuzz_banks.COUNT0
    return bank, g, list(zip(frames, acts, deferred))


def cross_plan(bank):
    """(sources, pre-pass levels) the library must report for `bank` (skred_bank_plan.c: sk_tape_plan_host): the distinct modulators outside
    their reader's 64-voice group; a source group's level is 0 when it reads no other group, else 1 + the highest it reads."""
    v = np.arange(bank.n)
    fm = np.asarray(bank["voice_freq_mod_osc"]).copy()
    fm[fm == v] = -1
    cz = np.where(np.asarray(bank["voice_cz_mode"]) != 0, np.asarray(bank["voice_cz_mod_osc"]), -1)
    reads, sources = {}, mod_forms.far_sources(bank)
    for m in (fm, np.asarray(bank["voice_amp_mod_osc"]), np.asarray(bank["voice_pan_mod_osc"]), cz):
        far = (m >= 0) & ((m >> 6) != (v >> 6))
        for rg, sg in set(zip((v[far] >> 6).tolist(), (m[far] >> 6).tolist())):
            reads.setdefault(rg, set()).add(sg)
    if not sources:
        return (0, 0)
    level = {}

    def lvl(g):
        if g not in level:
            level[g] = 1 + max(lvl(h) for h in reads[g]) if g in reads else 0
        return level[g]

    return (len(sources), 1 + max(lvl(s >> 6) for s in sources))


def form_of_groups(bank, frames, skew=1):
    """Per 64-voice group of an unpacked launch without stems: 'lag', 'loop', or None when the bank has no same-frame dependency."""
    if mod_forms.levels(bank).max() < 1:
        return [None] * ((bank.n + 63) // 64)
    lag = mod_forms.lag_groups(bank) & bool(skew and frames >= 2)
    return ["lag" if x else "loop" for x in lag]


@functools.lru_cache(maxsize=2)
def trajectory(routing, seed):
    """The oracle's side of plan(routing, seed), block by block: the state and globals after the block, the mix through
    cpuref.master, the stems (banks up to STEMS_UP_TO voices), and what the bank as it stood predicts about the launch."""
    tables = pool()[0]
    bank, g, blocks = plan(routing, seed)
    host, gl = bank.copy(), g.copy()
    out = []
    for frames, acts, deferred in blocks:
        rewired = False                                          # a voice that sounds gets another modulator, or loses one
        for a in acts:
            if a.kind in ("repoint_own", "repoint_far", "unplug"):
                rewired |= bool(((host["voice_amp"][a.voices] != 0) & (host["voice_finished"][a.voices] == 0)).any())
            a.apply(host, gl.synth_sample_count)
        sources = mod_forms.far_sources(host) if routing == "cross_group" else ()
        lanes = mod_forms.pack_lanes(host, sources)
        pre = {"forms": form_of_groups(host, frames), "counts": {s: mod_forms.expected_counts(host, frames, s) for s in (0, 1)},
               "pack": lanes, "rewired": rewired,
               "packed_counts": {s: mod_forms.expected_packed_counts(host, frames, s, sources) for s in (0, 1)} if lanes else None,
               "cross": cross_plan(host), "bank": host.copy() if routing == "cross_group" and host.n <= STEMS_UP_TO else None}
        r = cpuref.render(host, gl, tables, frames, 0, want_stems=host.n <= STEMS_UP_TO)
        mix = cpuref.master(gl, r["sum64"].astype(np.float32))
        out.append(dict(pre, frames=frames, state=host.copy(), g=gl.copy(), mix=mix, stems=r["stems"],
                        finite=bool(np.isfinite(r["sum64"]).all() and np.isfinite(mix).all()
                                    and (r["stems"] is None or np.isfinite(r["stems"]).all()))))
    return bank, g, blocks, out


# ---------------------------------------------------------------------------------------------- what the seeds must reach (no GPU)

def source_kinds(bank):
    """Which kinds of voice the cross-group sources of `bank` are."""
    v = np.arange(bank.n)
    cz_on = np.asarray(bank["voice_cz_mode"]) != 0
    src = set()
    for f in ("voice_freq_mod_osc", "voice_amp_mod_osc", "voice_pan_mod_osc", "voice_cz_mod_osc"):
        m = np.asarray(bank[f])
        far = (m >= 0) & ((m >> 6) != (v >> 6)) & (cz_on if f == "voice_cz_mod_osc" else True) & (m != v)
        src |= set(int(x) for x in m[far])
    s = np.array(sorted(src), np.int64)
    live = bank["voice_amp"][s] != 0
    kinds = {"one_shot": (bank["voice_one_shot"][s] != 0) & (bank["voice_loop_enabled"][s] == 0),
             "noise": bank["voice_wave_table_index"][s] == 6, "held": bank["voice_sample_hold_max"][s] > 0,
             "crushed": bank["voice_quantize"][s] > 0, "reversed": bank["voice_direction"][s] != 0,
             "cz_modulated": (bank["voice_cz_mode"][s] != 0) & (bank["voice_cz_mod_osc"][s] >= 0)}
    return {k for k, m in kinds.items() if (m & live).any()}


def test_fuzz_seeds_reach_every_form():
    """The conditions the default seeds are chosen to meet, from the generator, mod_forms and the oracle alone.  That the oracle's
    output is finite takes rendering every plan, the two of 65536 voices included: most of this test's time on a CPU."""
    lag = loop = packed_lag = packed_loop = 0
    changed = rewired_packed = False
    kinds, deepest, lanes = set(), 0, set()
    for routing in ("own_group", "cross_group"):
        for seed in DEFAULT_SEEDS:
            bank, g, blocks, traj = trajectory(routing, seed)
            assert all(t["finite"] for t in traj), f"{routing} seed {seed}: the oracle's output is not finite"
            for k, t in enumerate(traj):
                lag += t["counts"][1][0]
                loop += t["counts"][1][1]
                if sparse(routing, seed):                       # every block of a sparse plan runs packed under SKRED_OPT_PACK 2 ...
                    assert 0 < t["pack"] <= 32, f"{routing} seed {seed} block {k}: the busiest group needs too many lanes to pack"
                    lanes.add(t["pack"])
                    packed_lag += t["packed_counts"][1][0]
                    packed_loop += t["packed_counts"][1][1]
                    rewired_packed |= t["rewired"]
                else:                                           # ... and no block of a dense one
                    assert t["pack"] == 0, f"{routing} seed {seed} block {k}"
            for a, b in zip(traj, traj[1:]):
                if a["frames"] >= 2 and b["frames"] >= 2:       # (a 1-frame block never takes the lag form: not counted as a change)
                    changed |= any(x != y and x and y for x, y in zip(a["forms"], b["forms"]))
            if routing == "cross_group":
                deepest = max([deepest] + [t["cross"][1] for t in traj])
                if bank.n <= STEMS_UP_TO:
                    for t in traj:
                        kinds |= source_kinds(t["bank"])
    assert lag > 0 and loop > 0, (lag, loop)
    assert packed_lag > 0 and packed_loop > 0, (packed_lag, packed_loop)
    assert len(lanes) >= 2, f"packed launches of one width only: {lanes}"
    assert rewired_packed, "no re-pointed or unplugged modulator of a sounding voice lands in a packed launch"
    assert changed, "no group changes between the frame-lag form and the level loop from one block to the next"
    assert kinds == {"one_shot", "noise", "held", "crushed", "reversed", "cz_modulated"}, kinds
    assert deepest >= 3, deepest


# ---------------------------------------------------------------------------------------------- the device's side

def run_form(dev, routing, seed, stems=False, pack=None, skew=None, counts=False):
    """One form of the kernel over the whole plan on a fresh device bank, checked against the trajectory after every block.
    Returns per block (mix, last_cross_group, last_kernel, last_pack, form counts or None)."""
    tables = pool()[0]
    bank, g, blocks, traj = trajectory(routing, seed)
    db = dev.DeviceBank(bank.n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    if routing == "cross_group":
        db.set_cross_group(True)
    if pack is not None:
        db.set_pack(pack)
    if skew is not None:
        db.set_fm_skew(skew)
    if counts:
        import torch
        ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
        db.set_form_counter(ctr.data_ptr())
    out = []
    what = f"{routing} seed {seed} n={bank.n} stems={stems} pack={pack} skew={skew}"
    try:
        mirror, now = bank.copy(), int(g.synth_sample_count)
        for k, ((frames, acts, deferred), t) in enumerate(zip(blocks, traj)):
            queued = 0
            for a in acts:                                       # the same actions, on the state the oracle had (== the device's)
                voices, dirty = a.apply(mirror, now)
                if len(voices) == 0:
                    continue
                if deferred:
                    db.defer(now + min(frames, 1 + queued), mirror, voices, dirty)
                    queued += 1
                else:
                    db.update(mirror, voices, dirty)
            if deferred:
                assert db.run_queue(frames) == queued and db.queue_pending() == 0
            if counts:
                ctr.zero_()
                torch.cuda.synchronize()
            mix, st = db.render_host(frames, 2, 0, want_stems=stems)
            info = (db.last_cross_group(), db.last_kernel(), db.last_pack())
            fc = None
            if counts:
                torch.cuda.synchronize()
                fc = ctr.cpu().numpy().tolist()
            got = t["state"].copy()
            db.download(got)
            bad = got.rw_equal(t["state"])
            assert not bad, f"{what} block {k} ({frames} frames): voice state differs from the oracle: {bad}"
            gl = db.get_globals()
            assert gl.synth_sample_count == t["g"].synth_sample_count and gl.noise_rng == t["g"].noise_rng, f"{what} block {k}"
            assert np.float32(gl.volume_smoother_gain).tobytes() == np.float32(t["g"].volume_smoother_gain).tobytes(), f"{what} block {k}"
            if stems:
                assert (st.view(np.uint32) == t["stems"].view(np.uint32)).all(), f"{what} block {k} ({frames} frames): stems differ"
            err = rel_rms(mix, t["mix"])
            assert err <= MIX_TOL, f"{what} block {k} ({frames} frames): mix rel rms {err}"
            out.append((mix,) + info + (fc,))
            mirror, now = t["state"].copy(), now + frames
    finally:
        if counts:
            db.set_form_counter(0)
        db.close()
    return out


def all_forms(dev, routing, seed):
    """{pack 0, pack 2} x {skew 0, skew 1} without stems (+ one run with the stem buffer), and what must hold between them.  With
    SKRED_OPT_PACK 2 a block runs packed when the bank as it stands lets it (mod_forms.pack_lanes): every block of a sparse seed,
    none of a dense one."""
    bank, g, blocks, traj = trajectory(routing, seed)
    assert all(t["finite"] for t in traj)
    res = {(p, s): run_form(dev, routing, seed, pack=p, skew=s, counts=True) for p in (0, 2) for s in (0, 1)}
    for p in (0, 2):                                             # "same bits either way" (SKRED_OPT_FM_SKEW)
        for k, (a, b) in enumerate(zip(res[p, 0], res[p, 1])):
            assert (a[0].view(np.uint32) == b[0].view(np.uint32)).all(), f"{routing} seed {seed} pack {p} block {k}: skew 0 / 1 mixes differ"
    for s in (0, 1):                                             # packed lanes: the same state (checked above), the sum reordered
        for a, b in zip(res[0, s], res[2, s]):
            assert rel_rms(b[0], a[0]) <= MIX_TOL
            assert a[1] == b[1]
    for s in (0, 1):                                             # the form every wavefront took, block by block
        for k, (r, t) in enumerate(zip(res[0, s], traj)):
            assert r[3] == 0
            assert r[4] == t["counts"][s], f"{routing} seed {seed} skew {s} block {k}: forms {r[4]}, predicted {t['counts'][s]}"
        for k, (r, t) in enumerate(zip(res[2, s], traj)):
            what = f"{routing} seed {seed} pack 2 skew {s} block {k}"
            assert r[3] == t["pack"], f"{what}: {r[3]} lanes per group, the bank needs {t['pack']}"
            if sparse(routing, seed):
                assert 0 < r[3] <= 32, f"{what}: a sparse bank's block did not run packed"
            want = t["packed_counts"][s] if t["pack"] else t["counts"][s]
            assert r[4] == want, f"{what}: forms {r[4]}, predicted {want}"
    if bank.n <= STEMS_UP_TO:
        res["stems"] = run_form(dev, routing, seed, stems=True)
    return res, traj


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_own_group_fuzz(dev, seed):
    res, traj = all_forms(dev, "own_group", seed)
    for rs in res.values():
        assert all(r[2] == 2 and r[1] == (0, 0) for r in rs)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_cross_group_fuzz(dev, seed):
    res, traj = all_forms(dev, "cross_group", seed)
    for form, rs in res.items():
        for k, (r, t) in enumerate(zip(rs, traj)):
            assert r[2] == 2, (form, k, r[2])
            assert r[1] == t["cross"], f"seed {seed} {form} block {k}: tape {r[1]}, the bank needs {t['cross']}"


# ---------------------------------------------------------------------------------------------- the reference's own numbers

def render_segment(dev, g, seg, stems, skew=None):
    db = dev.DeviceBank(seg.bank_in.n)
    db.set_tables(g.tables)
    db.upload(seg.bank_in)
    db.set_globals(seg.g_in)
    if skew is not None:
        db.set_fm_skew(skew)
    mix = np.zeros((seg.frames, 2), np.float32)
    st = np.zeros((seg.frames, seg.bank_in.n, 2), np.float32) if stems else None
    p = 0
    try:
        while p < seg.frames:                                    # the callback structure the reference rendered with
            n = min(seg.block, seg.frames - p)
            buf, s = db.render_host(n, 2, 0, want_stems=stems)
            assert db.last_kernel() == 2
            mix[p:p + n] = buf
            if stems:
                st[p:p + n] = s
            p += n
        got = seg.bank_in.copy()
        db.download(got)
        gl = db.get_globals()
    finally:
        db.close()
    return mix, st, got, gl


@pytest.mark.gpu
@pytest.mark.parametrize("case", gio.FUZZ_CASES)
def test_reference_fuzz_fixtures_on_the_modulated_kernel(dev, case):
    """The fuzz fixtures (64 voices, modulators anywhere, actions between the segments) against the REFERENCE's own numbers: with
    the stem buffer (level loop) stems by sha256; without it with SKRED_OPT_FM_SKEW 0 and 1; state bit for bit, mix 1e-5."""
    g = gio.load(case)
    for seg in g.segments:
        mixes = {}
        for form, stems, skew in (("stems", True, None), ("skew0", False, 0), ("skew1", False, 1)):
            mix, st, got, gl = render_segment(dev, g, seg, stems, skew)
            what = f"{case} seg{seg.index} {form}"
            if stems:
                assert gio.sha256(st) == seg.stems_sha256, f"{what}: per-voice stems differ from the reference"
            bad = got.rw_equal(gio.expected_out_bank(seg))
            assert not bad, f"{what}: voice state differs from the reference: {bad}"
            assert gl.synth_sample_count == seg.g_out.synth_sample_count and gl.noise_rng == seg.g_out.noise_rng, what
            assert np.float32(gl.volume_smoother_gain).tobytes() == np.float32(seg.g_out.volume_smoother_gain).tobytes(), what
            assert rel_rms(mix, seg.mix) <= MIX_TOL, f"{what}: mix rel rms {rel_rms(mix, seg.mix)}"
            mixes[form] = mix
        assert gio.bits_equal(mixes["skew0"], mixes["skew1"]), f"{case} seg{seg.index}: skew 0 / 1 mixes differ"
