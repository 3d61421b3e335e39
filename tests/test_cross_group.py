"""Modulation across aligned 64-voice groups (SKRED_OPT_CROSS_GROUP): the per-block source tape.

A voice whose FM / AM / pan / CZ modulator sits in another 64-voice group of the bank reads that modulator's samples from a tape
the pre-pass launches of the modulated kernel render ahead of the block (skred_render_generic.hip: sk_render_mod_tape_kernel).
The oracle walks every voice in index order (synth.c:526-612), so a reader sees the same frame's sample of a source below it and
the previous frame's of a source above it (the state's voice_sample at frame 0).  Every test switches the option on, renders
several blocks with control actions between them and checks, after every block, the whole state bit for bit against
oracle.cpuref, stems bit for bit where they are cheap, and the mix within 1e-5.
"""
import os

import numpy as np
import pytest

import mod_forms
from oracle import cpuref
from skred_amd import banks
from skred_amd.bank import VoiceBank

pytestmark = pytest.mark.gpu

PATCH_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "skred_amd", "data", "patches")
MOD_FIELDS = ("voice_freq_mod_osc", "voice_amp_mod_osc", "voice_pan_mod_osc", "voice_cz_mod_osc")


@pytest.fixture(scope="module")
def dev():
    from skred_amd import device
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, np.float64) ** 2)))


def rel_rms(a, b):
    return rms(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(rms(b), 1e-30)


def open_bank(dev, bank, tables, g, pack=None, skew=None):
    db = dev.DeviceBank(bank.n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    db.set_cross_group(True)
    if pack is not None:
        db.set_pack(pack)
    if skew is not None:
        db.set_fm_skew(skew)
    return db


def run(dev, bank, tables, g, blocks, stems=False, pack=None, skew=None, counts=None):
    """Render `blocks` -- (frames, event) pairs; event(host, db, count) changes the host bank (the oracle's copy) and pushes the same
    change to the device, or is None -- on a fresh device bank and in the oracle, checking after every block.  Returns per block
    (mix, last_cross_group, last_kernel, last_pack, form counts or None)."""
    host, gl = bank.copy(), g.copy()
    db = open_bank(dev, host, tables, gl, pack, skew)
    if counts is not None:
        import torch
        ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
        db.set_form_counter(ctr.data_ptr())
    out = []
    try:
        for k, (frames, event) in enumerate(blocks):
            if event is not None:
                event(host, db, gl.synth_sample_count)
            if counts is not None:
                ctr.zero_()
                torch.cuda.synchronize()
            mix, st = db.render_host(frames, 2, 0, want_stems=stems)
            info = (db.last_cross_group(), db.last_kernel(), db.last_pack())
            fc = None
            if counts is not None:
                torch.cuda.synchronize()
                fc = ctr.cpu().numpy().tolist()
            r = cpuref.render(host, gl, tables, frames, 0, want_stems=stems)
            ref_mix = cpuref.master(gl, r["sum64"].astype(np.float32))
            got = host.copy()
            db.download(got)
            bad = got.rw_equal(host)
            assert not bad, f"block {k}: voice state differs from the oracle: {bad}"
            if stems:
                assert (st.view(np.uint32) == r["stems"].view(np.uint32)).all(), f"block {k}: stems differ from the oracle"
            err = rel_rms(mix, ref_mix)
            assert err <= 1e-5, f"block {k}: mix rel rms {err}"
            out.append((mix,) + info + (fc,))
    finally:
        if counts is not None:
            db.set_form_counter(0)
        db.close()
    return out


def params(*voices):
    """An event that pushes the parameters of `voices` as the host bank has them after `change(host)`."""
    def wrap(change):
        def event(host, db, count):
            change(host)
            db.update(host, np.array(voices, np.int32), dev_dirty_params())
        return event
    return wrap


def dev_dirty_params():
    from skred_amd import device
    return device.DIRTY_PARAMS


# ---------------------------------------------------------------------------------------------- 1. one LFO for the whole bank

def global_lfo_bank(n):
    bank, tables, g = banks.bank_c2(n)
    v = np.arange(n)
    bank["voice_phase_inc"][0] = np.float32(0.37)            # voice 0: a slow sine for everyone
    bank["voice_amp_mod_osc"][1:] = 0
    bank["voice_amp_mod_depth"][1:] = np.float32(0.8)
    third = (v % 3 == 0) & (v > 0)
    bank["voice_pan_mod_osc"][third] = 0
    bank["voice_pan_mod_depth"][third] = np.float32(0.5)
    seventh = (v % 7 == 0) & (v > 0)
    bank["voice_freq_mod_osc"][seventh] = 0
    bank["voice_freq_mod_depth"][seventh] = np.float32(0.02)
    bank["voice_freq_scale"][seventh] = np.float32(1.0)
    return bank, tables, g


def test_global_lfo_2e16(dev):
    bank, tables, g = global_lfo_bank(1 << 16)
    res = run(dev, bank, tables, g, [(256, None), (300, None), (64, None)])
    for _, cg, kern, _, _ in res:
        assert kern == 2 and cg == (1, 1)


def test_global_lfo_2e20(dev):
    bank, tables, g = global_lfo_bank(1 << 20)
    res = run(dev, bank, tables, g, [(128, None), (128, None)])
    assert all(r[2] == 2 and r[1] == (1, 1) for r in res)


# ---------------------------------------------------------------------------------------------- 2. sources of every kind

def sources_bank(n=4096, F=256):
    """Sources spread over the bank, each read from below and from above (other groups), each of a kind of its own."""
    bank, tables, g = banks.bank_c2(n)
    count0 = int(g.synth_sample_count)
    size = bank["voice_table_size"].astype(np.float32)

    def src(s, readers, field="voice_amp_mod_osc", depth=0.7):
        for r in readers:
            bank[field][r] = s
            bank[field.replace("_osc", "_depth")][r] = np.float32(depth)

    src(1000, [5, 70, 900, 1100, 2500])                                          # plain, readers on both sides
    src(2000, [100, 163, 2100], field="voice_pan_mod_osc", depth=0.6)           # muted between blocks (below: stale value at frame 0)
    for s, at in ((3000, 100), (3100, F - 1)):                                   # one-shots finishing mid-block / on the last frame
        bank["voice_one_shot"][s], bank["voice_loop_enabled"][s], bank["voice_direction"][s] = 1, 0, 0
        bank["voice_phase"][s] = np.float32(size[s] - bank["voice_phase_inc"][s] * np.float32(at + 0.5))
    src(3000, [200, 3070])
    src(3100, [300, 3200], field="voice_pan_mod_osc", depth=0.4)
    bank["voice_direction"][1500] = 1                                            # reversed
    src(1500, [400, 1600])
    bank["voice_wave_table_index"][1700] = 6                                     # noise (SKRED_WAVE_TABLE_NOISE_ALT)
    src(1700, [10, 1800])
    bank["voice_sample_hold_max"][1900] = 5                                      # sample & hold
    src(1900, [20, 2300])
    bank["voice_quantize"][2200] = 4                                             # bit-crush
    src(2200, [30, 2400])
    env = bank["voice_amp_envelope"]                                             # envelope in its attack through the blocks
    env["sample_start"][2600], env["sample_release"][2600], env["is_active"][2600] = count0 - 10, 0, 1
    src(2600, [40, 2700])
    bank["voice_freq_mod_osc"][[50, 2800]] = 2900                                # FM: voice_phase_inc changes between blocks
    bank["voice_freq_mod_depth"][[50, 2800]] = np.float32(0.05)
    bank["voice_freq_scale"][[50, 2800]] = np.float32(1.0)
    return bank, tables, g


def test_sources_of_every_kind(dev):
    F = 256
    bank, tables, g = sources_bank(4096, F)

    def mute(host):
        host["voice_amp"][2000] = 0.0

    def retune(host):
        host["voice_phase_inc"][2900] = host["voice_phase_inc"][2900] * np.float32(1.5)

    blocks = [(F, None), (F, params(2000)(mute)), (F, params(2900)(retune)), (100, None)]
    res = run(dev, bank, tables, g, blocks, stems=True)
    assert all(r[2] == 2 and r[1] == (10, 1) for r in res), [r[1:4] for r in res]
    res = run(dev, bank, tables, g, blocks, stems=False)                        # the frame-lag / level-loop forms, no stems
    assert all(r[1] == (10, 1) for r in res)


# ---------------------------------------------------------------------------------------------- 3. shipped patches across edges

def straddling_bank(patch, n, stride, offset):
    """`patch` (skred_amd/data/patches) laid out back to back: a copy every `stride` voices from `offset` on, modulator indices
    moved along, so that copies straddle the aligned 64-voice groups; the voices between copies stay empty."""
    one, tables, g = banks.bank_patch(patch, 64)
    z = np.load(os.path.join(PATCH_DIR, f"patch_{patch}.npz"))
    used = np.where((z["in_voice_amp"] != 0) & (z["in_voice_table_size"] > 0))[0]
    K = int(used.max()) + 1
    assert stride >= K
    b = VoiceBank(n)
    c = 0
    while offset + c * stride + K <= n:
        o = offset + c * stride
        for name in b.a:
            b.a[name][o:o + K] = one.a[name][:K]
        for f in MOD_FIELDS:
            m = one.a[f][:K]
            b.a[f][o:o + K] = np.where(m >= 0, m + o, m)
        c += 1
    return b, tables, g


# (18.sk -- voice 0 reads 1, 1 reads 2, 10 reads 0 -- makes two groups read each other when a group edge falls between its voices 0
# and 1 or 1 and 2: a cycle, refused.  Copies at multiples of 4 never put an edge there, and some put one between voices 2 and 10.)
@pytest.mark.parametrize("patch,stride,offset", [("3sk", 13, 5), ("7sk", 11, 1), ("18sk", 12, 4), ("37sk", 11, 7)])
def test_shipped_patches_straddling_group_edges(dev, patch, stride, offset):
    bank, tables, g = straddling_bank(patch, 4096, stride, offset)
    blocks = [(256, None), (256, None), (65, None)]
    mixes = {}
    for skew in (0, 1):
        res = run(dev, bank, tables, g, blocks, pack=0, skew=skew, counts=True)
        for (frames, _), r in zip(blocks, res):
            assert r[2] == 2 and r[1][0] > 0
            assert r[4] == mod_forms.expected_counts(bank, frames, skew), (skew, r[4])
        mixes[skew] = [r[0] for r in res]
    for a, b in zip(mixes[0], mixes[1]):
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), "the frame-lag form and the level loop differ"


# ---------------------------------------------------------------------------------------------- 4. chains and CZ

def test_chain_of_groups_and_cz(dev):
    bank, tables, g = banks.bank_c2(4096)
    bank["voice_amp_mod_osc"][130] = 70                       # group 2 reads group 1 ...
    bank["voice_amp_mod_depth"][130] = np.float32(0.9)
    bank["voice_freq_mod_osc"][70] = 5                        # ... which reads group 0
    bank["voice_freq_mod_depth"][70] = np.float32(0.03)
    bank["voice_freq_scale"][70] = np.float32(1.0)
    bank["voice_cz_mode"][200] = 1                            # a cross-group CZ amount with CZ on
    bank["voice_cz_mod_osc"][200] = 10
    bank["voice_cz_mod_depth"][200] = np.float32(0.3)
    bank["voice_cz_distortion"][200] = np.float32(0.2)
    bank["voice_cz_mode"][300] = 3                            # ... and one from above
    bank["voice_cz_mod_osc"][300] = 1000
    bank["voice_cz_mod_depth"][300] = np.float32(0.25)
    res = run(dev, bank, tables, g, [(256, None), (256, None)], stems=True)
    assert all(r[1] == (4, 2) for r in res), [r[1] for r in res]
    run(dev, bank, tables, g, [(256, None), (256, None)])


# ---------------------------------------------------------------------------------------------- 5. packed lanes

def test_packed_lanes_with_cross_group_sources(dev):
    bank, tables, g = straddling_bank("3sk", 8192, 13, 5)
    # a source whose only readers are in other groups, and that cannot sound itself after the first block
    bank["voice_amp_mod_osc"][[6, 700, 4000]] = 3000
    bank["voice_amp_mod_depth"][[6, 700, 4000]] = np.float32(0.5)
    blocks = [(256, None), (256, None)]
    packed = run(dev, bank, tables, g, blocks, pack=2)
    plain = run(dev, bank, tables, g, blocks, pack=0)
    assert all(r[3] > 0 for r in packed) and all(r[3] == 0 for r in plain)
    for a, b in zip(packed, plain):
        assert a[1] == b[1] and a[1][0] > 0
        assert rel_rms(a[0], b[0]) <= 1e-5


# ---------------------------------------------------------------------------------------------- 6. routings that change

def test_routing_changes_between_blocks(dev):
    from skred_amd import device
    bank, tables, g = banks.bank_c2(4096)
    bank["voice_amp_mod_osc"][100] = 10                        # group 1 reads group 0
    bank["voice_amp_mod_depth"][100] = np.float32(0.8)

    def to_own_group(host):
        host["voice_amp_mod_osc"][100] = 70

    def back_deferred(host, db, count):
        host["voice_amp_mod_osc"][100] = 10
        db.defer(count + 10, host, np.array([100], np.int32), device.DIRTY_PARAMS)
        assert db.run_queue(256) == 1

    def new_source(host):
        host["voice_pan_mod_osc"][300] = 3000
        host["voice_pan_mod_depth"][300] = np.float32(0.5)

    def drop_source(host):
        host["voice_amp_mod_osc"][100] = -1

    blocks = [(256, None), (256, params(100)(to_own_group)), (256, back_deferred), (256, params(300)(new_source)),
              (256, params(100)(drop_source))]
    res = run(dev, bank, tables, g, blocks)
    assert [r[1] for r in res] == [(1, 1), (0, 0), (1, 1), (2, 1), (1, 1)]


# ---------------------------------------------------------------------------------------------- 7. refusals

def refusal_case(dev, change, fix):
    """`change` makes the bank refused with the option on; after `fix` the same device bank renders as the oracle does."""
    bank, tables, g = banks.bank_c2(2048)
    host, gl = bank.copy(), g.copy()
    db = open_bank(dev, host, tables, gl)
    try:
        voices = change(host)
        db.update(host, np.array(voices, np.int32), dev.DIRTY_PARAMS)
        with pytest.raises(dev.SkredAmdError):
            db.render_host(64)
        voices = fix(host)
        db.update(host, np.array(voices, np.int32), dev.DIRTY_PARAMS)
        mix, _ = db.render_host(128)
        r = cpuref.render(host, gl, tables, 128, 0)
        got = host.copy()
        db.download(got)
        assert not got.rw_equal(host)
        assert rel_rms(mix, cpuref.master(gl, r["sum64"].astype(np.float32))) <= 1e-5
        return db.last_cross_group()
    finally:
        db.close()


def test_refusals(dev):
    def cycle(h):
        h["voice_amp_mod_osc"][10], h["voice_amp_mod_osc"][100] = 100, 10
        return [10, 100]

    def uncycle(h):
        h["voice_amp_mod_osc"][100] = -1
        return [100]

    assert refusal_case(dev, cycle, uncycle) == (1, 1)

    def chain18(h):                                            # 18 groups in a row: 17 pre-pass levels
        for k in range(1, 18):
            h["voice_amp_mod_osc"][64 * k + 1] = 64 * (k - 1) + 1
        return [64 * k + 1 for k in range(1, 18)]

    def cut(h):                                                # two chains of 9 groups: 8 source groups deep
        h["voice_amp_mod_osc"][64 * 9 + 1] = -1
        return [64 * 9 + 1]

    assert refusal_case(dev, chain18, cut) == (16, 8)

    def outside(h):
        h["voice_freq_mod_osc"][10] = h.n + 5
        return [10]

    def inside(h):
        h["voice_freq_mod_osc"][10] = 1000
        return [10]

    assert refusal_case(dev, outside, inside) == (1, 1)


def test_option_off_still_refuses(dev):
    bank, tables, g = banks.bank_c2(256)
    bank["voice_amp_mod_osc"][70] = 3
    db = dev.DeviceBank(bank.n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    try:
        with pytest.raises(dev.SkredAmdError):
            db.render_host(64)
        db.set_cross_group(True)
        db.render_host(64)
        assert db.last_cross_group() == (1, 1)
        db.set_cross_group(False)
        with pytest.raises(dev.SkredAmdError):
            db.render_host(64)
    finally:
        db.close()
