"""The free-voice query (skred_bank_find_idle): an ordered list of idle voices, built on the device.

Every expectation is computed in numpy, with exact comparisons, from the ORACLE's bank after cpuref.render of the same blocks and
events (the oracle's per-voice state is bit-identical to the device's: the project's standing contract), and a second time from
DeviceBank.download of a twin bank that ran the same blocks without ever being queried.  The two expectations must agree with each
other and with the query.  Before the device is consulted each case asserts on the oracle's state that it is not vacuous: every
selected criterion holds for at least one voice of the range and fails for at least one (a one-voice bank cannot do both: n = 1
runs once with an idle voice and once with a sounding one).  d_voices is pre-filled with -1; entries past `written` must stay -1.

The workgroup span is 256 voices (skred_launch.h: SK_IDLE_SPAN): 70 000 voices make 274 workgroups, more than the 256 threads of
the workgroup that scans the offsets, so that size needs no raising.
"""
import functools

import numpy as np
import pytest

from oracle import cpuref
from skred_amd import banks

FIN, ENV, AMP, UNNAMED = 1, 2, 4, 256
DIRTY_PARAMS, DIRTY_PHASE, STAMP_TRIGGER, STAMP_RELEASE = 1, 2, 256, 512
SPAN = 256
FRAMES = (65, 130)          # the blocks every scene renders before it is queried
SETTLE = np.float32(1e-3)


@pytest.fixture(scope="module")
def dev():
    from skred_amd import device
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


# ---------------------------------------------------------------------------------------------- the expectation (numpy, exact)

def named_set(host):
    """bit v: some voice of the bank names v -- FM by the voice itself and a CZ source with CZ off name nobody (include/skred_amd.h)."""
    a, n = host.a, host.n
    fm = np.where(a["voice_freq_mod_osc"] == np.arange(n), -1, a["voice_freq_mod_osc"])
    cz = np.where(a["voice_cz_mode"] != 0, a["voice_cz_mod_osc"], -1)
    ids = np.concatenate([fm, a["voice_amp_mod_osc"], a["voice_pan_mod_osc"], cz]).astype(np.int64)
    out = np.zeros(n, bool)
    out[ids[(ids >= 0) & (ids < n)]] = True
    return out


def criteria(host, v, settle):
    a = host.a
    e = a["voice_amp_envelope"]
    settled = (a["voice_smoother_enable"][v] == 0) | (np.abs(a["voice_smoother_gain"][v]) <= np.float32(settle))
    return {FIN: a["voice_finished"][v] != 0,
            ENV: (a["voice_use_amp_envelope"][v] != 0) & (e["is_active"][v] == 0) & settled,
            AMP: a["voice_amp"][v] == 0}


def expected(host, first, count, which, settle=0.0, start=None, check=False):
    v = np.arange(first, first + count)
    crit = criteria(host, v, settle)
    idle = np.zeros(count, bool)
    for bit, holds in crit.items():
        if which & bit:
            idle |= holds
            if check:
                assert holds.any() and not holds.all(), f"criterion {bit} is vacuous on [{first},+{count}): {int(holds.sum())} of {count}"
    if which & UNNAMED:
        named = named_set(host)[v]
        if check:
            assert (idle & named).any(), "no otherwise-idle voice is named"
        idle &= ~named
    lst = v[idle]
    k = int(np.searchsorted(lst, first if start is None else start))
    return np.concatenate([lst[k:], lst[:k]]).astype(np.int32)


# ---------------------------------------------------------------------------------------------- banks

def idle_bank(n, flavour="stops"):
    """bank_c2 with a role per voice (the first and the last twelve voices hold every role once, the rest are drawn):
    0 sustaining; 1 forward one-shot that finishes inside block 0; 2 one-shot that finishes on the LAST frame of block 0 (the first
    such voice whose table is long enough) or inside block 1; 3 one-shot that does not finish; 4 / 5 released so that the release
    ends mid-block, smoother fast (gain far below SETTLE afterwards, stalled on a subnormal) / slow (gain above SETTLE); 6 still in
    release; 7 amp 0; 8 enveloped WITHOUT smoother, release ends mid-block; 9 envelope inactive and gain exactly 0 from the start;
    10 no envelope, is_active 0 (ENV_DONE must not list it); 11 amp -0.0.
    flavour "fast2": nothing that keeps the bank off the two-per-lane kernel -- role 1 is a finished voice by state, 2 / 3 sustain,
    8 is role 4.  "sparse": only lanes 0..7 of every 64-voice group can sound (packed lanes).  "mod": in-group modulators, from below
    (same-frame: the modulated kernel) and from above."""
    bank, tables, g = banks.bank_c2(n)
    now = int(g.synth_sample_count)
    rng = np.random.default_rng(1000 + n)
    role = rng.integers(0, 12, n)
    role[:min(n, 12)] = np.arange(min(n, 12))
    if n >= 24:
        role[n - 12:] = np.arange(12)
    v = np.arange(n)
    size = bank["voice_table_size"].astype(np.int64)
    e = bank["voice_amp_envelope"]
    last_frame_voice = -1
    if flavour == "fast2":
        bank["voice_finished"][role == 1] = 1
        role = np.where(role == 8, 4, role)
    else:
        shot = (role >= 1) & (role <= 3)
        bank["voice_one_shot"][shot], bank["voice_loop_enabled"][shot], bank["voice_direction"][shot] = 1, 0, 0
        bank["voice_phase_inc"][shot] = np.float32(1.0)
        r1, r2, r3 = role == 1, role == 2, role == 3
        bank["voice_phase"][r1] = np.maximum(size[r1] - 1 - (v[r1] % 50), 0).astype(np.float32)
        bank["voice_phase"][r2] = np.maximum(size[r2] - FRAMES[0] - 1 - (v[r2] % 100), 0).astype(np.float32)
        cand = np.flatnonzero(r2 & (size > FRAMES[0]))
        if len(cand):
            last_frame_voice = int(cand[0])
            bank["voice_phase"][last_frame_voice] = np.float32(size[last_frame_voice] - FRAMES[0])
        bank["voice_phase"][r3] = 0.0
        bank["voice_phase_inc"][r3] = np.float32(0.001)
    rel = (role == 4) | (role == 5) | (role == 8)
    e["sample_release"][rel] = np.uint64(now - 10)
    e["release_time"][rel] = (10 + 20 + (v[rel] % 150)).astype(np.float32)
    bank["voice_smoother_smoothing"][role == 4] = np.float32(0.5)
    bank["voice_smoother_smoothing"][role == 5] = np.float32(0.002)
    bank["voice_smoother_gain"][rel] = np.float32(0.7)
    e["sample_release"][role == 6] = np.uint64(now - 10)
    e["release_time"][role == 6] = np.float32(1e6)
    bank["voice_amp"][role == 7] = 0.0
    bank["voice_smoother_enable"][role == 8] = 0
    e["is_active"][role == 9] = 0
    bank["voice_use_amp_envelope"][role == 10] = 0
    e["is_active"][role == 10] = 0
    bank["voice_amp"][role == 11] = np.float32(-0.0)
    if flavour == "sparse":
        bank["voice_amp"][(v % 64) >= 8] = 0.0
    if flavour == "mod":
        below = (v % 16 == 5)
        bank["voice_amp_mod_osc"][below] = v[below] - 2
        bank["voice_amp_mod_depth"][below] = np.float32(0.5)
        above = (v % 16 == 9) & (v + 3 < n)
        bank["voice_freq_mod_osc"][above] = v[above] + 3
        bank["voice_freq_mod_depth"][above] = np.float32(0.1)
        own = (v % 32 == 7)
        bank["voice_pan_mod_osc"][own] = v[own]              # a voice that names itself
        bank["voice_pan_mod_depth"][own] = np.float32(0.3)
        bank["voice_freq_mod_osc"][v % 32 == 12] = v[v % 32 == 12]   # FM by itself: ignored, names nobody
        bank["voice_cz_mod_osc"][v % 32 == 20] = v[v % 32 == 20] - 1  # a CZ source with CZ off: names nobody
    return bank, tables, g, role, last_frame_voice


@functools.lru_cache(maxsize=32)
def scene(n, flavour="stops"):
    """The bank and the oracle's bank after FRAMES.  The oracle renders block 0 in two pieces (per-voice results do not depend on the
    block length) to show that the chosen one-shot finishes on the block's last frame and not before."""
    bank, tables, g, role, lfv = idle_bank(n, flavour)
    truth, gl = bank.copy(), g.copy()
    cpuref.render(truth, gl, tables, FRAMES[0] - 1, 0)
    pinned = flavour == "stops" and n >= 63                       # (elsewhere the voice may be silent or frequency-modulated)
    if pinned:
        assert lfv >= 0 and truth["voice_finished"][lfv] == 0
    cpuref.render(truth, gl, tables, 1, 0)
    if pinned:
        assert truth["voice_finished"][lfv] == 1, "the one-shot did not finish on the last frame of block 0"
    for f in FRAMES[1:]:
        cpuref.render(truth, gl, tables, f, 0)
    if n >= 63 and flavour != "sparse":
        g_ = np.abs(truth["voice_smoother_gain"])
        ended = (truth["voice_amp_envelope"]["is_active"] == 0) & (truth["voice_use_amp_envelope"] != 0) & (truth["voice_smoother_enable"] != 0)
        assert (ended & (g_ > SETTLE)).any() and (ended & (g_ <= SETTLE) & (g_ > 0)).any() and (ended & (g_ == 0)).any()
        assert ((role == 6) & (truth["voice_amp_envelope"]["is_active"] != 0)).any()          # still in release
        if flavour != "fast2":
            assert (truth["voice_finished"][role == 1] == 1).any() and (truth["voice_finished"][role == 3] == 0).any()
            assert (truth["voice_finished"][role == 2] == 1).any()                            # ... inside block 1
            assert ((truth["voice_smoother_enable"] == 0) & (truth["voice_amp_envelope"]["is_active"] == 0)).any()
    return bank, tables, g, truth


def open_bank(dev, bank, tables, g, setup=None):
    db = dev.DeviceBank(bank.n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    if setup is not None:
        setup(db)
    return db


def render_blocks(db, frames_list):
    import torch
    out = []
    for f in frames_list:
        o = torch.zeros(f, 2, device="cuda")
        db.render_mix(f, o.data_ptr(), 2, 0, 0)
        out.append(o)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def reach(dev, n, flavour="stops", setup=None):
    """(queried bank, oracle's bank, the twin's downloaded bank) after FRAMES."""
    bank, tables, g, truth = scene(n, flavour)
    db, twin = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    render_blocks(db, FRAMES)
    render_blocks(twin, FRAMES)
    got = bank.copy()
    twin.download(got)
    twin.close()
    return db, truth, got


def query(db, first, count, which, settle=0.0, start=None, max_out=None, stream=0, sync=True):
    """Returns (d_voices with 8 guard entries, d_count) as numpy, buffers pre-filled with -1."""
    import torch
    mo = count if max_out is None else max_out
    dv = torch.full((mo + 8,), -1, dtype=torch.int32, device="cuda")
    dc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    db.find_idle(first, count, which, settle, start, mo, dv.data_ptr(), dc.data_ptr(), stream)
    if sync:
        torch.cuda.synchronize()
    return dv.cpu().numpy(), dc.cpu().numpy(), mo


def check(db, truth, got, first, count, which, settle=0.0, start=None, max_out=None, vacuous_ok=False):
    want = expected(truth, first, count, which, settle, start, check=not vacuous_ok)
    twin_want = expected(got, first, count, which, settle, start)
    assert np.array_equal(want, twin_want), "the oracle's state and the twin's downloaded state disagree"
    dv, dc, mo = query(db, first, count, which, settle, start, max_out)
    total, written = len(want), min(len(want), mo)
    tag = f"[{first},+{count}) which 0x{which:x} settle {settle} start {start} max_out {mo}"
    print(f"{tag}: total {total}, written {written}")
    assert (int(dc[0]), int(dc[1])) == (written, total), f"{tag}: d_count {dc.tolist()}, expected ({written}, {total})"
    assert np.array_equal(dv[:written], want[:written]), f"{tag}: first mismatch at {int(np.flatnonzero(dv[:written] != want[:written])[0])}"
    assert (dv[written:] == -1).all(), f"{tag}: entries past `written` were touched"
    return want


# ---------------------------------------------------------------------------------------------- sizes, criteria, ranges, order

@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, SPAN - 1, SPAN, SPAN + 1, 1000, 70000])
def test_sizes_and_criteria(dev, n):
    """Each criterion alone and all three together over the whole bank, at the wave edge, the workgroup span +- 1, a ragged size and
    274 workgroups; ENV_DONE at level 0 (a smoothed voice stalled on a subnormal is NOT listed) and at SETTLE."""
    db, truth, got = reach(dev, n)
    try:
        assert db.last_kernel() == 1
        lists = {}
        for which, settle in ((FIN, 0.0), (ENV, 0.0), (ENV, SETTLE), (AMP, 0.0), (FIN | ENV | AMP, SETTLE)):
            lists[(which, float(settle))] = check(db, truth, got, 0, n, which, settle)
        assert len(lists[(ENV, 0.0)]) < len(lists[(ENV, float(SETTLE))])
        all3 = lists[(FIN | ENV | AMP, float(SETTLE))]
        if n > 300:
            mid = int(all3[len(all3) // 2])
            check(db, truth, got, 0, n, FIN | ENV | AMP, SETTLE, start=mid + 1)      # the ascending list rotated
            check(db, truth, got, 0, n, FIN | ENV | AMP, SETTLE, start=n - 1)        # ... from the last voice
            check(db, truth, got, 37, 300, FIN | ENV | AMP, SETTLE)                  # off every 64 boundary
            check(db, truth, got, 37, 300, FIN | ENV | AMP, SETTLE, start=37 + 299)
            check(db, truth, got, 37, 300, ENV, SETTLE, start=200)
    finally:
        db.close()


@pytest.mark.gpu
def test_one_voice_banks(dev):
    """n = 1: one bank whose voice is idle (amp 0), one whose voice sounds -- `written == total == 1` and `== 0`."""
    for amp, total in ((0.0, 1), (1.0, 0)):
        bank, tables, g = banks.bank_c2(1)
        bank["voice_amp"][0] = amp
        db = open_bank(dev, bank, tables, g)
        try:
            render_blocks(db, (65,))
            truth = bank.copy()
            cpuref.render(truth, g.copy(), tables, 65, 0)
            got = bank.copy()
            db.download(got)
            want = check(db, truth, got, 0, 1, FIN | ENV | AMP, 0.0, vacuous_ok=True)
            assert len(want) == total
        finally:
            db.close()


@pytest.mark.gpu
def test_max_out_and_empty_and_full_ranges(dev):
    n = 1000
    db, truth, got = reach(dev, n)
    try:
        which = FIN | ENV | AMP
        total = len(expected(truth, 0, n, which, SETTLE))
        assert total > 8
        for mo in (0, 1, total - 1, total, total + 5):
            check(db, truth, got, 0, n, which, SETTLE, max_out=mo)
            check(db, truth, got, 0, n, which, SETTLE, start=n // 2, max_out=mo)
        # a range with no idle voice, and one where every voice is idle: runs of the all-criteria list and of its complement
        idle = np.zeros(n, bool)
        idle[expected(truth, 0, n, which, SETTLE)] = True
        edges = np.flatnonzero(np.diff(idle.astype(np.int8)) != 0) + 1
        runs = list(zip(np.r_[0, edges], np.r_[edges, n]))
        busy = max((r for r in runs if not idle[r[0]]), key=lambda r: r[1] - r[0])
        free = max((r for r in runs if idle[r[0]]), key=lambda r: r[1] - r[0])
        assert busy[1] - busy[0] >= 2 and free[1] - free[0] >= 2
        w = check(db, truth, got, int(busy[0]), int(busy[1] - busy[0]), which, SETTLE, vacuous_ok=True)
        assert len(w) == 0
        w = check(db, truth, got, int(free[0]), int(free[1] - free[0]), which, SETTLE, start=int(free[1]) - 1, vacuous_ok=True)
        assert len(w) == free[1] - free[0]
        # the host variant: waits for the stream only
        voices, tot = db.find_idle_host(0, n, which, float(SETTLE), n // 2, 16)
        want = expected(truth, 0, n, which, SETTLE, n // 2)
        assert tot == len(want) and np.array_equal(voices, want[:16])
        voices, tot = db.find_idle_host(0, n, which, float(SETTLE), max_out=0)
        assert tot == len(want) and len(voices) == 0
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- every kernel family that writes the state

FAMILIES = {
    "generic": ("stops", lambda db: db.force_generic(True), 0, False),
    "one_voice_stops": ("stops", None, 1, False),
    "fast2_beside": ("fast2", lambda db: (db.fast2_min_voices(0), db.in_place(0)), 3, False),
    "fast2_in_place": ("fast2", lambda db: (db.fast2_min_voices(0), db.in_place(2)), 3, False),
    "packed": ("sparse", lambda db: db.set_pack(2), 1, True),
    "modulated": ("mod", None, 2, False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_kernel_families(dev, family):
    flavour, setup, kernel, packed = FAMILIES[family]
    n = 4096
    db, truth, got = reach(dev, n, flavour, setup)
    try:
        assert db.last_kernel() == kernel, (family, db.last_kernel())
        assert (db.last_pack() > 0) == packed, (family, db.last_pack())
        assert db.list_violations() == 0
        for which, settle in ((FIN, 0.0), (ENV, SETTLE), (AMP, 0.0), (FIN | ENV | AMP, SETTLE)):
            check(db, truth, got, 0, n, which, settle, vacuous_ok=(flavour == "sparse" and which == ENV))
        check(db, truth, got, 37, 300, FIN | ENV | AMP, SETTLE, start=190, max_out=40)
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- fuzz_banks.py's generator

@pytest.mark.gpu
@pytest.mark.parametrize("routing,seed,n", [("own_group", 5001, 1000), ("cross_group", 5102, 4096)])
def test_fuzz_banks(dev, routing, seed, n):
    """wild_bank (every feature, modulators inside the group or across groups) over its own block lengths, on the modulated kernel."""
    import fuzz_banks
    import golden_io as gio
    gold = gio.load("c4_pcm_oneshot")
    tables, cat = gold.tables, fuzz_banks.catalogue(gold.segments[0].bank_in)
    rng = np.random.default_rng(seed)
    bank, _ = fuzz_banks.wild_bank(rng, n, cat, routing)
    g = gold.segments[0].g_in.copy()
    g.synth_sample_count = fuzz_banks.COUNT0
    frames = fuzz_banks.block_lengths(rng)
    setup = (lambda db: db.set_cross_group(True)) if routing == "cross_group" else None
    db, twin = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    try:
        render_blocks(db, frames)
        render_blocks(twin, frames)
        assert db.last_kernel() == 2
        truth, gl = bank.copy(), g.copy()
        for f in frames:
            cpuref.render(truth, gl, tables, f, 0)
        got = bank.copy()
        twin.download(got)
        for which in (FIN, ENV, AMP, FIN | ENV | AMP, FIN | ENV | AMP | UNNAMED):
            check(db, truth, got, 0, n, which, SETTLE)
        check(db, truth, got, 37, 300, FIN | ENV | AMP | UNNAMED, SETTLE, start=250, max_out=17)
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- UNNAMED

def routed_run(dev, bank, tables, g, setup, steps):
    """steps: callables(truth, mirror, db, twin) that change routing ahead of a block; after every block the UNNAMED query is checked
    against the oracle's bank and the twin's download."""
    truth, gl, mirror = bank.copy(), g.copy(), bank.copy()
    db, twin = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    lists = []
    try:
        for step in steps:
            if step is not None:
                step(truth, mirror, db, twin)
            render_blocks(db, (65,))
            render_blocks(twin, (65,))
            cpuref.render(truth, gl, tables, 65, 0)
            got = mirror.copy()
            twin.download(got)
            lists.append(check(db, truth, got, 0, bank.n, AMP | FIN | UNNAMED))
            check(db, truth, got, 37, 300, AMP | ENV | UNNAMED, SETTLE, start=100, vacuous_ok=True)
        return lists, db.last_kernel(), db.last_cross_group()
    finally:
        db.close()
        twin.close()


def set_route(field, depth, dst, src):
    def step(truth, mirror, db, twin):
        for h in (truth, mirror):
            h[field][dst] = src
            h[depth][dst] = np.float32(0.25)
        for d in (db, twin):
            d.update(mirror, dst, DIRTY_PARAMS)
    return step


@pytest.mark.gpu
def test_unnamed_in_group_and_updates(dev):
    """In-group modulators; a routing added and one removed by skred_bank_update(DIRTY_PARAMS) between two queries."""
    n = 1000
    bank, tables, g, role, _ = idle_bank(n, "mod")
    silent = np.flatnonzero(bank["voice_amp"] == 0)
    named0 = named_set(bank)
    newly = int(silent[~named0[silent]][0])                       # a silent voice nobody names: about to be named
    reader = (newly & ~63) + ((newly + 9) & 63)
    held = int(silent[named0[silent] & (silent % 16 == 3)][0])    # a silent voice named through amp_mod_osc only: about to be set free
    readers = np.flatnonzero(bank["voice_amp_mod_osc"] == held)
    assert len(readers) and not (bank["voice_pan_mod_osc"] == held).any() and not (bank["voice_freq_mod_osc"] == held).any()
    steps = [None,
             set_route("voice_pan_mod_osc", "voice_pan_mod_depth", np.array([reader], np.int32), newly),
             set_route("voice_amp_mod_osc", "voice_amp_mod_depth", readers.astype(np.int32), -1)]
    lists, kernel, _ = routed_run(dev, bank, tables, g, None, steps)
    assert kernel == 2
    assert newly in lists[0] and newly not in lists[1]
    assert held not in lists[1] and held in lists[2]
    own = np.flatnonzero(bank["voice_pan_mod_osc"] == np.arange(n))
    assert len(own) and not set(own) & set(lists[0])              # a voice that names itself is named


@pytest.mark.gpu
@pytest.mark.parametrize("cross", [1, 0])
def test_unnamed_cross_group(dev, cross):
    """A modulator in another 64-voice group, with SKRED_OPT_CROSS_GROUP on (rendered through the tape) and off (the bank refuses to
    render; the query still answers from the planes as they were uploaded)."""
    n = 1000
    bank, tables, g, role, _ = idle_bank(n, "mod")
    silent = np.flatnonzero((bank["voice_amp"] == 0) & ~named_set(bank))
    far = int(silent[silent < 64][0])
    bank["voice_amp_mod_osc"][700] = far
    bank["voice_amp_mod_depth"][700] = np.float32(0.4)
    bank["voice_pan_mod_osc"][701] = n + 5                        # outside the bank: names nobody (and with `cross` the bank is refused)
    if cross:
        bank["voice_pan_mod_osc"][701] = -1
        lists, kernel, cg = routed_run(dev, bank, tables, g, lambda db: db.set_cross_group(True), [None])
        assert kernel == 2 and cg[0] >= 1
        assert far not in lists[0]
    else:
        db = open_bank(dev, bank, tables, g)
        try:
            with pytest.raises(dev.SkredAmdError):
                render_blocks(db, (65,))
            check(db, bank, bank, 0, n, AMP | UNNAMED)
            assert far not in expected(bank, 0, n, AMP | UNNAMED) and far in expected(bank, 0, n, AMP)
        finally:
            db.close()


@pytest.mark.gpu
def test_unnamed_follows_a_pattern_step(dev):
    """A pattern step that changes routing: the named set is rebuilt by the query after the block whose run_queue fired it."""
    n = 1000
    bank, tables, g, role, _ = idle_bank(n, "mod")
    silent = np.flatnonzero((bank["voice_amp"] == 0) & ~named_set(bank))
    target = int(silent[0])
    reader = (target & ~63) + ((target + 5) & 63)
    truth, gl, mirror = bank.copy(), g.copy(), bank.copy()
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    try:
        mirror["voice_amp_mod_osc"][reader] = target
        mirror["voice_amp_mod_depth"][reader] = np.float32(0.3)
        for d in (db, twin):
            d.pattern_step_set(0, 0, mirror, [reader], DIRTY_PARAMS)
            s = d.seq()
            s.tempo(60.0 * 44100 / (4 * 60))                      # a step every 60 frames: the first 64-frame block fires it
            s.modulo(0, 1)
            s.state(0, 1)
        render_blocks(db, (64,)); render_blocks(twin, (64,))
        cpuref.render(truth, gl, tables, 64, 0)
        got = bank.copy()
        twin.download(got)
        assert target in check(db, truth, got, 0, n, AMP | FIN | UNNAMED)
        fired = [d.run_queue(64) for d in (db, twin)]
        assert fired == [1, 1], fired
        truth["voice_amp_mod_osc"][reader] = target               # what the step stores
        truth["voice_amp_mod_depth"][reader] = np.float32(0.3)
        render_blocks(db, (64,)); render_blocks(twin, (64,))
        cpuref.render(truth, gl, tables, 64, 0)
        got = mirror.copy()
        twin.download(got)
        assert target not in check(db, truth, got, 0, n, AMP | FIN | UNNAMED)
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- stream order, read-only, determinism

def traffic_bank(n):
    """bank_c2 with short attacks, decays and releases and fast smoothers; every eighth voice sounds (in sustain), the others are free
    from the start."""
    bank, tables, g = banks.bank_c2(n)
    e = bank["voice_amp_envelope"]
    e["attack_time"], e["decay_time"] = np.float32(20.0), np.float32(50.0)   # (a release only counts once attack and decay are over: synth.c:398-431)
    e["release_time"] = np.float32(200.0)
    e["sample_start"] = np.uint64(int(g.synth_sample_count) - 40000)         # every sounding voice is in its sustain stage
    bank["voice_smoother_smoothing"] = np.float32(0.5)
    free = np.arange(n) % 8 != 0
    e["is_active"][free] = 0
    return bank, tables, g


def do_release(truth, vs, now):
    e = truth["voice_amp_envelope"]
    act = e["is_active"][vs] != 0
    e["sample_release"][vs[act]] = now


def do_trigger(hosts, truth, vs, now):
    for h in hosts:
        h["voice_phase"][vs] = 0.0
        h["voice_finished"][vs] = 0
    e = truth["voice_amp_envelope"]
    e["sample_start"][vs] = now
    e["sample_release"][vs] = 0
    e["is_active"][vs] = 1


@pytest.mark.gpu
def test_stream_order_without_host_synchronisation(dev):
    """Releases stamped, a block long enough for them to end, the query -- all on one stream, nothing waited for in between."""
    import torch
    n, F = 1000, 512
    bank, tables, g = traffic_bank(n)
    db = open_bank(dev, bank, tables, g)
    try:
        s = torch.cuda.Stream()
        out = torch.zeros(F, 2, device="cuda")
        dv = torch.full((n + 8,), -1, dtype=torch.int32, device="cuda")
        dc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        released = np.arange(0, n, 16, dtype=np.int32)
        truth, gl = bank.copy(), g.copy()
        before = expected(truth, 0, n, ENV, SETTLE, check=True)
        assert not set(released) & set(before)
        torch.cuda.synchronize()
        db.update(bank, released, STAMP_RELEASE, s.cuda_stream)
        db.render_mix(F, out.data_ptr(), 2, 0, 0, s.cuda_stream)
        db.find_idle(0, n, ENV, float(SETTLE), None, n, dv.data_ptr(), dc.data_ptr(), s.cuda_stream)
        s.synchronize()
        do_release(truth, released, gl.synth_sample_count)
        cpuref.render(truth, gl, tables, F, 0)
        want = expected(truth, 0, n, ENV, SETTLE, check=True)
        assert set(released) <= set(want)
        got, cnt = dv.cpu().numpy(), dc.cpu().numpy()
        assert cnt.tolist() == [len(want), len(want)]
        assert np.array_equal(got[:len(want)], want) and (got[len(want):] == -1).all()
    finally:
        db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["one_voice", "fast2"])
def test_query_reads_the_bank_only(dev, family):
    """A bank queried after every block (all criteria, UNNAMED, a sub-range) against an unqueried twin under note traffic: state,
    globals and mix bit for bit, last_kernel, last_pack and list_violations."""
    import torch
    n, F = 4096, 256
    bank, tables, g = traffic_bank(n)
    setup = (lambda db: db.fast2_min_voices(0)) if family == "fast2" else None
    db, twin = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    mirror = bank.copy()
    rng = np.random.default_rng(5)
    try:
        for k in range(6):
            vs = np.sort(rng.choice(n, 24, replace=False)).astype(np.int32)
            mirror["voice_phase"][vs[12:]] = 0.0
            for d in (db, twin):
                d.update(mirror, vs[:12], STAMP_RELEASE)
                d.update(mirror, vs[12:], DIRTY_PARAMS | DIRTY_PHASE | STAMP_TRIGGER)
            mixes = [render_blocks(d, (F,))[0] for d in (db, twin)]
            assert (mixes[0].view(np.uint32) == mixes[1].view(np.uint32)).all(), f"block {k}: the query changed the mix"
            assert db.last_kernel() == twin.last_kernel() == (3 if family == "fast2" else 1)
            assert db.last_pack() == twin.last_pack() and db.list_violations() == twin.list_violations() == 0
            dv, dc, _ = query(db, 0, n, FIN | ENV | AMP | UNNAMED, SETTLE, start=n // 3)
            assert dc[1] > 0
            query(db, 37, 300, ENV, 0.0, max_out=0)
        a, b = bank.copy(), bank.copy()
        db.download(a)
        twin.download(b)
        assert not a.rw_equal(b), a.rw_equal(b)
        ga, gb = db.get_globals(), twin.get_globals()
        assert ga.synth_sample_count == gb.synth_sample_count and ga.noise_rng == gb.noise_rng
        assert np.float32(ga.volume_smoother_gain).tobytes() == np.float32(gb.volume_smoother_gain).tobytes()
    finally:
        db.close()
        twin.close()


@pytest.mark.gpu
def test_same_query_twice_same_bytes(dev):
    n = 70000
    db, truth, got = reach(dev, n)
    try:
        runs = [query(db, 11, n - 30, FIN | ENV | AMP | UNNAMED, SETTLE, start=40000) for _ in range(2)]
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
        assert runs[0][1][1] > SPAN
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- an allocator

@pytest.mark.gpu
def test_allocator_loop(dev):
    """Eight blocks on 4096 voices: query from the voice after the last pick, trigger the first 16 listed voices, release the ones
    triggered two blocks ago, render.  At every step the list equals the oracle's; a voice just triggered is not listed in the next
    query; no voice is handed out while it sounds."""
    n, F, K = 4096, 512, 16
    which = FIN | ENV
    bank, tables, g = traffic_bank(n)
    bank["voice_finished"][5::64] = 1                            # some free voices are free as finished voices too (a trigger clears it)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    truth, gl, mirror = bank.copy(), g.copy(), bank.copy()
    history, last, handed = [], n - 1, 0
    try:
        for k in range(8):
            got = mirror.copy()
            twin.download(got)
            start = (last + 1) % n
            want = check(db, truth, got, 0, n, which, SETTLE, start=start, max_out=K)
            picks = want[:K].copy()
            assert len(picks) == K
            sounding = set(np.flatnonzero(~np.isin(np.arange(n), expected(truth, 0, n, which, SETTLE))))
            assert not set(picks) & sounding, f"block {k}: a sounding voice was handed out"
            if history:
                assert not set(history[-1]) & set(want), f"block {k}: a voice triggered in the last block is listed"
            now = gl.synth_sample_count
            do_trigger((truth, mirror), truth, picks, now)
            older = history[-2] if len(history) >= 2 else np.zeros(0, np.int32)
            do_release(truth, older, now)
            for d in (db, twin):
                d.update(mirror, picks, DIRTY_PARAMS | DIRTY_PHASE | STAMP_TRIGGER)
                if len(older):
                    d.update(mirror, older, STAMP_RELEASE)
            history.append(picks)
            last, handed = int(picks[-1]), handed + K
            render_blocks(db, (F,))
            render_blocks(twin, (F,))
            cpuref.render(truth, gl, tables, F, 0)
        assert handed == 8 * K and len({int(v) for h in history[:3] for v in h}) == 3 * K
        final = expected(truth, 0, n, which, SETTLE)
        assert set(history[0]) <= set(final), "voices released four blocks ago are free again"
    finally:
        db.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_leave_the_bank_usable(dev):
    import ctypes as C
    import torch
    n = 1000
    bank, tables, g, truth = scene(n)
    db, twin = open_bank(dev, bank, tables, g), open_bank(dev, bank, tables, g)
    try:
        L = db.L
        dv = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        dc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        host = np.full(64, -1, np.int32)
        tot = C.c_int(-7)

        def rc(first=0, count=n, which=FIN, settle=0.0, start=0, max_out=8, voices=dv.data_ptr(), counts=dc.data_ptr(), bank_h=db.h, q=True):
            qq = dev.IdleQueryC(first, count, which, settle, start, max_out)
            return L.skred_bank_find_idle(bank_h, C.byref(qq) if q else None, voices or None, counts or None, None)

        BAD, RANGE = -2, -4
        assert rc(bank_h=None) == BAD and rc(q=False) == BAD
        assert rc(voices=0) == BAD and rc(counts=0) == BAD
        assert rc(voices=0, max_out=0) == 0                        # count only: no list needed
        assert rc(which=0) == BAD and rc(which=UNNAMED) == BAD     # no criterion
        assert rc(which=FIN | 8) == BAD and rc(which=FIN | (1 << 31)) == BAD
        assert rc(max_out=-1) == BAD
        for s in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert rc(which=ENV, settle=s) == BAD
        assert rc(which=ENV, settle=-0.0) == 0
        assert rc(count=0) == RANGE and rc(count=-3) == RANGE
        assert rc(first=-1) == RANGE and rc(first=n) == RANGE and rc(first=1, count=n) == RANGE
        assert rc(first=0, count=2**31 - 1) == RANGE and rc(first=2**31 - 1, count=2**31 - 1) == RANGE
        assert rc(first=10, count=20, start=9) == RANGE and rc(first=10, count=20, start=30) == RANGE
        assert rc(first=10, count=20, start=29) == 0
        qq = dev.IdleQueryC(0, n, FIN, 0.0, 0, 8)
        assert L.skred_bank_find_idle_host(db.h, C.byref(qq), None, C.byref(tot), None) == BAD
        assert L.skred_bank_find_idle_host(db.h, C.byref(qq), host.ctypes.data, None, None) >= 0      # total_out may be NULL
        qq.count = n + 1
        assert L.skred_bank_find_idle_host(db.h, C.byref(qq), host.ctypes.data, C.byref(tot), None) == RANGE
        assert tot.value == -7
        torch.cuda.synchronize()
        # the bank still renders, like its twin, and answers
        mixes = [render_blocks(d, FRAMES) for d in (db, twin)]
        for x, y in zip(*mixes):
            assert (x.view(np.uint32) == y.view(np.uint32)).all()
        got = bank.copy()
        twin.download(got)
        check(db, truth, got, 0, n, FIN | ENV | AMP, SETTLE)
    finally:
        db.close()
        twin.close()
