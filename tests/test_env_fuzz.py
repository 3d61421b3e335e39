"""Fuzz of MOVING envelopes on the two-per-lane family against the oracle (DESIGN "The motion list"): random clean banks whose
envelope regime is drawn per 64-voice group, control actions between blocks, block lengths that change from block to block
(tests/env_fuzz.py), and a numpy restatement of which form of sk_render_env2_kernel every wave and 64-frame chunk takes, how the
motion list evolves and when a block is rendered in place (tests/env_forms.py).

On the CPU: every case is a clean bank, the oracle renders it without a non-finite value, the predictor's is_active flags agree
with the oracle's after every block, and the default seeds together reach every form, every kind of 8-frame block, every trigger
of the frame-by-frame form and the list machinery's corners -- so that a quiet draw cannot hide a failure.  On the GPU: every
seed through four call forms (two-per-lane with the envelope kernel beside the steady one; two-per-lane in place; the one-voice
kernel; the generic kernel), per-voice state bit-equal to the oracle's at two random blocks and at the end, every block's mix
within 1e-5 relative RMS, no list violation, and last_in_place() as predicted block by block.  No number here is measured from
the code under test.
"""
import functools
import os

import numpy as np
import pytest

import env_forms
import env_fuzz
from oracle import cpuref

SEEDS = list(range(max(len(env_fuzz.SEEDS), int(os.environ.get("SKRED_FUZZ_SEEDS", "0")))))
DEFAULT = list(env_fuzz.SEEDS)
QUEUED_SEED = 4                     # blocks 0, 1, 2 are queued before the first synchronisation (and three more later in the run)
FORMS = ("env_beside", "in_place", "one_voice", "generic")


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


def without_guards(case):
    """The case's pool with the sample behind every table changed: no voice carries SKF_GUARD, the linear lookup keeps its fold
    test (tests/test_in_place.py: _c2_without_guards)."""
    t = case.tables.copy()
    b = case.bank
    pos = np.unique(b["voice_table_offset"].astype(np.int64) + b["voice_table_size"].astype(np.int64))
    t[pos[pos < len(t)]] = 7.0
    return t


class Truth:
    """The oracle's run of a case: pre[k] / post[k] the bank when block k starts (actions applied) / ends, refs[k] its mix."""

    def __init__(self, case, tables):
        truth, gl = case.bank.copy(), case.g.copy()
        self.pre, self.post, self.refs, self.finite = [], [], [], True
        for frames, actions in case.blocks:
            for a in actions:
                a.apply(truth, gl.synth_sample_count)
            self.pre.append(truth.copy())
            r = cpuref.render(truth, gl, tables, frames, case.interp)
            self.finite = self.finite and bool(np.isfinite(r["sum64"]).all())
            self.refs.append(cpuref.master(gl, r["sum64"].astype(np.float32)))
            self.post.append(truth.copy())
        for k in ("voice_phase", "voice_sample", "voice_smoother_gain"):
            self.finite = self.finite and bool(np.isfinite(truth[k]).all())
        self.final = truth


@functools.lru_cache(maxsize=None)
def get_case(seed):
    return env_fuzz.pinned(seed) if isinstance(seed, str) else env_fuzz.case(seed)


@functools.lru_cache(maxsize=None)
def get_truth(seed, guards=True):
    case = get_case(seed)
    return Truth(case, case.tables if guards else without_guards(case))


@functools.lru_cache(maxsize=None)
def get_walk(seed, mode, queued=(), observed=()):
    t = get_truth(seed)
    return env_forms.walk(get_case(seed), t.pre, t.post, mode, queued, dict(observed))


def queue_start(seed):
    """The first block k >= 4 such that k, k + 1, k + 2 can be issued without a synchronisation in between and the predictor's
    answer does not depend on when their reports arrive (an extra: the stretch whose answer DOES depend on it is blocks 0 .. 2)."""
    case = get_case(seed)
    for k in range(4, len(case.blocks) - 2):
        try:
            get_walk(seed, 2, (k + 1, k + 2))
            return k
        except env_forms.LateReport:
            continue
    raise AssertionError("no stretch of three blocks can be queued unambiguously")


# ---------------------------------------------------------------- CPU: the cases and the predictor

@pytest.mark.parametrize("seed", DEFAULT)
def test_bank_is_clean(seed):
    """VoiceBank fields only: nothing that would move the bank off the two-per-lane family; 1 000 to 6 000 voices, at most 12
    blocks and 2 500 frames."""
    c = get_case(seed)
    b = c.bank
    assert 1000 <= c.n <= env_fuzz.MAX_VOICES and len(c.blocks) <= env_fuzz.MAX_BLOCKS and c.frames <= env_fuzz.MAX_FRAMES
    assert all(x != y for (x, _), (y, _) in zip(c.blocks, c.blocks[1:]))          # the length changes from block to block
    assert not ((b["voice_one_shot"] != 0) & (b["voice_loop_enabled"] == 0)).any()      # no stopping one-shot
    for k in ("voice_direction", "voice_sample_hold_max", "voice_quantize", "voice_cz_mode", "voice_finished"):
        assert not b[k].any(), k
    assert (b["voice_smoother_enable"] == 1).all() and (b["voice_wave_table_index"] != 6).all()
    assert b.modulation_free()
    assert (b["voice_table_size"] > 0).all() and b["voice_use_amp_envelope"].any()
    assert np.isfinite(b["voice_phase"]).all() and np.isfinite(b["voice_phase_inc"]).all()
    for frames, actions in c.blocks:                        # ... and no action changes that
        for a in actions:
            assert a.kind in ("note_off", "retrigger", "ahead_chunk", "ahead_edge", "ahead_far", "amp", "mute", "unmute", "burst_beyond")


def test_sizes_cover_the_shapes():
    ns = [get_case(s).n for s in DEFAULT]
    assert any(n < 1024 for n in ns) and any(n % 128 == 1 for n in ns) and any(n % 1024 == 0 for n in ns) and any(n % 64 for n in ns)
    assert {get_case(s).recipe for s in DEFAULT} == {"c2", "c4"}
    assert {get_case(s).info["filter"] for s in DEFAULT} >= {"all", "mixed"} and "mixed" in {get_case(s).info["envelope"] for s in DEFAULT}


@pytest.mark.parametrize("seed", DEFAULT + list(env_fuzz.PINNED))
def test_oracle_renders_and_predictor_agrees_with_it(seed):
    """No non-finite value in the oracle's run; and the predictor, walking the ladder from the oracle's bank at every block start,
    leaves the same is_active flags on the listed voices as the oracle's envelope does -- for both ways of rendering the list."""
    t = get_truth(seed)
    assert t.finite
    for mode in (0, 2):
        for k, rec in enumerate(get_walk(seed, mode)):
            sel = rec["listed"] & (t.pre[k]["voice_use_amp_envelope"] != 0) & (t.pre[k]["voice_amp"] != 0)
            want = t.post[k]["voice_amp_envelope"]["is_active"][sel] != 0
            assert np.array_equal(rec["active_end"][sel], want), (seed, mode, k)


def _tally(seeds):
    rows = {}
    for s in seeds:
        c = get_case(s)
        row = {f"form{f}": 0 for f in range(1, 6)}
        row.update({k: 0 for k in env_forms.KINDS + env_forms.TRIGGERS})
        row.update(const_after_motion=0, cleared=0, sole_clock=0, sole_ragged=0, sole_untame=0)
        for rec in get_walk(s, 0):
            row["cleared"] += len(rec["cleared"])
            for r in rec["records"]:
                row[f"form{r['form']}"] += 1
                for kd in set(r["kinds"]):
                    row[kd] += 1
                for tg in r["triggers"]:
                    row[tg] += 1
                if len(r["triggers"]) == 1:
                    row["sole_" + r["triggers"][0]] += 1
                row["const_after_motion"] += r["form"] == 1 and r["moved_before"]
        rows[s] = (c.recipe, row)
    return rows


def test_coverage_of_forms_over_the_default_seeds(capsys):
    """Every form 1..5, every kind of 8-frame block inside form 4 and every trigger of form 5 (alone in its wave-chunk) is predicted
    on both table kinds and in at least 3 seeds; at most 40 % of all wave-chunks are constant."""
    rows = _tally(DEFAULT)
    keys = [f"form{f}" for f in range(1, 6)] + list(env_forms.KINDS) + ["sole_" + t for t in env_forms.TRIGGERS]
    with capsys.disabled():
        print("\nseed recipe " + " ".join(f"{k:>11}" for k in keys + ["const_after", "cleared"]))
        for s, (recipe, row) in rows.items():
            print(f"{s:>4} {recipe:>6} " + " ".join(f"{row[k]:>11}" for k in keys + ["const_after_motion", "cleared"]))
    for k in keys:
        hit = [s for s, (_, row) in rows.items() if row[k] > 0]
        assert len(hit) >= 3, (k, hit)
        assert {rows[s][0] for s in hit} == {"c2", "c4"}, (k, hit)
    total = sum(row[f"form{f}"] for _, row in rows.values() for f in range(1, 6))
    const = sum(row["form1"] for _, row in rows.values())
    assert const <= 0.40 * total, (const, total)
    assert sum(row["const_after_motion"] for _, row in rows.values()) > 0       # constant, reached by a wave that moved earlier in the launch
    assert sum(row["cleared"] for _, row in rows.values()) > 0                  # a release that ends inside a block


def test_coverage_of_the_list_machinery():
    """In place: a word above 8 listed voices, a wave above 32, a block whose proven bound exceeds the limit (after blocks that
    were taken in place), and blocks that are taken."""
    over_word = over_wave = beyond = taken = 0
    for s in DEFAULT:
        c = get_case(s)
        recs = get_walk(s, 2)
        for k, rec in enumerate(recs):
            ip = rec["in_place"] == {True}
            taken += ip
            over_word += ip and len(rec["words_over"]) > 0
            over_wave += ip and len(rec["waves_over"]) > 0
            beyond += c.lds_tables and rec["bound"] is not None and rec["bound"] > env_forms.in_place_limit(c.n) and not ip
        if not c.lds_tables:
            assert not any(rec["in_place"] == {True} for rec in recs)          # table windows: never in place
    assert over_word > 0 and over_wave > 0 and beyond > 0 and taken >= 8, (over_word, over_wave, beyond, taken)


@pytest.mark.parametrize("seed", DEFAULT)
def test_no_quiet_draw(seed):
    """At least 30 % of the voices can sound, and at least 5 % are on the list in at least half the blocks."""
    c, t = get_case(seed), get_truth(seed)
    heard = np.zeros(c.n, bool)
    for b in t.post:
        heard |= (b["voice_smoother_gain"] != 0) & (b["voice_disconnect"] == 0) & (b["voice_amp"] != 0)
    assert heard.mean() >= 0.30, heard.mean()
    on = np.sum([rec["listed"] for rec in get_walk(seed, 0)], axis=0)
    assert (on >= len(c.blocks) / 2).mean() >= 0.05, (on >= len(c.blocks) / 2).mean()


# the forms of the chunks of block 0.  (An edge on frame 0 of a chunk is no change INSIDE a chunk: the chunks before and after it are
# ramps; attack -> sustain skips a stage: no step form but the re-decision, then constant; the 2^41 decay refuses ramp and step.)
PINNED_FORMS = {"edge_on_frame_0": [2, 2, 2], "edge_on_frame_8": [2, 3, 2], "edge_on_frame_64": [2, 2, 2], "no_decay": [4, 1],
                "clock_crosses_mid_block": [2, 2, 5, 5], "stage_times_2_41": [4, 4], "block_of_65": [4, 1]}


@pytest.mark.parametrize("name", list(env_fuzz.PINNED))
def test_pinned_edges_are_what_they_claim(name):
    """The deterministic cases reach the code they are named for, by the predictor."""
    c = get_case(name)
    assert c.n <= 2048 and len(c.blocks) <= 6
    if name in PINNED_FORMS:
        forms = [r["form"] for r in get_walk(name, 0)[0]["records"]]
        assert forms == PINNED_FORMS[name], forms
    if name == "note_on_frame_63":                            # ahead of the clock in block 1: integer clocks; the attack runs in block 2
        w = get_walk(name, 0)
        assert [r["form"] for r in w[1]["records"]] == [5] and w[1]["records"][0]["triggers"] == ["clock"]
        assert w[2]["records"][0]["form"] in (2, 3)
    if name == "clock_crosses_mid_block":
        recs = get_walk(name, 0)[0]["records"]
        assert recs[2]["triggers"] == ["clock"]                 # (the test is made per chunk, 66 frames early)
    if name == "release_ends_on_block_edge":
        w = get_walk(name, 0)
        assert len(w[0]["cleared"]) == 64 and len(w[1]["cleared"]) == 64
    if name == "wave_of_33":
        assert any(rec["in_place"] == {True} and len(rec["waves_over"]) for rec in get_walk(name, 2))
    if name == "word_of_9":
        assert any(rec["in_place"] == {True} and len(rec["words_over"]) and not len(rec["waves_over"]) for rec in get_walk(name, 2))


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def dev():
    from skred_amd import device
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def run_device(dev, case, form, tables, queued=(), checks=()):
    """The case's block list through one call form, blocks issued asynchronously (a synchronisation after every block but those in
    `queued`).  Returns (mixes, kernels, taken, states {block: downloaded bank}, list violations)."""
    import torch
    db = dev.DeviceBank(case.n)
    db.set_tables(tables)
    db.upload(case.bank)
    db.set_globals(case.g)
    if form in ("env_beside", "in_place"):
        db.fast2_min_voices(0)
        db.in_place(2 if form == "in_place" else 0)
    elif form == "one_voice":
        db.fast2_min_voices(1 << 30)
    else:
        db.force_generic(True)
    mirror = case.bank.copy()
    now = int(case.g.synth_sample_count)
    outs, kernels, taken, states = [], [], [], {}
    for k, (frames, actions) in enumerate(case.blocks):
        for a in actions:
            vs, dirty = a.apply(mirror, now)
            db.update(mirror, vs, dirty, 0)
        out = torch.zeros(frames, 2, device="cuda")
        db.render_mix(frames, out.data_ptr(), 2, 0, case.interp)
        kernels.append(db.last_kernel())
        taken.append(db.last_in_place())
        outs.append(out)
        now += frames
        if (k + 1) not in queued:
            torch.cuda.synchronize()
        if k in checks or k == len(case.blocks) - 1:
            got = case.bank.copy()
            db.download(got)
            states[k] = got
    torch.cuda.synchronize()
    mixes = [o.cpu().numpy().copy() for o in outs]
    viol = db.list_violations()
    db.close()
    return mixes, kernels, taken, states, viol


def check_run(dev, seed, form, guards=True):
    case, truth = get_case(seed), get_truth(seed, guards)
    tables = case.tables if guards else without_guards(case)
    nb = len(case.blocks)
    queued = ()
    if seed == QUEUED_SEED and form in ("env_beside", "in_place"):
        # blocks 0, 1, 2 before the first synchronisation: no report yet after the rebuild, reports arriving inside the queue --
        # whether blocks 1 and 2 are taken in place depends on that; and a later stretch where it does not
        q = queue_start(seed)
        queued = (1, 2, q + 1, q + 2)
    rng = np.random.default_rng(seed if isinstance(seed, int) else 0)
    allowed = [k for k in range(nb - 1) if k + 1 not in queued]          # (a download waits for the device: not inside a queue)
    checks = [int(k) for k in rng.choice(allowed, min(2, len(allowed)), replace=False)]      # (a two-block pinned case has one earlier block)
    mixes, kernels, taken, states, viol = run_device(dev, case, form, tables, queued, checks)
    want_kernel = {"env_beside": 3, "in_place": 3, "one_voice": 1, "generic": 0}[form]
    assert kernels == [want_kernel] * nb, kernels
    if form == "in_place":
        # where a queued block has two possible answers, either is accepted and the walk follows the one observed; everything
        # else about that block -- state, mix, violations -- is asserted as for every other
        recs = get_walk(seed, 2, queued, tuple((k, bool(taken[k])) for k in queued))
        want = [rec["in_place"] for rec in recs]
        assert all(t in w for t, w in zip(taken, want)), (taken, want)
        if queued:
            print(f"seed {seed}: in place {taken}, predicted {want}")
    else:
        assert not any(taken), taken
    for k, got in states.items():
        bad = got.rw_equal(truth.post[k])
        assert not bad, (f"block {k}", bad)
    for k, (m, r) in enumerate(zip(mixes, truth.refs)):
        e = rel_rms(m, r)
        print(f"seed {seed} {form} block {k} ({case.blocks[k][0]} frames): mix rel rms {e:.3g}")
        assert e <= 1e-5, f"block {k}"
    assert viol == 0
    return taken


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("seed", SEEDS)
def test_moving_envelopes_fuzz_vs_oracle(dev, seed, form):
    check_run(dev, seed, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("env_beside", "in_place"))
@pytest.mark.parametrize("seed", [s for s in SEEDS if s % 4 == 2][:2])
def test_linear_lookup_without_guard_samples(dev, seed, form):
    """The LDS-table seeds with linear lookup once more on a pool without guard samples: the general linear form (INTERP 1) instead
    of the guarded one (INTERP 2) that test_moving_envelopes_fuzz_vs_oracle ran."""
    assert get_case(seed).recipe == "c2" and get_case(seed).interp == 1
    check_run(dev, seed, form, guards=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(env_fuzz.PINNED))
def test_pinned_edge(dev, name):
    """One stage edge, clock or list shape each (tests/env_fuzz.py: pinned), through the envelope kernel, in place and on the
    one-voice kernel's block form."""
    for form in ("env_beside", "in_place", "one_voice"):
        taken = check_run(dev, name, form)
        if form == "in_place" and name in ("wave_of_33", "word_of_9"):
            assert any(taken), taken
