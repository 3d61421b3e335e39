"""The fixed-point path against its definition on every block form (include/skred_amd_fxpt.h; oracle/cpu_ref_fxpt.c).

CPU tier: tests/fx_model.py (a second, independent statement of the definition) equals the C definition bit for bit on every
generated case (tests/fx_fuzz.py), no case makes the definition overflow an int32 product, and the kernel paths the model
predicts for the seed set cover every form sk_fx_render_kernel has.  GPU tier: DeviceFxBank against cpuref over the seed set
in three call forms, and pinned cases for the edges a random draw only meets by chance.  Expected values always come from
cpuref; the model's path prediction only names the wave and chunk in a failure message and feeds the coverage count.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import fx_fuzz
import fx_model
from fx_fuzz import Case
from oracle import cpuref
from skred_amd.fxbank import FX_RW, MASTER_K_Q15, MASTER_TARGET_Q31, FxVoiceBank

FORMS = ("host", "mix", "split")       # skred_fxbank_render_host | _render_mix | _render + _master
HANDFUL = 5                            # every path is predicted at least this often per interpolation mode and pool form


# ------------------------------------------------------------------------------------------------ one driver, three engines

def _copy_window(dst, src, src_first, dst_first, count):
    for k in dst.a:
        dst.a[k][dst_first:dst_first + count] = src.a[k][src_first:src_first + count]


def run_cpu(case, interp, engine, want_stems=True):
    """The case on the C definition ("ref") or on the numpy model ("model").  Returns (per segment: dict(mix, stems, out, rw,
    count, gain), the windows every download action is expected to return, the model's Report or None)."""
    bank, count = case.bank.copy(), case.count0
    target, k, gain = case.master0 or (MASTER_TARGET_Q31, MASTER_K_Q15, 0)
    rep = fx_model.Report() if engine == "model" else None
    any_filter = bool((bank["filter_mode"] != 0).any())
    segs, windows = [], []
    for frames, actions in case.segments:
        for act in actions:
            if act[0] == "stamp":
                fx_model.stamp(bank, act[1], act[2], count)
            elif act[0] == "upload":
                _copy_window(bank, case.patch, act[1], act[2], act[3])
                any_filter = any_filter or bool((case.patch["filter_mode"][act[1]:act[1] + act[3]] != 0).any())
            elif act[0] == "download":
                windows.append({f: bank[f][act[1]:act[1] + act[3]].copy() for f in FX_RW})
            elif act[0] == "master":
                target, k, gain = act[1:]
            elif act[0] == "count":
                count = act[1]
        if engine == "model":
            mix, stems, count = fx_model.render(bank, case.pool, count, frames, interp, want_stems, rep, any_filter)
            out, gain = fx_model.master(target, k, gain, mix)
        else:
            mix, stems, count = cpuref.fx_render(bank, case.pool, count, frames, interp, want_stems=want_stems)
            out, gain = cpuref.fx_master(target, k, gain, mix)
        segs.append(dict(mix=mix, stems=stems, out=out, rw={f: bank[f].copy() for f in FX_RW}, count=count, gain=gain))
    return segs, windows, rep


def _first_difference(case, interp, seg, got, want, what):
    """seed, segment, first differing frame and voice, and the path predicted for that wave and chunk."""
    bad = np.argwhere(got != want)[0]
    frame, voice = int(bad[0]), (int(bad[1]) if what == "stems" else None)
    where = f"frame {frame}" + (f", voice {voice} (lane {voice & 63})" if voice is not None else "")
    _, _, rep = run_cpu(case, interp, "model", want_stems=False)
    paths = [p for p in rep.paths[seg] if p.chunk == frame // 64 and (voice is None or p.wave == voice >> 6)]
    got_v, want_v = got[tuple(bad)], want[tuple(bad)]
    return (f"seed {case.seed} interp {interp} segment {seg}: {what} differ first at {where}: got {got_v}, definition {want_v}\n  predicted: "
            + "\n             ".join(str(p) for p in paths[:8]))


def run_device(case, interp, form, ref, want_stems=True):
    """The case on the GPU in one call form, every segment held against `ref` = run_cpu(case, interp, "ref")."""
    import torch
    from skred_amd import fxbank
    segs, windows = ref[0], list(ref[1])
    n = case.n
    db = fxbank.DeviceFxBank(n)
    L, h = db.L, db.h

    def window(fn, bank, src_first, dst_first, count):
        cb = bank.as_c()
        rc = fn(h, C.byref(cb), src_first, dst_first, count)
        assert rc == 0, (rc, L.skred_amd_last_error())

    try:
        db.set_tables(case.pool)
        db.upload(case.bank)
        db.set_sample_count(case.count0)
        if case.master0:
            db.set_master(*case.master0)
        last_set_gain = case.master0[2] if case.master0 else 0
        host = case.bank.copy()
        for s, (frames, actions) in enumerate(case.segments):
            for act in actions:
                if act[0] == "stamp":
                    db.stamp(act[1], act[2])
                elif act[0] == "upload":
                    window(L.skred_fxbank_upload, case.patch, act[1], act[2], act[3])
                elif act[0] == "download":
                    scratch = FxVoiceBank(n)
                    for f in FX_RW:
                        scratch[f] = 77                                    # a sentinel the window must not spill over
                    window(L.skred_fxbank_download, scratch, act[1], act[2], act[3])
                    want = windows.pop(0)
                    inside = np.zeros(n, bool)
                    inside[act[2]:act[2] + act[3]] = True
                    for f in FX_RW:
                        assert (scratch[f][inside] == want[f]).all(), f"seed {case.seed} segment {s}: download window {act[1:]} field {f}"
                        assert (scratch[f][~inside] == 77).all(), f"seed {case.seed} segment {s}: download {act[1:]} wrote outside its window ({f})"
                elif act[0] == "master":
                    db.set_master(*act[1:])
                    last_set_gain = act[3]
                elif act[0] == "count":
                    db.set_sample_count(act[1])
            want = segs[s]
            if form == "host":
                mix, stems = db.render_host(frames, interp, want_stems=want_stems)
                out = None
            else:
                d_out = torch.zeros(frames, 2, dtype=torch.int64, device="cuda")
                d_sum = torch.zeros(frames, 2, dtype=torch.int64, device="cuda")
                d_stems = torch.zeros(frames, n, 2, dtype=torch.int32, device="cuda") if want_stems else None
                p_stems = d_stems.data_ptr() if want_stems else 0
                if form == "mix":
                    db.render_mix(frames, d_out.data_ptr(), interp, p_stems)
                else:
                    db.render(frames, d_sum.data_ptr(), interp, p_stems)
                    db.master(d_sum.data_ptr(), frames, d_out.data_ptr())
                torch.cuda.synchronize()
                out = d_out.cpu().numpy()
                mix = d_sum.cpu().numpy() if form == "split" else None
                stems = d_stems.cpu().numpy() if want_stems else None
            if stems is not None and not (stems == want["stems"]).all():
                pytest.fail(f"[{form}] " + _first_difference(case, interp, s, stems, want["stems"], "stems"))
            if mix is not None and not (mix == want["mix"]).all():
                pytest.fail(f"[{form}] " + _first_difference(case, interp, s, mix, want["mix"], "integer mix"))
            if out is not None and not (out == want["out"]).all():
                pytest.fail(f"[{form}] " + _first_difference(case, interp, s, out, want["out"], "post-master output"))
            db.download(host)
            diff = {f: int(np.argmax(host[f] != want["rw"][f])) for f in FX_RW if (host[f] != want["rw"][f]).any()}
            assert not diff, f"[{form}] seed {case.seed} interp {interp} segment {s}: read-write state differs, first voice per field {diff}"
            assert db.sample_count() == want["count"], f"[{form}] seed {case.seed} segment {s}: clock"
            assert db.master_gain() == (last_set_gain if form == "host" else want["gain"]), f"[{form}] seed {case.seed} segment {s}: master gain"
        assert not windows
    finally:
        db.close()


def check_on_device(case, interps=(0, 1), forms=FORMS, want_stems=True):
    for interp in interps:
        ref = run_cpu(case, interp, "ref", want_stems)
        for form in forms:
            run_device(case, interp, form, ref, want_stems)


# ------------------------------------------------------------------------------------------------ CPU tier

@functools.lru_cache(maxsize=None)
def model_against_definition(seed, big=False):
    """One seed on both CPU engines.  Returns (differences, overflow, [(interp, Path)], inert pairs, pairs)."""
    case = fx_fuzz.case(seed, big)
    ref, ref_win, _ = run_cpu(case, case.interp, "ref", want_stems=not big)
    mod, mod_win, rep = run_cpu(case, case.interp, "model", want_stems=not big)
    diffs = []
    for s, (r, m) in enumerate(zip(ref, mod)):
        for key in ("stems", "mix", "out"):
            if r[key] is not None and not (r[key] == m[key]).all():
                diffs.append((s, key, tuple(int(x) for x in np.argwhere(r[key] != m[key])[0])))
        diffs += [(s, f, int(np.argmax(r["rw"][f] != m["rw"][f]))) for f in FX_RW if (r["rw"][f] != m["rw"][f]).any()]
        if r["count"] != m["count"] or r["gain"] != m["gain"]:
            diffs.append((s, "clock / master gain", r["count"], m["count"], r["gain"], m["gain"]))
    for i, (r, m) in enumerate(zip(ref_win, mod_win)):
        diffs += [("download", i, f) for f in FX_RW if (r[f] != m[f]).any()]
    inert, pairs = 0, 0
    state = {"finished": case.bank["finished"]}
    amp = case.bank["amp_q15"].copy()
    for s, (frames, actions) in enumerate(case.segments):
        for act in actions:
            if act[0] == "upload":
                amp[act[2]:act[2] + act[3]] = case.patch["amp_q15"][act[1]:act[1] + act[3]]
        fin = state["finished"] if s == 0 else ref[s - 1]["rw"]["finished"]
        inert += int(((amp == 0) | (fin != 0)).sum())
        pairs += case.n
    return diffs, dict(rep.overflow), [(case.interp, p) for launch in rep.paths for p in launch], inert, pairs


@pytest.mark.parametrize("seed,big", [(s, False) for s in fx_fuzz.SEEDS] + [(s, True) for s in fx_fuzz.BIG_SEEDS])
def test_model_equals_the_definition_and_nothing_overflows(seed, big):
    diffs, overflow, _, _, _ = model_against_definition(seed, big)
    assert not diffs, f"seed {seed}: fx_model and cpu_ref_fxpt.c disagree (segment, what, where): {diffs[:6]}"
    assert not overflow, f"seed {seed}: the definition's int32 products overflow -- the generator left the promised range: {overflow}"


def required_paths(lds):
    need = {"per-frame": lambda p: p.form == fx_model.FRAME,
            "spelled-out block": lambda p: p.form == fx_model.BLOCK,
            "narrow": lambda p: p.narrow is True, "wide": lambda p: p.narrow is False,
            "stalled": lambda p: p.stalled is True, "moving": lambda p: p.stalled is False,
            "filter on": lambda p: p.any_filter, "filter off": lambda p: not p.any_filter}
    if lds:      # the lean blocks read the pool from LDS only
        need["lean block"] = lambda p: p.form == fx_model.LEAN
        need["lean chunk that rolls a block back"] = lambda p: p.rollback
        need["lean without a rollback, filter on"] = lambda p: p.form == fx_model.LEAN and p.any_filter and not p.rollback
    return need


def test_predicted_paths_cover_every_kernel_form():
    paths = [ip for s in fx_fuzz.SEEDS for ip in model_against_definition(s)[2]]
    missing = []
    for interp in (0, 1):
        for lds in (True, False):
            mine = [p for i, p in paths if i == interp and p.lds == lds]
            for name, pred in required_paths(lds).items():
                count = sum(1 for p in mine if pred(p))
                if count < HANDFUL:
                    missing.append((f"interp {interp}", "LDS pool" if lds else "pool in memory", name, count))
    assert not missing, f"paths predicted fewer than {HANDFUL} times over the seed set: {missing}"


def test_inert_share_stays_under_the_generators_cap():
    inert = sum(model_against_definition(s)[3] for s in fx_fuzz.SEEDS)
    pairs = sum(model_against_definition(s)[4] for s in fx_fuzz.SEEDS)
    assert inert <= fx_fuzz.INERT_CAP * pairs, (inert, pairs, inert / pairs)


def test_model_master_and_stamps_equal_the_definition():
    rng = np.random.default_rng(11)
    mix = rng.integers(-(1 << 37), 1 << 37, (300, 2))
    for target, k, g in ((0, 0, 5), ((1 << 31) - 1, 32768, 0), (MASTER_TARGET_Q31, MASTER_K_Q15, 0), (12345, 1, (1 << 31) - 1)):
        want, wg = cpuref.fx_master(target, k, g, mix)
        got, gg = fx_model.master(target, k, g, mix)
        assert (got == want).all() and gg == wg, (target, k, g)


# ------------------------------------------------------------------------------------------------ GPU tier: the seed set

@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("in_lds", [True, False])
def test_fx_fuzz_gpu_equals_the_definition_in_three_call_forms(interp, in_lds):
    for seed in fx_fuzz.SEEDS:
        if (not (seed >> 1) & 1) == in_lds:
            check_on_device(fx_fuzz.case(seed), interps=(interp,))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", fx_fuzz.BIG_SEEDS)
def test_fx_fuzz_gpu_two_level_mix_down(seed):
    """64 * 256 + 1 voices: 65 workgroup rows, so skx_finish_block adds slabs first; mix and state only."""
    case = fx_fuzz.case(seed, big=True)
    check_on_device(case, interps=(case.interp,), want_stems=False)


# ------------------------------------------------------------------------------------------------ pinned cases

def pinned_pool(entries=4096, seed=7):
    pool = np.random.default_rng(seed).integers(-32768, 32768, entries).astype(np.int16)
    pool[:64] = 800                                     # a constant stretch: a voice on it feeds its filter a DC input
    return pool


def plain(n, entries=4096, count0=96000):
    """n sounding voices with nothing else on: no envelope, smoother or filter; tables of 32 entries spread over the pool."""
    b = FxVoiceBank(n)
    v = np.arange(n)
    b["log2_size"] = 5
    b["table_offset"] = 64 + (v * 37) % (entries - 64 - 32)
    b["phase"] = (v.astype(np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    b["phase_inc"] = (1 << 32) // (30 + v % 200)
    b["amp_q15"] = 20000 + v % 12000
    b["pan_left_q15"], b["pan_right_q15"] = 9000 + (v * 7) % 20000, 30000 - (v * 5) % 20000
    b["is_active"] = 1
    return b


def held(b, sel, count0, A=50, D=70, R=90, S=20000):
    b["use_envelope"][sel] = 1
    b["attack_frames"][sel], b["decay_frames"][sel], b["release_frames"][sel], b["sustain_q15"][sel] = A, D, R, S
    b["sample_start"][sel] = count0 - A - D - 10
    b["is_active"][sel] = 1


def at_rest(b, sel):
    """The smoother on and resting at the held level: with held() or no envelope such a wave is stalled and lean-eligible."""
    amp, S, vel = (b[k][sel].astype(np.int64) for k in ("amp_q15", "sustain_q15", "velocity_q15"))
    b["smoother_enable"][sel], b["smoother_k_q15"][sel] = 1, 655
    b["smoother_gain_q15"][sel] = np.where(b["use_envelope"][sel] != 0, (amp * ((S * vel) >> 15)) >> 15, amp)


COUNT0 = 96000


@pytest.mark.gpu
@pytest.mark.parametrize("field", ["sample_start", "sample_release"])
@pytest.mark.parametrize("others_steady", [True, False])
@pytest.mark.parametrize("ahead", [5, 64, 100, 300])
def test_note_time_ahead_of_the_clock(ahead, others_steady, field):
    """A note start (or release) stamped `ahead` frames after the clock -- inside the first chunk, on a chunk edge, in a
    later chunk, in a later launch (launches of 200 frames) -- in a wave of held notes.  Until `now` reaches it the 64-bit
    difference wraps and saturates (the level is S, or the release has run out); then t restarts at 0 INSIDE a chunk."""
    n = 130
    b = plain(n)
    held(b, slice(0, n), COUNT0)
    at_rest(b, slice(0, n))
    for lane, d in ((7, 0), (63, 1), (64 + 20, -1)):
        b[field][lane] = COUNT0 + ahead + d
    if not others_steady:
        b["sample_start"][3] = COUNT0 - 20                 # one lane in its attack: the wave runs frame by frame anyway
        b["sample_start"][64 + 3] = COUNT0 - 20
    check_on_device(Case(bank=b, pool=pinned_pool(), count0=COUNT0, interp=1, segments=[(200, []), (200, []), (9, [])]), interps=(1,))


@pytest.mark.gpu
def test_clock_rewound_between_launches_puts_note_starts_ahead_again():
    n = 70
    b = plain(n)
    held(b, slice(0, n), COUNT0, A=3, D=4)
    at_rest(b, slice(0, n))
    b["sample_start"][[5, 63, 66]] = COUNT0 + 10
    segs = [(128, []), (128, [("count", COUNT0 - 40)]), (64, [("count", COUNT0 + 9)]), (64, [("count", COUNT0 + 10)])]
    check_on_device(Case(bank=b, pool=pinned_pool(), count0=COUNT0, interp=0, segments=segs))


@pytest.mark.gpu
@pytest.mark.parametrize("count0", [(1 << 32) - 100, (1 << 33) + 5, 1 << 32])
def test_clock_across_2_pow_32_and_saturated_note_age(count0):
    """The low word of the clock wraps inside a launch; notes older than 2^32 frames (t saturated) with A + D below and above
    2^32; notes that start on either side of the wrap."""
    n = 128
    b = plain(n)
    held(b, slice(0, n), count0)
    at_rest(b, slice(0, 64))
    b["sample_start"][0:64:4] = 3                                           # ancient where count0 > 2^32
    b["attack_frames"][1:64:4], b["decay_frames"][1:64:4] = 0xFFFFFFFF, 0xFFFFFFFF   # A + D > 2^32: never past its decay
    b["sample_start"][1:64:4] = 3
    b["sample_start"][64:128] = count0 + np.arange(64) * 3 - 40             # starts around the clock, in wave 1
    b["sample_release"][64:128:2] = count0 + 90 + np.arange(32) * 2
    check_on_device(Case(bank=b, pool=pinned_pool(), count0=count0, interp=1, segments=[(64, []), (200, []), (65, [])]))


@pytest.mark.gpu
def test_zero_length_envelope_stages():
    """A, D and R each 0 and all 0, S 0 and 32768, at every age of the note: starting now, held, released."""
    combos = [(A, D, R, S) for A in (0, 2) for D in (0, 3) for R in (0, 4) for S in (0, 32768)]
    n = 64 * 3
    b = plain(n)
    for w in range(3):
        for i, (A, D, R, S) in enumerate(combos * 4):
            v = w * 64 + i
            held(b, v, COUNT0, A, D, R, S)
    b["sample_start"][0:64] = COUNT0 - np.arange(64) % 7                    # wave 0: just started
    b["sample_release"][128:192] = COUNT0 + 60 + np.arange(64) % 9          # wave 2: released around the first chunk edge
    stamp = np.arange(64, 128, dtype=np.int32)                              # wave 1: note-on, later note-off, between launches
    segs = [(70, []), (64, [("stamp", stamp, 1)]), (9, [("stamp", stamp, 2)]), (64, [])]
    check_on_device(Case(bank=b, pool=pinned_pool(), count0=COUNT0, interp=0, segments=segs))


@pytest.mark.gpu
@pytest.mark.parametrize("entries", [4096, 30000])
def test_one_shots_ending_on_block_chunk_and_launch_edges(entries):
    """One-shots whose cycle ends on frame 0, 7, 8, 63, 64 and on the last frame of a launch; phase_inc 0 (never ends) and
    >= 2^31; in wave 1 a one-shot that ended in the first launch shares its wave with steady, lean-eligible lanes."""
    n, F = 128, 137
    rng = np.random.default_rng(2)
    b = plain(n, entries)
    at_rest(b, slice(64, 128))
    ends = [0, 7, 8, 63, 64, F - 1, F, F + 7, 2 * F - 1]
    for i, e in enumerate(ends * 3):
        b["one_shot"][i] = 1
        (b["phase"][i],), (b["phase_inc"][i],) = fx_fuzz.one_shot_ending_at(rng, e)
        b["filter_mode"][i] = i % 2
    for k, v in fx_fuzz.coeffs(rng, "gentle", n).items():
        b[k] = v
    b["one_shot"][40:46] = 1
    b["phase_inc"][40:43], b["phase_inc"][43:46] = 0, ((1 << 31), (1 << 31) + 12345, 0xFFFFFFFF)
    b["one_shot"][64 + 9] = 1
    (b["phase"][64 + 9],), (b["phase_inc"][64 + 9],) = fx_fuzz.one_shot_ending_at(rng, 70)
    check_on_device(Case(bank=b, pool=pinned_pool(entries), count0=COUNT0, interp=0, segments=[(F, []), (F, []), (64, [])]))


@pytest.mark.gpu
@pytest.mark.parametrize("entries", [49152 // 2, 49154 // 2, 49152 // 2 - 5, 32768 + 5])
def test_tables_at_the_pools_end_and_pools_at_the_lds_limit(entries):
    """Pools of exactly 49152 bytes (the last that fits LDS), 49154 bytes (the first that does not), a size that is no multiple
    of 8 entries; tables of 2^3 and (where the pool has room) 2^15 entries ending at the pool's last entry, the phase one step
    before its wrap so that the linear neighbour folds to entry 0."""
    n = 96
    b = plain(n, entries)
    at_rest(b, slice(32, 96))
    big = 15 if entries >= 32768 else 14
    b["log2_size"][0:n:2], b["log2_size"][1:n:2] = 3, big
    b["table_offset"][0:n:2], b["table_offset"][1:n:2] = entries - 8, entries - (1 << big)
    inc = b["phase_inc"].astype(np.int64)
    b["phase"] = ((1 << 32) - inc * (1 + np.arange(n) % 3) - 1).astype(np.uint32)   # last entry after 1 .. 3 adds, then wraps
    check_on_device(Case(bank=b, pool=pinned_pool(entries), count0=COUNT0, interp=1, segments=[(72, []), (8, [])]))


@pytest.mark.gpu
def test_windowed_upload_and_download_across_a_group_edge():
    """upload / download with src_first != dst_first over the edge of a 256-voice group; the voices outside the window keep
    constants and state; the window brings the first filtered voices into a bank uploaded without any."""
    n = 600
    b = plain(n)
    at_rest(b, slice(0, n))
    rng = np.random.default_rng(4)
    patch = plain(n)
    patch["phase_inc"] = (patch["phase_inc"].astype(np.int64) * 3).astype(np.uint32)
    patch["filter_mode"] = 2
    for k, v in fx_fuzz.coeffs(rng, "gentle", n).items():
        patch[k] = v
    patch["x1"], patch["y2"] = 12345, -54321
    segs = [(72, []), (72, [("download", 250, 3, 20), ("upload", 10, 250, 20), ("download", 240, 100, 40)]),
            (64, [("upload", 599, 0, 1), ("download", 0, 599, 1)])]
    check_on_device(Case(bank=b, pool=pinned_pool(), count0=COUNT0, interp=1, segments=segs, patch=patch), interps=(1,))


@pytest.mark.gpu
def test_stamps_trigger_and_release_in_one_call_duplicates_and_inactive_voices():
    n = 200
    b = plain(n)
    held(b, slice(0, n), COUNT0, A=5, D=6, R=20)
    at_rest(b, slice(0, n))
    b["is_active"][::3] = 0
    both = np.array([0, 1, 1, 2, 3, 3, 3, 64, 199, 199], np.int32)         # which == 3: duplicates, active and inactive voices
    off = np.array([6, 6, 9, 12, 7, 150], np.int32)                         # releases: 6, 9, 12, 150 are inactive
    segs = [(64, []), (70, [("stamp", both, 3)]), (64, [("stamp", off, 2), ("stamp", np.zeros(0, np.int32), 1)]),
            (9, [("stamp", off, 1)]), (64, [("stamp", off, 2)])]
    check_on_device(Case(bank=b, pool=pinned_pool(), count0=COUNT0, interp=0, segments=segs))


@pytest.mark.gpu
def test_master_stage_extremes_and_a_carried_gain():
    """k 0 and 32768, target 0 and 2^31 - 1, a gain carried across a change of target, one-frame blocks."""
    n = 300
    b = plain(n)
    top = (1 << 31) - 1
    segs = [(64, []), (1, [("master", 0, 32768, top)]), (1, []), (65, [("master", top, 0, 12345)]),
            (64, [("master", top, 32768, 0)]), (1, [("master", 0, 66, top)]), (130, []), (7, [("master", top, 655, 1 << 20)]), (1, [])]
    case = Case(bank=b, pool=pinned_pool(), count0=COUNT0, interp=0, segments=segs, master0=(top, 66, 0))
    check_on_device(case, interps=(0,), forms=("mix", "split"))


@pytest.mark.gpu
def test_master_is_refused_without_a_render_of_the_same_length():
    import torch
    from skred_amd import device, fxbank
    db = fxbank.DeviceFxBank(64)
    db.set_tables(pinned_pool())
    db.upload(plain(64))
    buf = torch.zeros(64, 2, dtype=torch.int64, device="cuda")
    with pytest.raises(device.SkredAmdError):
        db.master(buf.data_ptr(), 64, buf.data_ptr())                      # nothing rendered yet
    db.render(64, buf.data_ptr())
    with pytest.raises(device.SkredAmdError):
        db.master(buf.data_ptr(), 32, buf.data_ptr())                      # another length
    db.master(buf.data_ptr(), 64, buf.data_ptr())
    with pytest.raises(device.SkredAmdError):
        db.master(buf.data_ptr(), 64, buf.data_ptr())                      # the block's gains are spent
    db.render_mix(64, buf.data_ptr())
    with pytest.raises(device.SkredAmdError):
        db.master(buf.data_ptr(), 64, buf.data_ptr())                      # render_mix applied the stage itself
    torch.cuda.synchronize()
    db.close()


@pytest.mark.gpu
def test_smoother_around_the_stall_tests_boundary():
    """One wave per (d, k): every lane's smoother at target + d, d in -3 .. 3, k in {1, 655, 32767, 32768}: the wave-wide stall
    test (((target - g) * k) >> 15 == 0) flips between d = 0 / 1 and d = -1 for every k."""
    combos = [(d, k) for d in range(-3, 4) for k in (1, 655, 32767, 32768)]
    n = 64 * len(combos)
    b = plain(n)
    b["smoother_enable"] = 1
    for w, (d, k) in enumerate(combos):
        sel = slice(64 * w, 64 * w + 64)
        b["smoother_k_q15"][sel] = k
        b["smoother_gain_q15"][sel] = b["amp_q15"][sel] + d
        if w % 2:
            held(b, sel, COUNT0, S=32768)                                   # (amp * 32768) >> 15: the same target, now held
    check_on_device(Case(bank=b, pool=pinned_pool(), count0=COUNT0, interp=1, segments=[(64, []), (9, [])]), interps=(1,))


def filter_ramp_bank(n=128):
    """Wave 0: lane 5 reads the pool's constant stretch (s = 800) through b0 = 1, a1 ~ -2, a2 = 1 -- a double pole at z = 1,
    y[m] = 800 * 4096 * m (m + 1) / 2 -- so its delay line passes 2^29 at m = 18, the chunk's THIRD block; the other lanes are
    steady and lean-eligible, filtered gently or not at all (those keep the delay line they were uploaded with)."""
    rng = np.random.default_rng(9)
    b = plain(n)
    at_rest(b, slice(0, n))
    for k, v in fx_fuzz.coeffs(rng, "gentle", n, high_pass=False).items():
        b[k] = v
    b["filter_mode"] = np.arange(n) % 3 != 0
    for k in ("x1", "x2", "y1", "y2"):
        b[k] = rng.integers(-(1 << 24), 1 << 24, n)
    for lane in (5, 64 + 63):
        b["table_offset"][lane], b["filter_mode"][lane] = 0, 1
        b["b0_q30"][lane], b["b1_q30"][lane], b["b2_q30"][lane] = 1 << 30, 0, 0
        b["a1_q30"][lane], b["a2_q30"][lane] = -((1 << 31) - 1), 1 << 30
        for k in ("x1", "x2", "y1", "y2"):
            b[k][lane] = 0
    return b


def test_filter_ramp_reaches_the_rail_in_the_third_block():
    """The pinned case is what its name says: per the model, blocks 0 and 1 stay lean, block 2 rolls back."""
    for frames, rolls in ((16, False), (24, True)):
        rep = fx_model.Report()
        fx_model.render(filter_ramp_bank(), pinned_pool(), COUNT0, frames, 1, report=rep)
        assert [(p.form, p.rollback) for p in rep.paths[0]] == [(fx_model.LEAN, rolls)] * 2, frames
    assert not rep.overflow


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1])
def test_filter_rail_in_the_third_block_of_a_lean_chunk(interp):
    """Lean blocks, a rollback, then spelled-out blocks in ONE chunk; unfiltered lanes beside filtered ones keep their delay line."""
    check_on_device(Case(bank=filter_ramp_bank(), pool=pinned_pool(), count0=COUNT0, interp=interp, segments=[(64, []), (72, []), (8, [])]),
                    interps=(interp,))


@pytest.mark.gpu
def test_filter_coefficient_int32_min_declines_the_lean_blocks():
    """a1 or a2 == INT32_MIN (-2.0 in Q2.30) cannot be negated: the wave takes the spelled-out blocks; its neighbour wave stays lean."""
    b = filter_ramp_bank()
    b["a1_q30"][5] = -(1 << 31)
    b["a2_q30"][9], b["filter_mode"][9] = -(1 << 31), 1
    rep = fx_model.Report()
    fx_model.render(b.copy(), pinned_pool(), COUNT0, 64, 1, report=rep)
    assert [p.form for p in rep.paths[0]] == [fx_model.BLOCK, fx_model.LEAN]
    check_on_device(Case(bank=b, pool=pinned_pool(), count0=COUNT0, interp=1, segments=[(64, []), (72, [])]), interps=(1,))
