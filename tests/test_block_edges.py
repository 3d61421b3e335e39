"""Block edges of the modulated kernel (skred_render_generic.hip: sk_render_mod_kernel) against the oracle.

The frame-lag form runs the level-1 lanes of a wavefront one frame behind its level-0 lanes, with one iteration more per launch
(the first without the level-1 lanes, the last without the level-0 lanes).  What a lane leaves in voice_sample at a launch's end,
and what its readers take at the next launch's frame 0, is decided in those two iterations -- so the banks here are built so that
voices finish, and are silenced or re-triggered, exactly at launch ends, chunk ends (SK_CHUNK = 64) and launch starts, in every
role a voice can have in such a wavefront.  After EVERY launch the whole state, the globals and the mix are checked against
cpuref, in five forms: frame-lag and level loop, each unpacked and packed, and the level loop with stems (bit for bit).  The
form counter (skred_bank_set_form_counter) shows that the lag form really ran where the waves were built for it.

A copy is eight voices; a 64-voice group holds two live copies (the other 48 voices are off: packed waves of 16 lanes per group,
some of them empty) of one kind:
  kind A (finishing):  v0 F1 (previous frame, from above)   v1 one-shot, level 0 (read by v0 a frame late, by v2 v4 v5 v7 in its frame)
                       v2 A1 F4 (level 1; reads v4 from above)   v3 one-shot nobody reads   v4 one-shot A1 (level 1, read from below by v2)
                       v5 noise A1 (level 1: the previous iteration's draw)   v6 plain   v7 F1 (level 1, muted; a one-shot in `fm_cut`)
  kind B (silencing):  v0 F3 P6   v1 F2 A0 (level 1)   v2 F0 (level 1, read from above by v1)   v3 source of v0 (below) and v4 v5 (above)
                       v4 A3   v5 noise A3   v6 amp 0, F7 (named by v0, names v7)   v7 amp 0, named by nobody that sounds
"""
import numpy as np
import pytest

import golden_io as gio
import mod_forms
from oracle import cpuref
from skred_amd import banks
from skred_amd.bank import VoiceBank

N_GROUPS = 16
N = 64 * N_GROUPS
SEGS = [64, 65, 1, 2, 3, 512, 63]            # launch lengths
BIG = (707, 8186)                            # (offset, size) of the fixture pool's longest one-shot table
LOOP = (15246, 4096)
SHOT_INC = {1: 1.0, 3: 0.5, 4: 1.0}          # the hand-timed one-shots of a kind-A copy and their (power of two) increments


def live_copies(g):
    return [g % 8, (g + 3) % 8]


def kind(g):
    return "A" if g % 2 == 0 else "B"


def copies(k):
    return [g * 64 + c * 8 for g in range(N_GROUPS) if kind(g) == k for c in live_copies(g)]


def resolve(segs, where):
    """('last', L) / ('first', L) / ('at', L, f) -> global frame index."""
    start = int(np.sum(segs[:where[1]]))
    if where[0] == "last":
        return start + segs[where[1]] - 1
    if where[0] == "first":
        return start
    assert where[2] < segs[where[1]]
    return start + where[2]


# where the one-shots of the 16 kind-A copies finish: every launch length, launch ends and starts, the chunk loop's edges, a middle
FINISH = [("last", 0), ("first", 1), ("at", 1, 62), ("at", 1, 63), ("last", 1), ("first", 2), ("last", 3), ("last", 4),
          ("first", 5), ("at", 5, 62), ("at", 5, 63), ("at", 5, 64), ("at", 5, 65), ("at", 5, 300), ("first", 6), ("last", 6)]


def _shot(b, v, inc, k, table=BIG):
    """A forward one-shot without loop whose phase reaches the table's end -- voice_finished -- on frame k exactly."""
    b["voice_table_offset"][v], b["voice_table_size"][v] = table
    b["voice_one_shot"][v] = 1
    b["voice_loop_enabled"][v] = 0
    b["voice_phase_inc"][v] = np.float32(inc)
    b["voice_phase"][v] = np.float32(table[1] - (k + 1) * inc)
    b["voice_finished"][v] = 0


def _rearm(host, copy, k):
    for o, inc in SHOT_INC.items():
        _shot(host, copy + o, inc, k)


def build(finish_at, fm_cut=False):
    """The bank (see the module docstring); finish_at[i]: global frame on which the one-shots of kind-A copy i finish."""
    gold = gio.load("c4_pcm_oneshot")
    tables = gold.tables
    b = VoiceBank(N)
    for f in ("voice_freq_mod_osc", "voice_amp_mod_osc", "voice_pan_mod_osc", "voice_cz_mod_osc"):
        b[f] = -1
    v = np.arange(N)
    b["voice_table_offset"], b["voice_table_size"] = LOOP
    b["voice_loop_enabled"] = 1
    b["voice_wave_table_index"] = 200
    b["voice_phase"] = (v * 37 % 4000).astype(np.float32)
    b["voice_phase_inc"] = (np.float32(1.3) + np.float32(0.07) * (v % 29)).astype(np.float32)
    b["voice_smoother_enable"] = 1
    b["voice_smoother_smoothing"] = np.float32(0.25)
    b["voice_freq_scale"] = (np.float32(0.5) + np.float32(0.01) * (v % 40)).astype(np.float32)
    b["voice_sample"] = ((v % 17) * 0.03 - 0.2).astype(np.float32)        # stale samples: the skip rule clears them
    pl, pr = banks.pan_gains(((v % 11) / 5.0 - 1.0).astype(np.float32))
    b["voice_pan_left"], b["voice_pan_right"] = pl, pr

    def mod(key, dst, src, depth):
        b[key + "_osc"][dst] = src
        b[key + "_depth"][dst] = np.float32(depth)

    live = np.zeros(N, bool)
    for i, c in enumerate(copies("A")):
        live[c:c + 8] = True
        mod("voice_freq_mod", c, c + 1, 0.3)
        _rearm(b, c, finish_at[i])
        mod("voice_amp_mod", c + 2, c + 1, 1.5); mod("voice_freq_mod", c + 2, c + 4, 0.2)
        mod("voice_amp_mod", c + 4, c + 1, 1.2)
        b["voice_wave_table_index"][c + 5] = 6                              # WAVE_TABLE_NOISE_ALT (synth.c:543)
        mod("voice_amp_mod", c + 5, c + 1, 0.9)
        mod("voice_freq_mod", c + 7, c + 1, 0.05 + 0.01 * i)
        b["voice_disconnect"][c + 7] = 1
        if fm_cut:                                                          # a frequency-modulated one-shot: its end is found, not set
            b["voice_table_offset"][c + 7], b["voice_table_size"][c + 7] = BIG
            b["voice_one_shot"][c + 7], b["voice_loop_enabled"][c + 7] = 1, 0
            b["voice_phase_inc"][c + 7] = np.float32(1.3)
            b["voice_phase"][c + 7] = np.float32(BIG[1] - 1.3 * (150 + 23 * i))
    for c in copies("B"):
        live[c:c + 8] = True
        mod("voice_freq_mod", c, c + 3, 0.25); mod("voice_pan_mod", c, c + 6, 0.8)
        mod("voice_freq_mod", c + 1, c + 2, 0.2); mod("voice_amp_mod", c + 1, c, 1.1)
        mod("voice_freq_mod", c + 2, c, 0.3)
        mod("voice_amp_mod", c + 4, c + 3, 1.4)
        b["voice_wave_table_index"][c + 5] = 6
        mod("voice_amp_mod", c + 5, c + 3, 0.7)
        mod("voice_freq_mod", c + 6, c + 7, 0.5)
    amp = (np.float32(0.2) + np.float32(0.05) * (v % 13)).astype(np.float32)
    amp[~live] = 0.0
    for c in copies("B"):
        amp[c + 6] = amp[c + 7] = 0.0
    b["voice_amp"] = amp
    g = banks.RECIPES["c2"](64)[2]
    return b, tables, g


def _silenced():
    """v2 of the first live copy of every kind-B group (a level-1 source read from above by the level-1 reader v1) and v3 of the
    second (a level-0 source with readers below and above)."""
    return sorted(c + (2 if i % 2 == 0 else 3) for i, c in enumerate(copies("B")))


def _set_amp(voices, amps):
    def ev(host, now):
        host["voice_amp"][voices] = amps
    return ev


def scenario(name):
    """-> (bank, tables, g, [(frames, event)], plan); plan: {"finish": {voice: (launch, frame)}, "silenced": {launch: [voices]}}."""
    segs = list(SEGS)
    finish_at = [resolve(segs, w) for w in FINISH]
    plan = {"finish": {}, "silenced": {}}
    events = [None] * len(segs)
    if name == "finish":
        bank, tables, g = build(finish_at)
        for i, c in enumerate(copies("A")):
            for o in SHOT_INC:
                plan["finish"][c + o] = FINISH[i]
    elif name == "retrigger":
        # every one-shot finishes on the last frame of launch 0 or 1; re-triggered (voice_finished = 0, phase reset) before launch 2,
        # 3 or 5 and timed afresh to the edges of the later launches
        first = [("last", 0) if i % 2 == 0 else ("last", 1) for i in range(16)]
        bank, tables, g = build([resolve(segs, w) for w in first])
        again = [("first", 5), ("last", 2), ("first", 3), ("last", 5), ("at", 5, 63), ("at", 5, 64), ("first", 6), ("last", 6)] * 2
        at = [2 if i % 4 < 2 else (3 if i % 4 == 2 else 5) for i in range(16)]
        at = [min(a, w[1]) for a, w in zip(at, again)]
        for L in sorted(set(at)):
            cs = [(c, resolve(segs, again[i]) - int(np.sum(segs[:L]))) for i, c in enumerate(copies("A")) if at[i] == L]
            events[L] = (lambda cs_: lambda host, now: [_rearm(host, c, k) for c, k in cs_])(cs)
        for i, c in enumerate(copies("A")):
            for o in SHOT_INC:
                plan["finish"][c + o] = [first[i], again[i]]
    elif name == "silence":
        bank, tables, g = build(finish_at)
        vs = _silenced()
        amps = np.asarray(bank["voice_amp"])[vs].copy()
        events[1], events[2] = _set_amp(vs, 0.0), _set_amp(vs, amps)          # off for one launch, then on again
        events[4], events[5] = _set_amp(vs, 0.0), _set_amp(vs, amps)
        plan["silenced"] = {1: vs, 4: vs}
        for i, c in enumerate(copies("A")):
            for o in SHOT_INC:
                plan["finish"][c + o] = FINISH[i]
    elif name == "fm_cut":
        bank, tables, g = build(finish_at, fm_cut=True)
        ends = _finish_frames(bank, tables, g, [(2000, None)], [c + 7 for c in copies("A")])
        f1, f2 = sorted(set(int(e) for e in ends.values()))[:2]
        segs = [f1 + 1, f2 - f1, 64, 3]                   # launches 0 and 1 end exactly where a modulated one-shot finishes
        events = [None] * len(segs)
        first_shot = {int(e): v for v, e in sorted(ends.items(), reverse=True)}
        plan["finish"] = {first_shot[f1]: ("last", 0), first_shot[f2]: ("last", 1)}
    else:
        raise KeyError(name)
    return bank, tables, g, list(zip(segs, events)), plan


NAMES = ["finish", "retrigger", "silence", "fm_cut"]


def _finish_frames(bank, tables, g, segments, voices):
    """Frame by frame through cpuref: the global frame on which each of `voices` first has voice_finished set."""
    host, gl = bank.copy(), g.copy()
    out, t = {}, 0
    for frames, event in segments:
        if event is not None:
            event(host, gl.synth_sample_count)
        for _ in range(frames):
            cpuref.render(host, gl, tables, 1, 0)
            fin = np.asarray(host["voice_finished"])
            for v in voices:
                if v not in out and fin[v]:
                    out[v] = t
            t += 1
    return out


def _timeline(bank, tables, g, segments):
    """Frame by frame through cpuref: {voice: [(launch, frame) of every 0 -> 1 flip of voice_finished]}, amp == 0 per launch."""
    host, gl = bank.copy(), g.copy()
    flips, silent = {}, []
    for L, (frames, event) in enumerate(segments):
        if event is not None:
            event(host, gl.synth_sample_count)
        silent.append(set(np.flatnonzero(np.asarray(host["voice_amp"]) == 0).tolist()))
        for f in range(frames):
            before = np.asarray(host["voice_finished"]).copy()
            cpuref.render(host, gl, tables, 1, 0)
            for v in np.flatnonzero((np.asarray(host["voice_finished"]) != 0) & (before == 0)):
                flips.setdefault(int(v), []).append((L, f))
    return flips, silent


def _as_lf(segs, where):
    return (where[1], resolve(segs, where) - int(np.sum(segs[:where[1]])))


@pytest.mark.parametrize("name", NAMES)
def test_scenarios_hit_their_edges(name):
    """(CPU) The builders do what the GPU tests rely on: every planned one-shot finishes on its frame of its launch and no other
    one-shot flips elsewhere, the silenced voices are off in exactly the planned launches, and the waves vote for the frame-lag form
    (one level, every edge fitting) -- checked through cpuref alone, frame by frame."""
    bank, tables, g, segments, plan = scenario(name)
    segs = [f for f, _ in segments]
    flips, silent = _timeline(bank, tables, g, segments)
    for v, want in plan["finish"].items():
        want = want if isinstance(want, list) else [want]
        assert flips.get(v) == [_as_lf(segs, w) for w in want], (v, flips.get(v), want)
    shots = set(plan["finish"])
    if name != "fm_cut":
        assert set(flips) == shots, sorted(set(flips) ^ shots)
        ends = {lf for v in shots for lf in flips[v]}
        lasts = {(L, f - 1) for L, f in enumerate(segs)}
        assert len(ends & lasts) >= 5 and {(L, 0) for L in range(len(segs))} & ends     # launch ends and launch starts
        if name == "finish":
            assert {(5, 62), (5, 63), (5, 64), (5, 65), (5, 300)} <= ends
    assert name == "fm_cut" or segs == SEGS
    base = set(np.flatnonzero(np.asarray(bank["voice_amp"]) == 0).tolist())
    for L, s in enumerate(silent):
        assert s - base == set(plan["silenced"].get(L, [])), (L, sorted(s - base))
    lv = mod_forms.levels(bank)
    for c in copies("A"):
        assert list(lv[c:c + 8]) == [0, 0, 1, 0, 1, 1, 0, 1]
    for c in copies("B"):
        assert list(lv[c:c + 8]) == [0, 1, 1, 0, 1, 1, 0, 0]
    assert mod_forms.lag_groups(bank).all()
    assert mod_forms.expected_counts(bank, 64, 1) == [N_GROUPS, 0] and mod_forms.expected_counts(bank, 64, 0) == [0, N_GROUPS]


# ----------------------------------------------------------------------------------------------------- on the GPU

FORMS = {"lag": (1, 0, False), "loop": (0, 0, False), "lag_packed": (1, 2, False), "loop_packed": (0, 2, False), "loop_stems": (1, 0, True)}


@pytest.fixture(scope="module")
def dev():
    from skred_amd import device
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


def oracle_launches(bank, tables, g, segments):
    host, gl = bank.copy(), g.copy()
    out = []
    for frames, event in segments:
        if event is not None:
            event(host, gl.synth_sample_count)
        r = cpuref.render(host, gl, tables, frames, 0, want_stems=True)
        out.append((cpuref.master(gl, r["sum64"].astype(np.float32)), host.copy(), gl.copy(), r["stems"]))
    return out


def device_launches(dev, bank, tables, g, segments, form):
    """Every launch on a fresh device bank in `form`; after each one the whole state is downloaded (download leaves the device bank
    as it is).  Returns per launch (mix, state, globals, stems, last_kernel, last_pack, form counts)."""
    import torch
    skew, pack, stems = FORMS[form]
    db = dev.DeviceBank(bank.n)
    db.set_tables(tables)
    host = bank.copy()
    db.upload(host)
    db.set_globals(g)
    db.set_fm_skew(skew)
    db.set_pack(pack)
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    db.set_form_counter(counts.data_ptr())
    out = []
    for frames, event in segments:
        if event is not None:
            db.download(host)
            event(host, db.get_globals().synth_sample_count)
            db.upload(host)
        counts.zero_()
        torch.cuda.synchronize()
        mix, st = db.render_host(frames, 2, 0, want_stems=stems)
        kern, pk = db.last_kernel(), db.last_pack()
        torch.cuda.synchronize()
        c = counts.cpu().numpy().tolist()
        db.download(host)
        out.append((mix, host.copy(), db.get_globals(), st, kern, pk, c))
    db.set_form_counter(0)
    db.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_block_edges_against_the_oracle(dev, name):
    bank, tables, g, segments, _ = scenario(name)
    ref = oracle_launches(bank, tables, g, segments)
    mixes = {}
    for form in FORMS:
        skew, pack, stems = FORMS[form]
        got = device_launches(dev, bank, tables, g, segments, form)
        for L, ((frames, _), (mix, state, gl, st, kern, pk, counts), (rmix, rstate, rgl, rstems)) in enumerate(zip(segments, got, ref)):
            where = f"{name} {form} launch {L} ({frames} frames)"
            assert kern == 2, (where, kern)
            assert pk == (16 if pack else 0), (where, pk)
            bad = state.rw_equal(rstate)
            assert not bad, (where, bad)
            assert (gl.noise_rng, gl.synth_sample_count) == (rgl.noise_rng, rgl.synth_sample_count), where
            assert rel_rms(mix, rmix) <= 1e-5, where
            if stems:
                d = np.argwhere(st.view(np.uint32) != rstems.view(np.uint32))
                assert len(d) == 0, f"{where}: {len(d)} stem values differ, first (frame, voice, ch) {d[0]}"
            waves = N_GROUPS // 4 if pack else N_GROUPS            # packed: 16 lanes per group, four groups per wave
            lag = skew and not stems and frames >= 2
            assert counts == ([waves, 0] if lag else [0, waves]), (where, counts)
        mixes[form] = np.concatenate([m[0] for m in got])
    assert gio.bits_equal(mixes["lag"], mixes["loop"]), "frame-lag form and level loop: same products, same sums"
    assert gio.bits_equal(mixes["lag_packed"], mixes["loop_packed"])


@pytest.mark.gpu
def test_silent_named_voice_leaves_no_violation(dev):
    """A voice that cannot sound (amp 0) keeps a packed lane because a sounding voice names it, and itself names a voice that has no
    lane (kind B's v6 -> v7).  Its routing is never used, so nothing may count it as a pack violation: after packed modulated blocks,
    the bank re-uploaded without modulation renders on the two-voices-per-lane kernel with envelopes in motion -- the family that
    reads the violation word back -- and must find nothing."""
    import torch
    from skred_amd import device
    bank, tables, g, segments, _ = scenario("silence")
    db = dev.DeviceBank(bank.n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    db.set_pack(2)
    db.fast2_min_voices(0)
    out = torch.zeros(512, 2, device="cuda")
    for frames in (64, 65, 3):
        db.render_mix(frames, out.data_ptr(), 2, 0, 0)
        assert db.last_kernel() == 2 and db.last_pack() == 16
    torch.cuda.synchronize()
    plain = bank.copy()
    for f in ("voice_freq_mod_osc", "voice_amp_mod_osc", "voice_pan_mod_osc", "voice_cz_mod_osc"):
        plain[f] = -1
    plain["voice_one_shot"] = 0
    plain["voice_finished"] = 0
    plain["voice_wave_table_index"] = 200
    c2 = banks.RECIPES["c2"](bank.n)[0]                                     # ADSR envelopes, note-ons ahead of the clock: in motion
    plain["voice_use_amp_envelope"] = c2["voice_use_amp_envelope"]
    plain["voice_amp_envelope"] = c2["voice_amp_envelope"]
    now = db.get_globals().synth_sample_count
    plain["voice_amp_envelope"]["sample_start"][::3] = now + 40
    db.set_pack(0)
    db.upload(plain)
    before = device.load().skred_amd_last_error().decode(errors="replace")
    for _ in range(6):
        db.render_mix(512, out.data_ptr(), 2, 0, 0)
        assert db.last_kernel() == 3
        torch.cuda.synchronize()
    after = device.load().skred_amd_last_error().decode(errors="replace")
    assert db.list_violations() == 0
    assert "motion list" not in after or after == before, after
    db.close()
