"""Random clean banks of the two-per-lane family with MOVING envelopes, control actions and block lists for
tests/test_env_fuzz.py.  numpy only: nothing here renders, predicts or checks anything, and everything is drawn from the numpy
Generator that is passed in, so a seed names one case.

sk_render_env2_kernel picks its code per wave of 128 list entries and 64-frame chunk, and a wave's form is the worst of its
lanes, so the envelope REGIME is drawn per 64-voice group (neighbouring groups mostly share it), not per voice:
  long        attack / decay / release of 200 .. 20 000 frames: ramp and step chunks
  short       stages of 0.5 .. 40 frames, fractional: re-decision per 8 frames, general frames
  degenerate  a random subset of the three times is exactly 0, sustain_level is 0 or 1
  extreme     one stage time below 2^-40 or above 2^40: the ramp form must be refused
  old         sample_start so far back that count - start crosses 2^24 - 66 during the run, a release running meanwhile
  resting     sustain or inactive: on the list only through control actions
Stage edges are PLACED -- on frames 0, 7, 8, 63 of a chunk (64: frame 0 of the next) and on the first and last frame of a block --
for about half of the long voices (through sample_start / sample_release) and half of the short ones (through the stage times,
counted from the note-on: block 0 and every re-trigger); a placed start ahead of the clock would put the voice's whole wave on
integer clocks, so the other regimes meet edges through their draws and through the actions' times only.
"""
import numpy as np

from fuzz_banks import Action, spread
from skred_amd import banks

# SKRED_DIRTY_* / SKRED_STAMP_* of include/skred_amd.h
DIRTY_PARAMS, DIRTY_PHASE, DIRTY_ENV_STATE, STAMP_TRIGGER, STAMP_RELEASE, DIRTY_ENV_CLOCK = 1, 2, 4, 256, 512, 1024

SEEDS = tuple(range(8))             # seed bits: 0 recipe (c2 LDS tables / c4 table windows), 1 interpolation
SIZES = (1000, 1025, 2048, 3000)    # n < 1024; n = 1 (mod 128); n = 0 (mod 1024); n no multiple of 64; then random 1000 .. 6000
BLOCK_CHOICES = (1, 7, 8, 63, 64, 65, 128, 300, 512)
MAX_BLOCKS, MAX_FRAMES, MAX_VOICES = 12, 2500, 6000
COUNT0 = (1 << 25) + 12345          # the clock the banks are drawn for: room for notes older than 2^24 frames
CLOCK_LIMIT = (1 << 24) - 66        # skred_render_fast2.hip: x + 1.0f stays exact below this clock difference
REGIMES = ("long", "short", "degenerate", "extreme", "old", "resting")
REGIME_P = (0.32, 0.24, 0.12, 0.08, 0.04, 0.20)    # (one old voice puts its whole wave on integer clocks: a small share)
IN_PLACE_DENOM, IN_PLACE_SLACK = 6, 64      # skred_bank_plan.h: lists up to n / 6 + 64 voices are rendered in place


class Case:
    """recipe, n, interp, bank, tables, g (globals), blocks = [(frames, [Action, ...])] -- a block's actions run before its frames --
    and `info`: the plan inputs that matter (filter / envelope for all, none or some; table kind) and the regime of every group."""

    def __init__(self, **kw):
        self.seed = -1
        self.__dict__.update(kw)
        self.n = self.bank.n

    @property
    def frames(self):
        return sum(f for f, _ in self.blocks)

    @property
    def lds_tables(self):
        return self.recipe == "c2"


def block_lengths(rng):
    """Lengths from BLOCK_CHOICES plus one in 513 .. 700; never the same twice in a row; at most MAX_FRAMES in all."""
    pool = [512, 300, 128, 64, 65, 63, 8, 7, 1, int(rng.integers(513, 701)), 128, 64, 300]
    out, total = [], 0
    for f in rng.permutation(pool):
        f = int(f)
        if len(out) == MAX_BLOCKS or total + f > MAX_FRAMES or (out and out[-1] == f):
            continue
        out.append(f)
        total += f
    return out


def edge_frames(lengths):
    """Run-relative frames on which a stage edge is worth placing: frames 0, 7, 8, 63 of every chunk (64: frame 0 of the next)
    and the first and last frame of every block."""
    pts, o = set(), 0
    for f in lengths:
        for c0 in range(0, f, 64):
            pts.update(o + c0 + j for j in (0, 7, 8, 63) if c0 + j < f)
        pts.update((o, o + f - 1))
        o += f
    return np.array(sorted(pts), np.int64)


def _times(rng, m, lo, hi, fractional):
    t = np.exp(rng.uniform(np.log(lo), np.log(hi), m))
    return np.where(fractional, t, np.maximum(np.round(t), 1.0)).astype(np.float32)


def draw_regimes(rng, n, sparse=False):
    """The regime of every 64-voice group.  `sparse`: about a ninth of the groups move, in adjacent pairs, the regimes in turn --
    a motion list short enough for the in-place path (at most n / 6 + 64 voices); the others rest."""
    G = (n + 63) // 64
    if sparse:
        reg = np.full(G, REGIMES.index("resting"))
        moving = [i for i in rng.permutation(len(REGIMES)) if REGIMES[i] != "resting"]
        pairs = rng.permutation(G // 2)[:max(1, round(0.11 * G / 2))]
        for i, p in enumerate(pairs):
            reg[2 * p] = moving[(2 * i) % len(moving)]
            reg[2 * p + 1] = moving[(2 * i + 1) % len(moving)] if rng.random() < 0.5 else reg[2 * p]
        return reg
    per4 = rng.choice(len(REGIMES), (G + 3) // 4, p=REGIME_P)
    reg = np.repeat(per4, 4)[:G]
    own = rng.random(G) < 0.25
    reg[own] = rng.choice(len(REGIMES), int(own.sum()), p=REGIME_P)
    return reg


def draw_envelopes(rng, bank, reg, lengths):
    """Envelope times, clocks, velocity and smoother of every voice from its group's regime."""
    n = bank.n
    e = bank["voice_amp_envelope"]
    r = reg[np.arange(n) >> 6]
    total = int(sum(lengths))
    frac = rng.random(n) < 0.5
    a, d, rl = (_times(rng, n, 200.0, 20000.0, frac) for _ in range(3))
    sus = rng.uniform(0.1, 0.9, n).astype(np.float32)
    start = COUNT0 - (rng.random(n) * (a + d) * 1.3).astype(np.int64)            # attack, decay or sustain at the first frame
    released = rng.random(n) < 0.3
    release = np.where(released, COUNT0 - (rng.random(n) * rl * 1.1).astype(np.int64), 0)
    active = np.ones(n, np.int32)

    s = r == REGIMES.index("short")
    for t in (a, d, rl):
        t[s] = rng.uniform(0.5, 40.0, int(s.sum())).astype(np.float32)
    start[s] = COUNT0 - rng.integers(0, 60, int(s.sum()))
    release[s] = np.where(rng.random(int(s.sum())) < 0.3, COUNT0 - rng.integers(0, 30, int(s.sum())), 0)

    g = r == REGIMES.index("degenerate")
    for t in (a, d, rl):
        t[g & (rng.random(n) < 0.5)] = 0.0
        small = g & (rng.random(n) < 0.3)
        t[small] = rng.uniform(0.5, 40.0, int(small.sum())).astype(np.float32)
    sus[g] = rng.integers(0, 2, int(g.sum())).astype(np.float32)
    start[g] = np.where(rng.random(int(g.sum())) < 0.5, COUNT0 - rng.integers(0, 40, int(g.sum())), start[g])

    x = r == REGIMES.index("extreme")
    which = rng.integers(0, 3, n)
    tiny = rng.random(n) < 0.5
    val = np.where(tiny, np.exp2(-rng.integers(41, 60, n).astype(np.float64)), np.exp2(rng.integers(41, 60, n).astype(np.float64))).astype(np.float32)
    for i, t in enumerate((a, d, rl)):
        sel = x & (which == i)
        t[sel] = val[sel]
    start[x] = COUNT0 - rng.integers(0, 3000, int(x.sum()))

    o = r == REGIMES.index("old")
    cross = rng.integers(0, max(total, 1), n)                                     # the run frame on which the clock difference gets there
    start[o] = (COUNT0 + cross - CLOCK_LIMIT)[o]
    rl[o] = _times(rng, int(o.sum()), 3000.0, 20000.0, frac[o])
    release[o] = COUNT0 - rng.integers(1, 200, int(o.sum()))

    q = r == REGIMES.index("resting")
    start[q] = COUNT0 - rng.integers(1 << 20, 1 << 21, int(q.sum()))
    release[q] = 0
    active[q & (rng.random(n) < 0.3)] = 0
    few = q & np.repeat(rng.random((n + 255) // 256) < 0.6, 256)[:n]            # (whole aligned 256-voice runs: see _voices "run")
    for t in (a, d, rl):
        t[few] = rng.uniform(0.5, 25.0, int(few.sum())).astype(np.float32)

    # stage edges on chosen frames of chunks and blocks (long voices: the edge is the end of attack or decay, or of the release)
    edges = edge_frames(lengths)
    lg = (r == REGIMES.index("long")) & (rng.random(n) < 0.5)
    F = rng.choice(edges, n)
    attdec = (a + d).astype(np.float32)
    for limit, sel in ((a, lg & ~released & (rng.random(n) < 0.5)), (attdec, lg & ~released)):
        s0 = COUNT0 + F + 1 - np.ceil(limit.astype(np.float64)).astype(np.int64)   # first frame with t >= limit is run frame F
        ok = sel & (s0 <= COUNT0) & (s0 > 0)
        start[ok] = s0[ok]
        lg = lg & ~ok
    r0 = COUNT0 + F + 1 - np.ceil(rl.astype(np.float64)).astype(np.int64)
    ok = (r == REGIMES.index("long")) & released & (r0 <= COUNT0) & (r0 > 0) & (rng.random(n) < 0.6)
    release[ok] = r0[ok]
    start[ok] = np.minimum(start[ok], r0[ok] - (a + d)[ok].astype(np.int64) - 1)     # released from sustain

    # short voices (half of them): attack or decay ends on frame 0, 7, 8, 63 or 64 counted from the note-on -- the first chunk of
    # block 0 for these starts, and of any block a re-trigger precedes
    sh = s & (rng.random(n) < 0.5)
    j = rng.choice((0, 7, 8, 63, 64), n)
    u = rng.uniform(0.05, 0.95, n)
    early = sh & (j <= 8)
    a[early] = (j + 1 - u)[early].astype(np.float32)                                # first frame with t >= att: frame j
    late = sh & (j > 8)
    d[late] = np.maximum(j + 1 - u - a, 0.5)[late].astype(np.float32)              # ... with t >= att + dec: frame j
    start[sh] = COUNT0
    release[sh] = 0

    e["attack_time"], e["decay_time"], e["release_time"], e["sustain_level"] = a, d, rl, sus
    e["sample_start"] = np.maximum(start, 1).astype(np.uint64)
    e["sample_release"] = np.maximum(release, 0).astype(np.uint64)
    e["is_active"] = active
    e["velocity"] = rng.uniform(0.2, 1.2, n).astype(np.float32)
    bank["voice_smoother_smoothing"] = np.exp(rng.uniform(np.log(0.001), np.log(0.5), n)).astype(np.float32)
    bank["voice_smoother_gain"] = np.where(rng.random(n) < 0.5, 0.0, rng.random(n)).astype(np.float32)


def clean_bank(rng, recipe, n, lengths):
    """A bank of this family: filter for all / none / some, envelope for all / some, mutes and zero amps; nothing exotic."""
    bank, tables, g = banks.RECIPES[recipe](n)
    g.synth_sample_count = COUNT0
    v = np.arange(n)
    filt = str(rng.choice(("all", "none", "mixed")))
    env = str(rng.choice(("all", "all", "mixed")))
    if recipe == "c4":
        bank["voice_filter_mode"][:] = 1 + (v % 4)
        c = banks.biquad_coeffs(bank["voice_filter_mode"], 200.0 + 37.0 * (v % 150), np.full(n, 0.9, np.float32), 48000)
        for k in ("b0", "b1", "b2", "a1", "a2"):
            bank["voice_filter"][k] = c[k]
    if filt == "none":
        bank["voice_filter_mode"][:] = 0
    elif filt == "mixed":
        bank["voice_filter_mode"][rng.random(n) < 0.4] = 0
    reg = draw_regimes(rng, n, sparse=recipe == "c2")
    draw_envelopes(rng, bank, reg, lengths)
    if env == "mixed":
        bank["voice_use_amp_envelope"][rng.random(n) < 0.25] = 0
    bank["voice_amp"] = rng.uniform(0.2, 1.5, n).astype(np.float32)
    bank["voice_amp"][rng.random(n) < 0.05] = 0.0
    muted_group = (rng.random((n + 63) // 64) < 0.12)[v >> 6]          # (one muted live lane takes its whole wave off the block forms)
    bank["voice_disconnect"][muted_group & (rng.random(n) < 0.1)] = 1
    return bank, tables, g, {"filter": filt, "envelope": env, "recipe": recipe, "regimes": reg}


# ---------------------------------------------------------------- control actions

def _note_off(h, vs, now):                                       # amp_envelope_release, synth.c:391-395
    e = h["voice_amp_envelope"]
    act = e["is_active"][vs] != 0
    e["sample_release"][vs[act]] = now
    return vs, STAMP_RELEASE


def _retrigger(h, vs, now):                                      # osc_trigger + amp_envelope_trigger
    h["voice_finished"][vs] = 0
    h["voice_phase"][vs] = np.where(h["voice_loop_enabled"][vs] != 0, h["voice_loop_start_f"][vs], np.float32(0.0))
    e = h["voice_amp_envelope"]
    e["sample_start"][vs] = now
    e["sample_release"][vs] = 0
    e["is_active"][vs] = 1
    return vs, DIRTY_PHASE | STAMP_TRIGGER


def _note_ahead(ahead):
    def fn(h, vs, now):                                          # a note-on `ahead` frames in front of the clock (synth.c:401)
        e = h["voice_amp_envelope"]
        e["sample_start"][vs] = now + np.asarray(ahead, np.uint64)
        e["sample_release"][vs] = 0
        e["is_active"][vs] = 1
        return vs, DIRTY_ENV_CLOCK | DIRTY_ENV_STATE
    return fn


def _set(field, value):
    def fn(h, vs, now):
        h[field][vs] = value
        return vs, DIRTY_PARAMS
    return fn


def _voices(rng, n, reg, kind):
    """Voice sets: a sparse random one, one 64-voice word, 44 consecutive voices of one 128-voice wave, 9 of one word, or more
    than the in-place path takes."""
    G = (n + 63) // 64
    if kind == "sparse":
        k = int(max(3, rng.integers(n // 200 + 1, n // 40 + 2)))
        return np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
    if kind == "word":
        g = int(rng.integers(0, G))
        return np.arange(g * 64, min(g * 64 + 64, n), dtype=np.int32)
    if kind == "wave44":
        w = int(rng.integers(0, max(1, n // 128)))
        o = int(rng.integers(0, 128 - 44 + 1))
        return np.arange(w * 128 + o, min(w * 128 + o + 44, n), dtype=np.int32)
    if kind == "word9":
        g = int(rng.integers(0, max(1, n // 64)))
        return (g * 64 + np.sort(rng.choice(64, 9, replace=False))).astype(np.int32)
    if kind == "run":                                             # 256 consecutive resting voices: at least one whole wave of the list
        rest = [b for b in range(n // 256) if (reg[4 * b:4 * b + 4] == REGIMES.index("resting")).all()]
        b = int(rng.choice(rest)) if rest else int(rng.integers(0, max(1, n // 256)))
        return np.arange(b * 256, min(b * 256 + 256, n), dtype=np.int32)
    if kind == "beyond":
        k = min(n, n // IN_PLACE_DENOM + IN_PLACE_SLACK + int(rng.integers(1, 200)))
        return np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
    raise ValueError(kind)


def draw_actions(rng, n, reg, lengths):
    """The actions of one case, dealt to the gaps between its blocks: every kind and every burst once, then repeats."""
    nb = len(lengths)
    kinds = ["note_off", "retrigger", "ahead_chunk", "ahead_edge", "ahead_far", "amp", "mute", "note_off", "retrigger"]
    # (a note-on ahead of the clock puts its wave on integer clocks until it lands: those go to whole words, not all over the list)
    sets = ["sparse", "word", "word", "word9", "word", "sparse", "word9", "wave44", "sparse"]
    acts, undo = [], []
    order = rng.permutation(len(kinds))
    for rep in range(2):
        for i in order:
            kind, vs = kinds[i], _voices(rng, n, reg, sets[i] if rep == 0 else str(rng.choice(("sparse", "word", "word9"))))
            if kind == "note_off":
                acts.append(Action(kind, vs, _note_off))
            elif kind == "retrigger":
                acts.append(Action(kind, vs, _retrigger))
            elif kind == "ahead_chunk":                          # lands inside a chunk
                acts.append(Action(kind, vs, _note_ahead(rng.integers(1, 64, len(vs)))))
            elif kind == "ahead_edge":                           # lands on a chunk edge of the block that follows
                acts.append(Action(kind, vs, _note_ahead(64 * rng.integers(1, 4, len(vs)))))
            elif kind == "ahead_far":                            # lands beyond the block
                acts.append(Action(kind, vs, _note_ahead(rng.integers(300, 701, len(vs)))))
            elif kind == "amp":                                  # no envelope effect: the voice is listed and only settles
                acts.append(Action(kind, vs, _set("voice_amp", rng.uniform(0.2, 1.5, len(vs)).astype(np.float32))))
            elif kind == "mute":
                m = Action("mute", vs, _set("voice_disconnect", np.int32(1)))
                acts.append(m)
                undo.append((m, Action("unmute", vs, _set("voice_disconnect", np.int32(0)))))
    for kind, fn in (("retrigger", _retrigger), ("amp", None), ("retrigger", _retrigger), ("note_off", _note_off), ("retrigger", _retrigger)):
        vs = _voices(rng, n, reg, "run")
        fn = fn or _set("voice_amp", rng.uniform(0.2, 1.5, len(vs)).astype(np.float32))
        acts.insert(int(rng.integers(0, len(acts) + 1)), Action(kind, vs, fn))
    acts.insert(int(rng.integers(len(acts) // 3, len(acts))), Action("burst_beyond", _voices(rng, n, reg, "beyond"), _retrigger if rng.random() < 0.5 else _note_off))
    for m, u in undo:
        i = [k for k, a in enumerate(acts) if a is m][0]
        acts.insert(int(rng.integers(i + 1, len(acts) + 1)), u)
    return spread(rng, acts, nb)


def case(seed):
    rng = np.random.default_rng(7000 + seed)
    recipe, interp = ("c2", "c4")[seed & 1], (seed >> 1) & 1
    n = SIZES[seed] if seed < len(SIZES) else int(rng.integers(3000 if recipe == "c2" else 1000, MAX_VOICES + 1))
    lengths = block_lengths(rng)
    bank, tables, g, info = clean_bank(rng, recipe, n, lengths)
    acts = draw_actions(rng, n, info["regimes"], lengths)
    return Case(seed=seed, recipe=recipe, interp=interp, bank=bank, tables=tables, g=g, blocks=list(zip(lengths, acts)), info=info)


# ---------------------------------------------------------------- pinned edges (deterministic, n <= 2048, at most 6 blocks)

def _resting(n=1024, recipe="c2"):
    """Every voice held in sustain since long ago: nothing moves until a test says so."""
    bank, tables, g = banks.RECIPES[recipe](n)
    g.synth_sample_count = COUNT0
    e = bank["voice_amp_envelope"]
    e["sample_start"] = np.uint64(COUNT0 - (1 << 20))
    e["sample_release"] = 0
    e["is_active"] = 1
    bank["voice_smoother_gain"] = (bank["voice_amp"] * (e["sustain_level"] * e["velocity"])).astype(np.float32)
    return bank, tables, g


def _pinned_case(name, bank, tables, g, blocks, recipe="c2", interp=0):
    return Case(seed=name, recipe=recipe, interp=interp, bank=bank, tables=tables, g=g, blocks=blocks,
                info={"filter": "all", "envelope": "all", "recipe": recipe, "regimes": None})


def pinned(name):
    """The deterministic cases of test_env_fuzz.py, by name."""
    bank, tables, g = _resting()
    e = bank["voice_amp_envelope"]
    n = bank.n
    vs = np.arange(128, 256)                                      # one whole wave of the list
    if name.startswith("edge_on_frame_"):                         # the attack of a whole wave ends exactly on frame J of the second chunk
        J = int(name.rsplit("_", 1)[1])
        e["attack_time"][vs], e["decay_time"][vs] = 300.0, 1000.0
        e["sample_start"][vs] = np.uint64(COUNT0 + 64 + J + 1 - 300)
        return _pinned_case(name, bank, tables, g, [(192, []), (128, [])])
    if name == "no_decay":                                        # attack -> sustain with decay_time == 0
        e["attack_time"][vs], e["decay_time"][vs] = 100.0, 0.0
        e["sample_start"][vs] = np.uint64(COUNT0 - 60)
        return _pinned_case(name, bank, tables, g, [(128, []), (64, [])])
    if name == "release_on_attack_end":                           # the release is stamped on the frame the attack ends
        e["attack_time"][vs], e["decay_time"][vs], e["release_time"][vs] = 64.0, 200.0, 150.0
        e["sample_start"][vs] = np.uint64(COUNT0)
        return _pinned_case(name, bank, tables, g, [(63, []), (128, [Action("note_off", vs.astype(np.int32), _note_off)]), (128, [])])
    if name == "release_ends_on_block_edge":                      # one release ends on a block's last frame, one on the next block's first
        a, b = vs[:64], vs[64:]
        e["release_time"][vs] = 500.0
        e["sample_release"][a] = np.uint64(COUNT0 + 128 - 500)    # t_release reaches 500 on frame 127 of block 0
        e["sample_release"][b] = np.uint64(COUNT0 + 129 - 500)    # ... on frame 0 of block 1
        return _pinned_case(name, bank, tables, g, [(128, []), (128, []), (64, [])])
    if name == "note_on_frame_63":                                # a note-on that lands on frame 63 of a 64-frame block
        return _pinned_case(name, bank, tables, g, [(64, []), (64, [Action("ahead", vs.astype(np.int32), _note_ahead(np.full(128, 64)))]), (64, []), (128, [])])
    if name == "clock_crosses_mid_block":                         # count - start crosses 2^24 - 66 on frame 100 with a release running
        e["sample_start"][vs] = np.uint64(COUNT0 + 100 - CLOCK_LIMIT)
        e["release_time"][vs] = 5000.0
        e["sample_release"][vs] = np.uint64(COUNT0 - 77)
        return _pinned_case(name, bank, tables, g, [(256, []), (128, [])])
    if name == "stage_times_2_41":
        # Stage times of 2^-41 and 2^41.  Only the 2^41 decay is ever a current stage's denominator (the upper bound of the
        # `same` / `ok` range): with t >= 1 > 2^-41 the tiny attack is never entered and the tiny release is over on its first
        # frame, so the LOWER bound cannot be reached on float clocks (t == 0 needs a note-on ahead: integer clocks anyway).
        # The tiny times are still rendered: attack skipped, release finished at once.
        a, b = vs[:64], vs[64:]
        e["attack_time"][a], e["release_time"][a] = 2.0 ** -41, 2.0 ** -41
        e["decay_time"][b] = 2.0 ** 41
        e["attack_time"][b] = 10.0
        e["sample_start"][vs] = np.uint64(COUNT0 - 3)
        rel = Action("note_off", a.astype(np.int32), _note_off)
        return _pinned_case(name, bank, tables, g, [(128, []), (128, [rel]), (64, [])])
    if name == "block_of_65":                                     # one full chunk and a one-frame ragged one
        e["attack_time"][vs], e["decay_time"][vs] = 30.0, 30.0
        e["sample_start"][vs] = np.uint64(COUNT0 - 10)
        return _pinned_case(name, bank, tables, g, [(65, []), (65, []), (64, [])])
    if name == "wave_of_33":                                      # 33 listed voices in one 128-voice wave, in place
        hit = np.arange(256, 256 + 33, dtype=np.int32)
        return _pinned_case(name, bank, tables, g, [(128, []), (128, [Action("retrigger", hit[:3], _retrigger)]),
                                                     (128, [Action("retrigger", hit, _retrigger)]), (128, []), (65, [])])
    if name == "word_of_9":                                       # 9 listed voices in one 64-voice word, in place
        hit = (320 + 7 * np.arange(9)).astype(np.int32)
        return _pinned_case(name, bank, tables, g, [(128, []), (128, [Action("note_off", hit[:2], _note_off)]),
                                                     (128, [Action("retrigger", hit, _retrigger)]), (128, []), (65, [])])
    raise ValueError(name)


PINNED = ("edge_on_frame_0", "edge_on_frame_8", "edge_on_frame_64", "no_decay", "release_on_attack_end", "release_ends_on_block_edge",
          "note_on_frame_63", "clock_crosses_mid_block", "stage_times_2_41", "block_of_65", "wave_of_33", "word_of_9")
