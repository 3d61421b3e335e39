"""Random fixed-point banks, pools, clocks and segment lists for tests/test_fx_fuzz.py.  numpy only: nothing here renders,
predicts or checks anything, and everything is drawn from one numpy Generator, so a seed names one case.

sk_fx_render_kernel chooses its code per aligned 64-voice wave, so the generator draws a CLASS per wave and then, for some
waves, replaces one or two lanes (lane 0, lane 63 or a random one) by a voice of another class: one lane decides for 64.

The draws stay inside what include/skred_amd_fxpt.h promises ("every other product is an int32 one"): gains, velocity and
smoother state non-negative, velocity <= 65535, filter state inside +-2^29, and no int32 product of the definition leaving the
int32 range.  tests/fx_model.py counts such products; test_fx_fuzz.py asserts that every case has none.
"""
import numpy as np

from skred_amd import banks
from skred_amd.fxbank import FxVoiceBank

N_CHOICES = (1, 63, 64, 65, 255, 256, 257, 700, 1537)
SEG_CHOICES = (1, 7, 8, 9, 63, 64, 65, 71, 128, 200, 513)
MAX_FRAMES = 1500
BIG_N = 64 * 256 + 1            # one voice beyond 64 workgroups: the two-level mix-down of skx_finish_block
SEEDS = tuple(range(36))        # seed bits: 0 interpolation, 1 pool form, then the index into N_CHOICES
BIG_SEEDS = (1000, 1001)
# share of (voice, segment) pairs that may be inert -- amp 0 or finished when the segment starts -- over the whole seed set
INERT_CAP = 0.30

CLASSES = ("noenv", "held", "moving", "released", "inactive", "amp0", "disconnected", "finished", "oneshot")
WEIGHTS = (0.17, 0.22, 0.16, 0.10, 0.06, 0.05, 0.06, 0.05, 0.13)
ENV_LENGTHS = (0, 1, 2, "small", "thousands")
SUSTAINS = (0, 16384, 32768)
SMOOTHER_K = (1, 655, 32767, 32768)
LDS_ENTRIES = 49152 // 2


class Case:
    """bank, pool, count0, interp, master0 = (target, k, gain), patch (the bank windowed uploads read from) and
    segments = [(frames, [action, ...])]; the actions of a segment run before its frames:
      ("stamp", voices int32[], which)      ("upload", src_first, dst_first, count)      ("download", src_first, dst_first, count)
      ("master", target_q31, k_q15, gain_q31)      ("count", synth_sample_count)"""

    def __init__(self, **kw):
        self.patch, self.master0, self.seed = None, None, -1
        self.__dict__.update(kw)
        self.n = self.bank.n

    @property
    def frames(self):
        return sum(f for f, _ in self.segments)


def _env_len(rng, m):
    kind = rng.integers(0, len(ENV_LENGTHS), m)
    out = np.where(kind <= 2, kind, np.where(kind == 3, rng.integers(3, 100, m), rng.integers(1000, 5000, m)))
    return out.astype(np.int64)


def edge_points(segments):
    """Frame offsets where a launch or one of its 64-frame chunks begins or ends."""
    pts, o = set(), 0
    for f, _ in segments:
        pts.update(range(o, o + f, 64))
        o += f
        pts.add(o)
    return np.array(sorted(pts), np.int64)


def _near_edge(rng, ctx, m):
    return ctx["count0"] + rng.choice(ctx["edges"], m) + rng.integers(-1, 2, m)


def coeffs(rng, kind, m, high_pass=True):
    """Q2.30 RBJ coefficients: "gentle" (Q 0.5..0.9; low-pass: never near the rail; high-pass: a full-scale noise table can
    touch it now and then) or "resonant" (low-pass, Q 40..80 at 100..600 Hz: rides the rail)."""
    if kind == "gentle":
        mode, f, q = rng.integers(1, 3 if high_pass else 2, m), rng.uniform(200.0, 8000.0, m), rng.uniform(0.5, 0.9, m)
    else:
        mode, f, q = np.ones(m, np.int64), rng.uniform(100.0, 600.0, m), rng.uniform(40.0, 80.0, m)
    co = banks.biquad_coeffs(mode, f.astype(np.float32), q.astype(np.float32), 48000)
    return {k + "_q30": np.clip(np.round(co[k].astype(np.float64) * (1 << 30)), -(1 << 31), (1 << 31) - 1).astype(np.int32)
            for k in ("b0", "b1", "b2", "a1", "a2")}


def one_shot_ending_at(rng, frame, m=1):
    """(phase, phase_inc) of a one-shot whose add carries first in the 0-based frame `frame` (counted from the phase given)."""
    frame = np.broadcast_to(np.asarray(frame, np.int64), (m,))
    inc = np.maximum(1, (rng.random(m) * ((1 << 32) // (frame + 1))).astype(np.int64))
    phase = (1 << 32) - inc * (frame + 1) + (rng.random(m) * inc).astype(np.int64)
    return np.clip(phase, 0, (1 << 32) - 1).astype(np.uint32), inc.astype(np.uint32)


def draw_wave(rng, cls, ctx, m=64):
    """m voices of class `cls` as an FxVoiceBank."""
    b = FxVoiceBank(m)
    a, count0, entries = b.a, ctx["count0"], ctx["entries"]
    lmax = min(15, int(np.log2(entries)))
    L = rng.integers(3, lmax + 1, m)
    size = (1 << L).astype(np.int64)
    off = (rng.random(m) * (entries - size + 1)).astype(np.int64)
    off = np.where(rng.random(m) < 0.2, entries - size, off)                 # flush against the pool's end
    a["log2_size"][:], a["table_offset"][:] = L, off
    a["phase"][:] = rng.integers(0, 1 << 32, m, dtype=np.uint64)
    slow = (1 << 32) // rng.integers(20, 2000, m)
    a["phase_inc"][:] = np.where(rng.random(m) < 0.3, rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.int64), slow)
    a["amp_q15"][:] = np.where(rng.random(m) < 0.5, 32768, rng.integers(1, 65536, m))
    a["pan_left_q15"][:] = np.where(rng.random(m) < 0.1, 0, rng.integers(0, 32769, m))
    a["pan_right_q15"][:] = rng.integers(0, 32769, m)
    a["velocity_q15"][:] = np.where(rng.random(m) < 0.5, 32768, rng.integers(0, 32769, m))
    A, D, R = _env_len(rng, m), _env_len(rng, m), _env_len(rng, m)
    S = rng.choice(SUSTAINS, m)
    a["attack_frames"][:], a["decay_frames"][:], a["release_frames"][:], a["sustain_q15"][:] = A, D, R, S
    a["use_envelope"][:], a["is_active"][:] = 1, 1
    past_decay = count0 + 1 - (A + D) - rng.choice((0, 1, 1000), m)         # t >= A + D from the first frame on
    if ctx["ancient"]:
        past_decay = np.where(rng.random(m) < 0.5, rng.integers(1, 1000, m), past_decay)   # t saturates: > 2^32 frames ago
    a["sample_start"][:] = past_decay
    target = (a["amp_q15"].astype(np.int64) * ((S * a["velocity_q15"].astype(np.int64)) >> 15)) >> 15
    if cls == "noenv":
        a["use_envelope"][:] = 0
        target = a["amp_q15"].astype(np.int64)
    elif cls == "held":
        pass
    elif cls == "moving":                        # in attack or decay, or starting at / around a launch or chunk edge
        on_edge = rng.random(m) < 0.5
        a["sample_start"][:] = np.where(on_edge, _near_edge(rng, ctx, m), count0 - (rng.random(m) * (A + D + 1)).astype(np.int64))
    elif cls == "released":                      # the release starts before or inside the case and mostly ends inside it
        on_edge = rng.random(m) < 0.6
        a["sample_release"][:] = np.where(on_edge, _near_edge(rng, ctx, m), count0 - (rng.random(m) * (R + 1)).astype(np.int64))
    elif cls == "inactive":
        a["is_active"][:] = 0
        target[:] = 0
    elif cls == "amp0":
        a["amp_q15"][:] = 0
    elif cls == "disconnected":
        a["disconnect"][:] = 1
        a["use_envelope"][:] = rng.integers(0, 2, m)
        target = np.where(a["use_envelope"] != 0, target, a["amp_q15"].astype(np.int64))
    elif cls == "finished":
        a["one_shot"][:], a["finished"][:], a["phase"][:] = 1, 1, 0xFFFFFFFF
    elif cls == "oneshot":                       # periods from 2 frames to never; half of them end at / around an edge
        a["one_shot"][:] = 1
        a["use_envelope"][:] = rng.integers(0, 2, m)
        kind = rng.integers(0, 6, m)
        end = np.maximum(0, rng.choice(ctx["edges"], m) + rng.integers(-1, 2, m))
        ph, inc = one_shot_ending_at(rng, end, m)
        period = np.select([kind == 3, kind == 4], [2, rng.integers(3, 70, m)], rng.integers(70, 3000, m))
        free_inc = np.where(kind == 5, 0, -(-(1 << 32) // period))
        a["phase_inc"][:] = np.where(kind <= 2, inc.astype(np.int64), np.minimum(free_inc, (1 << 32) - 1))
        a["phase"][:] = np.where(kind <= 2, ph, a["phase"])
    else:
        raise ValueError(cls)
    # the smoother: off, at rest, one LSB either side of its target, or far from it
    sk = ctx["smoother"] if ctx["smoother"] != "mixed" else rng.choice(("off", "rest", "plus", "minus", "far"), m)
    sk = np.broadcast_to(np.asarray(sk), (m,))
    a["smoother_enable"][:] = sk != "off"
    a["smoother_k_q15"][:] = np.where(rng.random(m) < 0.7, rng.choice(SMOOTHER_K, m), rng.integers(0, 32769, m))
    sg = np.select([sk == "rest", sk == "plus", sk == "minus", sk == "far"],
                   [target, target + 1, np.maximum(target - 1, 0), rng.integers(0, 65536, m)], rng.integers(0, 65536, m))
    a["smoother_gain_q15"][:] = sg
    # the biquad
    fk = ctx["filter"] if ctx["filter"] != "mixed" else rng.choice(("none", "none", "gentle", "gentle", "resonant"), m)
    fk = np.broadcast_to(np.asarray(fk), (m,))
    gentle, res = coeffs(rng, "gentle", m), coeffs(rng, "resonant", m)
    for k in gentle:
        a[k][:] = np.where(fk == "resonant", res[k], gentle[k])
    a["filter_mode"][:] = np.where(fk == "none", 0, rng.integers(1, 5, m))
    for k in ("x1", "x2", "y1", "y2"):           # unfiltered voices carry a delay line too: it must survive
        a[k][:] = rng.integers(-(1 << 27), 1 << 27, m)
    at_rail = (fk == "resonant") & (rng.random(m) < 0.5)
    a["y1"][:] = np.where(at_rail, (1 << 29) - 1, a["y1"])
    a["y2"][:] = np.where(at_rail, -(1 << 29), a["y2"])
    # wide parameters (tests/test_fxpt.py: test_fx_wide_parameters_bit_exact), scaled so that v * pan stays an int32 product
    if ctx["wide"]:
        kind = rng.integers(0, 3)
        if kind == 0:                            # a gain beyond 16 bits, a smoother state of 2^20
            a["velocity_q15"][:], a["amp_q15"][:] = 60000, np.where(a["amp_q15"] != 0, 65535, 0)
            a["pan_left_q15"][:], a["pan_right_q15"][:] = 1024, 512
            a["smoother_gain_q15"][:], a["smoother_k_q15"][:] = 1 << 20, 655
        elif kind == 1:                          # a pan gain beyond 24 bits on a quiet voice
            a["amp_q15"][:] = np.where(a["amp_q15"] != 0, 100, 0)
            a["pan_left_q15"][:] = 9_000_000
            a["smoother_gain_q15"][:] = np.minimum(a["smoother_gain_q15"], 100)
        elif cls in ("noenv", "held"):           # k above 1.0: the smoother overshoots its (constant) target, never below 0
            a["smoother_k_q15"][:] = 40000
            a["amp_q15"][:] = np.minimum(a["amp_q15"], 32768)
            a["smoother_gain_q15"][:] = (rng.random(m) * (np.minimum(target, 32768) + 1)).astype(np.int64)
    return b


def draw_bank(rng, n, ctx):
    """n voices, a class per aligned 64-voice wave, some waves with one or two foreign lanes."""
    b = FxVoiceBank(n)
    for w0 in range(0, n, 64):
        ctx["smoother"] = rng.choice(("off", "rest", "rest", "plus", "minus", "far", "far", "mixed"))
        ctx["filter"] = rng.choice(("none", "gentle", "gentle", "resonant", "mixed")) if ctx["filters"] else "none"
        ctx["wide"] = rng.random() < 0.3
        cls = rng.choice(CLASSES, p=WEIGHTS)
        wave = draw_wave(rng, cls, ctx)
        if rng.random() < 0.5:
            ctx["wide"] = False
            other = draw_wave(rng, rng.choice(CLASSES, p=WEIGHTS), ctx)
            lanes = rng.choice((0, 63, int(rng.integers(0, 64))), rng.integers(1, 3), replace=False)
            for k in wave.a:
                wave.a[k][lanes] = other.a[k][lanes]
        m = min(64, n - w0)
        for k in b.a:
            b.a[k][w0:w0 + m] = wave.a[k][:m]
    return b


def draw_pool(rng, in_lds):
    """int16 entries: full-scale noise (both rails of int16 included), then a quiet stretch, then noise again."""
    entries = int(rng.choice((4099, 9000, LDS_ENTRIES - 3, LDS_ENTRIES)) if in_lds else rng.choice((LDS_ENTRIES + 1, 40000, 70001)))
    pool = rng.integers(-32768, 32768, entries).astype(np.int16)
    pool[entries // 3: entries // 2] = rng.integers(-2000, 2000, entries // 2 - entries // 3)
    pool[:4] = (-32768, 32767, -32768, 32767)
    return pool


def draw_segments(rng, n, budget):
    segs, total = [], 0
    for _ in range(int(rng.integers(2, 9))):
        f = int(rng.choice(SEG_CHOICES))
        if total + f > budget:
            continue
        segs.append(f)
        total += f
    return segs or [8]


def draw_actions(rng, n):
    acts = []
    for _ in range(int(rng.integers(0, 4))):
        kind = rng.choice(("stamp", "stamp", "upload", "download", "master"))
        if kind == "stamp":
            v = rng.integers(0, n, int(rng.integers(1, 40))).astype(np.int32)
            v = np.concatenate([v, v[:2]])                                   # duplicates in one list
            acts.append(("stamp", v, int(rng.integers(1, 4))))
        elif kind == "master":
            acts.append(("master", int(rng.choice((0, (1 << 31) - 1, int(rng.integers(0, 1 << 31))))),
                         int(rng.choice((0, 66, 32768, int(rng.integers(0, 32769))))), int(rng.integers(0, 1 << 31))))
        else:
            cnt = int(rng.integers(1, min(n, 300) + 1))
            acts.append((kind, int(rng.integers(0, n - cnt + 1)), int(rng.integers(0, n - cnt + 1)), cnt))
    return acts


def case(seed, big=False):
    rng = np.random.default_rng(seed)
    interp, in_lds = seed & 1, not (seed >> 1) & 1
    n = BIG_N if big else N_CHOICES[(seed >> 2) % len(N_CHOICES)]
    pool = draw_pool(rng, in_lds)
    clock = rng.integers(0, 8)
    frames = draw_segments(rng, n, 200 if big else int(rng.choice((300, 800, MAX_FRAMES))))
    total = sum(frames)
    count0 = int(rng.integers(20000, 200000))
    if clock == 0:
        count0 = (1 << 32) - int(rng.integers(1, total + 1))                 # the low word wraps inside the case
    ancient = clock == 1
    if ancient:
        count0 = (1 << 33) + int(rng.integers(0, 100000))
    segments = [(f, draw_actions(rng, n) if i else []) for i, f in enumerate(frames)]
    ctx = {"count0": count0, "entries": len(pool), "edges": edge_points(segments), "ancient": ancient,
           "filters": bool(rng.random() < 0.75)}
    bank = draw_bank(rng, n, ctx)
    patch = draw_bank(rng, n, ctx)
    master0 = (int(rng.integers(0, 1 << 31)), int(rng.choice((66, 655, 32768))), int(rng.integers(0, 1 << 31)))
    return Case(seed=seed, bank=bank, pool=pool, count0=count0, interp=interp, segments=segments, patch=patch, master0=master0)

