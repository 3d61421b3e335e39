"""A second statement of the fixed-point definition (include/skred_amd_fxpt.h), vectorised over the voices in numpy.

Written from the header's "Arithmetic" block, not from oracle/cpu_ref_fxpt.c: tests/test_fx_fuzz.py holds the two against each
other bit for bit, so a slip in either shows.  Every value is an int64 array; wherever the definition's type is int32 the value
is wrapped to int32 explicitly (`wrap32`), and a product the definition forms in int32 is checked first: one that leaves the
int32 range is signed overflow in C, where the scalar definition defines nothing.  `Report.overflow` names such products
(the generator of fx_fuzz.py must cause none).

`Report.paths` is coverage accounting only: per launch, per aligned 64-voice wave and per 64-frame chunk, the code path
sk_fx_render_kernel is expected to take -- the kernel's own predicates restated on this model's state at the chunk's first
frame.  No expected value ever comes from it.
"""
import numpy as np

M32 = (1 << 32) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
CHUNK = 64                       # SKX_CHUNK
LDS_TABLE_MAX_BYTES = 49152      # SKX_LDS_TABLE_MAX_BYTES
RAIL = 1 << 29

FRAME, BLOCK, LEAN = "frame", "block", "lean"


def wrap32(x):
    return ((x + (1 << 31)) & M32) - (1 << 31)


def pool_in_lds(n_entries: int) -> bool:
    """The pool's form: its bytes, padded to 16, fit the workgroup's LDS share."""
    return ((n_entries * 2 + 15) & ~15) <= LDS_TABLE_MAX_BYTES


class Path(tuple):
    """(wave, chunk, form, narrow, stalled, rollback, any_filter, lds); narrow / stalled are None for a per-frame chunk."""
    __slots__ = ()
    wave = property(lambda s: s[0])
    chunk = property(lambda s: s[1])
    form = property(lambda s: s[2])
    narrow = property(lambda s: s[3])
    stalled = property(lambda s: s[4])
    rollback = property(lambda s: s[5])
    any_filter = property(lambda s: s[6])
    lds = property(lambda s: s[7])

    def __str__(self):
        if self.form == FRAME:
            kind = "per-frame"
        else:
            kind = "%s %s %s%s" % ("lean blocks" if self.form == LEAN else "spelled-out blocks", "narrow" if self.narrow else "wide",
                                   "stalled" if self.stalled else "moving", ", rolls a block back" if self.rollback else "")
        return "wave %d chunk %d: %s; filter %s bank-wide, pool in %s" % (self.wave, self.chunk, kind, "on" if self.any_filter else "off",
                                                                        "LDS" if self.lds else "memory")


class Report:
    def __init__(self):
        self.overflow = {}           # name of the int32 product -> how many times it left the int32 range
        self.paths = []              # one list of Path per render() call

    def check(self, name, value, where):
        bad = where & ((value > I32_MAX) | (value < I32_MIN))
        if bad.any():
            self.overflow[name] = self.overflow.get(name, 0) + int(bad.sum())


def _waves(x, n, fill):
    pad = (-n) % 64
    if pad:
        x = np.concatenate([x, np.full(pad, fill, x.dtype)])
    return x.reshape(-1, 64)


def render(bank, pool, count, frames, interp, want_stems=False, report=None, any_filter=None):
    """`frames` frames of the definition on `bank` (advanced in place).  Returns (mix int64 [F][2], stems int32 [F][n][2] | None,
    new count).  any_filter: what the device bank believes (some voice ever uploaded runs the biquad); default: this bank's."""
    rep = report if report is not None else Report()
    a, n = bank.a, bank.n
    i64 = lambda k: a[k].astype(np.int64)
    ph, inc, toff, L = i64("phase"), i64("phase_inc"), i64("table_offset"), i64("log2_size")
    amp, panl, panr = i64("amp_q15"), i64("pan_left_q15"), i64("pan_right_q15")
    disc, uenv = i64("disconnect"), i64("use_envelope")
    A, D, R = i64("attack_frames"), i64("decay_frames"), i64("release_frames")
    S, vel = i64("sustain_q15"), i64("velocity_q15")
    start, rel = a["sample_start"].astype(np.uint64), a["sample_release"].astype(np.uint64)
    active, smooth, k, sg = i64("is_active"), i64("smoother_enable"), i64("smoother_k_q15"), i64("smoother_gain_q15")
    vs, one, fin, fmode = i64("voice_sample"), i64("one_shot"), i64("finished"), i64("filter_mode")
    b0, b1, b2, a1, a2 = i64("b0_q30"), i64("b1_q30"), i64("b2_q30"), i64("a1_q30"), i64("a2_q30")
    x1, x2, y1, y2 = i64("x1"), i64("x2"), i64("y1"), i64("y2")
    pool64 = np.asarray(pool).astype(np.int64)
    mask = (1 << L) - 1
    recip = lambda x: np.where(x > 0, (1 << 32) // np.maximum(x, 1), 0).astype(np.uint64)
    rA, rD, rR = recip(A), recip(D), recip(R)
    u64 = lambda x: x.astype(np.uint64)
    mix = np.zeros((frames, 2), np.int64)
    stems = np.zeros((frames, n, 2), np.int32) if want_stems else None

    # ---- path accounting: launch-constant predicates
    lds = pool_in_lds(len(pool64))
    anyf = bool((fmode != 0).any()) if any_filter is None else bool(any_filter)
    dead0 = (amp == 0) | (fin != 0)
    fits24 = lambda x: (x >= -(1 << 23)) & (x < (1 << 23))
    w_dead0 = _waves(dead0, n, True)
    narrow_l = (w_dead0 | _waves(fits24(panl) & fits24(panr) & (k >= 0) & (k <= 32768) & (np.abs(sg) <= 65535), n, True)).all(1)
    lean_ok = (w_dead0 | _waves((fmode == 0) | ((a1 != I32_MIN) & (a2 != I32_MIN)), n, True)).all(1) & lds
    paths, open_chunk, railed = [], None, None

    def close_chunk():
        for w, (form, narrow, stalled) in enumerate(open_chunk[1]):
            paths.append(Path((w, open_chunk[0], form, narrow, stalled, bool(form == LEAN and railed[w]), anyf, lds)))

    for i in range(frames):
        if i % CHUNK == 0:
            if open_chunk is not None:
                close_chunk()
            cn = min(CHUNK, frames - i)
            first = np.uint64((count + i + 1) & ((1 << 64) - 1))
            t_first = np.minimum(first - start, np.uint64(M32)).astype(np.int64)
            held = (rel == 0) & (t_first >= A + D) & (start <= first)
            steady = (w_dead0 | _waves((uenv == 0) | (active == 0) | held, n, True)).all(1) & \
                ~_waves((one != 0) & ~dead0 & (fin == 0), n, False).any(1)
            lvl = np.where(active != 0, S, 0)
            e_c = np.where(uenv != 0, wrap32(lvl * vel) >> 15, 32768)
            target = wrap32((amp * e_c) >> 15)
            kk = np.where(dead0 | (fin != 0), 0, k)
            stalled = (w_dead0 | _waves((smooth == 0) | ((wrap32(wrap32(target - sg) * kk) >> 15) == 0), n, True)).all(1)
            narrow_c = narrow_l & (w_dead0 | _waves(np.abs(target) <= 65535, n, True)).all(1)
            forms = []
            for w in range(len(steady)):
                if steady[w] and cn >= 8:
                    forms.append((LEAN if narrow_c[w] and lean_ok[w] else BLOCK, bool(narrow_c[w]), bool(stalled[w])))
                else:
                    forms.append((FRAME, None, None))
            open_chunk = (i // CHUNK, forms, i + 8 * (cn // 8))
            railed = np.zeros(len(steady), bool)

        now = np.uint64((count + i + 1) & ((1 << 64) - 1))
        live = (amp != 0) & (fin == 0)
        # oscillator
        total = ph + inc
        ends = live & (one != 0) & (total > M32)
        fin = np.where(ends, 1, fin)
        ph = np.where(live, np.where(ends, M32, total & M32), ph)
        idx = ph >> (32 - L)
        s = pool64[toff + idx]
        if interp:
            nxt = np.where(ends, s, pool64[toff + ((idx + 1) & mask)])
            frac = ((ph << L) & M32) >> 17
            p = (nxt - s) * frac
            rep.check("(b - a) * f", p, live)
            s = s + (wrap32(p) >> 15)
        # biquad
        fl = live & (fmode != 0)
        x0 = s * 4096
        acc = b0 * x0 + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        y0u = (acc + (1 << 29)) >> 30
        y0 = np.clip(y0u, -RAIL, RAIL - 1)
        if i < open_chunk[2]:
            hit = fl & (y0u != y0)
            if hit.any():
                railed |= _waves(hit, n, False).any(1)
        x2, x1 = np.where(fl, x1, x2), np.where(fl, x0, x1)
        y2, y1 = np.where(fl, y1, y2), np.where(fl, y0, y1)
        s = np.where(fl, np.clip(y0 >> 12, -32768, 32767), s)
        # envelope
        ue = live & (uenv != 0)
        act = ue & (active != 0)
        t = np.minimum(now - start, np.uint64(M32)).astype(np.int64)
        in_a = act & (t < A)
        in_d = act & ~in_a & (t < A + D)
        past = act & ~in_a & ~in_d
        hold = past & (rel == 0)
        tr = np.minimum(now - rel, np.uint64(M32)).astype(np.int64)
        in_r = past & ~hold & (tr < R)
        over = past & ~hold & ~in_r
        lvl_a = (((u64(t) * rA) & np.uint64(M32)) >> np.uint64(17)).astype(np.int64)
        prog_d = (((u64(np.where(in_d, t - A, 0)) * rD) & np.uint64(M32)) >> np.uint64(17)).astype(np.int64)
        p_d = prog_d * (32768 - S)
        rep.check("decay progress * (32768 - S)", p_d, in_d)
        prog_r = (((u64(tr) * rR) & np.uint64(M32)) >> np.uint64(17)).astype(np.int64)
        p_r = prog_r * S
        rep.check("release progress * S", p_r, in_r)
        lvl = np.select([in_a, in_d, hold, in_r], [lvl_a, 32768 - (wrap32(p_d) >> 15), S, S - (wrap32(p_r) >> 15)], 0)
        active = np.where(over, 0, active)
        p_e = lvl * vel
        rep.check("e * velocity", p_e, ue)
        e = np.where(ue, wrap32(p_e) >> 15, 32768)
        # gain, smoother, output
        gain = wrap32((amp * e) >> 15)
        sm = live & (smooth != 0)
        diff = gain - sg
        rep.check("target - g", diff, sm)
        p_k = wrap32(diff) * k
        rep.check("(target - g) * k", p_k, sm)
        g = sg + (wrap32(p_k) >> 15)
        rep.check("g + step", g, sm)
        sg = np.where(sm, wrap32(g), sg)
        gain = np.where(sm, sg, gain)
        out = wrap32((s * gain) >> 15)
        vs = np.where(live, out, 0)
        con = live & (disc == 0)
        p_l, p_r2 = out * panl, out * panr
        rep.check("v * pan_left", p_l, con)
        rep.check("v * pan_right", p_r2, con)
        l = np.where(con, wrap32(p_l) >> 15, 0)
        r = np.where(con, wrap32(p_r2) >> 15, 0)
        mix[i, 0], mix[i, 1] = l.sum(), r.sum()
        if want_stems:
            stems[i, :, 0], stems[i, :, 1] = l, r
    if open_chunk is not None:
        close_chunk()
    rep.paths.append(paths)
    for name, val in (("phase", ph), ("is_active", active), ("smoother_gain_q15", sg), ("voice_sample", vs), ("finished", fin),
                      ("x1", x1), ("x2", x2), ("y1", y1), ("y2", y2)):
        a[name][...] = val.astype(a[name].dtype)
    return mix, stems, count + frames


def master(target_q31, k_q15, gain_q31, mix):
    """The master stage: g += ((target - g) * k) >> 15 per frame, out = (mix * (g >> 16)) >> 15.  Returns (out, new gain)."""
    g = int(gain_q31)
    g15 = np.zeros(len(mix), np.int64)
    for i in range(len(mix)):
        g += ((int(target_q31) - g) * int(k_q15)) >> 15
        g15[i] = g >> 16
    return (np.asarray(mix, np.int64) * g15[:, None]) >> 15, g


def stamp(bank, voices, which, now):
    """Stamps: note-on (which & 1): sample_start = now, sample_release = 0, is_active = 1; then note-off (which & 2): if
    is_active, sample_release = now.  A voice listed twice gets the same stores twice."""
    v = np.asarray(voices, np.int64)
    a = bank.a
    if which & 1:
        a["sample_start"][v] = now
        a["sample_release"][v] = 0
        a["is_active"][v] = 1
    if which & 2:
        on = v[a["is_active"][v] != 0]
        a["sample_release"][on] = now
