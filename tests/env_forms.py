"""Which code of the two-per-lane family's moving-envelope machinery runs where: a numpy restatement, written from the kernels'
code, of
  * sk_env_stage_code and sk_env_motion (skred_kernel_common.hpp),
  * the motion list's rule: the list after a block is the listed voices that are moving or settling (in place: moving) on the next
    block's first frame, plus every voice a control action touched; rebuilt by classification (sk_classify_kernel) after an upload,
  * the decision ladder of sk_render_env2_kernel per wave -- 128 consecutive entries of the ascending list, lane l holding entries
    l and 64 + l -- and 64-frame chunk (skred_render_fast2.hip, the loop over SK_CHUNK),
  * the in-place rule of sk_plan_finish / plan_inplace (skred_bank_plan.c) with the host's bookkeeping of launch reports
    (skred_bank_render.c: poll_reports), and which waves / words then exceed 32 staged voices / 8 own rows.
Its input is the ORACLE's bank at every block start and end (cpuref state, never device state).  Nothing here renders.

Forms of a wave-chunk: 1 constant, 2 ramp, 3 step, 4 re-decision per 8-frame block (kinds "const", "ramp", "step", "general"),
5 one frame at a time on integer clocks (triggers "clock", "ragged", "untame").
"""
import numpy as np

F32, U64 = np.float32, np.uint64
CHUNK = 64
CLOCK_LIM = (1 << 24) - CHUNK - 2
MAX_SETTLING = 16                   # SK_FAST2_MAX_SETTLING
WORD_ROWS, GT_RANKS = 8, 32         # SK_INPLACE_WORD_ROWS, SK_GT_RANKS
IN_PLACE_DENOM = 6                  # SK_INPLACE_DENOM
KINDS = ("const", "ramp", "step", "general")
TRIGGERS = ("clock", "ragged", "untame")
LO, HI = F32(2.0 ** -40), F32(2.0 ** 40)


def stage_code(active, released, t, tr, att, attdec, rel):
    """sk_env_stage_code: 0 inactive, 1 attack, 2 decay, 3 sustain, 4 release, 5 release finished.  float32 operands."""
    return np.where(~active, 0, np.where(t < att, 1, np.where(t < attdec, 2, np.where(~released, 3, np.where(tr < rel, 4, 5)))))


class Voices:
    """What fast2_load / sk_classify_kernel / sk_gain_kernel read of every voice, from a VoiceBank (padded to whole 128-voice slices
    with inert voices)."""

    def __init__(self, bank, count0):
        n = bank.n
        e = bank["voice_amp_envelope"]
        fake = bank["voice_use_amp_envelope"] == 0           # no envelope: a note held at level 1 with velocity 1 since "now"

        def f(x, fill):
            return np.where(fake, F32(fill), x).astype(F32)
        self.n = n
        self.fake = fake
        self.att, self.dec, self.rel = f(e["attack_time"], 0), f(e["decay_time"], 0), f(e["release_time"], 0)
        self.attdec = (self.att + self.dec).astype(F32)
        self.sus, self.vel = f(e["sustain_level"], 1), f(e["velocity"], 1)
        self.amp = bank["voice_amp"].astype(F32)
        self.k = bank["voice_smoother_smoothing"].astype(F32)
        self.sgain = bank["voice_smoother_gain"].astype(F32)
        self.t_start = np.where(fake, U64(count0), e["sample_start"]).astype(U64)
        self.t_release = np.where(fake, U64(0), e["sample_release"]).astype(U64)
        self.released = self.t_release != 0
        self.active = np.where(fake, True, e["is_active"] != 0)
        usable = bank["voice_table_size"] > 0
        self.dead = (bank["voice_finished"] != 0) | (self.amp == 0) | ~usable
        self.muted = (bank["voice_disconnect"] != 0) & ~self.dead
        windowed = (bank["voice_loop_enabled"] != 0) & (bank["voice_loop_valid"] != 0)
        size = bank["voice_table_size"].astype(F32)
        lo = np.where(windowed, bank["voice_loop_start_f"], F32(0)).astype(F32)
        hi = np.where(windowed, bank["voice_loop_end_f"], size).astype(F32)
        inc, ph = bank["voice_phase_inc"].astype(F32), bank["voice_phase"].astype(F32)
        self.tame = self.dead | ((inc >= 0) & (inc <= F32(0.5) * (hi - lo).astype(F32)) & (ph >= lo) & (ph <= hi) & (lo >= 0) & (hi <= size))

    def motion(self, first_now, active=None, sgain=None):
        """sk_env_motion on the frame whose clock is first_now: (code, moving, settling)."""
        active = self.active if active is None else active
        sgain = self.sgain if sgain is None else sgain
        with np.errstate(over="ignore"):
            d_on, d_off = U64(first_now) - self.t_start, U64(first_now) - self.t_release
            ahead = active & ((self.t_start - U64(first_now)).astype(np.int64) > 0)
        code = stage_code(active, self.released, d_on.astype(F32), d_off.astype(F32), self.att, self.attdec, self.rel)
        moving = ~self.dead & (ahead | ~np.isin(code, (0, 3, 5)))
        level = np.where(code == 3, self.sus, F32(0)).astype(F32)
        gain = (self.amp * (level * self.vel).astype(F32)).astype(F32)
        nxt = (sgain + (self.k * (gain - sgain).astype(F32)).astype(F32)).astype(F32)
        settling = ~self.dead & ~moving & (nxt.view(np.uint32) != sgain.view(np.uint32))
        return code, moving, settling


def classify(v, count0):
    """sk_classify_kernel: the list from scratch on the block's first frame."""
    _, mv, st = v.motion(count0 + 1)
    pad = (-v.n) % 128
    per_slice = np.pad(st, (0, pad)).reshape(-1, 128).sum(1)
    few = np.repeat(per_slice <= MAX_SETTLING, 128)[:v.n]
    return mv | (st & few)


def _span(v, ix, act, dead, t1, tr1, tN, trN):
    """fast2_env_span per lane: (constant level, keeps its stage with a tame denominator, active flag afterwards)."""
    a = lambda x: x[ix]
    c0 = stage_code(act, a(v.released), t1, tr1, a(v.att), a(v.attdec), a(v.rel))
    c1 = stage_code(act, a(v.released), tN, trN, a(v.att), a(v.attdec), a(v.rel))
    st = dead | np.isin(c0, (0, 3, 5))
    d = np.where(c0 == 1, a(v.att), np.where(c0 == 2, a(v.dec), np.where(c0 == 4, a(v.rel), F32(1)))).astype(F32)
    same = dead | ((c0 == c1) & (d >= LO) & (d <= HI))
    return st, same, act & ~(~dead & (c0 == 5))


def _span2(v, ix, act, dead, t1, tr1, tN, trN):
    """fast2_env_span2 per lane: (at most one change, to the stage that follows, tame denominators; the release runs out)."""
    a = lambda x: x[ix]
    c0 = stage_code(act, a(v.released), t1, tr1, a(v.att), a(v.attdec), a(v.rel))
    c1 = stage_code(act, a(v.released), tN, trN, a(v.att), a(v.attdec), a(v.rel))
    step = c0 != c1
    nxt = ((c0 == 1) & (c1 == 2)) | ((c0 == 2) & ((c1 == 3) | (c1 == 4))) | ((c0 == 4) & (c1 == 5))
    ok = ~step | nxt
    for c in (c0, c1):
        d = np.where(c == 1, a(v.att), np.where(c == 2, a(v.dec), np.where(c == 4, a(v.rel), F32(1)))).astype(F32)
        ok = ok & (d >= LO) & (d <= HI)
    return dead | ok, ~dead & ((c0 == 5) | (c1 == 5))


def ladder(v, listed, count0, frames):
    """The decision ladder of sk_render_env2_kernel for one block.  `listed`: bool per voice.  Returns (records, active): one record
    per wave-chunk -- dict(wave, chunk, form, kinds (form 4), triggers (form 5), moved_before) -- and the is_active flag of every
    voice after the block as the kernel leaves it (listed voices only; the others as they came)."""
    idx = np.flatnonzero(listed)
    recs = []
    active_out = v.active.copy()
    if len(idx) == 0:
        return recs, active_out
    W = (len(idx) + 127) // 128
    absent = np.ones(W * 128, bool)
    absent[:len(idx)] = False
    ix = np.zeros(W * 128, np.int64)
    ix[:len(idx)] = idx
    ix, absent = ix.reshape(W, 128), absent.reshape(W, 128)
    dead = v.dead[ix] | absent
    act = v.active[ix] & ~dead                            # fast2_make_inert clears the flag of a dead lane
    tame = np.all(dead | (v.tame[ix] & ~v.muted[ix]), axis=1)
    rel_l, ts, tr_ = v.released[ix], v.t_start[ix], v.t_release[ix]
    all_const = np.zeros(W, bool)
    moved = np.zeros(W, bool)
    with np.errstate(over="ignore"):
        for ci, c0 in enumerate(range(0, frames, CHUNK)):
            cn = min(CHUNK, frames - c0)
            base = U64(count0 + c0)
            d_on, d_off = base - ts, base - tr_
            ex = np.all(dead | ((d_on < U64(CLOCK_LIM)) & (~rel_l | (d_off < U64(CLOCK_LIM)))), axis=1)
            cb_t, cb_tr = d_on.astype(F32), np.where(rel_l, d_off.astype(F32), F32(0)).astype(F32)
            t1, tr1 = (d_on + U64(1)).astype(F32), (d_off + U64(1)).astype(F32)
            tN, trN = (d_on + U64(cn)).astype(F32), (d_off + U64(cn)).astype(F32)
            live = ~all_const
            st, same, act1 = _span(v, ix, act, dead, t1, tr1, tN, trN)
            act = np.where(live[:, None], act1, act)
            ahead = ~dead & act & ((ts - (base + U64(1))).astype(np.int64) > 0)
            steady = all_const | np.all(st & ~ahead, axis=1)
            ramp = ~steady & ex & np.all(same, axis=1)
            all_const = steady
            try2 = ~steady & ~ramp & ex
            ok2, out = _span2(v, ix, act, dead, t1, tr1, tN, trN)
            step = try2 & np.all(ok2, axis=1)
            act = np.where(step[:, None], act & ~out, act)
            form = np.where(steady, 1, np.where(ramp, 2, np.where(step, 3, np.where(ex & tame & (cn % 8 == 0), 4, 5))))
            kinds = {w: [] for w in np.flatnonzero(form == 4)}
            if kinds:
                w4 = form == 4
                for jb in range(0, cn, 8):
                    fb = F32(jb)
                    a1, b1 = (cb_t + fb + F32(1)).astype(F32), (cb_tr + fb + F32(1)).astype(F32)
                    a8, b8 = (cb_t + fb + F32(8)).astype(F32), (cb_tr + fb + F32(8)).astype(F32)
                    st, same, act1 = _span(v, ix, act, dead, a1, b1, a8, b8)
                    act = np.where(w4[:, None], act1, act)
                    b_const, b_ramp = np.all(st, axis=1), np.all(same, axis=1)
                    ok2, out = _span2(v, ix, act, dead, a1, b1, a8, b8)
                    b_step = ~b_const & ~b_ramp & np.all(ok2, axis=1)
                    act = np.where((w4 & b_step)[:, None], act & ~out, act)
                    general = w4 & ~b_const & ~b_ramp & ~b_step
                    # general frames (fast2_env_general): the flag goes on the first frame that finds the release run out
                    c8 = stage_code(act, rel_l, a8, b8, v.att[ix], v.attdec[ix], v.rel[ix])
                    act = np.where(general[:, None], act & ~(c8 == 5), act)
                    for w in kinds:
                        kinds[w].append("const" if b_const[w] else "ramp" if b_ramp[w] else "step" if b_step[w] else "general")
            w5 = form == 5
            if w5.any():
                for j in range(cn):                      # integer clocks, one frame at a time
                    now = U64(count0 + c0 + j + 1)
                    c = stage_code(act, rel_l, (now - ts).astype(F32), (now - tr_).astype(F32), v.att[ix], v.attdec[ix], v.rel[ix])
                    act = np.where(w5[:, None], act & ~(c == 5), act)
            for w in range(W):
                trig = [t for t, on in (("clock", not ex[w]), ("ragged", cn % 8 != 0), ("untame", not tame[w])) if on] if form[w] == 5 else []
                recs.append({"wave": w, "chunk": ci, "form": int(form[w]), "kinds": kinds.get(w, []), "triggers": trig,
                             "moved_before": bool(moved[w])})
            moved |= form != 1
    real = ~absent & ~v.dead[ix]
    active_out[ix[real]] = act[real]
    return recs, active_out


def gain_active(v, listed, count0, frames):
    """sk_gain_kernel: the is_active flag of the listed voices after the block (integer clocks, every frame)."""
    act = v.active.copy()
    sel = listed & ~v.dead & ~v.fake
    with np.errstate(over="ignore"):
        for j in range(frames):
            now = U64(count0 + j + 1)
            c = stage_code(act, v.released, (now - v.t_start).astype(F32), (now - v.t_release).astype(F32), v.att, v.attdec, v.rel)
            act = np.where(sel, act & ~(c == 5), act)
    return act


class LateReport(Exception):
    """walk(): a queued block's path depends on whether an earlier block's report has arrived, and no observation settles it."""


def in_place_limit(n):
    return n // IN_PLACE_DENOM + 64


def walk(case, pre, post, mode, queued=(), observed=None):
    """The whole block list of `case` under SKRED_OPT_IN_PLACE `mode` (0: the envelope kernel beside the steady one; 2: in place
    whenever the gain rows provably suffice).  pre[k] / post[k]: the oracle's bank when block k starts (its actions applied) / ends.
    `queued`: blocks issued without a synchronisation before them -- the host may or may not have seen the reports of the blocks
    before them, so such a block can have two possible answers; `observed` ({block: last_in_place()}) then says which path the
    run took, so that the list can be followed (without it: LateReport).  Returns one dict per block: listed (bool per voice),
    in_place (the set of possible answers: {True}, {False} or both), taken (the path followed), bound, records (the ladder, when
    the envelope kernel runs), waves_over (128-voice waves of the bank with more than 32 listed voices), words_over (64-voice words
    with more than 8), cleared (voices whose release ended inside the block), active_end."""
    n = case.n
    observed = dict(observed or {})
    count = int(case.g.synth_sample_count)
    out = []
    listed = np.zeros(n, bool)
    touched_total = 0
    # what the host may hold when it plans a block: the report its bound comes from -- None, or (list length, touched_total when
    # that launch was issued) -- and whether it knows the list to be empty; several alternatives while a report may be late
    bounds, empties = [None], {False}
    lim = in_place_limit(n)
    for k, (frames, actions) in enumerate(case.blocks):
        v = Voices(pre[k], count)
        for a in actions:
            listed[a.voices] = True
            touched_total += len(a.voices)
        if actions:
            empties = {False}
        if k == 0:
            listed = classify(v, count)
            bounds, empties = [None], {False}
        answers = set()
        for empty in empties:
            for b in bounds:
                answers.add(bool(mode == 2 and case.lds_tables and not empty and b is not None and b[0] + (touched_total - b[1]) <= lim))
        if len(answers) == 1:
            inplace = True in answers
        elif k in observed:
            inplace = bool(observed[k])
        else:
            raise LateReport(f"block {k}: whether it is rendered in place depends on a report that may be late")
        last = bounds[-1]
        rec = {"listed": listed.copy(), "in_place": answers, "taken": inplace, "frames": frames, "count0": count, "records": [],
               "bound": None if last is None else last[0] + (touched_total - last[1]), "list_empty": empties == {True}}
        pad = (-n) % 128
        per_wave = np.pad(listed, (0, pad)).reshape(-1, 128).sum(1)
        per_word = np.pad(listed, (0, pad)).reshape(-1, 64).sum(1)
        rec["waves_over"], rec["words_over"] = np.flatnonzero(per_wave > GT_RANKS), np.flatnonzero(per_word > WORD_ROWS)
        ve = Voices(post[k], count)
        ve.dead = v.dead                                  # (decided when the block loads its voices)
        length = int(listed.sum())
        if length == 0:                                   # (nothing to render, whether or not the host knows)
            act_end = v.active
            keep = np.zeros(n, bool)
        elif inplace:
            act_end = gain_active(v, listed, count, frames)
            _, keep, _ = ve.motion(count + frames + 1, active=act_end)
        else:
            rec["records"], act_end = ladder(v, listed, count, frames)
            _, mv, st = ve.motion(count + frames + 1, active=act_end)
            keep = mv | st
        rec["active_end"] = act_end
        rec["cleared"] = np.flatnonzero(listed & v.active & ~act_end & ~v.fake & ~v.dead)
        out.append(rec)
        # the report of this block, read when the next one is planned: certainly (a synchronisation in between) or perhaps (queued).
        # A block whose list the host knows to be empty runs nothing beside the steady kernel and reports nothing.
        late = (k + 1) in queued
        nxt_actions = case.blocks[k + 1][1] if k + 1 < len(case.blocks) else []
        if empties != {True}:
            new = (length, touched_total)
            bounds = bounds + [new] if (late or True in empties) else [new]
            if length == 0 and not nxt_actions:           # ... empty, and nothing added since: the host stops listing
                empties = {True, False} if (late or True in empties) else {True}
        listed = listed & keep
        count += frames
    return out
