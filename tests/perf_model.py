"""The whole control plane of the float bank on one stage: the oracle's bank with an owner array (tests/owner_model.py), a pedal array
(tests/pedal_model.py) and a glide array (tests/glide_model.py) beside it, and one method per interface call.  No rule is stated
here but the wrong model (f)'s loop (last_product): every method delegates to the model that defines its call, and the only thing
this file adds is where those models share state --

  * the glide model's `inc` IS the truth's voice_phase_inc (a view, not a copy): note-ons, controller bends and glides act on one
    array;
  * every path that tags (tag_slots, the tags of note_on_channel) goes through Stage.tag: owner_model.tag_slots, then the pedal word
    of the tagged slots and the glide words of all their K voices are cleared (pedal_model.tag_slots, glide_model.tag_clear);
  * a release -- by note id, by match, by a pedal-up -- is slot_model.stamp and nothing else: it leaves the glide words alone, so a
    released note goes on gliding through its tail, and pedal_latch reads `held` from the envelope only: a gliding note is latched
    like any other (include/skred_amd.h says both since this file was written).

WRONG names the wrong models: each switch breaks one rule, so that tests/test_perf_fuzz_cpu.py can show that a performance of
tests/perf_fuzz.py ends differently without it.  Stage.events counts the interactions a performance really reached, from the state
and the result words of the model itself.  Stage.log holds every call's result words and lists: what a device has to reproduce.
"""
import hashlib
from collections import Counter

import numpy as np

import chan_model as CHM
import ctl_model as CTL
import expr_model as EM
import glide_model as GM
import owner_model as OM
import pedal_model as PM
import slot_model as SM
import slot_steal_model as SSM
import timbre_model as TM
from oracle import cpuref

REL, TRIG = SM.STAMP_RELEASE, SM.STAMP_TRIGGER
PENDING, LATCHED = PM.PENDING, PM.LATCHED
TINY = np.float32(2.0 ** -126)
INC_BITS = CTL.PHASE_INC | CTL.INC_SCALE

# (a) .. (g) of the wrong models
WRONG = {"a": "no pedal clear behind a tag", "b": "no glide clear behind a tag", "c": "release_tags takes the highest carrier",
         "d": "a pedal-up stamps the held note-off's clock", "e": "hold_all == 0 ignores LATCHED",
         "f": "a glide's arrival stores the last product", "g": "a channel burst steals from another channel"}

INTERACTIONS = ("theft of a pending slot", "theft of a gliding slot", "re-strike on the same slot while pending",
                "note-off takes the lowest of two carriers", "note-off misses a stolen note", "latch skips a pending slot",
                "pedal-up with SUSTAIN_DOWN", "pedal-up that releases nothing", "glide arrives on a held note",
                "glide arrives in the block of its release", "TO_SCALE on a gliding voice", "INC bend on a gliding voice",
                "burst placed, stolen and dropped", "burst above a lowered cap", "stamp_match on pending bits",
                "withheld: zero amp product", "withheld: non-finite increment product")


class Out:
    """What one call leaves on the device: the d_result words and the list it wrote (d_assigned, or None); `touched`: what the call
    adds to the planner's bound on the motion list (include/skred_amd.h states it call by call)."""

    def __init__(self, kind, res, assigned=None, touched=0):
        self.kind, self.res, self.assigned, self.touched = kind, [int(x) for x in res], assigned, int(touched)


# the calls whose addition to the bound does not depend on the records they carry
STAMPS = ("note_on_channel", "note_on_steal_slots", "note_on_idle_slots", "release_tags", "release_tags_pedal", "stamp_owned_pedal",
          "pedal_up", "stamp_match")


class Stage:
    def __init__(self, bank, tables, g, K, vmask, mmask, wrong=""):
        self.bank, self.tables = bank, tables
        self.truth, self.gl = bank.copy(), g.copy()
        self.n, self.K, self.vmask, self.mmask = bank.n, K, vmask, mmask
        self.owner, self.pedal, self.glide = OM.new(bank.n), PM.new(bank.n), GM.new(bank.n)
        self.wrong = set(wrong)
        assert self.wrong <= set(WRONG)
        self.whole = (0, bank.n - bank.n % K)
        self.events, self.log, self.lists = Counter(), [], {}
        self.ever, self.held_at, self.arrived = set(), {}, set()
        self.pop = bin(vmask).count("1")
        self.struck = np.zeros(bank.n, bool)                                      # voices a note-on of the performance triggered
        self.fronts, self.at_front = [], 0                                        # per block: what the planner's in-place rule reads
        self.in_motion = [self.motion_count()]
        e = self.truth["voice_amp_envelope"]
        self.start, self.release = e["sample_start"].copy(), e["sample_release"].copy()   # the clocks the stamps imply
        self.last_state = self.state_hash()

    # ---- shared state
    def now(self):
        return int(self.gl.synth_sample_count)

    def inc(self):
        return self.truth["voice_phase_inc"]

    def state_hash(self):
        h = hashlib.sha256()
        for a in (self.owner, self.pedal, self.glide):
            h.update(a.tobytes())
        for name in sorted(self.truth.a):
            h.update(self.truth[name].tobytes())
        return h.digest()

    def out(self, kind, res, assigned=None, touched=0):
        """One call's record.  inert: every result word 0, nothing placed, and no word of the arrays or the bank changed."""
        o = Out(kind, res, assigned, touched)
        state = self.state_hash()
        o.inert = not any(o.res) and (assigned is None or (assigned < 0).all()) and state == self.last_state
        self.last_state = state
        self.log.append(o)
        return o

    def normal(self, voices):
        """increments stay normal fp32 numbers: the one place numpy's multiply and the device's could part (tests/glide_model.py)"""
        w = np.abs(self.inc()[np.asarray(voices, np.int64)])
        assert (np.isfinite(w) & (w >= TINY) & (w < np.float32(64.0))).all(), "an increment left the range the performance promises"
        t = self.glide[:, GM.TARGET].view(np.float32)
        on = self.glide[:, GM.TARGET] != 0
        assert (np.abs(t[on]) >= TINY).all() and np.isfinite(t[on]).all()

    def stamped(self, voices, stamps, now):
        """the shadow clocks: what slot_model.stamp's rule implies, kept apart from the bank the oracle renders"""
        act = self.truth["voice_amp_envelope"]["is_active"]
        for v in np.asarray(voices, np.int64):
            if stamps & TRIG:
                self.start[v], self.release[v] = now, 0
            if stamps & REL and (stamps & TRIG or act[v] != 0):
                self.release[v] = now

    def slot_voices(self, slots, mask=None):
        return np.array([int(s) + l for s in slots for l in SM.lanes(self.vmask if mask is None else mask, self.K)], np.int64)

    # ---- the one tag rule
    def tag(self, entries, tags, count=None):
        K = self.K
        for k, e in enumerate(OM.looked(entries, len(tags), count)):
            if not CTL.slot_valid(e, K, self.n):
                continue
            old, new = int(self.owner[e]), int(tags[k])
            if old and old != new:
                self.events["theft of a pending slot"] += bool(self.pedal[e] & PENDING)
                self.events["theft of a gliding slot"] += bool(self.glide[e:e + K, GM.TARGET].any())
            if old == new and self.pedal[e] & PENDING:
                self.events["re-strike on the same slot while pending"] += 1
            self.ever.add(new)
        res = PM.tag_slots(self.owner, self.pedal, entries, tags, count, K, clear_rule="a" not in self.wrong)
        if "b" not in self.wrong:
            assert GM.CLEAR_RULE
            GM.tag_clear(self.glide, entries, len(tags), count, K)
        return res

    def tag_slots(self, ref, tags):
        """skred_bank_tag_slots on the d_assigned an earlier note-on left (`ref`: that call's place in the log)"""
        return self.out("tag_slots", self.tag(self.lists[ref], tags))

    # ---- note-ons
    def placed(self, notes, assigned):
        now = self.now()
        touched = SM.store_notes((self.truth,), self.truth, notes, self.K, self.vmask, assigned, now)
        self.struck[touched] = True
        self.stamped(touched, TRIG, now)
        self.normal(touched)

    def note_on_channel(self, notes, tags, iq, sq, match, cap):
        n = len(tags)
        m = (0, 0) if "g" in self.wrong else match
        assigned, res, _ = CHM.burst(self.truth, self.now(), self.owner, iq, sq, m, cap, n)
        self.events["burst placed, stolen and dropped"] += bool(res[0] and res[1] and res[2])
        self.events["burst above a lowered cap"] += res[3] > cap
        self.placed(notes, assigned)
        self.tag(assigned, tags)
        self.lists[len(self.log)] = assigned
        return self.out("note_on_channel", res, assigned, n * self.pop)

    def note_on_steal_slots(self, notes, n, iq, sq):
        idle = SM.idle_slots(self.truth, iq.first, iq.count, self.K, iq.member_mask, iq.which, iq.settle_level, iq.start)[:n]
        q = sq.but(exclude_idle=iq.which, settle_level=float(iq.settle_level), max_out=min(n, SSM.STEAL_MAX))
        victims = SSM.victim_slots(self.truth, self.now(), q)[:q.max_out]
        joined = np.concatenate([idle, victims]).astype(np.int32)[:n]
        assigned = np.full(n, -1, np.int32)
        assigned[:len(joined)] = joined
        self.placed(notes, assigned)
        self.lists[len(self.log)] = assigned
        return self.out("note_on_steal_slots", [len(joined), n - len(joined), len(joined) - len(idle)], assigned, n * self.pop)

    def note_on_idle_slots(self, notes, n, iq):
        idle = SM.idle_slots(self.truth, iq.first, iq.count, self.K, iq.member_mask, iq.which, iq.settle_level, iq.start)[:n]
        assigned = SM.place(n, self.K, idle, len(idle), 0, self.n)
        self.placed(notes, assigned)
        self.lists[len(self.log)] = assigned
        return self.out("note_on_idle_slots", [int((assigned >= 0).sum()), int((assigned < 0).sum())], assigned, n * self.pop)

    # ---- note-offs
    def find(self, first, count, tags):
        lst = OM.find_owned(self.owner, first, count, self.K, tags)
        heads = np.arange(first, first + count, self.K)
        for k, t in enumerate(tags):
            carriers = heads[self.owner[heads] == np.uint32(t)]
            self.events["note-off takes the lowest of two carriers"] += len(carriers) > 1
            self.events["note-off misses a stolen note"] += len(carriers) == 0 and int(t) in self.ever
            if "c" in self.wrong and len(carriers):
                lst[k] = carriers.max()
        return lst

    def release_tags(self, first, count, tags):
        lst = self.find(first, count, tags)
        now = self.now()
        res, voices = OM.stamp_owned(self.owner, self.truth, lst, tags, None, self.K, self.vmask, REL, now)
        self.stamped(voices, REL, now)
        return self.out("release_tags", res, touched=len(tags) * self.pop)

    def off_list(self, kind, lst, tags, hold_all):
        now = self.now()
        pedal = self.pedal
        if "e" in self.wrong and not hold_all:
            pedal = self.pedal & np.uint32(~LATCHED & 0xFFFFFFFF)                 # (nothing is held back then: the copy stays unwritten)
        before = self.pedal.copy()
        res, voices = PM.stamp_owned_pedal(self.owner, pedal, self.truth, lst, tags, None, self.K, self.vmask, hold_all, now)
        self.stamped(voices, REL, now)
        for e in np.flatnonzero((self.pedal & PENDING) & ~(before & PENDING)):
            self.held_at[int(e)] = now
        return self.out(kind, res, touched=len(tags) * self.pop)

    def release_tags_pedal(self, first, count, tags, hold_all):
        return self.off_list("release_tags_pedal", self.find(first, count, tags), tags, hold_all)

    def stamp_owned_pedal(self, ref, tags, hold_all):
        return self.off_list("stamp_owned_pedal", self.lists[ref], tags, hold_all)

    # ---- pedals
    def pedal_latch(self, first, count, match):
        heads = np.arange(first, first + count, self.K)
        hit = CHM.matches(self.owner[heads], match) & ((self.pedal[heads] & PENDING) != 0)
        h = PM.held(self.truth)
        self.events["latch skips a pending slot"] += int(sum(h[self.slot_voices([s])].any() for s in heads[hit]))
        res = PM.latch(self.owner, self.pedal, self.truth, first, count, self.K, self.vmask, match)
        return self.out("pedal_latch", res)

    def pedal_up(self, first, count, match, flags):
        now = self.now()
        before = self.pedal.copy()
        res, voices = PM.up(self.owner, self.pedal, self.truth, first, count, self.K, self.vmask, match, flags, now)
        self.stamped(voices, REL, now)
        if "d" in self.wrong:
            e = self.truth["voice_amp_envelope"]
            for s in np.flatnonzero((before & PENDING) & ~(self.pedal & PENDING)):
                vs = self.slot_voices([s])
                vs = vs[e["sample_release"][vs] == now]
                e["sample_release"][vs] = self.release[vs] = self.held_at.get(int(s), now)
        self.events["pedal-up with SUSTAIN_DOWN"] += bool(flags & PM.SUSTAIN_DOWN)
        self.events["pedal-up that releases nothing"] += res[0] == 0
        return self.out("pedal_up", res, touched=count // self.K * self.pop)

    def pedal_clear(self, first, count):
        PM.clear(self.pedal, first, count)
        return self.out("pedal_clear", [])

    # ---- channels and controllers
    def bend(self, voices, bits):
        if bits & INC_BITS and len(voices):
            self.events["INC bend on a gliding voice"] += bool(self.glide[np.asarray(voices, np.int64), GM.TARGET].any())

    def stamp_match(self, first, count, match):
        heads = np.arange(first, first + count, self.K)
        hit = CHM.matches(self.owner[heads], match)
        self.events["stamp_match on pending bits"] += bool((self.pedal[heads[hit]] & PENDING).any())
        now = self.now()
        res, voices = EM.stamp_match(self.owner, self.truth, first, count, self.K, self.vmask, match[0], match[1], REL, now)
        self.stamped(voices, REL, now)
        return self.out("stamp_match", res, touched=count // self.K * self.pop)

    def ctl_range(self, ctls, first, count):
        res, touched = CTL.ctl_range((self.truth,), ctls, first, count, self.vmask)
        self.bend(touched, sets_of(ctls))
        self.normal(touched)
        return self.out("ctl_range", res, touched=count // self.K * bin(CTL.listed(ctls, self.vmask)).count("1"))

    def ctl_match(self, ctls, first, count, match):
        heads = np.arange(first, first + count, self.K)
        self.bend(self.slot_voices(heads[CHM.matches(self.owner[heads], match)]), sets_of(ctls))
        res, touched = EM.ctl_match(self.owner, (self.truth,), ctls, first, count, self.vmask, match[0], match[1])
        self.normal(touched)
        return self.out("ctl_match", res, touched=EM.lists_range(ctls, self.vmask, first, count))

    def each_events(self, each, res, touched):
        sets = sets_of(each or ())
        self.bend(touched, INC_BITS if sets & EM.EACH_INC_SCALE else 0)
        if res[1]:
            self.events["withheld: zero amp product"] += bool(sets & EM.EACH_AMP_SCALE)
            self.events["withheld: non-finite increment product"] += bool(sets & EM.EACH_INC_SCALE)
        self.normal(touched)

    def ctl_owned_each(self, ctls, each, ref, tags):
        pre = self.gliding_in(self.lists[ref], tags)
        res, touched = EM.ctl_owned_each(self.owner, (self.truth,), ctls, each, self.K, self.vmask, self.lists[ref], tags, None)
        self.each_events(each, res, pre if len(pre) else touched)
        return self.out("ctl_owned_each", res, touched=EM.lists_each(ctls, each, self.K, self.vmask, len(tags)))

    def ctl_tags_each(self, ctls, each, first, count, tags):
        lst = OM.find_owned(self.owner, first, count, self.K, tags)
        pre = self.gliding_in(lst, tags)
        res, touched, _ = EM.ctl_tags_each(self.owner, (self.truth,), ctls, each, first, count, self.K, self.vmask, tags)
        self.each_events(each, res, pre if len(pre) else touched)
        return self.out("ctl_tags_each", res, touched=EM.lists_each(ctls, each, self.K, self.vmask, len(tags)))

    def ctl_owned_each_filter(self, ctls, each, filt, fmask, ref, tags):
        res, touched = TM.ctl_owned_each_filter(self.owner, (self.truth,), ctls, each, filt, self.K, self.vmask, fmask, self.lists[ref],
                                                tags, None)
        self.each_events(each, res, touched)
        return self.out("ctl_owned_each_filter", res, touched=TM.lists(ctls, each, self.K, self.vmask, len(tags)))

    def ctl_tags_each_filter(self, ctls, each, filt, fmask, first, count, tags):
        res, touched, _ = TM.ctl_tags_each_filter(self.owner, (self.truth,), ctls, each, filt, first, count, self.K, self.vmask, fmask, tags)
        self.each_events(each, res, touched)
        return self.out("ctl_tags_each_filter", res, touched=TM.lists(ctls, each, self.K, self.vmask, len(tags)))

    def gliding_in(self, lst, tags):
        """the gliding voices among the slots a guarded list call will write"""
        ok = [int(e) for k, e in enumerate(lst[:len(tags)]) if CTL.slot_valid(int(e), self.K, self.n) and int(self.owner[e]) == int(tags[k])]
        vs = self.slot_voices(ok)
        return vs[self.glide[vs, GM.TARGET] != 0] if len(vs) else vs

    # ---- portamento
    def glide_events(self, glides, lst, tags):
        for k, e in enumerate(lst[:len(tags)]):
            if glides[k].set == GM.TO_SCALE and CTL.slot_valid(int(e), self.K, self.n) and int(self.owner[e]) == int(tags[k]):
                self.events["TO_SCALE on a gliding voice"] += bool(self.glide[self.slot_voices([e]), GM.TARGET].any())

    def glide_tags(self, glides, first, count, tags):
        self.glide_events(glides, OM.find_owned(self.owner, first, count, self.K, tags), tags)
        res, lst = GM.start_tags(self.owner, self.glide, self.inc(), glides, first, count, self.K, self.vmask, tags)
        self.normal(self.slot_voices(lst[lst >= 0]))
        return self.out("glide_tags", res)

    def glide_owned(self, glides, ref, tags):
        self.glide_events(glides, self.lists[ref], tags)
        res = GM.start_owned(self.owner, self.glide, self.inc(), glides, self.K, self.vmask, self.lists[ref], tags)
        self.normal(np.arange(self.n))
        return self.out("glide_owned", res)

    def glide_advance(self, first, count, frames):
        on = np.flatnonzero(self.glide[first:first + count, GM.TARGET] != 0) + first
        before, words = self.inc()[on].copy(), self.glide[on].copy()
        res = GM.advance(self.glide, self.inc(), first, count, frames)
        there = self.glide[on, GM.TARGET] == 0
        if "f" in self.wrong:
            for v, cur, g in zip(on[there], before[there].view(np.uint32), words[there]):
                self.inc().view(np.uint32)[v] = last_product(cur, g, frames)
        self.events["glide arrives on a held note"] += bool(PM.held(self.truth)[on[there]].any())
        self.arrived |= set(on[there].tolist())
        self.normal(on)
        return self.out("glide_advance", res)

    def glide_stop(self, first, count, snap):
        GM.stop(self.glide, self.inc(), first, count, snap)
        self.normal(np.arange(first, first + count))
        return self.out("glide_stop", [])

    # ---- the census and the block
    def census(self, sq, match):
        """skred_bank_find_steal_slots_match with max_out = 0: d_count = [0, candidates, the channel's sounding slots]"""
        _, res = CHM.query(self.truth, self.now(), sq.but(max_out=0), self.owner, match)
        return self.out("census", res)

    def block(self, frames, stems=False):
        now = self.now()
        vs = np.array(sorted(self.arrived), np.int64)
        if len(vs):
            self.events["glide arrives in the block of its release"] += bool((self.release[vs] == now).any())
        self.arrived = set()
        ref = cpuref.render(self.truth, self.gl, self.tables, frames, 0, want_stems=stems)
        ref["mix"] = cpuref.master(self.gl, ref["sum64"].astype(np.float32))         # (the master stage's smoother moves with the blocks)
        e = self.truth["voice_amp_envelope"]
        assert np.array_equal(e["sample_start"], self.start) and np.array_equal(e["sample_release"], self.release), \
            "the oracle's clocks are not the ones the model's stamps imply"
        # the flag the stamps imply (oracle/cpu_ref.c: adsr_level): a note struck in the performance and not released stays active
        held = self.struck & (self.release == 0)
        assert (e["is_active"][held] != 0).all(), "a note the model holds is not active in the oracle"
        front = self.log[self.at_front:]
        self.fronts.append({"touched": sum(o.touched for o in front), "stamped": sum(o.touched for o in front if o.kind in STAMPS),
                            "kinds": [o.kind for o in front if o.touched], "frames": frames})
        self.at_front = len(self.log)
        self.in_motion.append(self.motion_count())
        return ref

    def motion_count(self):
        """voices whose envelope or smoother is in motion on the next frame (tests/env_forms.py: sk_env_motion): the motion list a
        block leaves behind is a subset of them"""
        import env_forms
        _, moving, settling = env_forms.Voices(self.truth, self.now()).motion(self.now() + 1)
        return int((moving | settling).sum())

    # ---- what a run ends with
    def digest(self):
        h = hashlib.sha256()
        h.update(self.state_hash())
        for o in self.log:
            h.update(np.array(o.res, np.uint32).tobytes())
            if o.assigned is not None:
                h.update(o.assigned.tobytes())
        return h.hexdigest()


def sets_of(records):
    bits = 0
    for r in records:
        bits |= int(r.set)
    return bits


def in_place_verdicts(stage):
    """Per block of a performance on a two-per-lane bank under SKRED_OPT_IN_PLACE = 2, read block by block (every report has
    arrived): True -- the block MUST run in place, False -- it must NOT, None -- the rule's inputs are not pinned by this reasoning.
    skred_bank_plan.c takes the in-place path when the list is not known to be empty and
        bound = (the list's length at the latest reporting launch) + (voices touched since that launch was issued) <= n / 6 + 64.
    The list at block b - 1's launch is what survived block b - 2 -- a subset of the voices in motion after it, in_motion[b - 1] --
    plus at most touched[b - 1]; so bound(b) <= in_motion[b - 1] + touched[b - 1] + touched[b].  A call that touches voices also
    tells the planner the list is not empty.  From below, bound(b) >= the part of touched[b] that does not depend on records.
    Block 0 builds its list from scratch and has no bound."""
    import env_forms
    limit = env_forms.in_place_limit(stage.n)
    out = []
    for b, f in enumerate(stage.fronts):
        if b == 0 or f["stamped"] > limit:
            out.append(False)
        elif f["stamped"] > 0 and stage.in_motion[b - 1] + stage.fronts[b - 1]["touched"] + f["touched"] <= limit:
            out.append(True)
        else:
            out.append(None)
    return out


def last_product(cur, g, frames):
    """the wrong model (f): the value the advance loop held when it found the voice arrived"""
    t = np.uint32(g[GM.TARGET]) & GM.ABS
    cur = np.uint32(cur)
    if not GM.usable(cur) or (cur ^ np.uint32(g[GM.TARGET])) >> np.uint32(31):
        return np.uint32(g[GM.TARGET])
    for _ in range((int(g[GM.CARRY]) + frames) >> 6):
        a = cur & GM.ABS
        if a == t:
            break
        cur = np.uint32(GM.mul(cur, g[GM.RATE_UP] if a < t else g[GM.RATE_DOWN]))
        if not GM.finite(cur) or ((cur & GM.ABS) >= t) == bool(a < t):
            break
    return cur if GM.finite(cur) else np.uint32(g[GM.TARGET])


def perform(stage, script, stems=False, after_block=None):
    """The script on a stage: the calls queued in front of each block, then the block.  Returns the blocks' oracle results."""
    refs = []
    for b, blk in enumerate(script):
        for kind, kw in blk["calls"]:
            getattr(stage, kind)(**kw)
        refs.append(stage.block(blk["frames"], stems))
        if after_block is not None:
            after_block(b, refs[-1])
    return refs
