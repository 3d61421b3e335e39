"""Whole performances on the device: tests/perf_fuzz.py's scripts on a device bank beside tests/perf_model.py's composed model, for every
default seed and configuration, in two forms.

CHECKED: after every call the call's d_result words (with the guard words behind them), its d_assigned, the owner, pedal and glide
arrays on every voice, the envelope clocks and every word a controller can store are the model's; after every block the state is the
oracle's bit for bit, the motion list missed nobody and the block ran on the kernel family the configuration names; on plain2 every
block's skred_bank_last_in_place is held to what the planner's rule pins (in_place_ok).  A failure names the block and the call.

FREE-RUNNING: the same script with no host synchronisation from the first control call to the end of the last block: every d_result,
d_assigned and count word of the performance lies in one device arena filled beforehand, every list a call reads is an earlier
call's d_assigned in that arena, and the stems of 64 tapped voices are copied on the stream into a per-block region of a second
arena (skred_bank_set_taps waits for the device, so the taps are set once, on one block-sized buffer, before the first call; the
pedal and the glide array, whose first call waits for the device too, are made to exist before the clock starts).  After
The model runs the whole script beforehand, so the timed loop holds device calls only.  The in-place verdicts are not checked in this
form: a queued block may be planned before the report of the one before it has arrived.  After ONE synchronise: the result arena word for word, the side arrays, clocks and controller words, the state, every block's tapped
stems bit for bit, the last block's mix within smoke()'s relative RMS of 1e-5, and less than 4 s of wall time (tests/test_updates.py's
bound for "no call sat out the staging ring's 5 s limit", not a performance claim).  A red free-running case replays in the checked
form: same seed, same configuration.
"""
import time

import numpy as np
import pytest

import chan_model as CHM
import ctl_model as CTL
import glide_model as GM
import pedal_model as PM
import perf_fuzz as PF
import perf_model as PMD
import slot_model as SM
from skred_amd import device
from test_idle import open_bank

FILL = -7
ARENA = 1 << 16
MAXF = max(PF.FRAMES)


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


class DeviceStage(PMD.Stage):
    """perf_model.Stage with a device bank beside it.  Every call is issued on the device with its result words (and its list) in the
    arena, then on the model; `free` defers every comparison to the end of the performance."""

    def __init__(self, dev, cfg, seed, free, bank=None):
        import torch
        bank, tables, g = bank or PF.make_bank(cfg, seed)
        super().__init__(bank, tables, g, cfg.K, cfg.vmask, cfg.mmask)
        self.cfg, self.seed, self.free = cfg, seed, free
        self.db = open_bank(dev, bank, tables, g, PF.setup(cfg))
        self.arena = torch.full((ARENA,), FILL, dtype=torch.int32, device="cuda")
        self.at, self.offsets, self.todo, self.where = 0, {}, [], "setup"
        self.mixes, self.families, self.in_place = [], [], []
        self.block_no = self.call_no = self.serial = 0
        self.twin = None
        torch.cuda.synchronize()

    def close(self):
        self.db.set_taps([], 0)
        self.db.close()

    def tell(self, what):
        return f"seed {self.seed}, {self.cfg.name}, {'free-running' if self.free else 'checked'}, {self.where}: {what}"

    def model(self, kind, *args):
        """the model's record of this call: computed here, or -- `twin`: a model that ran the whole script beforehand, so that the
        free-running form spends no host time between device calls -- looked up by the call's serial number"""
        if self.twin is None:
            return getattr(PMD.Stage, kind)(self, *args)
        out = self.twin.log[self.serial]
        assert out.kind == kind
        return out

    # ---- the arena
    def alloc(self, words):
        off = self.at
        self.at += words + 2                                                      # two guard words behind every region
        assert self.at <= ARENA
        return off

    def ptr(self, off):
        return self.arena.data_ptr() + 4 * off

    def put_list(self, entries):
        """a hand-made list into the arena (the pinned scenes; a performance's lists are d_assigned words)"""
        import torch
        entries = np.asarray(entries, np.int32)
        off = self.alloc(len(entries))
        self.arena[off:off + len(entries)] = torch.from_numpy(entries).cuda()
        torch.cuda.synchronize()
        ref = -1 - len(self.offsets)
        self.offsets[ref], self.lists[ref] = off, entries
        return ref

    def done(self, out, r=None, a=None):
        self.where = f"block {self.block_no}, call {self.call_no} ({out.kind})"
        self.call_no, self.serial = self.call_no + 1, self.serial + 1
        self.todo.append((out, r, a, self.where))
        if not self.free:
            import torch
            torch.cuda.synchronize()
            self.compare(self.arena[:self.at].cpu().numpy())
            self.same()
        return out

    def compare(self, words):
        for out, r, a, where in self.todo:
            self.where = where
            if r is not None:
                got = words[r:r + len(out.res) + 2]
                assert got[:len(out.res)].view(np.uint32).tolist() == out.res and (got[len(out.res):] == FILL).all(), \
                    self.tell(f"{out.kind}: d_result and its guard words {got.tolist()}, the model {out.res}")
            if a is not None:
                got, want = words[a:a + len(out.assigned) + 2], out.assigned
                bad = np.flatnonzero(got[:len(want)] != want)
                assert not len(bad), self.tell(f"{out.kind}: d_assigned[{bad[0]}] = {got[bad[0]]}, the model {want[bad[0]]}")
                assert (got[len(want):] == FILL).all(), self.tell(f"{out.kind}: words past d_assigned were written")
        self.todo = []

    def same(self):
        """the three side arrays, the envelope clocks and the controller words on every voice"""
        for name, got, want in (("owner", self.db.download_owners(), self.owner), ("pedal", self.db.download_pedals(), self.pedal),
                                ("glide", self.db.download_glide(), self.glide)):
            bad = np.flatnonzero((got != want).reshape(self.n, -1).any(axis=1))
            assert not len(bad), self.tell(f"{name} words differ at voice {bad[0]}: {got[bad[0]].tolist()} / the model {want[bad[0]].tolist()}")
        start, release = self.db.download_env_clocks()
        e = self.truth["voice_amp_envelope"]
        for name, got, want in (("sample_start", start, e["sample_start"]), ("sample_release", release, e["sample_release"])):
            bad = np.flatnonzero(got != want.astype(np.uint64))
            assert not len(bad), self.tell(f"{name} differs at voice {bad[0]}: {got[bad[0]]} / the model {want[bad[0]]}")
        a = self.bank.copy()
        self.db.download_ctl(a)
        assert not CTL.words_differ(a, self.truth), self.tell(f"controller words differ from the model: {CTL.words_differ(a, self.truth)}")

    # ---- one method per call: the device first, then the model
    def note_on_channel(self, notes, tags, iq, sq, match, cap):
        a, r = self.alloc(len(tags)), self.alloc(4)
        self.db.note_on_channel(notes, tags, iq, sq.c(), device.owner_match(*match), cap, self.vmask, self.ptr(a), self.ptr(r))
        self.offsets[self.serial] = a
        return self.done(self.model("note_on_channel", notes, tags, iq, sq, match, cap), r, a)

    def note_on_steal_slots(self, notes, n, iq, sq):
        a, r = self.alloc(n), self.alloc(3)
        self.db.note_on_steal_slots(notes, iq, sq.c(), self.vmask, self.ptr(a), self.ptr(r))
        self.offsets[self.serial] = a
        return self.done(self.model("note_on_steal_slots", notes, n, iq, sq), r, a)

    def note_on_idle_slots(self, notes, n, iq):
        a, r = self.alloc(n), self.alloc(2)
        self.db.note_on_idle_slots(notes, iq, self.vmask, self.ptr(a), self.ptr(r))
        self.offsets[self.serial] = a
        return self.done(self.model("note_on_idle_slots", notes, n, iq), r, a)

    def tag_slots(self, ref, tags):
        r = self.alloc(2)
        self.db.tag_slots(self.ptr(self.offsets[ref]), tags, self.K, 0, self.ptr(r))
        return self.done(self.model("tag_slots", ref, tags), r)

    def release_tags(self, first, count, tags):
        r = self.alloc(3)
        self.db.release_tags(first, count, self.K, self.vmask, tags, SM.STAMP_RELEASE, self.ptr(r))
        return self.done(self.model("release_tags", first, count, tags), r)

    def release_tags_pedal(self, first, count, tags, hold_all):
        r = self.alloc(4)
        self.db.release_tags_pedal(first, count, self.K, self.vmask, tags, hold_all, self.ptr(r))
        return self.done(self.model("release_tags_pedal", first, count, tags, hold_all), r)

    def stamp_owned_pedal(self, ref, tags, hold_all):
        r = self.alloc(4)
        self.db.stamp_owned_pedal(self.ptr(self.offsets[ref]), tags, self.K, self.vmask, hold_all, self.ptr(r))
        return self.done(self.model("stamp_owned_pedal", ref, tags, hold_all), r)

    def pedal_latch(self, first, count, match):
        r = self.alloc(2)
        self.db.pedal_latch(first, count, self.K, self.vmask, device.owner_match(*match), self.ptr(r))
        return self.done(self.model("pedal_latch", first, count, match), r)

    def pedal_up(self, first, count, match, flags):
        r = self.alloc(3)
        self.db.pedal_up(first, count, self.K, self.vmask, device.owner_match(*match), flags, self.ptr(r))
        return self.done(self.model("pedal_up", first, count, match, flags), r)

    def pedal_clear(self, first, count):
        self.db.pedal_clear(first, count)
        return self.done(self.model("pedal_clear", first, count))

    def stamp_match(self, first, count, match):
        r = self.alloc(2)
        self.db.stamp_match(first, count, self.K, self.vmask, device.owner_match(*match), SM.STAMP_RELEASE, self.ptr(r))
        return self.done(self.model("stamp_match", first, count, match), r)

    def ctl_range(self, ctls, first, count):
        r = self.alloc(2)
        self.db.ctl_range(ctls, first, count, self.vmask, self.ptr(r))
        return self.done(self.model("ctl_range", ctls, first, count), r)

    def ctl_match(self, ctls, first, count, match):
        r = self.alloc(3)
        self.db.ctl_match(ctls, first, count, self.vmask, device.owner_match(*match), self.ptr(r))
        return self.done(self.model("ctl_match", ctls, first, count, match), r)

    def ctl_owned_each(self, ctls, each, ref, tags):
        r = self.alloc(3)
        self.db.ctl_owned_each(ctls, each, self.vmask, self.ptr(self.offsets[ref]), tags, self.K, 0, self.ptr(r))
        return self.done(self.model("ctl_owned_each", ctls, each, ref, tags), r)

    def ctl_tags_each(self, ctls, each, first, count, tags):
        r = self.alloc(3)
        self.db.ctl_tags_each(ctls, each, first, count, self.vmask, tags, self.K, self.ptr(r))
        return self.done(self.model("ctl_tags_each", ctls, each, first, count, tags), r)

    def ctl_owned_each_filter(self, ctls, each, filt, fmask, ref, tags):
        r = self.alloc(3)
        self.db.ctl_owned_each_filter(ctls, each, filt, self.vmask, fmask, self.ptr(self.offsets[ref]), tags, self.K, 0, self.ptr(r))
        return self.done(self.model("ctl_owned_each_filter", ctls, each, filt, fmask, ref, tags), r)

    def ctl_tags_each_filter(self, ctls, each, filt, fmask, first, count, tags):
        r = self.alloc(3)
        self.db.ctl_tags_each_filter(ctls, each, filt, first, count, self.vmask, fmask, tags, self.K, self.ptr(r))
        return self.done(self.model("ctl_tags_each_filter", ctls, each, filt, fmask, first, count, tags), r)

    def glide_tags(self, glides, first, count, tags):
        r = self.alloc(3)
        self.db.glide_tags([g.c() for g in glides], first, count, self.K, self.vmask, tags, self.ptr(r))
        return self.done(self.model("glide_tags", glides, first, count, tags), r)

    def glide_owned(self, glides, ref, tags):
        r = self.alloc(3)
        self.db.glide_owned([g.c() for g in glides], self.K, self.vmask, self.ptr(self.offsets[ref]), tags, 0, self.ptr(r))
        return self.done(self.model("glide_owned", glides, ref, tags), r)

    def glide_advance(self, first, count, frames):
        r = self.alloc(2)
        self.db.glide_advance(first, count, frames, self.ptr(r))
        return self.done(self.model("glide_advance", first, count, frames), r)

    def glide_stop(self, first, count, snap):
        self.db.glide_stop(first, count, snap)
        return self.done(self.model("glide_stop", first, count, snap))

    def census(self, sq, match):
        r = self.alloc(3)
        self.db.find_steal_slots_match(sq.but(max_out=0).c(), device.owner_match(*match), 0, self.ptr(r))
        return self.done(self.model("census", sq, match), r)

    # ---- blocks
    def render(self, frames, out):
        self.db.render_mix(frames, out.data_ptr(), 2, 0, 0)
        self.families.append(self.db.last_kernel())
        if not self.free:                                                         # (queued blocks may plan before a report arrives: read block by block only)
            self.in_place.append(self.db.last_in_place())
        self.where = f"block {self.block_no} ({frames} frames)"
        self.block_no, self.call_no = self.block_no + 1, 0

    def family_ok(self):
        want = "two per lane" if self.cfg.two_per_lane else "one voice per lane"
        bad = [k for k in self.families if k != (3 if self.cfg.two_per_lane else 1)]      # SKRED_KERNEL_FAST2 / SKRED_KERNEL_FAST
        assert not bad, self.tell(f"a block ran on kernel family {bad[0]}, the configuration names {want}: {self.families}")

    def state_ok(self):
        a = self.bank.copy()
        self.db.download(a)
        bad = a.rw_equal(self.truth)
        assert not bad, self.tell(f"state differs from the oracle: {bad}")
        assert self.db.list_violations() == 0, self.tell(f"{self.db.list_violations()} voices moved off the motion list")

    def block(self, frames, stems=False):
        import torch
        out = torch.zeros(frames, 2, device="cuda")
        self.render(frames, out)
        ref = super().block(frames, stems)
        torch.cuda.synchronize()
        self.state_ok()
        self.same()
        self.family_ok()
        self.mixes.append(out.cpu().numpy())
        return ref


def mix_ok(st, got, ref):
    want = ref["mix"]
    err = float(np.sqrt(np.mean((got.astype(np.float64) - want) ** 2)) / np.sqrt(np.mean(want.astype(np.float64) ** 2)))
    print(st.tell(f"the last block's mix: relative rms {err:.2e}"))
    assert err <= 1e-5, st.tell(f"mix relative rms error {err}")


def run_script(st, script):
    refs = []
    for blk in script:
        for kind, kw in blk["calls"]:
            getattr(st, kind)(**kw)
        refs.append(st.block(blk["frames"]))
    return refs


def in_place_ok(st):
    """SKRED_OPT_IN_PLACE = 2, read block by block: skred_bank_last_in_place of every block whose answer perf_model.in_place_verdicts
    pins -- the blocks behind stamps, pedal-ups, AMP sweeps and velocities among them -- and at least PF.MIN_IN_PLACE of them in place."""
    want = PMD.in_place_verdicts(st)
    print(st.tell(f"in place per block {[int(x) for x in st.in_place]}, pinned {want}"))
    for b, (got, w) in enumerate(zip(st.in_place, want)):
        assert w is None or got == w, st.tell(f"block {b} behind {st.fronts[b]['kinds']}: in place {got}, the planner's rule says {w}")
    assert sum(1 for w in want if w) >= PF.MIN_IN_PLACE


# ---------------------------------------------------------------------------------------------- the two forms

@pytest.mark.gpu
@pytest.mark.parametrize("seed", PF.SEEDS)
@pytest.mark.parametrize("name", tuple(PF.CONFIGS))
def test_checked(dev, name, seed):
    cfg = PF.CONFIGS[name]
    st = DeviceStage(dev, cfg, seed, free=False)
    try:
        refs = run_script(st, PF.performance(seed, cfg))
        mix_ok(st, st.mixes[-1], refs[-1])
        if cfg.in_place == 2:
            in_place_ok(st)
        print(st.tell(f"{len(st.log)} calls, kernel families {sorted(set(st.families))}"))
    finally:
        st.close()


def tap_voices(st):
    """64 voices spread over the channels: the voices of the slots at rest (where the first notes land), then their neighbours"""
    out = []
    for first, count in st.cfg.ranges():
        idle = SM.idle_slots(st.truth, first, count, st.K, st.mmask, PF.WHICH, PF.SETTLE)
        vs = [int(s) + l for s in idle for l in range(st.K)][:14] + [first, first + count - 1]
        out.extend(vs)
    out = sorted(set(out))
    out += [v for v in range(st.n) if v not in set(out)][:64 - len(out)]
    return np.array(sorted(out[:64]), np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", PF.SEEDS)
@pytest.mark.parametrize("name", tuple(PF.CONFIGS))
def test_free_running(dev, name, seed):
    import torch
    cfg = PF.CONFIGS[name]
    script = PF.performance(seed, cfg)
    st = DeviceStage(dev, cfg, seed, free=True)
    try:
        voices = tap_voices(st)
        taps = torch.zeros((MAXF, len(voices), 2), dtype=torch.float32, device="cuda")
        stems = torch.zeros((len(script), MAXF, len(voices), 2), dtype=torch.float32, device="cuda")
        outs = [torch.zeros(blk["frames"], 2, device="cuda") for blk in script]
        st.db.set_taps(voices, taps.data_ptr())
        # the pedal array and the glide array come into being on their first call, which waits for the device once: both are made to
        # exist here, by calls on a tag nobody carries, so that nothing inside the performance waits (the late allocation has its own test)
        nobody = np.array([PF.tag_of(PF.CHANNELS[0], 1)], np.uint32)
        prime = (("release_tags_pedal", (0, st.whole[1], nobody, True)), ("glide_tags", ([GM.Glide(GM.FROM_SCALE, 1.01, 0.99, 0.5)], 0, st.whole[1], nobody)))
        for kind, args in prime:
            assert not any(getattr(st, kind)(*args).res[:2])
        torch.cuda.synchronize()
        st.compare(st.arena[:st.at].cpu().numpy())
        # the model runs the whole script first: the timed loop below holds device calls only
        twin = PMD.Stage(st.bank, st.tables, st.gl, cfg.K, cfg.vmask, cfg.mmask)
        for kind, args in prime:
            getattr(twin, kind)(*args)
        del twin.log[:]                                                           # (the script's `ref` serials count from its own first call)
        twin.at_front = 0
        refs = PMD.perform(twin, script, stems=True)
        st.twin, st.block_no, st.call_no, st.serial = twin, 0, 0, 0
        t0 = None
        for b, blk in enumerate(script):
            for kind, kw in blk["calls"]:
                t0 = t0 or time.perf_counter()
                getattr(st, kind)(**kw)
            st.render(blk["frames"], outs[b])
            stems[b, :blk["frames"]].copy_(taps[:blk["frames"]], non_blocking=True)   # on the stream, behind the block
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        for k in ("owner", "pedal", "glide", "truth", "gl", "log"):              # what the device is held to: the twin's end state
            setattr(st, k, getattr(twin, k))
        words = st.arena.cpu().numpy()
        st.compare(words)
        st.where = "the end"
        assert (words[st.at:] == FILL).all(), st.tell("arena words past the last region were written")
        st.same()
        st.state_ok()
        st.family_ok()
        got = stems.cpu().numpy()
        for b, (blk, ref) in enumerate(zip(script, refs)):
            want = np.ascontiguousarray(ref["stems"][:, voices, :])
            x = got[b, :blk["frames"]]
            bad = np.argwhere(x.view(np.uint32) != want.view(np.uint32))
            assert not len(bad), st.tell(f"block {b}: the stem of voice {voices[bad[0][1]]} differs at frame {bad[0][0]}: "
                                         f"{x[tuple(bad[0])]} / the oracle {want[tuple(bad[0])]}")
        mix_ok(st, outs[-1].cpu().numpy(), refs[-1])
        print(st.tell(f"{len(st.log)} calls, {wall:.3f} s from the first call to the synchronise, families {sorted(set(st.families))}"))
        assert wall < 4.0, st.tell(f"{wall:.2f} s from the first call to the synchronise")
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- pinned edges

def chord(gen, h, keys, cap=CHM.NO_CAP, min_age=0):
    iq, sq = gen.queries(h, min_age)
    return dict(notes=gen.notes(keys), tags=gen.tags(h, keys), iq=iq, sq=sq, match=CHM.channel(h.ch), cap=cap)


def late_script(gen, early):
    """a chord, blocks, and the first pedal call and the first glide call in the middle (`early`: ahead of the first note too)"""
    h = gen.hosts[1]
    keys = [60, 64, 67]
    tags = gen.tags(h, keys)
    nobody = gen.tags(h, [1])
    pre = [("release_tags_pedal", dict(first=h.range[0], count=h.range[1], tags=nobody, hold_all=True)),
           ("glide_tags", dict(glides=[GM.Glide(GM.FROM_SCALE, 1.01, 0.99, 0.5)], first=h.range[0], count=h.range[1], tags=nobody))]
    up, down = GM.per_64(400.0)
    return [dict(frames=64, calls=pre if early else []),
            dict(frames=37, calls=[("note_on_channel", chord(gen, h, keys))]),
            dict(frames=128, calls=[]),
            dict(frames=64, calls=[("release_tags_pedal", dict(first=h.range[0], count=h.range[1], tags=tags[:2], hold_all=True)),
                                   ("glide_tags", dict(glides=[GM.Glide(GM.FROM_SCALE, up, down, 0.5)] * 3, first=h.range[0],
                                                       count=h.range[1], tags=tags)),
                                   ("glide_advance", dict(first=h.range[0], count=h.range[1], frames=64))]),
            dict(frames=27, calls=[("glide_advance", dict(first=h.range[0], count=h.range[1], frames=27)),
                                   ("pedal_up", dict(first=h.range[0], count=h.range[1], match=CHM.channel(h.ch), flags=PM.LIFT_SUSTAIN))]),
            dict(frames=64, calls=[("glide_advance", dict(first=h.range[0], count=h.range[1], frames=64))])]


@pytest.mark.gpu
def test_side_arrays_allocated_in_the_middle_of_a_performance(dev):
    """The pedal array and the glide array come into being behind the first note (their allocation waits for the device once); a twin
    had both before its first note.  Both are held to the model call by call, and end with the same bytes."""
    cfg = PF.CONFIGS["patch"]
    late, twin = DeviceStage(dev, cfg, 0, free=False), DeviceStage(dev, cfg, 0, free=False)
    try:
        run_script(late, late_script(PF.Gen(0, cfg), False))
        run_script(twin, late_script(PF.Gen(0, cfg), True))
        assert [o.res for o in late.log] == [o.res for o in twin.log[2:]] and twin.log[0].res == [0, 0, 1, 0]
        assert late.log[2].res == [3 * cfg.K, 0, 0] and late.log[5].res[0] == 2
        a, b = late.bank.copy(), late.bank.copy()
        for st, x in ((late, a), (twin, b)):
            st.db.download(x)
            st.db.download_ctl(x)
        assert not a.rw_equal(b) and not CTL.words_differ(a, b)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(late.mixes, twin.mixes)), "the mixes of the two banks differ"
    finally:
        late.close()
        twin.close()


@pytest.mark.gpu
def test_victims_all_pending_and_all_gliding(dev):
    """Cap at count: three keys glide and are lifted under the pedal; three more keys steal exactly their slots.  The thieves' tag
    launch clears three pedal words and 3 * K glide words: the next advance moves nothing and the pedal-up releases nobody."""
    cfg = PF.CONFIGS["patch"]
    st = DeviceStage(dev, cfg, 0, free=False)
    gen = PF.Gen(0, cfg)
    h = gen.hosts[1]
    first, count = h.range
    old, new = [60, 64, 67], [72, 76, 79]
    up, down = GM.per_64(150.0)
    try:
        st.block(64)
        a = st.note_on_channel(**chord(gen, h, old))
        assert a.res == [3, 0, 0, 0]
        st.block(128)
        assert st.glide_tags([GM.Glide(GM.FROM_SCALE, up, down, 0.5)] * 3, first, count, gen.tags(h, old)).res == [3 * cfg.K, 0, 0]
        assert st.glide_advance(first, count, 64).res == [3 * cfg.K, 0]
        assert st.release_tags_pedal(first, count, gen.tags(h, old), True).res == [0, 0, 0, 3]
        st.block(37)
        b = st.note_on_channel(**chord(gen, h, new, cap=3))
        assert b.res == [3, 0, 3, 3] and sorted(b.assigned.tolist()) == sorted(a.assigned.tolist())
        assert st.events["theft of a pending slot"] == st.events["theft of a gliding slot"] == 3
        assert not st.pedal.any() and not st.glide.any()
        assert st.glide_advance(first, count, 37).res == [0, 0]
        assert st.pedal_up(first, count, CHM.channel(h.ch), PM.LIFT_SUSTAIN).res[:2] == [0, 0]
        st.block(64)
        assert st.release_tags_pedal(first, count, gen.tags(h, old + new), False).res == [3, 0, 3, 0]
        st.block(64)
    finally:
        st.close()


@pytest.mark.gpu
def test_1024_tags_in_one_note_off_under_the_pedal(dev):
    """The plain bank: 512 slots carry a tag each, the note-off names 1024 tags in an order of its own, every other one carried by
    nobody; the pedal holds all 512 back and its lift releases them."""
    cfg = PF.CONFIGS["plain"]
    st = DeviceStage(dev, cfg, 0, free=False)
    try:
        slots = np.random.default_rng(5).permutation(st.n)[:512].astype(np.int32)
        carried = (np.uint32(7 << 24) + np.arange(512, dtype=np.uint32) * np.uint32(2) + np.uint32(1)).astype(np.uint32)
        tags = np.random.default_rng(6).permutation(np.concatenate([carried, carried + np.uint32(1)]))
        assert st.tag_slots(st.put_list(slots), carried).res == [512, 0]
        st.block(64)
        assert st.release_tags_pedal(0, st.n, tags, True).res == [0, 0, 512, 512]
        assert int((st.pedal == PM.PENDING).sum()) == 512
        st.block(37)
        assert st.pedal_up(0, st.n, CHM.channel(7), PM.LIFT_SUSTAIN).res == [512, 0, st.n - 512]
        st.block(64)
    finally:
        st.close()


@pytest.mark.gpu
def test_a_sustained_gliding_chord_is_safe_from_the_neighbour_channel(dev):
    """A chord is struck, glides and is lifted under the pedal.  The neighbour channel then asks for more notes than its range has
    idle slots, with a steal range over the whole bank: the rest is dropped, because a burst cannot steal from another channel.  The
    pedal-up releases the chord, which glided on all the while."""
    cfg = PF.CONFIGS["patch"]
    st = DeviceStage(dev, cfg, 0, free=False)
    gen = PF.Gen(0, cfg)
    h, other = gen.hosts[1], gen.hosts[2]
    first, count = h.range
    keys = [60, 64, 67]
    up, down = GM.per_64(150.0)
    try:
        st.block(64)
        a = st.note_on_channel(**chord(gen, h, keys))
        assert st.glide_owned([GM.Glide(GM.FROM_SCALE, up, down, 0.5)] * 3, len(st.log) - 1, gen.tags(h, keys)).res == [3 * cfg.K, 0, 0]
        st.block(128)
        assert st.release_tags_pedal(first, count, gen.tags(h, keys), True).res == [0, 0, 0, 3]
        idle = len(SM.idle_slots(st.truth, other.range[0], other.range[1], cfg.K, cfg.mmask, PF.WHICH, PF.SETTLE))
        b = st.note_on_channel(**chord(gen, other, list(range(40, 40 + idle + 3))))
        assert b.res == [idle, 3, 0, 0] and not set(b.assigned.tolist()) & set(a.assigned.tolist())
        assert (st.owner[a.assigned] == gen.tags(h, keys)).all() and (st.pedal[a.assigned] == PM.PENDING).all()
        assert st.glide_advance(first, count, 128).res == [3 * cfg.K, 0]
        st.block(27)
        t_up = st.now()
        assert st.pedal_up(first, count, CHM.channel(h.ch), PM.LIFT_SUSTAIN).res[:2] == [3, 0]
        assert (st.truth["voice_amp_envelope"]["sample_release"][a.assigned] == t_up).all()
        assert st.glide_advance(first, count, 27).res[0] == 3 * cfg.K
        st.block(64)
    finally:
        st.close()
