"""The filter envelope of the fixed-point bank on the GPU (skred_fxbank_fenv_match / _fenv_owned_each / _fenv_tags_each / _download_fenv,
and the cutoff calls on a bank that has an fenv array), byte for byte.

After every call the device is held to tests/fx_fenv_model.py on top of tests/fx_cutoff_model.py: download_fenv == the model's eight
words per voice, download_cutoff == the model's cutoff words, the pedal, bend, glide and owner arrays == the model's, every word of the
bank (skred_fxbank_download and _download_params: the five coefficient words and their neighbours, the clocks) == the oracle's bank
after the model's stores, every d_result word == the model's count with the guard words past it untouched; mixes and stems of every
rendered block are compared bit for bit with oracle.cpuref.fx_render driven through the model.  The release clock the advance pass
reads is the oracle bank's sample_release, which every note-off path moves on the device and on the model together.

The scenes marked CLEAR RULE fail on tests/fx_fenv_model.py with CLEAR_RULE = False, those marked READ THE CLOCK with
READ_RELEASE_CLOCK = False (asserted here on the model alone) -- and on a library without the rule the device fails them against the
model as it stands.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import chan_model as CM
import fx_bend_model as BM
import fx_chan_model as FCM
import fx_cutoff_model as M
import fx_fenv_model as FM
import fx_glide_model as GM
import fx_live_model as live
import fx_pedal_model as PM
from skred_amd import fxbank as fxb
from test_fx_bend import mono_args
from test_fx_chan import assert_same_bank, whole_bank
from test_fx_cutoff import DeviceCutoffStage
from test_fx_fenv_cpu import cuttings
from test_fx_glide import FILL, dev_count, dev_list, padded_tags, ptr, sync
from test_fx_live import dev_i32, host_of, open_fx

pytestmark = pytest.mark.gpu

BAD, RANGE = -2, -4
SPAN = 256                                                       # SK_CONTROL_SPAN: voices or entries per workgroup of the control kernels
N = 600
R, E = M.Rec, FM.Rec
BOTH = M.BOTH
CH = 3
CHAN = (CH << 24, 0xFF000000)
ANY = (0, 0)
FAST = 0xFFFFFFFF                                                # a rate that lands in two steps at the most
CONTOUR = E(FM.REL, 8 << 16, 2 << 16, 1 << 15, 1 << 29, 1 << 28, 1 << 28)


def es(recs):
    return [r.c() for r in recs]


class DeviceFenvStage(DeviceCutoffStage, FM.FxFenvStage):
    """fx_fenv_model.FxFenvStage with a device bank beside it: every call runs on both, and the device is compared with the model."""

    def same(self, what):
        got = self.db.download_fenv()
        bad = np.flatnonzero((got != self.fenv).any(axis=1))
        assert not len(bad), f"{what}: fenv words differ at {bad[:8].tolist()}: {got[bad[:4]].tolist()} / {self.fenv[bad[:4]].tolist()}"
        got = self.db.download_pedals()
        assert np.array_equal(got, self.pedal), f"{what}: pedal words differ at {np.flatnonzero(got != self.pedal)[:8].tolist()}"
        super().same(what)

    def fenv_match(self, match, rec, rng=None):
        first, count = rng or self.whole
        res = self.result(4)
        self.db.fenv_match(first, count, match[0], match[1], rec.c(), res.data_ptr())
        return self.read(res, 4, "fenv_match", super().fenv_match(match, rec, rng))

    def fenv_tags(self, recs, tags, rng=None):
        first, count = rng or self.whole
        res = self.result(4)
        self.db.fenv_tags_each(es(recs), first, count, tags, res.data_ptr())
        return self.read(res, 4, f"fenv_tags_each of {len(tags)}", super().fenv_tags(recs, tags, rng))

    def fenv_list(self, recs, entries, tags, count=None):
        dl, dc, res = dev_list(entries), dev_count(count), self.result(4)
        self.db.fenv_owned_each(es(recs), dl.data_ptr(), tags, ptr(dc), res.data_ptr())
        return self.read(res, 4, "fenv_owned_each", super().fenv_list(recs, entries, tags, count))

    # the note-off paths
    def off(self, tags, hold_all, rng=None):
        first, count = rng or self.whole
        res = self.result(4)
        self.db.release_tags_pedal(first, count, tags, hold_all, res.data_ptr())
        return self.read(res, 4, "release_tags_pedal", super().off(tags, hold_all, rng))

    def plain_off(self, tags, rng=None):
        first, count = rng or self.whole
        res = self.result(3)
        self.db.release_tags(first, count, tags, fxb.STAMP_RELEASE, res.data_ptr())
        return self.read(res, 3, "release_tags", super().plain_off(tags, rng))

    def off_match(self, match, rng=None):
        first, count = rng or self.whole
        res = self.result(2)
        self.db.stamp_match(first, count, match[0], match[1], fxb.STAMP_RELEASE, res.data_ptr())
        return self.read(res, 2, "stamp_match", super().off_match(match, rng))

    def latch(self, match, rng=None):
        first, count = rng or self.whole
        res = self.result(2)
        self.db.pedal_latch(first, count, match[0], match[1], res.data_ptr())
        return self.read(res, 2, "pedal_latch", super().latch(match, rng))

    def up(self, match, flags, rng=None):
        first, count = rng or self.whole
        res = self.result(3)
        self.db.pedal_up(first, count, match[0], match[1], flags, res.data_ptr())
        return self.read(res, 3, "pedal_up", super().up(match, flags, rng))

    def retrigger(self, voices):
        self.db.stamp_list(dev_list(voices).data_ptr(), len(voices), fxb.STAMP_TRIGGER)
        super().retrigger(voices)
        self.same("a trigger stamp")


def stage(n=N, **kw):
    bank, pool, c0 = fxb.bank_fx(n)
    return DeviceFenvStage(bank, pool, c0, **kw)


def model_stage(n=N):
    bank, pool, c0 = fxb.bank_fx(n)
    return FM.FxFenvStage(bank, pool, c0)


def coeffs_of(st, v):
    return [int(st.filt[name][v]) for name in M.COEFFS]


# ---------------------------------------------------------------------------------------------- every call against the model

@pytest.mark.parametrize("n", [1, 65, SPAN - 1, SPAN + 1])
def test_every_call_against_the_model(n):
    """Banks of 1, 65, 255 and 257 voices, two channels interleaved.  A record on a bank without any side array (all withheld, and
    nothing but the arrays' allocation happens); the channel sweep with REL | START; records by note id in no order, ABS with a peak
    equal to the sustain; a list with a hole, an entry past the bank, a stolen tag and a count word; clamped voices; advances of
    several lengths with a note-off of the channel in between; blocks rendered between; a cutoff record and stops at the end."""
    st = stage(n, stems=n <= SPAN + 1)
    gen = np.random.default_rng(400 + n)
    try:
        v = np.arange(n, dtype=np.int32)
        tags = (((v % 2 + CH).astype(np.uint32)) << np.uint32(24)) | (1 + v).astype(np.uint32)
        st.strike(v, tags)
        mine = int((v % 2 == 0).sum())
        assert not st.db.download_fenv().any()
        assert st.fenv_match(CHAN, CONTOUR) == [0, mine, n - mine, 0] and not st.fenv.any() and not st.cut.any()
        res = st.cut_match(ANY, R(M.TRACK | BOTH, M.track_q24(2), 3 << 15, 1))
        has = int((st.cut[:, M.W] != 0).sum())
        assert res[0] == has and has >= 1
        res = st.fenv_match(CHAN, E(FM.REL | FM.START, 40 << 16, 2 << 16, 1 << 15, 1 << 29, 1 << 28, 1 << 28, start=1 << 15))
        assert res[0] + res[1] == mine and res[2] == n - mine and (n < 65 or res[3] >= 1)
        assert st.cut_advance(64)[0] == res[0]
        st.block()
        order = gen.permutation(n)
        recs = [E(FM.ABS, 1 << 27, 1 << 27, 1 << 22, FAST, 1 << 30, 1 << 30) if k % 3 else
                E(FM.ABS | FM.START, int(st.cut[k, M.W]) or (1 << 24), 1 << 25, 1 << 23, 5, 1 << 29, FAST, start=int(st.cut[k, M.W]) or (1 << 24))
                for k in range(n)]
        for at in range(0, n, 100):
            pick = order[at:at + 100]
            st.fenv_tags([recs[i] for i in pick], tags[pick])
        lst = v[order].tolist() + [-1, n, n + 7]
        ltags = tags[order].tolist() + [5, 6, 7]
        if n > 1:
            ltags[0] ^= 1
        lrecs = [CONTOUR] * (n + 3)
        st.fenv_list(lrecs, lst, ltags, count=max(1, n // 2))
        res = st.fenv_list(lrecs, lst, ltags)
        assert res[2] == (1 if n > 1 else 0) and res[0] + res[1] == n - res[2]
        st.fenv_list(lrecs, lst, ltags, count=5000)
        for k, frames in enumerate((64, 100, 28, 1, 63, 640, 64)):
            if k == 3:
                assert st.off_match(CHAN)[0] == mine               # the channel's note-offs: its contours release in the next pass
            st.cut_advance(frames)
            if k in (0, 3, 4, 6):
                st.block()
        released = (st.fenv[:, FM.STAGE] == FM.RELEASE).sum() + (st.fenv[v % 2 == 0, FM.STAGE] == FM.OFF).sum()
        assert released >= min(mine, has)
        if n > 1:
            st.cut_tags([R(M.TRACK, M.track_q24(1))], tags[1:2])
        third = max(1, n // 3)
        st.cut_stop(True, (0, third))
        if n > third:
            st.cut_stop(False, (third, n - third))
        assert not st.fenv.any() and not st.cut[:, M.TARGET].any()
        assert st.cut_advance(64) == [0, 0]
        st.block()
    finally:
        st.close()


def test_counts_with_holes_stolen_tags_a_count_below_n_and_a_channel_match():
    """600 voices, the range [37, 537): 1, 2, 1 023 and 1 024 tags in no order with tags nobody carries and tags carried outside the
    range; four channels interleaved, one of them swept; voices stolen between the cutoff and the envelope keep no record."""
    st, rng = stage(N, stems=False), (37, 500)
    gen = np.random.default_rng(611)
    try:
        heads = np.arange(rng[0], rng[0] + rng[1], dtype=np.int32)
        tags = ((((heads % 4) + CH).astype(np.uint32)) << np.uint32(24)) | (1 + np.arange(len(heads))).astype(np.uint32)
        tagged = np.arange(len(heads)) % 5 != 4
        own, own_tags = heads[tagged], tags[tagged]
        st.strike(own, own_tags)
        st.tag([0, N - 1], [(CH << 24) | 0xFFFF, (CH << 24) | 0xFFFE])
        st.cut_match(ANY, R(M.TRACK | BOTH, M.track_q24(3), 1 << 16, 2))
        res = st.fenv_match(CHAN, CONTOUR, rng)
        mine = int(((own_tags >> 24) == CH).sum())
        assert res[0] + res[1] == mine and res[2] == rng[1] - mine and mine > 80
        order, at = gen.permutation(len(own)), 0
        for m in (1, 2, 1023, 1024):
            pick = order[at:at + min(m, 120)]
            at += len(pick)
            t = padded_tags(own_tags[pick], m)
            recs = [E(FM.REL if k % 2 else FM.ABS, (3 << 16) if k % 2 else (1 << 27), (1 << 16) if k % 2 else (1 << 25), (1 << 14) if k % 2 else (1 << 21),
                      1 + k, 1 << 27, 1 << 27) for k in range(m)]
            p = gen.permutation(m)
            res = st.fenv_tags([recs[i] for i in p], t[p], rng)                       # the records must follow their tags through the sort
            assert res[0] + res[1] == len(pick) and res[2] == 0
        assert st.fenv_tags([CONTOUR], [(CH << 24) | 0xFFFF], rng) == [0, 0, 0, 0]   # carried below the range only
        st.tag(own[:3], own_tags[:3] + np.uint32(0x100))                              # three voices stolen: the old tags find nobody
        assert not st.fenv[own[:3]].any()
        assert st.fenv_tags([CONTOUR] * 3, own_tags[:3], rng) == [0, 0, 0, 0]
        assert st.fenv_list([CONTOUR] * 4, [int(own[0]), int(own[5]), -1, N], [int(own_tags[0]), int(own_tags[5]), 5, 6]) == [1, 0, 1, 0]
        assert st.fenv_list([CONTOUR] * 4, own[4:8], own_tags[4:8], count=2)[0] + 0 <= 2
        st.cut_advance(64)
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- cuttings, the landed release

def test_three_block_cuttings_and_a_landed_release_equals_an_abs_twin():
    """3 072 frames advanced in 64-frame blocks, in odd blocks of 1 to 200 frames and in one large block per call, on three banks of
    130 voices, with note-offs at four frames on and off the grid (a block is cut at every call): each bank is held to the model after
    every call, and every pair is compared at every multiple of 64 both stop at.  Then the contours run out, and every voice whose
    release landed equals a twin set with ABS at w_end in all eight cutoff words and the five coefficients."""
    n, total, marks = 130, 64 * 48, (64 * 7, 777, 1601, 64 * 40 + 63)
    at64, stages = [], []
    try:
        for blocks in cuttings(total, marks, 3):
            st = stage(n, stems=False)
            stages.append(st)
            v = np.arange(n, dtype=np.int32)
            tags = (0x03000001 + v).astype(np.uint32)
            st.strike(v, tags)
            gen = np.random.default_rng(5)
            w0 = [int(np.exp2(gen.uniform(20, 30))) for _ in range(n)]
            assert st.cut_tags([R(M.ABS | BOTH, w, 3 << 15, 1 + k % 5) for k, w in enumerate(w0)], tags) == [n, 0, 0, 0]
            recs = [E(FM.REL, int(np.exp2(gen.uniform(14, 19))), int(np.exp2(gen.uniform(14, 18))), int(np.exp2(gen.uniform(13, 17))),
                      int(np.exp2(gen.uniform(22, 31.9))), int(np.exp2(gen.uniform(22, 31.9))), int(np.exp2(gen.uniform(24, 31.9)))) for _ in range(n)]
            assert st.fenv_tags(recs, tags)[0] == n
            seen, t = {}, 0
            for frames in blocks:
                for k, m in enumerate(marks):
                    if t == m:
                        group = v[v % 5 == k]
                        assert st.plain_off(tags[group])[0] == len(group)
                st.cut_advance(frames)
                t += frames
                if t % 64 == 0:
                    seen[t] = (st.db.download_cutoff()[:, :2].copy(), whole_bank(st.db, st.truth))
            at64.append(seen)
        assert len(at64[0]) == 48 and len(at64[2]) >= 2
        compared = 0
        for a, b in itertools.combinations(range(3), 2):                             # every pair, at every multiple of 64 both stop at
            for t in sorted(set(at64[a]) & set(at64[b])):
                assert np.array_equal(at64[a][t][0], at64[b][t][0]), (a, b, t)
                assert_same_bank(at64[b][t][1], at64[a][t][1], f"cuttings {a} and {b} at frame {t}")
                compared += 1
        assert compared >= 5
        st, twin = stages[0], stages[1]
        for _ in range(40):
            if st.cut_advance(65536) == [0, 0]:
                break
        landed = np.flatnonzero((v % 5 != 4) & (st.fenv[:, FM.STAGE] == FM.OFF))
        assert len(landed) >= n // 2 and not st.cut[landed, M.TARGET].any() and not st.cut[landed, M.CARRY].any()
        twin.cut_stop(False)
        assert twin.cut_tags([R(M.ABS, int(st.cut[x, M.W])) for x in landed], tags[landed]) == [len(landed), 0, 0, 0]
        assert np.array_equal(twin.db.download_cutoff()[landed], st.db.download_cutoff()[landed])
        a, b = whole_bank(st.db, st.truth), whole_bank(twin.db, twin.truth)
        for name in M.COEFFS:
            assert np.array_equal(a[name][landed], b[name][landed]), name
    finally:
        for st in stages:
            st.close()


# ---------------------------------------------------------------------------------------------- READ THE CLOCK

def release_scene(st):
    """READ THE CLOCK.  Four notes rest in sustain.  A note-off held back by the sustain pedal, one held back by sostenuto, then
    stamp_match and release_tags: no envelope call at any of them -- each contour enters its release in the first advance after ITS
    clock was stamped, and not before."""
    v = np.array([10, 64, 255, 300], np.int32)
    tags = ((CH << 24) + 60 + np.arange(4)).astype(np.uint32)
    st.strike(v, tags)
    assert st.cut_tags([R(M.ABS | BOTH, 1 << 26, 3 << 15, 1)] * 4, tags) == [4, 0, 0, 0]
    assert st.fenv_tags([E(FM.ABS, 1 << 26, 1 << 26, 1 << 22, 5, 6, 1 << 27)] * 4, tags) == [4, 0, 0, 0]
    stages = lambda: st.fenv[v, FM.STAGE].tolist()
    assert st.cut_advance(64) == [0, 0] and stages() == [FM.SUSTAIN] * 4
    st.block()
    assert st.latch(CHAN)[0] == 4                                    # sostenuto down: all four latched
    assert st.off(tags[:1], True) == [0, 0, 0, 1]                    # note-off of voice 10 with the sustain pedal down: held back
    assert st.off(tags[1:2], False) == [0, 0, 0, 1]                  # note-off of voice 64 without it: held back by the latch
    assert st.cut_advance(64) == [0, 0] and stages() == [FM.SUSTAIN] * 4, "a held-back note-off released a contour"
    st.block()
    assert st.up(CHAN, PM.LIFT_SOSTENUTO | PM.SUSTAIN_DOWN)[0] == 0  # sostenuto up under sustain: both still held back
    assert st.cut_advance(64) == [0, 0] and stages() == [FM.SUSTAIN] * 4
    assert st.up(CHAN, PM.LIFT_SUSTAIN)[0] == 2                      # the sustain pedal goes up: both clocks are stamped now
    assert st.cut_advance(64) == [2, 0] and stages() == [FM.RELEASE, FM.RELEASE, FM.SUSTAIN, FM.SUSTAIN], "READ THE CLOCK: let go by the pedal"
    assert (st.cut[v[:2], M.W] < 1 << 26).all() and all(coeffs_of(st, x) == M.coeffs(1, int(st.cut[x, M.W]), 3 << 15) for x in v[:2])
    st.block()
    assert st.off_match((int(tags[2]), 0xFFFFFFFF))[0] == 1
    assert st.cut_advance(1) == [3, 0] and stages()[2] == FM.RELEASE, "READ THE CLOCK: stamp_match"
    assert st.plain_off(tags[3:])[0] == 1
    assert st.cut_advance(63) == [4, 0] and stages() == [FM.RELEASE] * 4, "READ THE CLOCK: release_tags"
    st.block()
    st.retrigger(v[:1])                                              # a trigger stamp alone does not restart: it goes on releasing
    assert st.cut_advance(64) == [4, 0] and stages()[0] == FM.RELEASE
    for _ in range(60):
        if st.cut_advance(4096) == [0, 0]:
            break
    assert not st.fenv[v].any() and (st.cut[v, :5] == [1 << 22, 0, 0, 0, 0]).all()
    st.block()


def test_release_without_a_host_call():
    st = stage()
    try:
        release_scene(st)
    finally:
        st.close()


def test_the_release_scene_fails_on_a_model_that_does_not_read_the_clock(monkeypatch):
    release_scene(model_stage())
    monkeypatch.setattr(FM, "READ_RELEASE_CLOCK", False)
    with pytest.raises(AssertionError, match="READ THE CLOCK"):
        release_scene(model_stage())


# ---------------------------------------------------------------------------------------------- CLEAR RULE

def clear_scene(st):
    """CLEAR RULE.  A thief's tag launch, a cutoff record and cutoff_stop each end the contours they touch -- a moving one and one
    resting in sustain -- and leave the others; a withheld cutoff record leaves the contour."""
    v = np.arange(100, 108, dtype=np.int32)
    tags = ((CH << 24) + 1 + np.arange(8)).astype(np.uint32)
    st.strike(v, tags)
    assert st.cut_tags([R(M.ABS | BOTH, 1 << 26, 3 << 15, 1)] * 8, tags) == [8, 0, 0, 0]
    moving, resting = E(FM.ABS, 1 << 28, 1 << 25, 1 << 22, 1 << 24, 6, 7), E(FM.ABS, 1 << 26, 1 << 26, 1 << 22, 5, 6, 7)
    assert st.fenv_tags([moving, resting] * 4, tags) == [8, 0, 0, 0]
    assert st.cut_advance(64) == [4, 0] and st.fenv[v, FM.STAGE].tolist() == [FM.ATTACK, FM.SUSTAIN] * 4
    st.strike(v[:2], tags[:2] + np.uint32(0x100))                    # two thieves
    assert not st.fenv[v[:2]].any() and not st.cut[v[:2]].any(), "CLEAR RULE: the thief inherited a contour"
    assert st.cut_advance(64) == [3, 0]
    assert st.cut_tags([R(M.ABS, 1 << 25), R(M.ABS | M.GLIDE, 1 << 27, up_q32=9, down_q32=9)], tags[2:4]) == [2, 0, 0, 0]
    assert not st.fenv[v[2:4]].any(), "CLEAR RULE: a cutoff record left the contour"
    assert st.cut[v[2]].tolist() == [1 << 25, 0, 0, 0, 0, 3 << 15, 1, 0] and st.cut[v[3], :5].tolist() == [1 << 26, 1 << 27, 9, 9, 0]
    st.cut_stop(False, (int(v[4]), 2))
    assert not st.fenv[v[4:6]].any(), "CLEAR RULE: cutoff_stop left a contour (the one resting in sustain has no target)"
    assert st.cut[v[5]].tolist() == [1 << 26, 0, 0, 0, 0, 3 << 15, 1, 0] and st.cut[v[4], M.TARGET] == 0
    assert st.fenv[v[6:], FM.STAGE].tolist() == [FM.ATTACK, FM.SUSTAIN]
    assert st.cut_advance(64) == [2, 0]                              # the glide of voice 103 and the attack of voice 106
    st.off_match(ANY)
    assert st.cut_advance(64) == [3, 0] and st.fenv[v, FM.STAGE].tolist() == [0] * 6 + [FM.RELEASE] * 2
    st.block()


def test_cutoff_records_stops_and_thieves_end_contours():
    st = stage()
    try:
        clear_scene(st)
    finally:
        st.close()


def test_the_clear_scene_fails_on_a_model_without_the_clear_rule(monkeypatch):
    clear_scene(model_stage())
    monkeypatch.setattr(FM, "CLEAR_RULE", False)
    with pytest.raises(AssertionError, match="CLEAR RULE"):
        clear_scene(model_stage())


def test_thief_and_restruck_key_through_note_on_channel():
    """Mono mode (cap 1, min_age 0) under a contour: the key is struck again through skred_fxbank_note_on_channel, so the new note takes
    the old note's voice and the call's own tag launch is the one that clears the fenv words beside the others; the coefficients stay.
    Then the header's order on the new note: cutoff, then fenv."""
    st = stage()
    tag, v = [(CH << 24) | 60], 300
    try:
        st.strike([v], tag, [40000003])
        assert st.cut_tags([R(M.TRACK | BOTH, M.track_q24(1), 2 << 16, 1)], tag) == [1, 0, 0, 0]
        assert st.fenv_tags([CONTOUR], tag) == [1, 0, 0, 0]
        assert st.cut_advance(64) == [1, 0] and st.fenv[v, FM.STAGE] == FM.ATTACK
        st.block()
        held = coeffs_of(st, v)
        iq, sq, chan = mono_args(st.n, CH)
        want, res, _ = FCM.burst(st.truth, st.now(), st.owner, iq, sq, chan, 1, 1)
        assert want.tolist() == [v] and res == [1, 0, 1, 1], "the new note must steal the channel's only voice"
        notes = [fxb.FxNoteC(53393781, 20000, 0x01234567, 700, 32000, fxb.NOTE_SET_PHASE | fxb.NOTE_SET_PAN)]
        da, dr = dev_i32(3), dev_i32(6)
        sync()
        st.db.note_on_channel(notes, iq, sq.c(), chan[0], chan[1], 1, tag, da.data_ptr(), dr.data_ptr())
        live.place_notes(st.truth, notes, want, 1, 0, st.now())
        GM.tag_list(st.owner, st.glide, want, tag)
        BM.tag_clear(st.bend, want, 1)
        M.tag_clear(st.cut, want, 1)
        FM.tag_clear(st.fenv, want, 1)
        sync()
        assert host_of(da).tolist() == [v, FILL, FILL] and host_of(dr).tolist() == res + [FILL, FILL]
        assert not st.fenv[v].any() and not st.cut[v].any()
        st.same("the re-strike")
        assert st.cut_advance(64) == [0, 0] and coeffs_of(st, v) == held
        st.block()
        assert st.fenv_tags([CONTOUR], tag) == [0, 1, 0, 0], "the new note inherited the old note's cutoff word"
        assert st.cut_tags([R(M.TRACK | BOTH, M.track_q24(2), 3 << 16, 1)], tag) == [1, 0, 0, 0]
        assert st.fenv_tags([CONTOUR], tag) == [1, 0, 0, 0]
        w = (53393781 * M.track_q24(2)) >> 27
        assert st.fenv[v, 1:4].tolist() == [min(M.W_MAX, w * 8), w * 2, w >> 1]
        st.cut_advance(64)
        st.block()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- rendered, purity

def test_an_enveloped_filtered_chord_renders_as_the_oracle_fed_the_model_coefficients():
    """Eight filtered notes under contours that open, fall and close: every block of the device equals oracle.cpuref.fx_render on the
    bank that received the model's coefficient stores (st.block compares mix and stems bit for bit)."""
    st = stage()
    try:
        filtered = np.flatnonzero(st.bank["filter_mode"] != 0)
        assert len(filtered) >= 8
        v = filtered[:: max(1, len(filtered) // 8)][:8].astype(np.int32)
        tags = ((CH << 24) + 60 + np.arange(8)).astype(np.uint32)
        st.strike(v, tags)
        assert st.cut_tags([R(M.TRACK | BOTH, M.track_q24(2), 3 << 16, 1 + k % 5) for k in range(8)], tags)[0] == 8
        assert st.fenv_tags([E(FM.REL | FM.START, 6 << 16, 2 << 16, 1 << 15, 1 << 30, 1 << 29, 1 << 29, start=1 << 15)] * 8, tags)[0] == 8
        before = [coeffs_of(st, x) for x in v]
        for k in range(10):
            if k == 6:
                assert st.plain_off(tags)[0] == 8
            st.cut_advance(64)
            mix, _ = st.block()
            assert np.abs(mix).max() > 0
        assert [coeffs_of(st, x) for x in v] != before and (st.fenv[v, FM.STAGE] == FM.RELEASE).any()
    finally:
        st.close()


def test_calls_that_list_nobody_leave_the_bank_and_the_render_alone():
    """Envelope calls that reach nobody -- a match nobody satisfies, foreign tags, a list of holes, advances over no contour -- leave
    every byte of the bank and the rendered blocks identical to a twin without them; a bank without the array downloads zeros."""
    st = stage()
    bare = open_fx(st.bank, st.pool, st.now())
    try:
        assert not bare.download_fenv().any() and not bare.download_cutoff().any()
        voices = np.arange(100, 140, dtype=np.int32)
        tags = ((CH << 24) + 1 + np.arange(40)).astype(np.uint32)
        bare.tag_list(dev_list(voices).data_ptr(), tags)
        st.tag(voices, tags)
        for k in range(4):
            if k == 1:
                assert st.fenv_match(CM.channel(9), CONTOUR) == [0, 0, N, 0]
                assert st.fenv_tags([CONTOUR] * 3, [0x09000001, 0x09000002, 0x09000003]) == [0, 0, 0, 0]
                assert st.fenv_list([CONTOUR] * 3, [100, 101, -1], [0x09000009, int(tags[1]) ^ 1, 5]) == [0, 0, 2, 0]
                assert st.fenv_match(CHAN, CONTOUR) == [0, 40, N - 40, 0]            # no cutoff word yet: every record withheld
            if k == 2:
                assert st.cut_advance(64) == [0, 0]
                st.cut_stop(True)
            mix, stems = st.block()
            got_mix, got_stems = bare.render_host(st.F, st.INTERP, want_stems=True)
            assert (got_mix == mix).all() and (got_stems == stems).all(), f"block {k}: the bank without envelope calls renders another block"
        assert_same_bank(whole_bank(bare, st.truth), st.truth, "the bank without envelope calls")
        assert not st.fenv.any() and not st.cut.any() and not bare.download_fenv().any()
    finally:
        st.close()
        bare.close()


# ---------------------------------------------------------------------------------------------- combinations

def test_all_side_arrays_at_once():
    """A bank that holds the owner, pedal, glide, bend, cutoff and fenv arrays: a REL contour on a tracked base read under a bend while
    the voice glides; one tag launch is followed by the pedal, glide, bend, cutoff and fenv clears, each on the tagged voices only."""
    st = stage()
    try:
        v = np.arange(200, 232, dtype=np.int32)
        tags = ((CH << 24) + 1 + np.arange(32)).astype(np.uint32)
        st.strike(v, tags)
        assert st.off(tags[:20], True) == [0, 0, 0, 20]                              # sustain is down: held back, PENDING
        assert st.wheel(CHAN, BM.ratio_of(7.0)) == [32, 0, N - 32]
        u, d = GM.per_64(100.0)
        assert st.start([GM.Glide(GM.FROM_SCALE, u, d, GM.scale_q16(-3))] * 32, tags) == [32, 0, 0]
        assert st.advance(64) == [32, 0]
        assert st.cut_match(CHAN, R(M.TRACK | BOTH, M.track_q24(2), 1 << 16, 1)) == [32, 0, N - 32, 0]
        assert st.fenv_match(CHAN, CONTOUR)[:3] == [32, 0, N - 32]                   # (8 x a tracked base leaves the box on some: clamped)
        assert (st.fenv[v, FM.W_SUSTAIN] == np.minimum(M.W_MAX, 2 * st.cut[v, M.W].astype(np.int64))).all()
        assert st.cut_advance(64) == [32, 0] and st.pedal[v[:20]].all()
        st.block()
        again = v[8:24]
        st.tag(list(again) + [-1, N], list(tags[8:24] + np.uint32(0x100)) + [5, 6])   # new notes on sixteen of the voices
        assert not st.fenv[again].any() and not st.cut[again].any() and not st.bend[again].any() and not st.glide[again].any()
        assert not st.pedal[again].any() and st.pedal[v[:8]].all()
        assert st.fenv[v[:8], FM.STAGE].all() and st.fenv[v[24:], FM.STAGE].all()
        assert st.cut_advance(64) == [16, 0] and st.advance(64) == [16, 0]
        assert st.up(CHAN, PM.LIFT_SUSTAIN)[0] == 8                                  # the pedal goes up: eight held-back note-offs
        assert st.cut_advance(64) == [16, 0] and (st.fenv[v[:8], FM.STAGE] == FM.RELEASE).all() and (st.fenv[v[24:], FM.STAGE] != FM.RELEASE).all()
        st.block()
    finally:
        st.close()


def test_envelopes_through_a_shard():
    """One rank, local indices: the channel sweep, records by id, an advance that releases and a stop through skred_fxshard_bank()."""
    from skred_amd.sharded import _lib
    b, pool, c0 = fxb.bank_fx(N)
    L = fxb._bind(_lib())
    L.skred_shard_destroy.argtypes = [C.c_void_p]
    L.skred_shard_destroy.restype = None
    h = C.c_void_p()
    assert L.skred_fxshard_create(0, 0, 1, 0, b.n, C.byref(h)) == 0
    try:
        fx = fxb.DeviceFxBank.borrowed(L.skred_fxshard_bank(h), b.n)
        fx.set_tables(pool)
        cb = b.as_c()
        assert L.skred_fxshard_upload(h, C.byref(cb)) == 0
        fx.set_sample_count(c0)
        st = DeviceFenvStage(b, pool, c0, db=fx)
        t = [(CH << 24) | (60 + k) for k in range(3)]
        st.strike([63, 64, 256], t)
        assert st.cut_match(CHAN, R(M.TRACK | BOTH, M.track_q24(2), 1 << 16, 1), (37, 500)) == [3, 0, 497, 0]
        assert st.fenv_match(CHAN, CONTOUR, (37, 500)) == [3, 0, 497, 0]
        st.block()
        assert st.fenv_tags([E(FM.ABS | FM.START, 1 << 27, 1 << 27, 1 << 23, FAST, 5, FAST, start=1 << 26)] * 2, t[:2], (37, 500)) == [2, 0, 0, 0]
        assert st.cut_advance(128, (37, 500)) == [1, 2]
        assert st.plain_off(t[:1], (37, 500))[0] == 1
        assert st.cut_advance(128, (37, 500)) == [1, 1] and not st.fenv[63].any() and st.cut[63, :5].tolist() == [1 << 23, 0, 0, 0, 0]
        st.block()
        st.cut_stop(True)
        assert not st.fenv.any()
        st.block()
    finally:
        L.skred_shard_destroy(h)


def test_refusals_write_nothing():
    st = stage()
    n = st.n
    try:
        L = st.db.L
        st.tag([8, 16], [5, 6])
        assert st.cut_tags([R(M.ABS | BOTH, 1 << 25, 1 << 16, 1)], [5]) == [1, 0, 0, 0]
        assert st.fenv_tags([CONTOUR], [5]) == [1, 0, 0, 0]                          # the array exists, voice 8 has a contour
        dl = dev_list([8, 16, 24, 32])
        res = dev_i32(5)
        sync()
        good, zero, dup = fxb._tags([5, 6, 7, 8]), fxb._tags([5, 0, 7, 8]), fxb._tags([5, 6, 5, 8])
        ok = fxb.fx_fenv_array(es([CONTOUR] * 4))
        bad = fxb.fx_fenv_array(es([CONTOUR] * 3 + [E(FM.ABS | FM.REL, 1 << 24, 1 << 24, 1 << 24, 5, 6, 7)]))
        far = fxb.fx_fenv_array(es([E(FM.ABS, M.W_MAX + 1, 1 << 24, 1 << 24, 5, 6, 7)]))
        still = fxb.fx_fenv_array(es([E(FM.REL, 1 << 16, 1 << 16, 1 << 16, 5, 0, 7)]))
        m, never = fxb.OwnerMatchC(int(CHAN[0]), int(CHAN[1])), fxb.OwnerMatchC(1, 0xFF000000)
        vp = lambda a: C.cast(a, C.c_void_p)
        h, d, rs, r, t = st.db.h, dl.data_ptr(), res.data_ptr(), vp(ok), good.ctypes.data
        FMt, FO, FT, DF = L.skred_fxbank_fenv_match, L.skred_fxbank_fenv_owned_each, L.skred_fxbank_fenv_tags_each, L.skred_fxbank_download_fenv
        assert FMt(None, 0, n, C.byref(m), r, rs, None) == BAD and FMt(h, 0, n, None, r, rs, None) == BAD and FMt(h, 0, n, C.byref(m), None, rs, None) == BAD
        assert FMt(h, 0, n, C.byref(m), vp(far), rs, None) == RANGE and FMt(h, 0, n, C.byref(m), vp(still), rs, None) == BAD
        assert FMt(h, 0, n, C.byref(never), r, rs, None) == BAD and FMt(h, 0, n + 1, C.byref(m), r, rs, None) == RANGE
        assert FMt(h, 0, 0, C.byref(m), r, rs, None) == RANGE and FMt(h, -1, 4, C.byref(m), r, rs, None) == RANGE and FMt(h, n, 1, C.byref(m), r, rs, None) == RANGE
        assert FO(None, r, d, t, 4, None, rs, None) == BAD and FO(h, None, d, t, 4, None, rs, None) == BAD
        assert FO(h, r, None, t, 4, None, rs, None) == BAD and FO(h, r, d, None, 4, None, rs, None) == BAD
        assert FO(h, r, d, zero.ctypes.data, 4, None, rs, None) == BAD and FO(h, r, d, t, -1, None, rs, None) == BAD
        assert FO(h, vp(bad), d, t, 4, None, rs, None) == BAD
        assert FT(None, r, 0, n, t, 4, rs, None) == BAD and FT(h, None, 0, n, t, 4, rs, None) == BAD
        assert FT(h, r, 0, n, dup.ctypes.data, 4, rs, None) == BAD and FT(h, r, 0, n, zero.ctypes.data, 4, rs, None) == BAD
        assert FT(h, vp(bad), 0, n, t, 4, rs, None) == BAD and FT(h, vp(bad), 0, n + 1, t, 4, rs, None) == BAD
        assert FT(h, r, 0, n + 1, t, 4, rs, None) == RANGE and FT(h, r, -1, 4, t, 4, rs, None) == RANGE and FT(h, r, 0, 0, t, 4, rs, None) == RANGE
        out = np.full(64, 9, np.uint32)
        assert DF(h, out.ctypes.data, n - 2, 4) == RANGE and DF(h, None, 0, 4) == BAD and DF(h, out.ctypes.data, 0, -1) == BAD
        assert (out == 9).all()
        assert FO(h, r, d, t, 0, None, rs, None) == 0 and FT(h, r, 0, n, t, 0, rs, None) == 0     # nothing to do
        sync()
        assert (host_of(res) == FILL).all()
        st.same("after the refusals")                                             # fenv, cutoff, pedal, bend and glide words, owners, every word of the bank
        assert st.fenv[8, FM.STAGE] == FM.ATTACK and not st.fenv[16].any()
        assert st.fenv_match(ANY, CONTOUR) == [1, 1, n - 2, 0]                       # ... and the bank still answers
        st.block()
    finally:
        st.close()


def test_more_fenv_calls_than_the_ring_has_slots():
    """3 x SKRED_FX_RING_SLOTS fenv_tags_each calls (two slots each) and as many fenv_owned_each calls back to back on one stream, no
    host wait in between: a slot that is still in flight is waited for through its own event, and every record arrives."""
    st = stage()
    try:
        v = np.arange(N, dtype=np.int32)
        tags = (0x03000001 + v).astype(np.uint32)
        st.tag(v, tags)
        assert st.cut_match(ANY, R(M.ABS | BOTH, 1 << 25, 1 << 16, 1))[0] == N
        calls, per = 3 * fxb.FX_RING_SLOTS, 12
        bufs, lists = [dev_i32(6) for _ in range(2 * calls)], []
        sync()
        want = []
        for c in range(calls):
            a = v[c * 2 * per:c * 2 * per + per][::-1].copy()                       # the tags in descending order
            b = v[c * 2 * per + per:(c + 1) * 2 * per]
            ra = [E(FM.ABS, (1 << 26) + 1000 * c + j, (1 << 24) + j, 1 << 22, 5 + j, 6, 7) for j in range(per)]
            rb = [E(FM.REL | FM.START, (2 << 16) + c, (1 << 16) + j, 1 << 15, 5, 6 + c, 7, start=(1 << 16) + 100 * c + j) for j in range(per)]
            lists.append(dev_list(b))
            st.db.fenv_tags_each(es(ra), 0, N, tags[a], bufs[2 * c].data_ptr())
            st.db.fenv_owned_each(es(rb), lists[-1].data_ptr(), tags[b], 0, bufs[2 * c + 1].data_ptr())
            want.append(FM.fenv_tags_each(st.owner, st.cut, st.fenv, st.filt, ra, 0, N, tags[a])[0])
            want.append(FM.fenv_owned_each(st.owner, st.cut, st.fenv, st.filt, rb, b, tags[b]))
        sync()
        for b, w in zip(bufs, want):
            assert w[:3] == [per, 0, 0] and host_of(b).tolist() == w + [FILL, FILL]
        st.same("the run of records")
        assert int((st.fenv[:, FM.STAGE] != 0).sum()) == 2 * per * calls
        st.cut_advance(64)
        st.block()
    finally:
        st.close()
