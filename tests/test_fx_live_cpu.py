"""Live control of the fixed-point bank, the part that needs no device: the exported symbols, the pure-host check functions, the
claim that the integer smoother reaches exactly 0 (so settle_q15 = 0 is a usable level), and the listing rule of the model the
GPU tests compare against (tests/fx_live_model.py)."""
import ctypes as C

import numpy as np
import pytest

import fx_live_model as model
from oracle import cpuref
from skred_amd import device, fxbank as fxb

BAD, RANGE = -2, -4
FIN, ENV, AMP = fxb.IDLE_FINISHED, fxb.IDLE_ENV_DONE, fxb.IDLE_AMP_ZERO
NEW_SYMBOLS = ["skred_fxbank_update", "skred_fx_idle_check", "skred_fxbank_find_idle", "skred_fxbank_find_idle_host",
               "skred_fx_notes_check", "skred_fxbank_notes_on_list", "skred_fxbank_note_on_idle", "skred_fxbank_stamp_list"]


def test_fx_live_symbols_exported():
    L = device.load()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
        assert s in fxb.FX_ABI_SYMBOLS + fxb.FX_HOST_ABI_SYMBOLS, s


def note(inc=1 << 20, vel=32768, phase=0, pl=16384, pr=16384, flags=0, reserved=(0, 0)):
    return fxb.FxNoteC(inc, vel, phase, pl, pr, flags, (C.c_uint32 * 2)(*reserved))


def test_fx_notes_check_accepts_the_boundaries():
    both = fxb.NOTE_SET_PHASE | fxb.NOTE_SET_PAN
    good = [note(vel=0), note(vel=65535), note(inc=0xFFFFFFFF, phase=0xFFFFFFFF, flags=fxb.NOTE_SET_PHASE),
            note(pl=0, pr=65535, flags=both), note(pl=65535, pr=0, flags=fxb.NOTE_SET_PAN),
            note(pl=-1, pr=1 << 20, flags=fxb.NOTE_SET_PHASE)]            # pans a note does not set are not looked at
    assert fxb.fx_notes_check(good) == 0
    L = fxb._bind(device.load())
    arr = fxb.fx_note_array(good)
    assert L.skred_fx_notes_check(C.cast(arr, C.c_void_p), 0) == 0
    assert L.skred_fx_notes_check(None, 1) == BAD and L.skred_fx_notes_check(C.cast(arr, C.c_void_p), -1) == BAD


BAD_NOTES = {
    "unknown_flag": note(flags=4),
    "high_flag": note(flags=fxb.NOTE_SET_PHASE | (1 << 31)),
    "reserved0": note(reserved=(1, 0)),
    "reserved1": note(reserved=(0, 9)),
    "velocity_negative": note(vel=-1),
    "velocity_high": note(vel=65536),
    "pan_left_negative": note(pl=-1, flags=fxb.NOTE_SET_PAN),
    "pan_left_high": note(pl=65536, flags=fxb.NOTE_SET_PAN),
    "pan_right_negative": note(pr=-1, flags=fxb.NOTE_SET_PAN | fxb.NOTE_SET_PHASE),
    "pan_right_high": note(pr=65536, flags=fxb.NOTE_SET_PAN),
}


@pytest.mark.parametrize("case", list(BAD_NOTES))
def test_fx_notes_check_refuses(case):
    good = [note(inc=1000 + k, vel=100 * k) for k in range(5)]
    assert fxb.fx_notes_check(good) == 0
    for at in (0, 2, 4):                                   # the bad note anywhere in the batch
        batch = list(good)
        batch[at] = BAD_NOTES[case]
        assert fxb.fx_notes_check(batch) == BAD, (case, at)


def query(first=0, count=100, which=ENV, settle=0, start=None, max_out=0):
    return fxb.FxIdleQueryC(first, count, which, settle, first if start is None else start, max_out)


def test_fx_idle_check_accepts_the_boundaries():
    n = 100
    for q in (query(), query(which=FIN | ENV | AMP), query(settle=0x7FFFFFFF), query(first=99, count=1, start=99),
              query(first=0, count=100, start=99), query(max_out=0x7FFFFFFF), query(first=37, count=63, start=37)):
        assert fxb.fx_idle_check(q, n) == 0


BAD_QUERIES = {
    "max_out_negative": (query(max_out=-1), BAD),
    "no_criterion": (query(which=0), BAD),
    "unknown_bit": (query(which=ENV | 8), BAD),
    "unnamed": (query(which=ENV | fxb.IDLE_UNNAMED), BAD),
    "settle_negative": (query(settle=-1), BAD),
    "count_zero": (query(count=0), RANGE),
    "first_negative": (query(first=-1, count=10, start=0), RANGE),
    "first_outside": (query(first=100, count=1, start=100), RANGE),
    "range_outside": (query(first=50, count=51, start=50), RANGE),
    "from_below": (query(first=10, count=10, start=9), RANGE),
    "from_above": (query(first=10, count=10, start=20), RANGE),
}


@pytest.mark.parametrize("case", list(BAD_QUERIES))
def test_fx_idle_check_refuses(case):
    q, rc = BAD_QUERIES[case]
    assert fxb.fx_idle_check(q, 100) == rc
    assert fxb.fx_idle_check(None, 100) == BAD


def test_fx_refusals_without_a_device():
    L = fxb._bind(device.load())
    word = (C.c_uint32 * 8)()                              # stands in for device memory: a refusal never reads it
    notes = fxb.fx_note_array([note()])
    p, q = C.cast(notes, C.c_void_p), query()
    assert L.skred_fxbank_update(None, None, word, 1, fxb.DIRTY_PAN, None) == BAD
    assert L.skred_fxbank_find_idle(None, C.byref(q), word, word, None) == BAD
    assert L.skred_fxbank_find_idle_host(None, C.byref(q), word, None, None) == BAD
    assert L.skred_fxbank_notes_on_list(None, p, 1, word, word, 0, word, word, None) == BAD
    assert L.skred_fxbank_note_on_idle(None, C.byref(q), p, 1, word, word, None) == BAD
    assert L.skred_fxbank_stamp_list(None, word, 4, None, fxb.STAMP_RELEASE, None) == BAD
    assert b"stamp_list" in L.skred_amd_last_error()


@pytest.mark.parametrize("k_q15", [1, 655, 32768])
def test_fx_smoother_reaches_exactly_zero(k_q15):
    """With k_q15 > 0 the integer smoother g += ((0 - g) * k) >> 15 moves a positive g down by at least 1 per frame: a released,
    smoothed voice is listed with settle_q15 = 0 after finitely many blocks, its gain exactly 0 -- on the definition itself."""
    b, pool, c0 = fxb.bank_fx(8, with_filter=False)
    b["smoother_k_q15"] = k_q15
    b["release_frames"] = 16
    b["attack_frames"] = 4
    b["decay_frames"] = 4
    b["sample_start"] = c0 - 1000                          # in sustain
    b["smoother_gain_q15"] = 20000                         # has sounded (k = 1 would never leave 0 upwards: the shift floors)
    cnt = c0
    _, _, cnt = cpuref.fx_render(b, pool, cnt, 256, 1)
    g0 = b["smoother_gain_q15"].copy()
    assert (g0 > 0).all() and (b["is_active"] == 1).all()
    assert model.idle_list(b, 0, 8, ENV, 0)[1] == 0
    model.stamp(b, np.arange(8), fxb.STAMP_RELEASE, cnt)
    bound = 16 + int(g0.max()) + 1                         # the release, then at most one frame per unit of gain
    blocks = 0
    while model.idle_list(b, 0, 8, ENV, 0)[1] < 8:
        _, _, cnt = cpuref.fx_render(b, pool, cnt, 512, 1)
        blocks += 1
        assert blocks * 512 <= bound + 512, "the smoother did not reach 0 within its bound"
    assert (b["smoother_gain_q15"] == 0).all() and (b["is_active"] == 0).all()
    voices, total = model.idle_list(b, 0, 8, ENV, 0)
    assert total == 8 and (voices == np.arange(8)).all()


def test_fx_listing_is_ascending_from_start_and_wraps():
    b = fxb.FxVoiceBank(600)
    rng = np.random.default_rng(5)
    b["use_envelope"] = 1
    b["is_active"] = rng.integers(0, 2, 600)
    b["finished"] = rng.integers(0, 8, 600) == 0
    b["amp_q15"] = rng.integers(0, 3, 600) * 1000
    b["smoother_enable"] = rng.integers(0, 2, 600)
    b["smoother_gain_q15"] = rng.integers(-3, 4, 600)
    for which in (FIN, ENV, AMP, FIN | ENV | AMP):
        for settle in (0, 2):
            m = model.idle_mask(b, which, settle)
            first, count = 37, 500
            inside = np.flatnonzero(m[first:first + count]) + first
            for start in (37, 300, 536):
                for max_out in (0, 5, 10000):
                    got, total = model.idle_list(b, first, count, which, settle, start, max_out)
                    assert total == inside.size and got.size == min(total, max_out)
                    want = np.concatenate([inside[inside >= start], inside[inside < start]])[:max_out]
                    assert (got == want).all()
                    k = int((got >= start).sum())          # ascending from start, then ascending from first
                    assert (np.diff(got[:k]) > 0).all() and (np.diff(got[k:]) > 0).all() and (got[k:] < start).all()
    # settle: the absolute value, exactly
    b["smoother_enable"], b["is_active"], b["finished"] = 1, 0, 0
    b["smoother_gain_q15"][:4] = [-(1 << 31), -3, 3, 2]
    m = model.idle_mask(b, ENV, 2)
    assert list(m[:4]) == [False, False, False, True]
