"""Patch notes without a GPU: every refusal of skred_slot_query_check and skred_slot_notes_check with the accepted edges beside it,
the model (tests/slot_model.py) against the per-voice listing it must reduce to, and the scenes of tests/test_slots.py -- each must
hold a listed slot, a slot kept off the list by one member alone, and a listed slot whose voices outside the mask all sound, so a
kernel that ignores the mask, or looks at one member only, cannot pass.
"""
import ctypes as C

import numpy as np
import pytest

import slot_model as M
import slot_scenes as S
from skred_amd import device
from skred_amd.bank import SlotQueryC, slot_query
from test_idle import expected

BAD, RANGE = -2, -4
NAN = float("nan")
N = 1024


def q_(first=0, count=N, K=8, mask=0xFF, which=M.FIN | M.ENV, settle=0.0, start=None, max_out=4):
    return slot_query(first, count, K, mask, which, settle, start, max_out)


def test_struct_matches_the_header():
    assert C.sizeof(SlotQueryC) == 40 and SlotQueryC.member_mask.offset == 16 and SlotQueryC.which.offset == 24
    assert SlotQueryC.start.offset == 32 and SlotQueryC.max_out.offset == 36


def test_query_check_accepts_the_edges():
    assert device.slot_query_check(q_(), N) == 0
    assert device.slot_query_check(q_(K=1, mask=1), N) == 0
    assert device.slot_query_check(q_(K=64, mask=(1 << 64) - 1), N) == 0
    assert device.slot_query_check(q_(K=64, mask=1 << 63), N) == 0                     # only bit K - 1
    assert device.slot_query_check(q_(K=8, mask=0x80), N) == 0
    assert device.slot_query_check(q_(K=1, mask=1, first=N - 1, count=1, start=N - 1), N) == 0
    assert device.slot_query_check(q_(start=N - 8), N) == 0                            # `from` on the last slot
    assert device.slot_query_check(q_(first=24, count=296, start=312), 320) == 0       # K-aligned, not 64-aligned
    assert device.slot_query_check(q_(max_out=0), N) == 0
    assert device.slot_query_check(q_(which=M.FIN | M.ENV | M.AMP, settle=1e-3), N) == 0
    assert device.slot_query_check(q_(K=64, mask=5, first=0, count=64), 64) == 0       # the whole bank is one slot


QUERY_REFUSALS = {
    "k_zero": (q_(K=0, mask=1), RANGE), "k_three": (q_(K=3, mask=1), RANGE), "k_128": (q_(K=128, mask=1), RANGE),
    "k_negative": (q_(K=-8, mask=1), RANGE),
    "mask_zero": (q_(mask=0), BAD), "mask_stray": (q_(mask=0x100), BAD), "mask_stray_k1": (q_(K=1, mask=3), BAD),
    "mask_top": (q_(K=32, mask=1 << 63), BAD),
    "which_none": (q_(which=0), BAD), "which_unknown": (q_(which=M.ENV | 8), BAD), "which_unnamed": (q_(which=M.ENV | M.UNNAMED), BAD),
    "settle_negative": (q_(settle=-1.0), BAD), "settle_nan": (q_(settle=NAN), BAD), "settle_inf": (q_(settle=float("inf")), BAD),
    "max_out_negative": (q_(max_out=-1), BAD),
    "count_zero": (q_(count=0), RANGE), "count_negative": (q_(count=-8), RANGE), "first_negative": (q_(first=-8, start=0), RANGE),
    "past_the_bank": (q_(first=N - 8, count=16, start=N - 8), RANGE), "first_past": (q_(first=N, count=8, start=N), RANGE),
    "first_misaligned": (q_(first=4, count=8, start=4), RANGE), "count_misaligned": (q_(count=12), RANGE),
    "from_misaligned": (q_(start=4), RANGE), "from_below": (q_(first=8, count=16, start=0), RANGE),
    "from_past": (q_(first=8, count=16, start=24), RANGE),
}


@pytest.mark.parametrize("case", list(QUERY_REFUSALS))
def test_query_check_refuses(case):
    q, rc = QUERY_REFUSALS[case]
    assert device.slot_query_check(q, N) == rc, case
    assert device.load().skred_amd_last_error()


def test_query_check_refuses_no_query_and_small_banks():
    assert device.load().skred_slot_query_check(None, N) == BAD
    assert device.slot_query_check(q_(K=64, mask=1, count=64), 32) == RANGE            # a bank smaller than a slot


def rec(flags=M.SET_PHASE, inc=0.5, vel=1.0, phase=0.0, pl=0.5, pr=0.5, reserved=(0, 0)):
    return device.NoteC(inc, vel, phase, pl, pr, flags, (C.c_uint32 * 2)(*reserved))


BAD_RECORDS = {
    "unknown_flag": rec(flags=4), "reserved": rec(reserved=(0, 3)), "inc_nan": rec(inc=NAN), "velocity_inf": rec(vel=float("inf")),
    "phase_nan": rec(phase=NAN), "pan_nan": rec(flags=M.SET_PAN, pl=NAN),
}


def test_notes_check_accepts_the_edges():
    L = device.load()
    good = [rec() for _ in range(16)]
    assert device.slot_notes_check(good, 8, 0xFF) == 0 and device.slot_notes_check(good, 1, 1) == 0
    assert device.slot_notes_check(good, 8, 0x80) == 0 and device.slot_notes_check(good, 16, 0xA5A5) == 0
    assert device.slot_notes_check([rec() for _ in range(64)], 64, 1 << 63) == 0
    arr = device.note_array(good)
    assert L.skred_slot_notes_check(C.cast(arr, C.c_void_p), 0, 8, 0xFF) == 0          # no notes


@pytest.mark.parametrize("case", list(BAD_RECORDS))
def test_notes_check_looks_at_masked_records_only(case):
    """A record skred_notes_check refuses is refused at a masked position and not looked at elsewhere; with K = 1, mask 1 the
    verdict is skred_notes_check's."""
    K, mask = 8, 0b10010010
    for k in (0, 2):
        for l in range(K):
            batch = [rec() for _ in range(3 * K)]
            batch[k * K + l] = BAD_RECORDS[case]
            want = BAD if (mask >> l) & 1 else 0
            assert device.slot_notes_check(batch, K, mask) == want, (case, k, l)
    batch = [rec() for _ in range(5)]
    batch[3] = BAD_RECORDS[case]
    assert device.slot_notes_check(batch, 1, 1) == device.notes_check(batch) == BAD


def test_notes_check_refuses_shapes():
    L = device.load()
    good = device.note_array([rec() for _ in range(16)])
    p = C.cast(good, C.c_void_p)
    assert L.skred_slot_notes_check(None, 2, 8, 0xFF) == BAD and L.skred_slot_notes_check(p, -1, 8, 0xFF) == BAD
    assert L.skred_slot_notes_check(p, 2, 0, 1) == RANGE and L.skred_slot_notes_check(p, 2, 6, 1) == RANGE
    assert L.skred_slot_notes_check(p, 2, 128, 1) == RANGE
    assert L.skred_slot_notes_check(p, 2, 8, 0) == BAD and L.skred_slot_notes_check(p, 2, 8, 0x100) == BAD
    assert L.skred_slot_notes_check(p, 16, 1, 2) == BAD


def test_entry_points_refuse_without_a_device():
    L = device.load()
    notes = device.note_array([rec() for _ in range(16)])
    p = C.cast(notes, C.c_void_p)
    word = (C.c_uint32 * 8)()                              # stands in for device memory: a refusal never reads it
    q = q_()
    assert L.skred_bank_find_idle_slots(None, C.byref(q), word, word, None) == BAD
    assert L.skred_bank_find_idle_slots_host(None, C.byref(q), word, None, None) == BAD
    assert L.skred_bank_notes_on_slots(None, p, 2, 8, 0xFF, word, word, 0, word, word, None) == BAD
    assert L.skred_bank_note_on_idle_slots(None, C.byref(q), p, 2, 0xFF, word, word, None) == BAD
    assert L.skred_bank_stamp_slots(None, word, 2, None, 8, 0xFF, M.STAMP_RELEASE, None) == BAD
    assert b"stamp_slots" in L.skred_amd_last_error()


# ---------------------------------------------------------------------------------------------- the model and the scenes

@pytest.mark.parametrize("n", [64, 320, 1088])
def test_model_with_one_voice_slots_is_the_voice_listing(n):
    _, _, _, truth, _ = S.scene(n, 1, 1)
    for which, settle in ((S.WHICH_ALL, S.SETTLE), (S.WHICH_NOTES, S.SETTLE), (M.ENV, 0.0), (M.FIN, 0.0), (M.AMP, 0.0)):
        for first, count, start in ((0, n, None), (0, n, n // 2), (0, n, n - 1), (5, n - 9, 17)):
            want = expected(truth, first, count, which, settle, start)
            got = M.idle_slots(truth, first, count, 1, 1, which, settle, start)
            assert np.array_equal(got, want), (n, which, first, count, start)
    assert len(M.idle_slots(truth, 0, n, 1, 1, S.WHICH_ALL, S.SETTLE)) not in (0, n)


def test_model_listing_order_and_wrap():
    _, _, _, truth, _ = S.scene(320, 8, 0xFF)
    lst = M.idle_slots(truth, 0, 320, 8, 0xFF, S.WHICH_ALL, S.SETTLE)
    assert len(lst) >= 3 and (np.diff(lst) > 0).all() and (lst % 8 == 0).all()
    mid = int(lst[len(lst) // 2])
    rot = M.idle_slots(truth, 0, 320, 8, 0xFF, S.WHICH_ALL, S.SETTLE, mid)
    assert rot[0] == mid and sorted(rot.tolist()) == lst.tolist()
    rot = M.idle_slots(truth, 0, 320, 8, 0xFF, S.WHICH_ALL, S.SETTLE, mid + 8)           # from a slot that may be busy: the next idle one
    assert rot[-1] == mid
    assert np.array_equal(M.place(4, 8, np.array([8, -1, 12, 320, 16]), 3, 1, 320), [-1, -1, -1, -1])
    assert np.array_equal(M.place(3, 8, np.array([8, 312, 16]), 3, 0, 320), [8, 312, 16])


def scene_cases():
    out = [(n, K, name, True) for n, K, name in S.QUERY_CASES + [S.BIG_CASE]]
    out += [(n, K, name, False) for n, K, name in NOTE_SCENES]
    return out


# the scenes of the note, stamp and K = 1 tests of tests/test_slots.py (queried with FINISHED | ENV_DONE)
NOTE_SCENES = [(1088, 2, "low"), (1088, 2, "all"), (4160, 64, "alt"), (320, 8, "alt"), (320, 8, "high"), (1088, 1, "all")]


@pytest.mark.parametrize("n,K,name,with_amp", scene_cases())
def test_scenes_are_not_vacuous(n, K, name, with_amp):
    mask = S.masks(K)[name]
    which = S.WHICH_ALL if with_amp else S.WHICH_NOTES
    _, _, _, truth, _ = S.scene(n, K, mask, with_amp)
    listed, one_short, shadowed = S.conditions(truth, 0, n, K, mask, which)
    assert listed, "no slot is listed"
    assert one_short, "no slot is kept off the list by a single member"
    assert shadowed, "no listed slot has every voice outside the mask sounding"
    heads, ok = M.slot_idle(truth, 0, n, K, mask, which, S.SETTLE)
    assert 0 < int(ok.sum()) < len(heads)
    if K > 1 and mask != (1 << K) - 1:
        # ... and the mask matters: the listing differs from the one every voice would vote in
        assert not np.array_equal(M.idle_slots(truth, 0, n, K, mask, which, S.SETTLE),
                                  M.idle_slots(truth, 0, n, K, (1 << K) - 1, which, S.SETTLE))


def test_the_sub_range_scene():
    """first = 24, count = 296 on 320 voices with K = 8: the same three conditions inside the range."""
    _, _, _, truth, _ = S.scene(320, 8, 0x55)
    assert all(S.conditions(truth, 24, 296, 8, 0x55, S.WHICH_ALL))
