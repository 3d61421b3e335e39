"""Slot stealing without a GPU: the struct against the header, every refusal of skred_slot_steal_check beside the accepted edge, the
model (tests/slot_steal_model.py) against a brute-force restatement and -- with K = 1, mask 1 -- against the per-voice model on the
scenes of tests/test_steal.py, and the scenes of tests/test_slot_steal.py on the oracle's state: none of them is vacuous.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import slot_steal_model as M
import slot_steal_scenes as S
import steal_model as sm
import test_steal as TS
from skred_amd import banks, device
from skred_amd.bank import SlotStealQueryC, slot_steal_query
from slot_scenes import masks
from steal_model import OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, STEAL_UNNAMED, STEAL_MAX, FIN, ENV, AMP, UNNAMED

BAD, RANGE = -2, -4
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "skred_amd.h")


# ---------------------------------------------------------------------------------------------- the struct

def test_struct_matches_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct skred_slot_steal_query \{[^\n]*\n(.*?)\} skred_slot_steal_query_t;", text, re.S).group(1)
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    declared = []
    for line in body.splitlines():
        m = re.match(r"\s*(int32_t|uint32_t|uint64_t|float)\s+([^;]+);", line)
        assert m, line
        for name in m.group(2).split(","):
            name = name.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", name)
            declared.append((arr.group(1), ctype[m.group(1)] * int(arr.group(2))) if arr else (name, ctype[m.group(1)]))
    assert [(n, t) for n, t in SlotStealQueryC._fields_] == declared
    offs = {n: getattr(SlotStealQueryC, n).offset for n, _ in SlotStealQueryC._fields_}
    assert offs == dict(first=0, count=4, slot_voices=8, policy=12, member_mask=16, min_age=24, flags=32, exclude_idle=36,
                        settle_level=40, max_out=44, reserved=48)
    assert C.sizeof(SlotStealQueryC) == 56
    for s in ("skred_slot_steal_check", "skred_bank_find_steal_slots", "skred_bank_find_steal_slots_host", "skred_bank_note_on_steal_slots"):
        assert re.search(r"\b%s\(" % s, text) and hasattr(device.load(), s), s


# ---------------------------------------------------------------------------------------------- the check function

def good(**kw):
    args = dict(first=0, count=1024, slot_voices=8, member_mask=0x55, policy=OLDEST, flags=0, min_age=0, exclude_idle=0,
                settle_level=0.0, max_out=16)
    args.update(kw)
    return slot_steal_query(**args)


ACCEPTED = {
    "plain": dict(),
    "K1": dict(slot_voices=1, member_mask=1, first=999, count=1),
    "K64": dict(slot_voices=64, member_mask=(1 << 64) - 1, first=64, count=960),
    "K64_top_bit_only": dict(slot_voices=64, member_mask=1 << 63),
    "mask_top_bit_only": dict(member_mask=0x80),
    "not_64_aligned": dict(first=24, count=296),
    "max_out_0": dict(max_out=0), "max_out_1024": dict(max_out=STEAL_MAX),
    "everything": dict(policy=QUIETEST, flags=RELEASED_FIRST | RELEASED_ONLY, min_age=2**63, exclude_idle=FIN | ENV | AMP, settle_level=1e-3),
    "settle_minus_zero": dict(settle_level=-0.0),
    "whole_bank": dict(count=1024), "last_slot": dict(first=1016, count=8),
}
REFUSED = {
    "policy": (dict(policy=2), BAD), "policy_high": (dict(policy=1 << 31), BAD),
    "flags": (dict(flags=4), BAD), "flags_high": (dict(flags=RELEASED_FIRST | (1 << 31)), BAD),
    "flags_unnamed": (dict(flags=STEAL_UNNAMED), BAD), "flags_unnamed_and_more": (dict(flags=STEAL_UNNAMED | RELEASED_FIRST), BAD),
    "exclude_unknown": (dict(exclude_idle=8), BAD), "exclude_unnamed": (dict(exclude_idle=FIN | UNNAMED), BAD),
    "reserved0": (dict(), BAD), "reserved1": (dict(), BAD),
    "max_out_negative": (dict(max_out=-1), BAD), "max_out_large": (dict(max_out=STEAL_MAX + 1), BAD),
    "settle_negative": (dict(settle_level=-1.0), BAD), "settle_nan": (dict(settle_level=float("nan")), BAD),
    "settle_inf": (dict(settle_level=float("inf")), BAD),
    "mask_zero": (dict(member_mask=0), BAD), "mask_above_K": (dict(member_mask=0x100), BAD), "mask_K1_above": (dict(slot_voices=1, member_mask=2), BAD),
    "K_zero": (dict(slot_voices=0), RANGE), "K_three": (dict(slot_voices=3, member_mask=1), RANGE), "K_128": (dict(slot_voices=128), RANGE),
    "K_negative": (dict(slot_voices=-8), RANGE),
    "count_zero": (dict(count=0), RANGE), "count_negative": (dict(count=-8), RANGE), "first_negative": (dict(first=-8), RANGE),
    "first_behind": (dict(first=1024), RANGE), "range_behind": (dict(first=8, count=1024), RANGE),
    "range_overflow": (dict(first=2**31 - 8, count=2**31 - 8), RANGE),
    "first_misaligned": (dict(first=4, count=8), RANGE), "count_misaligned": (dict(count=1020), RANGE),
    "K64_misaligned": (dict(slot_voices=64, member_mask=1, first=32, count=64), RANGE),
}


def refused_query(case):
    q = good(**REFUSED[case][0])
    if case.startswith("reserved"):
        q.reserved[int(case[-1])] = 1
    return q


@pytest.mark.parametrize("case", list(ACCEPTED))
def test_check_accepts(case):
    assert device.slot_steal_check(good(**ACCEPTED[case]), 1024) == 0, case


@pytest.mark.parametrize("case", list(REFUSED))
def test_check_refuses(case):
    assert device.slot_steal_check(refused_query(case), 1024) == REFUSED[case][1], case
    assert device.load().skred_amd_last_error()


def test_refusals_without_a_device():
    L = device.load()
    assert L.skred_slot_steal_check(None, 1024) == BAD
    q, iq = good(max_out=0), device.slot_query(0, 1024, 8, 0x55, ENV)
    word = (C.c_uint32 * 8)()
    fake = C.c_void_p(C.addressof(word))                  # stands in for a bank: a NULL query is refused before the bank is followed
    total = C.c_int(0)
    assert L.skred_bank_find_steal_slots(None, C.byref(q), None, word, None) == BAD
    assert L.skred_bank_find_steal_slots(fake, None, None, word, None) == BAD
    assert L.skred_bank_find_steal_slots_host(None, C.byref(q), None, C.byref(total), None) == BAD
    assert L.skred_bank_find_steal_slots_host(fake, None, None, C.byref(total), None) == BAD
    notes = device.note_array([device.NoteC(0.3, 0.5, 0.0, 0.5, 0.5, 0) for _ in range(16)])
    p = C.cast(notes, C.c_void_p)
    on = L.skred_bank_note_on_steal_slots
    assert on(None, C.byref(iq), C.byref(q), p, 2, 0x55, word, word, None) == BAD
    assert on(fake, None, C.byref(q), p, 2, 0x55, word, word, None) == BAD
    assert on(fake, C.byref(iq), None, p, 2, 0x55, word, word, None) == BAD
    assert on(fake, C.byref(iq), C.byref(q), None, 2, 0x55, word, word, None) == BAD
    assert on(fake, C.byref(iq), C.byref(q), p, 2, 0x55, word, None, None) == BAD
    assert on(fake, C.byref(iq), C.byref(q), p, -1, 0x55, word, word, None) == BAD
    assert b"note_on_steal_slots" in L.skred_amd_last_error()


# ---------------------------------------------------------------------------------------------- the model

def test_model_against_brute_force():
    rng = np.random.default_rng(78)
    seen = 0
    for _ in range(300):
        bank, now = TS.random_small_bank(rng)
        K = int(rng.choice([1, 2, 4, 8, 16, 32, 64]))
        slots = bank.n // K
        if slots == 0:
            continue
        first = int(rng.integers(0, slots)) * K
        count = int(rng.integers(1, slots - first // K + 1)) * K
        mask = int(rng.integers(1, 1 << min(K, 62))) if K > 1 else 1
        mask = int(rng.choice([mask, (1 << K) - 1, 1, 1 << (K - 1)]))
        q = M.SlotQuery(first, count, K, mask, int(rng.integers(0, 2)),
                        int(rng.choice([0, RELEASED_FIRST, RELEASED_ONLY, RELEASED_FIRST | RELEASED_ONLY])),
                        int(rng.choice([0, 0, 7, 8, 500])), int(rng.choice([0, FIN, ENV, FIN | ENV | AMP])), float(rng.choice([0.0, 1e-3])))
        want, got = M.brute_force(bank, now, q), M.victim_slots(bank, now, q)
        assert np.array_equal(want, got), (q, want, got)
        seen += len(want) > 1
    assert seen > 40, seen


@pytest.mark.parametrize("name", [s for s in TS.SCENES if TS.SCENES[s][0] <= 5000 and s != "unnamed_mod"])
def test_one_voice_slots_are_the_voice_model(name):
    n, flavour, variant, make, kernel, setup = TS.SCENES[name]
    bank, tables, g, truth, now, role, special = TS.scene(n, flavour, variant)
    ran = 0
    for q, _ in TS.scene_queries(name):
        if (q.flags & STEAL_UNNAMED) or (q.exclude_idle & UNNAMED):
            continue
        sq = M.SlotQuery(q.first, q.count, 1, 1, q.policy, q.flags, q.min_age, q.exclude_idle, q.settle_level, q.max_out)
        assert np.array_equal(M.victim_slots(truth, now, sq), sm.victim_order(truth, now, q)), q
        v, cand, key = sm.keys(truth, now, q)
        h, scand, skey = M.keys(truth, now, sq)
        assert np.array_equal(cand, scand) and np.array_equal(key[cand], skey[scand])
        ran += 1
    assert ran > 0


# ---------------------------------------------------------------------------------------------- the scenes of the GPU tests

def order(host, now, q):
    return M.victim_slots(host, now, q).tolist()


def check_not_vacuous(n, K, mask, first=0, count=None, seed=0):
    bank, tables, g, truth, now, kind = S.scene(n, K, mask, seed)
    count = n - first if count is None else count
    slots = count // K
    mem = M.lanes(mask, K)
    full = (1 << K) - 1
    base = M.SlotQuery(first, count, K, mask)
    heads, cand, cls, primary, t = M.terms(truth, now, base)
    live, released, age = t["live"], t["released"], t["age"]
    # caps: at least a quarter of the slots are candidates of the plain query, and not all of them
    assert slots / 4 <= cand.sum() < slots, (int(cand.sum()), slots)
    # a slot with no live member, which is no candidate
    assert (~live.any(1)).any() and not cand[~live.any(1)].any()
    # kept out by one member alone that is too young
    young = live & (age < S.MIN_AGE)
    _, cand_age, _, _, _ = M.terms(truth, now, base.but(min_age=S.MIN_AGE))
    assert (cand & ~cand_age & (young.sum(1) == 1)).any(), "no slot is kept off a min_age query by one member alone"
    assert (cand & cand_age).any()
    # kept out of RELEASED_ONLY, and moved from class 0 to class 1, by one held member
    heldm = live & ~released
    _, cand_ro, _, _, _ = M.terms(truth, now, base.but(flags=RELEASED_ONLY))
    one_held = cand & (heldm.sum(1) == 1) & ((live.sum(1) > 1) | (len(mem) == 1))
    assert (one_held & ~cand_ro).any(), "no slot is kept out of RELEASED_ONLY by one held member"
    _, _, cls_rf, _, _ = M.terms(truth, now, base.but(flags=RELEASED_FIRST))
    assert (one_held & (cls_rf == 1)).any() and (cand & (cls_rf == 0)).any() and (cand_ro & (cls_rf == 0)).any()
    # a candidate although some members are idle; every member idle and live: the exclusion's own case
    if len(mem) > 1:
        _, cand_ex, _, _, tex = M.terms(truth, now, base.but(exclude_idle=S.EXCLUDE, settle_level=float(S.SETTLE)))
        idle = tex["idle"]
        assert (cand_ex & idle.any(1) & ~idle.all(1)).any(), "no candidate has idle members"
    _, cand_ex, _, _, tex = M.terms(truth, now, base.but(exclude_idle=S.EXCLUDE, settle_level=float(S.SETTLE)))
    assert (cand & ~cand_ex).any(), "the exclusion excludes nobody"
    # the deciding member at the lowest member lane, at the highest, and for K = 64 at a lane >= 32 (where the mask has one)
    for q in (base, base.but(flags=RELEASED_FIRST), base.but(policy=QUIETEST)):
        heads, c, _, primary, t = M.terms(truth, now, q)
        offer = np.where(t["live"], t["offer"], np.uint64(0))
        arg = np.array(mem)[offer.argmax(1)]                                 # (the first member lane that holds the maximum)
        unique = (offer == offer.max(1)[:, None]).sum(1) == 1
        lanes_seen = set(arg[c & unique].tolist())
        if q.policy == OLDEST:
            assert mem[0] in lanes_seen and mem[-1] in lanes_seen, (q, sorted(lanes_seen))
            if K == 64 and mem[-1] >= 32:
                assert any(l >= 32 for l in lanes_seen)
        if len(mem) > 1:
            assert len(lanes_seen) > 1, (q, lanes_seen)
    # every query: the flag bits exclude somebody, both classes occur, and the lists a wrong key pass would write differ
    for q in S.queries(n, K, mask, first, count):
        got = order(truth, now, q)
        if q.max_out == 0:
            continue
        assert got, q
        if q.flags & RELEASED_ONLY:
            assert len(order(truth, now, q.but(flags=q.flags & ~RELEASED_ONLY))) > len(got), q
        if q.min_age:
            assert len(order(truth, now, q.but(min_age=0))) > len(got), q
        if q.exclude_idle:
            assert len(order(truth, now, q.but(exclude_idle=0))) > len(got), q
        if (q.flags & RELEASED_FIRST) and not (q.flags & RELEASED_ONLY):
            _, c, cl, _, _ = M.terms(truth, now, q)
            assert (cl[c] == 0).any() and (cl[c] == 1).any(), q
        if mask != full:
            assert order(truth, now, q.but(mask=full)) != got, f"{q}: a key pass that ignored the mask would pass"
        if len(mem) > 1:
            assert order(truth, now, q.but(mask=1 << mem[0])) != got, f"{q}: a key pass that read one member would pass"
    assert np.array_equal(M.victim_slots(truth, now, base), M.brute_force(truth, now, base))
    return truth, now


@pytest.mark.parametrize("n,K,name", S.FULL_CASES)
def test_scenes_are_not_vacuous(n, K, name):
    mask = masks(K)[name]
    truth, now = check_not_vacuous(n, K, mask)
    th = S.threshold_queries(truth, now, n, K, mask)
    if n // K >= 32:
        assert len(th) >= 2, "no short list cuts a run of equal keys"
    for q in th:
        lst = order(truth, now, q)
        assert len(lst) > q.max_out
        _, cand, key = M.keys(truth, now, q)
        ks = np.sort(key[cand])
        assert ks[q.max_out - 1] == ks[q.max_out], q                             # more candidates than max_out, a tie at the threshold


def test_unaligned_scene_is_not_vacuous():
    n, K, mask, first, count = S.UNALIGNED
    check_not_vacuous(n, K, mask, first, count)
    bank, tables, g, truth, now, kind = S.scene(n, K, mask)
    inside = M.victim_slots(truth, now, M.SlotQuery(first, count, K, mask))
    whole = M.victim_slots(truth, now, M.SlotQuery(0, n, K, mask))
    assert set(whole) - set(inside), "no candidate lies outside the range"       # slots below 24 and from 320 - ... are cut off
    assert set(inside) == {h for h in whole if first <= h < first + count}


@pytest.mark.parametrize("n,K,name", S.SMALL_CASES)
def test_small_scenes_have_candidates_and_others(n, K, name):
    """Banks of one to eight slots cannot hold every kind; what they must hold is a candidate, and -- from two slots on -- a slot
    that is none (from eight slots on: the first eight hold every kind)."""
    mask = masks(K)[name]
    bank, tables, g, truth, now, kind = S.scene(n, K, mask)
    got = M.victim_slots(truth, now, M.SlotQuery(0, n, K, mask))
    assert len(got) >= 1
    if n // K >= 8:
        assert len(got) < n // K
    assert np.array_equal(got, M.brute_force(truth, now, M.SlotQuery(0, n, K, mask)))


def test_special_scenes_on_the_model():
    """The hand-made scenes of tests/test_slot_steal.py do what they are for (stated on the model, before any device is asked)."""
    import test_slot_steal as G
    # 64-bit keys: the deciding member is never the slot's first voice; a reduction of the low word alone orders differently
    bank, now, q, facts = G.wide_scene()
    lst = order(bank, now, q)
    e = bank["voice_amp_envelope"]
    assert lst[:len(facts["expect_head"])] == facts["expect_head"] and lst[-2:] == facts["saturated"]
    low = bank.copy()
    low["voice_amp_envelope"]["sample_start"][:] = e["sample_start"] & np.uint64(0xFFFFFFFF)
    assert order(low, now, q) != lst, "the low words alone give the same order"
    halves = bank.copy()                                                         # slot 10 as a word-by-word maximum would make it
    halves["voice_amp_envelope"]["sample_start"][10 * q.K + 3] = np.uint64((1 << 32) + 777)
    assert order(halves, now, q) != lst, "a maximum taken on the two words independently gives the same order"
    first_only = order(bank, now, q.but(mask=1))
    assert first_only != lst
    # ties across workgroups
    bank, now, q = G.ties_scene()
    lst = order(bank, now, q)
    assert len(lst) == 4160 // 2 and lst == sorted(lst)
    # age: a member ahead of the clock; min_age at, one below, one above the youngest live member of a slot
    bank, now, q, facts = G.age_scene()
    assert order(bank, now, q)[-1] == facts["ahead_slot"] and facts["ahead_slot"] not in order(bank, now, q.but(min_age=1))
    a = facts["age"]
    assert facts["slot"] in order(bank, now, q.but(min_age=a)) and facts["slot"] in order(bank, now, q.but(min_age=a - 1))
    assert facts["slot"] not in order(bank, now, q.but(min_age=a + 1))
