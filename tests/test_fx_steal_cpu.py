"""Voice stealing on the fixed-point bank, the part that needs no device: the exported symbols, skred_fx_steal_check, the refusals
that come before the bank is followed, the model (tests/fx_steal_model.py) against a brute-force statement of the definition in
Python integers, and the claim that no scene of tests/test_fx_steal.py is vacuous."""
import ctypes as C

import numpy as np
import pytest

import fx_steal_model as sm
import fx_steal_scenes as sc
from fx_steal_model import AMP, ENV, FIN, OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, STEAL_MAX, Query
from skred_amd import device, fxbank as fxb

BAD, RANGE = -2, -4
NEW_SYMBOLS = ["skred_fx_steal_check", "skred_fxbank_find_steal", "skred_fxbank_find_steal_host", "skred_fxbank_note_on_steal"]


def test_fx_steal_symbols_exported():
    L = device.load()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), f"libskred_amd.so does not export {s}"
        assert s in fxb.FX_ABI_SYMBOLS + fxb.FX_HOST_ABI_SYMBOLS, s
    assert C.sizeof(fxb.FxStealQueryC) == 40
    assert (fxb.STEAL_OLDEST, fxb.STEAL_QUIETEST, fxb.STEAL_RELEASED_FIRST, fxb.STEAL_RELEASED_ONLY, fxb.STEAL_UNNAMED, fxb.STEAL_MAX) == \
        (device.STEAL_OLDEST, device.STEAL_QUIETEST, device.STEAL_RELEASED_FIRST, device.STEAL_RELEASED_ONLY, device.STEAL_UNNAMED,
         device.STEAL_MAX) == (0, 1, 1, 2, 256, 1024)


VALID = [
    dict(max_out=16),
    dict(first=37, count=300, policy=QUIETEST, flags=RELEASED_FIRST | RELEASED_ONLY, min_age=2**63, exclude_idle=FIN | ENV | AMP,
         settle_q15=0x7FFFFFFF, max_out=STEAL_MAX),
    dict(first=999, count=1, max_out=0),
    dict(first=0, count=1000, exclude_idle=AMP, settle_q15=3, max_out=1),
    dict(first=1, count=999, flags=RELEASED_ONLY, min_age=1, max_out=STEAL_MAX),
]


@pytest.mark.parametrize("k", range(len(VALID)))
def test_fx_steal_check_accepts(k):
    kw = dict(first=0, count=1000)
    kw.update(VALID[k])
    assert fxb.fx_steal_check(fxb.fx_steal_query(**kw), 1000) == 0


BAD_QUERIES = {
    "policy": (dict(policy=2), BAD), "policy_high": (dict(policy=1 << 31), BAD),
    "flags": (dict(flags=4), BAD), "flags_high": (dict(flags=RELEASED_FIRST | (1 << 31)), BAD),
    "flags_unnamed": (dict(flags=RELEASED_FIRST | fxb.STEAL_UNNAMED), BAD),
    "exclude_idle": (dict(exclude_idle=8), BAD), "exclude_idle_high": (dict(exclude_idle=FIN | (1 << 9)), BAD),
    "exclude_idle_unnamed": (dict(exclude_idle=FIN | fxb.IDLE_UNNAMED), BAD),
    "reserved": (dict(reserved=1), BAD),
    "max_out_negative": (dict(max_out=-1), BAD), "max_out_large": (dict(max_out=STEAL_MAX + 1), BAD),
    "settle_negative": (dict(settle_q15=-1), BAD),
    "count_zero": (dict(count=0), RANGE), "count_negative": (dict(count=-3), RANGE),
    "first_negative": (dict(first=-1), RANGE), "first_behind": (dict(first=1000), RANGE),
    "range_behind": (dict(first=1, count=1000), RANGE), "range_overflow": (dict(first=2**31 - 1, count=2**31 - 1), RANGE),
}


def bad_query(case):
    q = fxb.fx_steal_query(0, 1000, max_out=16)
    for k, v in BAD_QUERIES[case][0].items():
        setattr(q, k, v)
    return q


@pytest.mark.parametrize("case", list(BAD_QUERIES))
def test_fx_steal_check_refuses(case):
    assert fxb.fx_steal_check(bad_query(case), 1000) == BAD_QUERIES[case][1], case
    assert device.load().skred_amd_last_error()


def test_fx_steal_check_refuses_no_query():
    assert fxb.fx_steal_check(None, 1000) == BAD


def test_fx_steal_refusals_without_a_device():
    """NULL arguments are refused before the bank is followed (as tests/test_fx_live_cpu.py shows for the live calls)."""
    L = fxb._bind(device.load())
    q, iq = fxb.fx_steal_query(0, 1, max_out=0), fxb.FxIdleQueryC(0, 1, ENV, 0, 0, 0)
    word = (C.c_uint32 * 8)()                              # stands in for device memory: a refusal never reads it
    fake = C.c_void_p(C.addressof(word))                   # ... and for a bank: a NULL query is refused before the bank is followed
    total = C.c_int(0)
    assert L.skred_fxbank_find_steal(None, C.byref(q), None, word, None) == BAD
    assert L.skred_fxbank_find_steal(fake, None, None, word, None) == BAD
    assert L.skred_fxbank_find_steal_host(None, C.byref(q), None, C.byref(total), None) == BAD
    assert L.skred_fxbank_find_steal_host(fake, None, None, C.byref(total), None) == BAD
    notes = fxb.fx_note_array([fxb.FxNoteC(1 << 20, 32768, 0, 16384, 16384, 0)] * 4)
    p = C.cast(notes, C.c_void_p)
    assert L.skred_fxbank_note_on_steal(None, C.byref(iq), C.byref(q), p, 4, word, word, None) == BAD
    assert L.skred_fxbank_note_on_steal(fake, None, C.byref(q), p, 4, word, word, None) == BAD
    assert L.skred_fxbank_note_on_steal(fake, C.byref(iq), None, p, 4, word, word, None) == BAD
    assert L.skred_fxbank_note_on_steal(fake, C.byref(iq), C.byref(q), None, 4, word, word, None) == BAD
    assert L.skred_fxbank_note_on_steal(fake, C.byref(iq), C.byref(q), p, 4, word, None, None) == BAD
    assert b"note_on_steal" in L.skred_amd_last_error()


def random_small_bank(rng):
    n = int(rng.integers(1, 120))
    b = fxb.FxVoiceBank(n)
    now = 96000
    b["sample_start"] = rng.choice([now - 7, now - 7, now - 500, now + 3, 5, (1 << 62) + 1, (1 << 63) + 5, (3 << 32) + 5, 6], n).astype(np.uint64)
    b["sample_release"] = rng.choice([0, 0, now - 3, now - 3, 9, 1 << 40, (1 << 62) + 7], n).astype(np.uint64)
    b["is_active"] = rng.integers(0, 4, n) != 0
    b["use_envelope"] = rng.integers(0, 5, n) != 0
    b["smoother_enable"] = rng.integers(0, 4, n) != 0
    b["smoother_gain_q15"] = rng.choice([0, 0, 3, -3, 4, 20000, -(1 << 31), (1 << 31) - 1], n)
    b["finished"] = rng.integers(0, 3, n) == 0
    b["amp_q15"] = rng.choice([0, 32768, 1, 65535], n)
    return b, now


def test_fx_model_against_brute_force():
    rng = np.random.default_rng(77)
    seen = 0
    for _ in range(300):
        bank, now = random_small_bank(rng)
        first = int(rng.integers(0, bank.n))
        q = Query(first, int(rng.integers(1, bank.n - first + 1)), int(rng.integers(0, 2)),
                  int(rng.choice([0, RELEASED_FIRST, RELEASED_ONLY, RELEASED_FIRST | RELEASED_ONLY])),
                  int(rng.choice([0, 0, 7, 8, 500])), int(rng.choice([0, FIN, ENV, FIN | ENV | AMP, AMP])), int(rng.choice([0, 3])),
                  int(rng.choice([0, 1, 5, STEAL_MAX])))
        want, got = sm.brute_force(bank, now, q), sm.victim_order(bank, now, q)
        assert np.array_equal(want, got), (q, want, got)
        listed, total = sm.victims(bank, now, q)
        assert total == len(want) and np.array_equal(listed, want[:q.max_out])
        seen += len(want) > 1
    assert seen > 100


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_fx_scenes_are_not_vacuous(name):
    n, variant, make = sc.SCENES[name]
    b, pool, c0, truth, now, role, special = sc.scene(n, variant)
    queries = sc.scene_queries(name)
    for q, threshold in queries:
        if n > 1 and threshold is not None:
            sm.assert_not_vacuous(truth, now, q, bool(threshold))
        if n <= 5000:
            assert np.array_equal(sm.victim_order(truth, now, q), sm.brute_force(truth, now, q))
    totals = [(sm.victims(truth, now, q)[1], q.max_out) for q, _ in queries]
    if n > 1:
        assert any(t > m for t, m in totals) and any(t <= m for t, m in totals if m > 0), "totals on one side of max_out only"
    assert (truth["smoother_gain_q15"] != b["smoother_gain_q15"]).any(), "the blocks moved no gain: the state is the host's"
