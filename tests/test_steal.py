"""Voice stealing (skred_steal_check, skred_bank_find_steal / _find_steal_host, skred_bank_note_on_steal).

The expectation is tests/steal_model.py: the definition of include/skred_amd.h in numpy, exact.  On the GPU it is computed twice --
from the ORACLE's bank after cpuref.render of the same blocks and events, and from the download of a TWIN bank that was never
queried (DeviceBank.download returns the read-write fields; the envelope clocks, which only stamps change, are the oracle's) --
and both must equal the device's list byte for byte.  d_voices is pre-filled with -1; entries past `written` must stay -1.
The CPU part checks the argument checks, the model against a brute-force sort, and that no GPU scene is vacuous: on the oracle's
state every active restriction excludes a candidate, both classes occur under RELEASED_FIRST, and the scenes about the threshold
have more candidates than max_out.  Banks and blocks are tests/test_idle.py's (bank_c2 with a role per voice, 65 + 130 frames).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import steal_model as sm
from oracle import cpuref
from skred_amd import banks, device
from steal_model import OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, STEAL_UNNAMED, STEAL_MAX, Query
from test_idle import (AMP, DIRTY_PARAMS, DIRTY_PHASE, ENV, FIN, FRAMES, SETTLE, STAMP_RELEASE, STAMP_TRIGGER, UNNAMED, do_release,
                       expected, idle_bank, open_bank, render_blocks, traffic_bank)
from test_notes import make_notes, same_mix, same_state, store_notes

BAD, RANGE = -2, -4
WHICH = FIN | ENV


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


# ---------------------------------------------------------------------------------------------- banks and scenes

def steal_bank(n, flavour="stops", variant="plain"):
    """test_idle.idle_bank (staggered sample_start, released / finished / inactive / silent roles) with a variant on top:
    "ties"    every voice has the same sample_start, every released voice the same sample_release;
    "quiet"   two silent voices (amp 0: the render skips them, their state stays) whose smoother gains differ in sign only, and two
              sustaining voices without a smoother;
    "wide"    the clock lies past 2^32; sustaining voices get sample_start values that differ only above bit 32, two that differ only in
              bit 0, and two at or above 2^62 (they saturate to one primary: the tie goes by index);
    "ahead"   one sustaining voice is stamped ahead of the clock (age 0)."""
    bank, tables, g, role, _ = idle_bank(n, flavour)
    e = bank["voice_amp_envelope"]
    now = int(g.synth_sample_count)
    special = {}
    if variant == "ties":
        e["sample_start"][:] = np.uint64(now - 5000)
        e["sample_release"][e["sample_release"] != 0] = np.uint64(now - 10)
    if variant == "quiet":
        silent = np.flatnonzero((role == 7) & (bank["voice_smoother_enable"] != 0) & (e["is_active"] != 0))
        assert len(silent) >= 2
        a, b = int(silent[0]), int(silent[1])
        bank["voice_smoother_gain"][a], bank["voice_smoother_gain"][b] = np.float32(-0.25), np.float32(0.25)
        special["sign_pair"] = (a, b)
        hold = np.flatnonzero(role == 0)
        bank["voice_smoother_enable"][hold[[2, 5]]] = 0                      # sustaining voices without a smoother: they sort last
    if variant == "wide":
        g.synth_sample_count = (1 << 33) + 12345
        now = int(g.synth_sample_count)
        rel = e["sample_release"] != 0
        e["sample_release"][rel] = np.uint64(now - 10)
        hold = np.flatnonzero(role == 0)
        assert len(hold) >= 12
        e["sample_start"][:] = np.uint64(now - 3000)
        for k, v in enumerate(hold[:6]):
            e["sample_start"][v] = np.uint64(777 + ((k % 3) << 32))          # differ only above bit 32 (and pairwise equal: ties)
        e["sample_start"][hold[6]], e["sample_start"][hold[7]] = np.uint64(4001), np.uint64(4000)   # differ only in bit 0
        e["sample_start"][hold[8]], e["sample_start"][hold[9]] = np.uint64((1 << 62) + 9), np.uint64(1 << 62)   # saturate
        special["hold"] = hold[:10].astype(int).tolist()
    if variant == "ahead":
        hold = np.flatnonzero(role == 0)
        e["sample_start"][hold[1]] = np.uint64(now + 100000)
        special["ahead"] = int(hold[1])
    return bank, tables, g, role, special


@functools.lru_cache(maxsize=16)
def scene(n, flavour="stops", variant="plain"):
    """(bank, tables, globals, the oracle's bank after FRAMES, now after FRAMES, role, special)"""
    bank, tables, g, role, special = steal_bank(n, flavour, variant)
    truth, gl = bank.copy(), g.copy()
    for f in FRAMES:
        cpuref.render(truth, gl, tables, f, 0)
    return bank, tables, g, truth, int(gl.synth_sample_count), role, special


def q_all(n, **kw):
    return Query(0, n, **kw)


def queries_sizes(n, truth, now, role, special):
    """what every size runs: (query, about the threshold)"""
    k = min(n, 16)
    return [(q_all(n, max_out=k), n > 100),
            (q_all(n, flags=RELEASED_FIRST, max_out=min(n, STEAL_MAX)), False),
            (q_all(n, flags=RELEASED_ONLY, max_out=k), False),
            (q_all(n, policy=QUIETEST, flags=RELEASED_FIRST, max_out=k), n > 100),
            (q_all(n, exclude_idle=FIN | ENV, settle_level=float(SETTLE), max_out=k), n > 100),
            (Query(37, 300, flags=RELEASED_FIRST, exclude_idle=FIN, max_out=40) if n > 400 else q_all(n, max_out=1), n > 400)]


def queries_min_age(n, truth, now, role, special):
    e = truth["voice_amp_envelope"]
    w = int(np.flatnonzero((role == 0) & (e["is_active"] != 0))[3])
    age = now - int(e["sample_start"][w])
    out = []
    for d, inside in ((0, True), (1, False), (-1, True)):      # min_age exactly at, one above, one below w's age
        q = q_all(n, min_age=age + d, max_out=STEAL_MAX)
        assert (w in sm.victim_order(truth, now, q)) == inside
        out.append((q, False))
    ahead = special["ahead"]                                     # stamped ahead of the clock: age 0
    assert ahead in sm.victim_order(truth, now, q_all(n)) and ahead not in sm.victim_order(truth, now, q_all(n, min_age=1))
    assert sm.victim_order(truth, now, q_all(n))[-1] == ahead    # ... and the youngest of all
    out.append((q_all(n, min_age=1, max_out=STEAL_MAX), False))
    return out


def queries_quiet(n, truth, now, role, special):
    a, b = special["sign_pair"]
    order = sm.victim_order(truth, now, q_all(n, policy=QUIETEST)).tolist()
    assert order.index(b) == order.index(a) + 1, "the two gains that differ in sign only are not neighbours in index order"
    off = np.flatnonzero(truth["voice_smoother_enable"] == 0)
    cand_off = [v for v in off if v in set(order)]
    assert cand_off and set(order[-len(cand_off):]) == set(cand_off), "smoother-off candidates do not sort last"
    return [(q_all(n, policy=QUIETEST, max_out=STEAL_MAX), False), (q_all(n, policy=QUIETEST, max_out=order.index(b)), True),
            (q_all(n, policy=QUIETEST, flags=RELEASED_ONLY, max_out=8), False)]


def queries_wide(n, truth, now, role, special):
    hold = special["hold"]
    order = sm.victim_order(truth, now, q_all(n)).tolist()
    first10 = order[:8]
    assert set(first10) == set(hold[:8]), "the early starts are not the oldest voices"
    assert order.index(hold[7]) < order.index(hold[6])          # 4000 before 4001: bit 0 decides
    assert order[-2:] == sorted(hold[8:10]), "the two saturated keys tie and go by index"
    return [(q_all(n, max_out=STEAL_MAX), False), (q_all(n, max_out=3), True), (q_all(n, max_out=7), True),
            (q_all(n, flags=RELEASED_FIRST, max_out=STEAL_MAX), False)]


def queries_ties(n, truth, now, role, special):
    total = len(sm.victim_order(truth, now, q_all(n)))
    assert total > 20000, total
    return [(q_all(n, max_out=STEAL_MAX), True), (q_all(n, max_out=1), True),
            (q_all(n, flags=RELEASED_FIRST, max_out=STEAL_MAX), True),
            (Query(11, n - 30, flags=RELEASED_FIRST, max_out=STEAL_MAX), True)]


def queries_counts(n, truth, now, role, special):
    rel = len(sm.victim_order(truth, now, q_all(n, flags=RELEASED_ONLY)))
    assert 0 < rel < STEAL_MAX
    return [(q_all(n, max_out=0), False), (q_all(n, flags=RELEASED_ONLY, max_out=STEAL_MAX), False),    # total < max_out
            (q_all(n, flags=RELEASED_ONLY, max_out=rel), False), (q_all(n, max_out=STEAL_MAX), True)]


def queries_mod(n, truth, now, role, special):
    return [(q_all(n, flags=STEAL_UNNAMED, max_out=STEAL_MAX), False),
            (q_all(n, flags=STEAL_UNNAMED | RELEASED_FIRST, exclude_idle=FIN | UNNAMED, max_out=50), True),
            (q_all(n, policy=QUIETEST, flags=STEAL_UNNAMED, max_out=50), True)]


def queries_finished(n, truth, now, role, special):
    """FINISHED one-shots whose envelope is still active: candidates, unless the idle query would list them."""
    a = truth.a
    still = (a["voice_finished"] != 0) & (a["voice_amp_envelope"]["is_active"] != 0) & (a["voice_use_amp_envelope"] != 0)
    assert still.any()
    v = int(np.flatnonzero(still)[0])
    assert v in sm.victim_order(truth, now, q_all(n)) and v not in sm.victim_order(truth, now, q_all(n, exclude_idle=FIN))
    return [(q_all(n, exclude_idle=FIN, max_out=STEAL_MAX), False), (q_all(n, exclude_idle=FIN | AMP, max_out=STEAL_MAX), False)]


SETUP_FAST2 = "fast2"
SCENES = {
    # id: (n, flavour, variant, queries, kernel the blocks must have run on, setup)
    "n63": (63, "stops", "plain", queries_sizes, 1, None),
    "n64": (64, "stops", "plain", queries_sizes, 1, None),
    "n65": (65, "stops", "plain", queries_sizes, 1, None),
    "n1000_one_voice": (1000, "stops", "plain", queries_sizes, 1, None),
    "n4096_two_per_lane": (4096, "fast2", "plain", queries_sizes, 3, SETUP_FAST2),
    "n70000": (70000, "stops", "plain", queries_sizes, 1, None),
    "min_age_and_ahead": (1000, "stops", "ahead", queries_min_age, 1, None),
    "quietest": (1000, "stops", "quiet", queries_quiet, 1, None),
    "key_width": (1000, "stops", "wide", queries_wide, 1, None),
    "ties_70000": (70000, "stops", "ties", queries_ties, 1, None),
    "counts": (4096, "stops", "plain", queries_counts, 1, None),
    "unnamed_mod": (1000, "mod", "plain", queries_mod, 2, None),
    "finished_one_shots": (1000, "stops", "plain", queries_finished, 1, None),
}


def scene_queries(name):
    n, flavour, variant, make, kernel, setup = SCENES[name]
    bank, tables, g, truth, now, role, special = scene(n, flavour, variant)
    return make(n, truth, now, role, special)


# ---------------------------------------------------------------------------------------------- CPU: checks, model, scenes

def test_steal_check_accepts_valid_queries():
    assert device.steal_check(device.steal_query(0, 1000, max_out=16), 1000) == 0
    assert device.steal_check(device.steal_query(37, 300, QUIETEST, RELEASED_FIRST | RELEASED_ONLY | STEAL_UNNAMED, 2**63, FIN | ENV | AMP | UNNAMED,
                                                 1e-3, STEAL_MAX), 1000) == 0
    assert device.steal_check(device.steal_query(999, 1, max_out=0, settle_level=-0.0), 1000) == 0
    assert C.sizeof(device.StealQueryC) == 40
    assert (device.STEAL_OLDEST, device.STEAL_QUIETEST, device.STEAL_RELEASED_FIRST, device.STEAL_RELEASED_ONLY, device.STEAL_UNNAMED,
            device.STEAL_MAX) == (0, 1, 1, 2, 256, 1024)


BAD_QUERIES = {
    "policy": (dict(policy=2), BAD), "policy_high": (dict(policy=1 << 31), BAD),
    "flags": (dict(flags=4), BAD), "flags_high": (dict(flags=RELEASED_FIRST | (1 << 31)), BAD),
    "exclude_idle": (dict(exclude_idle=8), BAD), "exclude_idle_high": (dict(exclude_idle=FIN | (1 << 9)), BAD),
    "reserved": (dict(reserved=1), BAD),
    "max_out_negative": (dict(max_out=-1), BAD), "max_out_large": (dict(max_out=STEAL_MAX + 1), BAD),
    "settle_negative": (dict(settle_level=-1.0), BAD), "settle_nan": (dict(settle_level=float("nan")), BAD),
    "settle_inf": (dict(settle_level=float("inf")), BAD),
    "count_zero": (dict(count=0), RANGE), "count_negative": (dict(count=-3), RANGE),
    "first_negative": (dict(first=-1), RANGE), "first_behind": (dict(first=1000), RANGE),
    "range_behind": (dict(first=1, count=1000), RANGE), "range_overflow": (dict(first=2**31 - 1, count=2**31 - 1), RANGE),
}


def bad_query(case):
    q = device.steal_query(0, 1000, max_out=16)
    for k, v in BAD_QUERIES[case][0].items():
        setattr(q, k, v)
    return q


@pytest.mark.parametrize("case", list(BAD_QUERIES))
def test_steal_check_refuses(case):
    assert device.steal_check(bad_query(case), 1000) == BAD_QUERIES[case][1], case
    assert device.load().skred_amd_last_error()


def test_refusals_without_a_device():
    L = device.load()
    for s in ("skred_steal_check", "skred_bank_find_steal", "skred_bank_find_steal_host", "skred_bank_note_on_steal"):
        assert hasattr(L, s), f"libskred_amd.so does not export {s}"
    assert L.skred_steal_check(None, 1000) == BAD
    q, iq = device.steal_query(0, 1, max_out=0), device.IdleQueryC(0, 1, ENV, 0.0, 0, 0)
    word = (C.c_uint32 * 8)()                             # stands in for device memory: a refusal never reads it
    fake = C.c_void_p(C.addressof(word))                  # ... and for a bank: a NULL query is refused before the bank is followed
    total = C.c_int(0)
    assert L.skred_bank_find_steal(None, C.byref(q), None, word, None) == BAD
    assert L.skred_bank_find_steal(fake, None, None, word, None) == BAD
    assert L.skred_bank_find_steal_host(None, C.byref(q), None, C.byref(total), None) == BAD
    assert L.skred_bank_find_steal_host(fake, None, None, C.byref(total), None) == BAD
    notes = device.note_array(make_notes(4, 2))
    p = C.cast(notes, C.c_void_p)
    assert L.skred_bank_note_on_steal(None, C.byref(iq), C.byref(q), p, 4, word, word, None) == BAD
    assert L.skred_bank_note_on_steal(fake, None, C.byref(q), p, 4, word, word, None) == BAD
    assert L.skred_bank_note_on_steal(fake, C.byref(iq), None, p, 4, word, word, None) == BAD
    assert L.skred_bank_note_on_steal(fake, C.byref(iq), C.byref(q), None, 4, word, word, None) == BAD
    assert L.skred_bank_note_on_steal(fake, C.byref(iq), C.byref(q), p, 4, word, None, None) == BAD
    assert b"note_on_steal" in L.skred_amd_last_error()


def random_small_bank(rng):
    n = int(rng.integers(1, 120))
    bank, _, g = banks.bank_c2(n)
    e = bank["voice_amp_envelope"]
    now = int(g.synth_sample_count)
    e["sample_start"][:] = rng.choice([now - 7, now - 7, now - 500, now + 3, 5, (1 << 62) + 1, (1 << 63) + 5, (3 << 32) + 5, 6], n).astype(np.uint64)
    e["sample_release"][:] = rng.choice([0, 0, now - 3, now - 3, 9, 1 << 40], n).astype(np.uint64)
    e["is_active"][:] = rng.integers(0, 4, n) != 0
    bank["voice_use_amp_envelope"][:] = rng.integers(0, 5, n) != 0
    bank["voice_smoother_enable"][:] = rng.integers(0, 4, n) != 0
    bank["voice_smoother_gain"][:] = rng.choice(np.array([0.0, -0.0, 0.5, -0.5, 1e-4, -1e-40, 3.0, np.nan], np.float32), n)
    bank["voice_finished"][:] = rng.integers(0, 3, n) == 0
    bank["voice_amp"][:] = rng.choice(np.array([0.0, 1.0, -0.0, 0.3], np.float32), n)
    mod = rng.integers(0, 3, n) == 0
    bank["voice_amp_mod_osc"][mod] = rng.integers(0, n, int(mod.sum()))
    return bank, now


def test_model_against_brute_force():
    rng = np.random.default_rng(77)
    seen = 0
    for _ in range(300):
        bank, now = random_small_bank(rng)
        first = int(rng.integers(0, bank.n))
        q = Query(first, int(rng.integers(1, bank.n - first + 1)), int(rng.integers(0, 2)),
                  int(rng.choice([0, RELEASED_FIRST, RELEASED_ONLY, RELEASED_FIRST | STEAL_UNNAMED, RELEASED_FIRST | RELEASED_ONLY])),
                  int(rng.choice([0, 0, 7, 8, 500])), int(rng.choice([0, FIN, ENV, FIN | ENV | AMP, AMP | UNNAMED])),
                  float(rng.choice([0.0, 1e-3])))
        want, got = sm.brute_force(bank, now, q), sm.victim_order(bank, now, q)
        assert np.array_equal(want, got), (q, want, got)
        seen += len(want) > 1
    assert seen > 100


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_are_not_vacuous(name):
    n, flavour, variant, make, kernel, setup = SCENES[name]
    bank, tables, g, truth, now, role, special = scene(n, flavour, variant)
    for q, threshold in scene_queries(name):
        sm.assert_not_vacuous(truth, now, q, threshold)
        if n <= 5000:
            assert np.array_equal(sm.victim_order(truth, now, q), sm.brute_force(truth, now, q))


# ---------------------------------------------------------------------------------------------- GPU: the list

def reach(dev, name):
    """(queried bank, oracle's bank, the twin's state on the oracle's clocks, now) after FRAMES"""
    n, flavour, variant, make, kernel, setup = SCENES[name]
    bank, tables, g, truth, now, role, special = scene(n, flavour, variant)
    su = (lambda d: d.fast2_min_voices(0)) if setup == SETUP_FAST2 else None
    db, twin = open_bank(dev, bank, tables, g, su), open_bank(dev, bank, tables, g, su)
    render_blocks(db, FRAMES)
    render_blocks(twin, FRAMES)
    assert db.last_kernel() == kernel, (name, db.last_kernel())
    got = truth.copy()
    twin.download(got)
    twin.close()
    return db, truth, got, now


def query(db, q, stream=0, sync=True):
    import torch
    dv = torch.full((q.max_out + 8,), -1, dtype=torch.int32, device="cuda")
    dc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    db.find_steal(q.c(), dv.data_ptr(), dc.data_ptr(), stream)
    if sync:
        torch.cuda.synchronize()
    return dv.cpu().numpy(), dc.cpu().numpy()


def check(db, truth, got, now, q):
    want = sm.victim_order(truth, now, q)
    assert np.array_equal(want, sm.victim_order(got, now, q)), "the oracle's state and the twin's downloaded state disagree"
    dv, dc = query(db, q)
    total, written = len(want), min(len(want), q.max_out)
    print(f"{q}: total {total}, written {written}")
    assert (int(dc[0]), int(dc[1])) == (written, total), f"{q}: d_count {dc.tolist()}, expected ({written}, {total})"
    assert np.array_equal(dv[:written], want[:written]), f"{q}: first mismatch at {int(np.flatnonzero(dv[:written] != want[:written])[0])}"
    assert (dv[written:] == -1).all(), f"{q}: entries past `written` were touched"
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_scenes(dev, name):
    db, truth, got, now = reach(dev, name)
    try:
        for q, _ in scene_queries(name):
            check(db, truth, got, now, q)
        q = scene_queries(name)[0][0]
        a, b = query(db, q), query(db, q)                       # the same state gives the same bytes
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    finally:
        db.close()


@pytest.mark.gpu
def test_one_voice_banks(dev):
    """n = 1: a bank whose voice is a candidate, one whose voice is not (no envelope), and an empty list with max_out > 0."""
    for use_env, total in ((1, 1), (0, 0)):
        bank, tables, g = banks.bank_c2(1)
        bank["voice_use_amp_envelope"][0] = use_env
        db = open_bank(dev, bank, tables, g)
        try:
            render_blocks(db, FRAMES)
            truth, gl = bank.copy(), g.copy()
            for f in FRAMES:
                cpuref.render(truth, gl, tables, f, 0)
            got = truth.copy()
            db.download(got)
            now = int(gl.synth_sample_count)
            for q in (Query(0, 1, max_out=1), Query(0, 1, QUIETEST, RELEASED_FIRST, max_out=5), Query(0, 1, max_out=0)):
                assert len(check(db, truth, got, now, q)) == total
            voices, tot = db.find_steal_host(Query(0, 1, max_out=4).c())
            assert tot == total and len(voices) == total
        finally:
            db.close()


@pytest.mark.gpu
def test_host_variant(dev):
    db, truth, got, now = reach(dev, "n1000_one_voice")
    try:
        for q in (Query(0, 1000, flags=RELEASED_FIRST, max_out=16), Query(0, 1000, QUIETEST, max_out=STEAL_MAX), Query(5, 100, max_out=0)):
            want = sm.victim_order(truth, now, q)
            voices, tot = db.find_steal_host(q.c())
            assert tot == len(want) and np.array_equal(voices, want[:q.max_out])
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- purity, stream order

def varied_traffic_bank(n):
    bank, tables, g = traffic_bank(n)
    v = np.arange(n)
    bank["voice_amp_envelope"]["sample_start"][:] = (int(g.synth_sample_count) - 40000 - (v * 7919) % 1000).astype(np.uint64)
    return bank, tables, g


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["one_voice", "fast2"])
def test_query_reads_the_bank_only(dev, family):
    """A bank queried after every block against an unqueried twin under note traffic: state, globals and mix bit for bit."""
    n, F = 4096, 256
    bank, tables, g = varied_traffic_bank(n)
    setup = (lambda d: d.fast2_min_voices(0)) if family == "fast2" else None
    db, twin = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    mirror = bank.copy()
    rng = np.random.default_rng(5)
    try:
        for k in range(5):
            vs = np.sort(rng.choice(n, 24, replace=False)).astype(np.int32)
            mirror["voice_phase"][vs[12:]] = 0.0
            for d in (db, twin):
                d.update(mirror, vs[:12], STAMP_RELEASE)
                d.update(mirror, vs[12:], DIRTY_PARAMS | DIRTY_PHASE | STAMP_TRIGGER)
            mixes = [render_blocks(d, (F,))[0] for d in (db, twin)]
            assert (mixes[0].view(np.uint32) == mixes[1].view(np.uint32)).all(), f"block {k}: the query changed the mix"
            assert db.last_kernel() == twin.last_kernel() == (3 if family == "fast2" else 1)
            assert db.last_pack() == twin.last_pack() and db.list_violations() == twin.list_violations() == 0
            dv, dc = query(db, Query(0, n, OLDEST, RELEASED_FIRST | STEAL_UNNAMED, 10, FIN | ENV | UNNAMED, float(SETTLE), STEAL_MAX))
            assert dc[1] > 0
            query(db, Query(37, 300, QUIETEST, max_out=0))
        a, b = bank.copy(), bank.copy()
        db.download(a)
        twin.download(b)
        assert not a.rw_equal(b), a.rw_equal(b)
        ga, gb = db.get_globals(), twin.get_globals()
        assert ga.synth_sample_count == gb.synth_sample_count and ga.noise_rng == gb.noise_rng
        assert np.float32(ga.volume_smoother_gain).tobytes() == np.float32(gb.volume_smoother_gain).tobytes()
    finally:
        db.close()
        twin.close()


@pytest.mark.gpu
def test_stream_order_without_a_host_wait(dev):
    """A release stamp and the query behind it on one stream, nothing waited for in between: the query sees the release."""
    import torch
    n = 1000
    bank, tables, g = varied_traffic_bank(n)
    db = open_bank(dev, bank, tables, g)
    try:
        s = torch.cuda.Stream()
        q = Query(0, n, flags=RELEASED_ONLY, max_out=n if n < STEAL_MAX else STEAL_MAX)
        truth = bank.copy()
        now = int(g.synth_sample_count)
        assert len(sm.victim_order(truth, now, q)) == 0
        released = np.arange(0, n, 16, dtype=np.int32)
        dv = torch.full((q.max_out + 8,), -1, dtype=torch.int32, device="cuda")
        dc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        db.update(bank, released, STAMP_RELEASE, s.cuda_stream)
        db.find_steal(q.c(), dv.data_ptr(), dc.data_ptr(), s.cuda_stream)
        s.synchronize()
        do_release(truth, released, now)
        want = sm.victim_order(truth, now, q)
        assert set(want) == set(released[released % 8 == 0]) and len(want) > 0
        got, cnt = dv.cpu().numpy(), dc.cpu().numpy()
        assert cnt.tolist() == [len(want), len(want)]
        assert np.array_equal(got[:len(want)], want) and (got[len(want):] == -1).all()
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- note_on_steal

def outputs3(K, fill=-7):
    import torch
    return (torch.full((K + 8,), fill, dtype=torch.int32, device="cuda"), torch.full((3,), fill, dtype=torch.int32, device="cuda"))


def model_placement(truth, now, idle_range, sq, K):
    """(voices the K notes go to, -1 for dropped ones; placed, dropped, stolen)"""
    idle = expected(truth, idle_range[0], idle_range[1], WHICH, SETTLE)[:K]
    q = sq.but(exclude_idle=WHICH, settle_level=float(SETTLE), max_out=min(K, STEAL_MAX))
    victims = sm.victim_order(truth, now, q)[:q.max_out]
    assert not set(idle) & set(victims)
    joined = np.concatenate([idle, victims]).astype(np.int32)[:K]
    stolen = len(joined) - len(idle)
    out = np.full(K, -1, np.int32)
    out[:len(joined)] = joined
    return out, (len(joined), K - len(joined), stolen)


@pytest.mark.gpu
@pytest.mark.parametrize("n,family", [(1000, 1), (4096, 3)])
def test_note_on_steal_same_as_the_host_path(dev, n, family):
    """A batch larger than the idle list: `db` places it with note_on_steal; `twin` asks find_idle_host and find_steal_host, writes the
    host view and sends one update.  Mix and state bit-equal after two further blocks, and equal to the oracle's."""
    import torch
    K, F = 16, 256
    bank, tables, g = varied_traffic_bank(n)
    setup = (lambda d: d.fast2_min_voices(0)) if family == 3 else None
    db, twin = open_bank(dev, bank, tables, g, setup), open_bank(dev, bank, tables, g, setup)
    truth, gl, mirror = bank.copy(), g.copy(), bank.copy()
    try:
        for d in (db, twin):
            render_blocks(d, (F,))
        cpuref.render(truth, gl, tables, F, 0)
        now = int(gl.synth_sample_count)
        notes = make_notes(K, 4)
        sq = Query(0, n, OLDEST, RELEASED_FIRST, min_age=1)
        want, counts = model_placement(truth, now, (3, 7), sq, K)
        assert counts[0] == K and 0 < counts[2] < K, counts
        idle, _ = twin.find_idle_host(3, 7, WHICH, float(SETTLE), None, K)
        victims, _ = twin.find_steal_host(sq.but(exclude_idle=WHICH, settle_level=float(SETTLE), max_out=K).c())
        picks = np.concatenate([idle, victims]).astype(np.int32)[:K]
        assert np.array_equal(picks, want)
        da, dr = outputs3(K)
        torch.cuda.synchronize()
        db.note_on_steal(notes, device.IdleQueryC(3, 7, WHICH, float(SETTLE), 3, 0), sq.c(), da.data_ptr(), dr.data_ptr())
        store_notes((truth, mirror), truth, notes, picks, now)
        twin.update(mirror, picks, DIRTY_PARAMS | DIRTY_PHASE | STAMP_TRIGGER)
        for k in range(2):
            same_mix(db, twin, F, f"n {n} block {k}")
            cpuref.render(truth, gl, tables, F, 0)
        got, res = da.cpu().numpy(), dr.cpu().numpy()
        assert np.array_equal(got[:K], want) and (got[K:] == -7).all(), (got.tolist(), want.tolist())
        assert tuple(res.tolist()) == counts, (res.tolist(), counts)
        same_state(db, twin, truth, bank, f"n {n}")
        assert db.last_kernel() == twin.last_kernel() == family
        assert db.list_violations() == twin.list_violations() == 0
    finally:
        db.close()
        twin.close()


@pytest.mark.gpu
def test_note_on_steal_counts_and_note_off(dev):
    """d_result and d_assigned against the model: nothing stolen, everything stolen, more notes than idle voices plus victims; then
    stamp_list on a returned d_assigned releases exactly those voices."""
    import torch
    n, K, F = 1000, 16, 256
    bank, tables, g = varied_traffic_bank(n)
    db = open_bank(dev, bank, tables, g)
    truth, gl = bank.copy(), g.copy()
    try:
        render_blocks(db, (F,))
        cpuref.render(truth, gl, tables, F, 0)
        now = int(gl.synth_sample_count)
        last = None
        for tag, idle_range, sq, shape in (("nothing stolen", (0, n), Query(0, n), (K, 0, 0)),
                                           ("all stolen", (8, 1), Query(0, n, QUIETEST), (K, 0, K)),
                                           ("some dropped", (17, 7), Query(0, 4, OLDEST, RELEASED_FIRST), None)):
            notes = make_notes(K, 9)
            want, counts = model_placement(truth, now, idle_range, sq, K)
            if shape is not None:
                assert counts == shape, (tag, counts)
            else:
                assert counts[1] > 0 and counts[2] > 0 and counts[0] > counts[2], (tag, counts)
            da, dr = outputs3(K)
            torch.cuda.synchronize()
            db.note_on_steal(notes, device.IdleQueryC(idle_range[0], idle_range[1], WHICH, float(SETTLE), idle_range[0], 0), sq.c(),
                             da.data_ptr(), dr.data_ptr())
            torch.cuda.synchronize()
            got, res = da.cpu().numpy(), dr.cpu().numpy()
            assert tuple(res.tolist()) == counts, (tag, res.tolist(), counts)
            assert np.array_equal(got[:K], want) and (got[K:] == -7).all(), (tag, got.tolist(), want.tolist())
            store_notes((truth,), truth, notes, want, now)
            last = (da, want)
        # n == 0: nothing happens
        da0, dr0 = outputs3(K)
        torch.cuda.synchronize()
        db.note_on_steal([], device.IdleQueryC(0, n, WHICH, float(SETTLE), 0, 0), Query(0, n).c(), da0.data_ptr(), dr0.data_ptr())
        torch.cuda.synchronize()
        assert (dr0.cpu().numpy() == -7).all() and (da0.cpu().numpy() == -7).all()
        # the note-off list: exactly the placed voices of the last batch are in release afterwards
        q = Query(0, n, flags=RELEASED_ONLY, max_out=STEAL_MAX)
        assert len(sm.victim_order(truth, now, q)) == 0
        da, want = last
        db.stamp_list(da.data_ptr(), K, STAMP_RELEASE)
        do_release(truth, want[want >= 0], now)
        dv, dc = query(db, q)
        assert set(dv[:dc[0]].tolist()) == set(want[want >= 0].tolist()) and dc[0] == (want >= 0).sum()
        assert np.array_equal(dv[:dc[0]], sm.victim_order(truth, now, q))
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_leave_the_bank_usable(dev):
    import torch
    db, truth, got, now = reach(dev, "n1000_one_voice")
    try:
        L = db.L
        dv = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        dc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        dr = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        good = Query(0, 1000, flags=RELEASED_FIRST, max_out=16)
        notes = device.note_array(make_notes(4, 1))
        p = C.cast(notes, C.c_void_p)
        iq = device.IdleQueryC(0, 1000, WHICH, float(SETTLE), 0, 0)
        for case, (_, code) in BAD_QUERIES.items():
            q = bad_query(case)
            assert L.skred_bank_find_steal(db.h, C.byref(q), dv.data_ptr(), dc.data_ptr(), None) == code, case
            host = np.full(STEAL_MAX, -1, np.int32)
            assert L.skred_bank_find_steal_host(db.h, C.byref(q), host.ctypes.data, None, None) == code, case
            if case not in ("exclude_idle", "exclude_idle_high", "max_out_negative", "max_out_large", "settle_negative", "settle_nan", "settle_inf"):
                # (the library overrides exclude_idle, settle_level and max_out from the idle query)
                assert L.skred_bank_note_on_steal(db.h, C.byref(iq), C.byref(q), p, 4, None, dr.data_ptr(), None) == code, case
            check(db, truth, got, now, good)                     # a valid query works after each refusal
        g = good.c()
        assert L.skred_bank_find_steal(db.h, C.byref(g), None, dc.data_ptr(), None) == BAD          # max_out > 0 and no list
        assert L.skred_bank_find_steal(db.h, C.byref(g), dv.data_ptr(), None, None) == BAD
        bad_iq = device.IdleQueryC(0, 1000, WHICH | AMP, float(SETTLE), 0, 0)
        assert L.skred_bank_note_on_steal(db.h, C.byref(bad_iq), C.byref(g), p, 4, None, dr.data_ptr(), None) == BAD
        bad_iq = device.IdleQueryC(0, 1001, WHICH, float(SETTLE), 0, 0)
        assert L.skred_bank_note_on_steal(db.h, C.byref(bad_iq), C.byref(g), p, 4, None, dr.data_ptr(), None) == RANGE
        notes[2].flags = 4
        assert L.skred_bank_note_on_steal(db.h, C.byref(iq), C.byref(g), p, 4, None, dr.data_ptr(), None) == BAD
        torch.cuda.synchronize()
        assert (dr.cpu().numpy() == -1).all()
        check(db, truth, got, now, good)
    finally:
        db.close()
