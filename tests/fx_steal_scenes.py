"""Banks and queries of the fixed-point voice-stealing tests (tests/test_fx_steal_cpu.py shows that none is vacuous,
tests/test_fx_steal.py runs them on the GPU).  A scene is a host-written bank, the blocks rendered on it by oracle.cpuref.fx_render
-- the state "as the device holds it" -- and the queries asked after them."""
import functools

import numpy as np

import fx_steal_model as sm
from fx_steal_model import AMP, ENV, FIN, OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, STEAL_MAX, Query
from oracle import cpuref
from skred_amd import fxbank as fxb

FRAMES = ((65, 1), (130, 0))            # (frames, interp) rendered before the queries
WIDE_CLOCK = (1 << 33) + 12345
DIGIT_BITS = [55, 44, 33, 22, 11, 0]    # the lowest bit of each of the select's six 11-bit digits (the first holds the top 9 bits)


def steal_bank(n, variant="plain"):
    """bank_fx without filters, a role per voice (v mod 8):
      0 held   1 released, still sounding   2 released long ago: the envelope ends in the first block   3 no envelope
      4 a one-shot that finished while active   5 amp_q15 == 0 (skipped: its state stays)   6 held, no smoother   7 inactive, gain 0
    Variants: "ties" one sample_start, one sample_release for all; "quiet" frozen gains 0, 0, 7, -7, 7, -2^31 on role-5 voices;
    "wide" the clock past 2^32 and pairs of held voices whose starts differ in one bit of each of the six digits; "ahead" one held
    voice stamped ahead of the clock."""
    b, pool, c0 = fxb.bank_fx(n, with_filter=False)
    if variant == "wide":
        b["sample_start"] = b["sample_start"] + np.uint64(WIDE_CLOCK - c0)
        c0 = WIDE_CLOCK
    v = np.arange(n)
    role = v % 8
    special = {}
    b["release_frames"] = 9600
    b["sample_release"][role == 1] = (c0 - 1 - (v[role == 1] * 7) % 50).astype(np.uint64)
    b["sample_release"][role == 2] = np.uint64(c0 - 20000)
    b["use_envelope"][role == 3] = 0
    one = v[role == 4]
    b["one_shot"][one], b["finished"][one], b["phase"][one], b["smoother_gain_q15"][one] = 1, 1, 0xFFFFFFFF, 50
    b["amp_q15"][role == 5] = 0
    b["smoother_gain_q15"][role == 5] = 100 + (v[role == 5] % 5)
    b["smoother_enable"][role == 6] = 0
    b["is_active"][role == 7], b["smoother_gain_q15"][role == 7] = 0, 0
    if variant == "ties":
        b["sample_start"] = np.uint64(c0 - 5000)
        b["sample_release"][b["sample_release"] != 0] = np.uint64(c0 - 10)
    if variant == "quiet":
        frozen = v[role == 5][:6]
        b["smoother_gain_q15"][frozen] = [0, 0, 7, -7, 7, -(1 << 31)]
        special["frozen"] = frozen.tolist()
    if variant == "wide":
        held = v[role == 0]
        base = WIDE_CLOCK - 11345                    # 2^33 + 1000: bit 33 set, the bits the pairs flip clear (but 33)
        pairs = []
        for k, bit in enumerate(DIGIT_BITS):
            a, c = int(held[2 * k]), int(held[2 * k + 1])
            b["sample_start"][a], b["sample_start"][c] = np.uint64(base), np.uint64(base ^ (1 << bit))
            pairs.append((a, c))
        sat = (int(held[12]), int(held[13]))         # at and above 2^62: one primary, the tie goes by index
        b["sample_start"][sat[0]], b["sample_start"][sat[1]] = np.uint64((1 << 62) + 9), np.uint64(1 << 62)
        special["pairs"], special["saturated"] = pairs, sat
    if variant == "ahead":
        w = int(v[role == 0][1])
        b["sample_start"][w] = np.uint64(c0 + 100000)
        special["ahead"] = w
    return b, pool, c0, role, special


@functools.lru_cache(maxsize=16)
def scene(n, variant="plain"):
    """(bank, pool, c0, the oracle's bank after FRAMES, now after FRAMES, role, special)"""
    b, pool, c0, role, special = steal_bank(n, variant)
    truth, cnt = b.copy(), c0
    for frames, interp in FRAMES:
        _, _, cnt = cpuref.fx_render(truth, pool, cnt, frames, interp)
    return b, pool, c0, truth, int(cnt), role, special


def q_all(n, **kw):
    return Query(0, n, **kw)


def queries_sizes(n, truth, now, role, special):
    """what every size runs: (query, about the threshold -- None: too small a range to hold candidates AND non-candidates)"""
    k = min(n, 16)
    out = [(q_all(n, max_out=k), False), (q_all(n, max_out=0), False), (q_all(n, max_out=1), False)]
    if n >= 63:
        out += [(q_all(n, flags=RELEASED_FIRST, max_out=min(n, STEAL_MAX)), False),
                (q_all(n, flags=RELEASED_ONLY, max_out=k), False),
                (q_all(n, flags=RELEASED_FIRST | RELEASED_ONLY, max_out=k), False),
                (q_all(n, policy=QUIETEST, flags=RELEASED_FIRST, max_out=k), False),
                (q_all(n, policy=QUIETEST, max_out=STEAL_MAX), False),
                (q_all(n, exclude_idle=FIN, max_out=k), False), (q_all(n, exclude_idle=AMP, settle_q15=3, max_out=k), False),
                (q_all(n, exclude_idle=ENV, max_out=k), False), (q_all(n, exclude_idle=ENV, settle_q15=3, max_out=k), False),
                (q_all(n, exclude_idle=FIN | ENV | AMP, settle_q15=3, max_out=STEAL_MAX), False),
                (Query(n - 1, 1, max_out=4), None), (Query(n // 2 + 1, 1, max_out=4), None)]              # one-voice ranges
    if n > 400:
        out += [(Query(37, 300, flags=RELEASED_FIRST, exclude_idle=FIN, max_out=40), False),            # first % 64 != 0, the end inside a span
                (Query(70, 40, policy=QUIETEST, max_out=STEAL_MAX), False)]
    return out


def queries_min_age(n, truth, now, role, special):
    w = int(np.flatnonzero(role == 0)[3])
    age = now - int(truth["sample_start"][w])
    out = []
    for d, inside in ((0, True), (1, False), (-1, True)):      # min_age exactly at, one above, one below w's age
        q = q_all(n, min_age=age + d, max_out=STEAL_MAX)
        assert (w in sm.victim_order(truth, now, q)) == inside
        out.append((q, False))
    ahead = special["ahead"]                                     # stamped ahead of the clock: age 0, the youngest of all
    assert sm.victim_order(truth, now, q_all(n))[-1] == ahead and ahead not in sm.victim_order(truth, now, q_all(n, min_age=1))
    out.append((q_all(n, min_age=1, max_out=STEAL_MAX), False))
    out.append((q_all(n, min_age=age, max_out=16), False))
    return out


def queries_quiet(n, truth, now, role, special):
    f = special["frozen"]
    order = sm.victim_order(truth, now, q_all(n, policy=QUIETEST)).tolist()
    assert order[:2] == f[:2], "the two gains of 0 do not lead, in index order"
    assert order[2:5] == f[2:5], "7, -7 and 7 are not one key, in index order"
    off = [v for v in np.flatnonzero(truth["smoother_enable"] == 0) if v in set(order)]
    assert off and sorted(order[-len(off) - 1:]) == sorted(off + [f[5]]), "unsmoothed voices and |-2^31| do not share the last key"
    return [(q_all(n, policy=QUIETEST, max_out=STEAL_MAX), False), (q_all(n, policy=QUIETEST, max_out=1), True),
            (q_all(n, policy=QUIETEST, max_out=3), True), (q_all(n, policy=QUIETEST, max_out=4), True),
            (q_all(n, policy=QUIETEST, flags=RELEASED_ONLY, max_out=8), False)]


def queries_wide(n, truth, now, role, special):
    order = sm.victim_order(truth, now, q_all(n)).tolist()
    v, _, key = sm.keys(truth, now, q_all(n))
    out = []
    for (a, c), bit in zip(special["pairs"], DIGIT_BITS):
        diff = int(key[a]) ^ int(key[c])
        assert diff == 1 << bit, "the pair's keys differ in more than one digit"
        lo, hi = (a, c) if key[a] < key[c] else (c, a)
        assert order.index(lo) < order.index(hi)
        if 0 < order.index(hi) <= STEAL_MAX:
            out.append((q_all(n, max_out=order.index(hi)), False))       # the list ends between the two
    assert len(out) >= 4
    assert order[-2:] == sorted(special["saturated"]), "the two saturated keys tie and go by index"
    rel = sm.victim_order(truth, now, q_all(n, flags=RELEASED_ONLY))
    assert (truth["sample_release"][rel] > np.uint64(1 << 32)).all()
    return out + [(q_all(n, max_out=STEAL_MAX), False), (q_all(n, flags=RELEASED_FIRST, max_out=STEAL_MAX), False),
                  (q_all(n, flags=RELEASED_FIRST, max_out=7), False)]


def queries_ties(n, truth, now, role, special):
    total = len(sm.victim_order(truth, now, q_all(n)))
    assert total > 20000, total
    return [(q_all(n, max_out=STEAL_MAX), True), (q_all(n, max_out=1), True),
            (q_all(n, flags=RELEASED_FIRST, max_out=STEAL_MAX), True),
            (Query(11, n - 30, flags=RELEASED_FIRST, max_out=STEAL_MAX), True),
            (Query(11, 300, flags=RELEASED_FIRST, max_out=STEAL_MAX), False)]


def queries_counts(n, truth, now, role, special):
    """total below, at and above max_out; zero candidates with max_out > 0"""
    rel = len(sm.victim_order(truth, now, q_all(n, flags=RELEASED_ONLY)))
    assert 0 < rel < STEAL_MAX
    none = q_all(n, min_age=1 << 40, max_out=8)
    assert len(sm.victim_order(truth, now, none)) == 0
    return [(q_all(n, max_out=0), False), (q_all(n, flags=RELEASED_ONLY, max_out=STEAL_MAX), False),
            (q_all(n, flags=RELEASED_ONLY, max_out=rel), False), (q_all(n, flags=RELEASED_ONLY, max_out=rel - 1), False),
            (q_all(n, max_out=STEAL_MAX), False), (none, None)]


def queries_finished(n, truth, now, role, special):
    """one-shots that finished while active and voices with amp_q15 == 0: candidates, unless the exclusion names them"""
    fin = int(np.flatnonzero((truth["finished"] != 0) & (truth["is_active"] != 0))[0])
    amp = int(np.flatnonzero((truth["amp_q15"] == 0) & (truth["is_active"] != 0) & (truth["use_envelope"] != 0))[0])
    everyone = sm.victim_order(truth, now, q_all(n))
    assert fin in everyone and amp in everyone
    assert fin not in sm.victim_order(truth, now, q_all(n, exclude_idle=FIN)) and amp in sm.victim_order(truth, now, q_all(n, exclude_idle=FIN))
    assert amp not in sm.victim_order(truth, now, q_all(n, exclude_idle=AMP))
    return [(q_all(n, exclude_idle=FIN, max_out=STEAL_MAX), False), (q_all(n, exclude_idle=FIN | AMP, max_out=STEAL_MAX), False),
            (q_all(n, exclude_idle=FIN | AMP, max_out=16), False)]


SCENES = {
    "n1": (1, "plain", queries_sizes), "n63": (63, "plain", queries_sizes), "n64": (64, "plain", queries_sizes),
    "n65": (65, "plain", queries_sizes), "n255": (255, "plain", queries_sizes), "n256": (256, "plain", queries_sizes),
    "n257": (257, "plain", queries_sizes), "n1000": (1000, "plain", queries_sizes), "n70000": (70000, "plain", queries_sizes),
    "min_age_and_ahead": (1000, "ahead", queries_min_age),
    "quietest": (1000, "quiet", queries_quiet),
    "key_digits": (1000, "wide", queries_wide),
    "ties_70000": (70000, "ties", queries_ties),
    "counts": (4096, "plain", queries_counts),
    "finished_and_silent": (1000, "plain", queries_finished),
}


def scene_queries(name):
    n, variant, make = SCENES[name]
    b, pool, c0, truth, now, role, special = scene(n, variant)
    return make(n, truth, now, role, special)
