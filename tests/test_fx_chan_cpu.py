"""Channel polyphony on the fixed-point bank without a GPU: the symbols against the header, the model (tests/fx_chan_model.py) against
a brute-force loop over every voice, the a / b rule against a loop, every refusal and the packing of the burst's queries (through
tests/c_fx_chan_host.c, a program of its own on a bank that is nothing but its size), and the scenes of tests/test_fx_chan.py on the
oracle's state alone: none of them is vacuous, and the burst script shows every kind of outcome.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import fx_chan_model as CM
import fx_chan_scenes as CS
import fx_steal_model as sm
import fx_steal_scenes as sc
from fx_steal_model import AMP, ENV, FIN, OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, STEAL_MAX, Query
from skred_amd import device, fxbank as fxb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd_fxpt.h")).read()
    L = fxb._bind(device.load())
    for s in ("skred_fx_chan_check", "skred_fxbank_find_steal_match", "skred_fxbank_find_steal_match_host", "skred_fxbank_note_on_channel"):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in fxb.FX_ABI_SYMBOLS + fxb.FX_HOST_ABI_SYMBOLS
    assert "skred_fx_chan_check" in fxb.FX_HOST_ABI_SYMBOLS
    assert fxb.CHAN_NO_CAP == CM.NO_CAP == 0xFFFFFFFF
    for hdr in ("include/skred_amd.h", "skred_amd/csrc/skred_bank_slots.c", "DESIGN.md"):       # the twin is no longer out of scope
        assert "a twin on the fixed-point bank" not in open(os.path.join(ROOT, hdr)).read(), hdr


# ---------------------------------------------------------------------------------------------- the model

def random_bank(rng, n):
    b, _, c0 = fxb.bank_fx(n, with_filter=False)
    now = c0 + 1000
    b["sample_start"] = rng.choice(np.array([now - 7, now - 7, now - 500, now + 3, 5, (1 << 62) + 1, (1 << 63) + 5, (3 << 32) + 5, now], np.uint64), n)
    b["sample_release"] = rng.choice(np.array([0, 0, now - 3, now - 3, 9, 1 << 40], np.uint64), n)
    b["is_active"] = (rng.integers(0, 4, n) != 0) * rng.integers(1, 9, n)
    b["use_envelope"] = rng.integers(0, 5, n) != 0
    b["smoother_enable"] = rng.integers(0, 4, n) != 0
    b["smoother_gain_q15"] = rng.choice(np.array([0, 0, 1, -1, 3, 4, -4, 20000, -(1 << 31), (1 << 31) - 1], np.int64), n).astype(np.int32)
    b["finished"] = rng.integers(0, 3, n) == 0
    b["amp_q15"] = rng.choice(np.array([0, 32768, 1, 65535], np.int32), n)
    return b, now


def brute_force(bank, now, q, own, match):
    """Voice by voice with Python integers and sorted(): (victim order, sounding count)."""
    value, mask = match
    rows, sounding = [], 0
    for v in range(q.first, q.first + q.count):
        o = int(own[v])
        if o == 0 or (o & mask) != value:
            continue
        active, smooth = int(bank["is_active"][v]) != 0, int(bank["smoother_enable"][v]) != 0
        if int(bank["use_envelope"][v]) == 0 or not active:
            continue
        gain = abs(int(bank["smoother_gain_q15"][v]))
        idle = False
        if q.exclude_idle & FIN:
            idle |= int(bank["finished"][v]) != 0
        if q.exclude_idle & ENV:
            idle |= (not active) and (not smooth or gain <= q.settle_q15)
        if q.exclude_idle & AMP:
            idle |= int(bank["amp_q15"][v]) == 0
        if idle:
            continue
        sounding += 1
        start, release = int(bank["sample_start"][v]), int(bank["sample_release"][v])
        released = release != 0
        if (0 if start > now else now - start) < q.min_age:
            continue
        if (q.flags & RELEASED_ONLY) and not released:
            continue
        cls = 0 if (q.flags & RELEASED_FIRST) and released else 1
        primary = (release if cls == 0 else start) if q.policy == OLDEST else (min(gain, sm.NO_GAIN) if smooth else sm.NO_GAIN)
        rows.append(((cls << 62) | min(primary, sm.CAP), v))
    return np.array([v for _, v in sorted(rows)], np.int32), sounding


def test_model_against_brute_force():
    rng = np.random.default_rng(5300)
    n = 300
    lists = counted = 0
    for trial in range(16):
        bank, now = random_bank(rng, n)
        own = rng.choice(np.array([0, CS.tag_of(CS.A, 1), CS.tag_of(CS.A, 2), CS.tag_of(CS.B, 1), 0xFFFFFFFF, 0x00FFFFFF], np.uint32), n)
        first = int(rng.integers(0, n - 1)) if trial % 3 else 0
        count = int(rng.integers(1, n - first + 1)) if trial % 3 else n
        for match in ((0, 0), CM.channel(CS.A), CM.channel(0), (0xFFFFFFFF, 0xFFFFFFFF), (CS.tag_of(CS.A, 2), 0xFFFFFFFF)):   # mask 0, a channel byte, all 32 bits
            for policy in (OLDEST, QUIETEST):
                for flags in (0, RELEASED_FIRST, RELEASED_ONLY, RELEASED_FIRST | RELEASED_ONLY):
                    q = Query(first, count, policy, flags, int(rng.choice([0, 0, 7, 8, 500])),
                              int(rng.choice([0, FIN, ENV, ENV, FIN | ENV | AMP])), int(rng.choice([0, 0, 3])), STEAL_MAX)
                    want, snd = brute_force(bank, now, q, own, match)
                    got, got_snd = CM.victim_order(bank, now, q, own, match)
                    assert np.array_equal(want, got) and snd == got_snd, (q, match, want, got, snd, got_snd)
                    lists += len(want) > 1
                    counted += snd > len(want)
    assert lists > 40 and counted > 40, (lists, counted)


def test_the_split_rule_against_a_loop():
    caps = (0, 1, 2, 3, 5, 9, CM.NO_CAP)
    seen = set()
    for n in range(0, 5):
        for idle in range(0, 6):
            for snd in range(0, 6):
                for vic in range(0, 5):
                    for cap in caps:
                        a = b = 0
                        room = cap - snd if cap > snd else 0
                        for _ in range(n):                                       # note by note: an idle voice while the cap has room, else a victim
                            if a < idle and a < room:
                                a += 1
                            elif b < vic:
                                b += 1
                        assert CM.split(n, idle, snd, vic, cap) == (a, b), (n, idle, snd, vic, cap)
                        seen.add((cap == 0, cap < snd, cap == CM.NO_CAP, a > 0, b > 0, a + b < n))
    assert len(seen) > 20
    assert CM.split(3, 9, 0, 3, 0) == (0, 3) and CM.split(4, 9, 7, 4, 5) == (0, 4) and CM.split(4, 1, 0, 1, CM.NO_CAP) == (1, 1)


def test_mask_zero_with_everything_tagged_is_the_steal_model():
    b, pool, c0, truth, now, own = CS.query_scene()
    tagged = np.full(truth.n, 5, np.uint32)
    for q in CS.queries():
        got, counts = CM.query(truth, now, q, tagged, (0, 0))
        want, total = sm.victims(truth, now, q)
        assert got.tobytes() == want.tobytes() and counts[:2] == [len(want), total] and counts[2] >= total
    lst, counts = CM.query(truth, now, CS.queries()[0], np.zeros(truth.n, np.uint32), (0, 0))     # nobody tagged: nothing sounds, nothing is stolen
    assert len(lst) == 0 and counts == [0, 0, 0]


# ---------------------------------------------------------------------------------------------- the entry points' host checks

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fxchan") / "c_fx_chan_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_fx_chan_host.c"), os.path.join(CSRC, "skred_fx_steal.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"),
           "-lskred_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-lm", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "skred_amd"),
           "-Wl,-rpath," + os.path.join(rocm, "lib")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return out.stdout.strip().splitlines()


def test_host_program(host_lines):
    bad = [l for l in host_lines[:-1] if not l.endswith(" ok")]
    assert not bad, bad
    assert host_lines[-1] == "OK" and len(host_lines) == 79
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "check", "pack", "find", "find_host", "on", "untouched"}, groups


def test_check_through_ctypes():
    iq = fxb.FxIdleQueryC(0, 1024, FIN | ENV, 3, 0, 0)
    sq = fxb.fx_steal_query(0, 1024)
    m = device.owner_match(*CM.channel(3))
    tags = [CS.tag_of(3, 1), CS.tag_of(3, 2)]
    assert fxb.fx_chan_check(iq, sq, m, 4, tags, 1024) == 0
    assert fxb.fx_chan_check(iq, sq, m, 4, [CS.tag_of(4, 1)], 1024) == BAD and b"does not satisfy" in device.load().skred_amd_last_error()
    assert fxb.fx_chan_check(iq, sq, m, 4, [0], 1024) == BAD
    assert fxb.fx_chan_check(None, sq, m, 4, tags, 1024) == BAD and fxb.fx_chan_check(iq, None, m, 4, tags, 1024) == BAD
    assert fxb.fx_chan_check(iq, sq, None, 4, tags, 1024) == BAD and fxb.fx_chan_check(iq, sq, m, 4, None, 1024) == BAD
    assert fxb.fx_chan_check(iq, sq, m, 4, tags, 1000) == RANGE
    assert fxb.fx_chan_check(fxb.FxIdleQueryC(0, 1024, FIN | ENV | AMP, 3, 0, 0), sq, m, 4, tags, 1024) == BAD
    for cap in (0, 1, CM.NO_CAP):
        assert fxb.fx_chan_check(iq, sq, m, cap, tags, 1024) == 0


# ---------------------------------------------------------------------------------------------- the scenes of the GPU tests

def test_query_scene_is_not_vacuous():
    b, pool, c0, truth, now, own = CS.query_scene()
    n = truth.n
    q = Query(0, n, max_out=STEAL_MAX, exclude_idle=CS.WHICH, settle_q15=CS.SETTLE)
    everybody, snd_all = CM.victim_order(truth, now, q, own, (0, 0))
    plain = sm.victim_order(truth, now, q)
    a, snd_a = CM.victim_order(truth, now, q, own, CM.channel(CS.A))
    c, snd_b = CM.victim_order(truth, now, q, own, CM.channel(CS.B))
    assert len(a) > 100 and len(c) > 100 and snd_a == len(a) and snd_b == len(c)
    assert not set(a.tolist()) & set(c.tolist()) and len(everybody) > len(a) + len(c) and len(plain) > len(everybody), "untagged sounding voices exist beside tagged ones"
    assert [v for v in everybody.tolist() if v in set(a.tolist())] == a.tolist(), "a channel's victims keep the victim order"
    for m, snd in ((CM.channel(CS.A), snd_a), (CM.channel(CS.B), snd_b)):
        for guarded in (q.but(min_age=CS.MIN_AGE), q.but(flags=RELEASED_ONLY)):
            lst, counts = CM.query(truth, now, guarded, own, m)
            assert 0 < counts[1] < counts[2] == snd, "no sounding voice of the channel is protected: the two counts cannot differ"
    part = Query(70, 1300, max_out=STEAL_MAX)
    assert 0 < CM.query(truth, now, part, own, CM.channel(CS.A))[1][2] < CM.query(truth, now, q.but(exclude_idle=0), own, CM.channel(CS.A))[1][2]
    ms = CS.matches(own, truth)
    assert CM.query(truth, now, q, own, ms[3])[1] == [1, 1, 1], "the one note is sounding and alone"
    assert CM.query(truth, now, q, own, ms[5])[1] == [0, 0, 0] and CM.query(truth, now, q, own, ms[6])[1] == [0, 0, 0]
    assert CM.query(truth, now, q, own, ms[4])[1][2] > 0
    # the ENV_DONE exclusion at settle_q15 = 0 takes voices away from the sounding count of no channel (an ENV_DONE voice is not
    # active), FIN does: the count words differ between the exclusions
    assert CM.query(truth, now, q.but(exclude_idle=FIN), own, ms[0])[1][2] < CM.query(truth, now, q.but(exclude_idle=ENV, settle_q15=0), own, ms[0])[1][2]
    seen = set()
    for qq in CS.queries():
        for m in ms:
            lst, counts = CM.query(truth, now, qq, own, m)
            seen.add((counts[0] < counts[1], counts[1] < counts[2], counts[2] == 0, counts[0] == 0))
    assert len(seen) >= 5, seen


def test_ties_scene_is_not_vacuous():
    b, pool, c0, truth, now, role, special = sc.scene(CS.N_TIES, "ties")
    own = CS.ties_owners()
    for q in CS.ties_queries()[:4]:
        for ch in (CS.A, CS.B):
            order, snd = CM.victim_order(truth, now, q, own, CM.channel(ch))
            v, _, _, key = CM.terms(truth, now, q, own, CM.channel(ch))
            key_of = dict(zip(v.tolist(), key.tolist()))
            at = key_of[int(order[q.max_out - 1])]
            tied = [int(x) for x in order if key_of[int(x)] == at]
            assert len(tied) > STEAL_MAX and key_of[int(order[q.max_out])] == at, "no tie of more than SKRED_STEAL_MAX keys straddles max_out"
            lo, hi = min(tied), max(tied)
            other = own[lo:hi] >> np.uint32(24) != ch
            assert other.any() and (np.diff(np.array(tied)) > 1).any(), "the other channel's voices lie between the tied ones"
            everyone = sm.victim_order(truth, now, q)
            assert len(everyone) > len(order) and set(order.tolist()) < set(everyone.tolist())


def test_burst_script_shows_every_kind():
    """On the oracle alone: the seven kinds, each at least once; the assertions of the script itself (victims from the channel only,
    the other channel's owners and clocks unchanged, no growth above a cap, mono mode) run on the way."""
    seen, log = CS.run_burst_script(None)
    assert seen >= CS.KINDS, (seen, log)
    by_name = {row[0]: row for row in log}
    assert by_name["other channel under, no cap"][4][2] == 0 and by_name["dropped, no cap"][4][1] == 2 and by_name["dropped"][4][1] == 2
    assert by_name["dropped, no cap"][3] > 0 and by_name["dropped, no cap"][4][2] > 0, "the uncapped burst used idle voices AND victims before it dropped"
    assert by_name["above"][4][3] > by_name["above"][2] and by_name["above"][4][2] == by_name["above"][1], "above a lowered cap every note steals"
