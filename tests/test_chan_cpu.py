"""Channel polyphony without a GPU: the symbols against the header, the model (tests/chan_model.py) against a brute-force loop over
slots, every refusal and the packing of the burst's queries (through tests/c_chan_host.c, a program of its own on a bank that is
nothing but its size), and the scenes of tests/test_chan.py on the oracle's state alone: none of them is vacuous, and the burst
script shows every kind the GPU test asserts.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import chan_model as CM
import chan_scenes as CS
import slot_model as SM
import slot_steal_model as M
import slot_steal_scenes as S
import steal_model as sm
from oracle import cpuref
from skred_amd import banks, device
from steal_model import OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, FIN, ENV, AMP

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    L = device.load()
    for s in ("skred_chan_check", "skred_bank_find_steal_slots_match", "skred_bank_find_steal_slots_match_host", "skred_bank_note_on_channel"):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in device.ABI_SYMBOLS + device.HOST_ABI_SYMBOLS
    assert re.search(r"#define SKRED_CHAN_NO_CAP 0xFFFFFFFFu", text) and device.CHAN_NO_CAP == CM.NO_CAP == 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- the model

def random_bank(rng, n):
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
    return bank, now


def brute_force(host, now, q, own, match):
    """Slot by slot and voice by voice with Python integers and sorted(): (victim order, sounding count)."""
    a = host.a
    e = a["voice_amp_envelope"]
    value, mask = match
    rows, sounding = [], 0
    for h in range(q.first, q.first + q.count, q.K):
        o = int(own[h])
        if o == 0 or (o & mask) != value:
            continue
        members = [h + l for l in M.lanes(q.mask, q.K)]
        live = [v for v in members if a["voice_use_amp_envelope"][v] != 0 and e["is_active"][v] != 0]
        if not live:
            continue
        if q.exclude_idle and sm.idle_pred(host, np.array(members), q.exclude_idle, q.settle_level).all():
            continue
        sounding += 1
        ages = [0 if int(e["sample_start"][v]) > now else now - int(e["sample_start"][v]) for v in live]
        if min(ages) < q.min_age:
            continue
        all_released = all(int(e["sample_release"][v]) != 0 for v in live)
        if (q.flags & RELEASED_ONLY) and not all_released:
            continue
        cls = 0 if (q.flags & RELEASED_FIRST) and all_released else 1
        if q.policy == OLDEST:
            primary = max(int(e["sample_release"][v]) if cls == 0 else int(e["sample_start"][v]) for v in live)
        else:
            primary = max(int(np.abs(np.float32(a["voice_smoother_gain"][v])).view(np.uint32)) if a["voice_smoother_enable"][v] != 0
                          else 0x7fffffff for v in live)
        rows.append(((cls << 62) | min(primary, M.CAP), h))
    return np.array([h for _, h in sorted(rows)], np.int32), sounding


@pytest.mark.parametrize("K", [1, 2, 8, 64])
def test_model_against_brute_force(K):
    rng = np.random.default_rng(5200 + K)
    n = max(256, 16 * K)                                                         # at least sixteen slots
    lists = counted = 0
    for trial in range(24):
        bank, now = random_bank(rng, n)
        own = rng.choice(np.array([0, CS.tag_of(CS.A, 1), CS.tag_of(CS.A, 2), CS.tag_of(CS.B, 1), 0xFFFFFFFF, 0x00FFFFFF], np.uint32), n)
        slots = n // K
        first = int(rng.integers(0, slots)) * K if trial % 3 else 0
        count = int(rng.integers(1, slots - first // K + 1)) * K if trial % 3 else n
        mask = (1 << K) - 1 if trial % 2 or K == 1 else int(rng.integers(1, 1 << min(K, 62)))
        for match in ((0, 0), CM.channel(CS.A), CM.channel(0), (0xFFFFFFFF, 0xFFFFFFFF), (CS.tag_of(CS.A, 2), 0xFFFFFFFF)):   # mask 0, one channel byte, all 32 bits
            for policy in (OLDEST, QUIETEST):
                for flags in (0, RELEASED_FIRST, RELEASED_ONLY, RELEASED_FIRST | RELEASED_ONLY):
                    q = M.SlotQuery(first, count, K, mask, policy, flags, int(rng.choice([0, 0, 7, 8, 500])),
                                    int(rng.choice([0, FIN, ENV, FIN | ENV | AMP])), float(rng.choice([0.0, 1e-3])))
                    want, snd = brute_force(bank, now, q, own, match)
                    got, got_snd = CM.victim_slots(bank, now, q, own, match)
                    assert np.array_equal(want, got) and snd == got_snd, (q, match, want, got, snd, got_snd)
                    lists += len(want) > 1
                    counted += snd > len(want)
    assert lists > 40 and counted > 40, (lists, counted)


def test_mask_zero_with_everything_tagged_is_the_slot_model():
    n, K, mask = 1088, 8, 0x55
    bank, tables, g, truth, now, kind = S.scene(n, K, mask)
    own = np.full(n, 5, np.uint32)
    for q in S.queries(n, K, mask):
        got, snd = CM.victim_slots(truth, now, q, own, (0, 0))
        assert np.array_equal(got, M.victim_slots(truth, now, q))
        assert snd >= len(got)
    own[::K] = 0                                                                 # nobody tagged: nothing sounds, nothing is stolen
    lst, counts = CM.query(truth, now, S.queries(n, K, mask)[0], own, (0, 0))
    assert len(lst) == 0 and counts == [0, 0, 0]


def test_the_split_rule():
    # (n, idle, sounding, victims, cap) -> (a, b)
    for args, want in (((4, 9, 3, 4, 10), (4, 0)), ((4, 9, 3, 4, 5), (2, 2)), ((4, 9, 5, 4, 5), (0, 4)), ((4, 9, 7, 4, 5), (0, 4)),
                       ((4, 1, 0, 1, CM.NO_CAP), (1, 1)), ((4, 0, 0, 0, CM.NO_CAP), (0, 0)), ((1, 5, 1, 1, 1), (0, 1)), ((1, 5, 0, 0, 1), (1, 0)),
                       ((3, 9, 0, 3, 0), (0, 3)), ((6, 2, 1, 3, 2), (1, 3))):
        assert CM.split(*args) == want, (args, CM.split(*args), want)


# ---------------------------------------------------------------------------------------------- the entry points' host checks

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chan") / "c_chan_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_chan_host.c"), os.path.join(CSRC, "skred_bank_slots.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"),
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
    assert host_lines[-1] == "OK" and len(host_lines) == 81
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "check", "pack", "find", "find_host", "on", "untouched"}, groups


def test_check_through_ctypes():
    from skred_amd.bank import slot_query, slot_steal_query
    iq = slot_query(0, 1024, 8, 0x55, FIN | ENV, 1e-3, 0, 0)
    sq = slot_steal_query(0, 1024, 8, 0x55)
    m = device.owner_match(*CM.channel(3))
    tags = [CS.tag_of(3, 1), CS.tag_of(3, 2)]
    assert device.chan_check(iq, sq, m, 4, tags, 1024) == 0
    assert device.chan_check(iq, sq, m, 4, [CS.tag_of(4, 1)], 1024) == BAD and b"does not satisfy" in device.load().skred_amd_last_error()
    assert device.chan_check(iq, sq, m, 4, [0], 1024) == BAD
    assert device.chan_check(None, sq, m, 4, tags, 1024) == BAD and device.chan_check(iq, None, m, 4, tags, 1024) == BAD
    assert device.chan_check(iq, sq, None, 4, tags, 1024) == BAD and device.chan_check(iq, sq, m, 4, None, 1024) == BAD
    assert device.chan_check(iq, sq, m, 4, tags, 1000) == RANGE
    assert device.chan_check(slot_query(0, 1024, 8, 0x55, FIN | ENV | AMP, 1e-3, 0, 0), sq, m, 4, tags, 1024) == BAD


# ---------------------------------------------------------------------------------------------- the scenes of the GPU tests

@pytest.mark.parametrize("K", [1, 2, 8, 64])
def test_query_scenes_are_not_vacuous(K):
    n = 1500
    mask = (1 << K) - 1
    count = n - n % K
    bank, tables, g, truth, now, kind = S.scene(n, K, mask)
    own = CS.owners(n, K)
    q = M.SlotQuery(0, count, K, mask, max_out=M.STEAL_MAX, exclude_idle=S.EXCLUDE, settle_level=float(S.SETTLE))
    everybody, _ = CM.victim_slots(truth, now, q, own, (0, 0))
    plain = M.victim_slots(truth, now, q)
    a, snd_a = CM.victim_slots(truth, now, q, own, CM.channel(CS.A))
    b, snd_b = CM.victim_slots(truth, now, q, own, CM.channel(CS.B))
    few = 3 if K == 64 else 8                                                    # (1 500 voices are 23 slots of 64)
    assert len(a) > few and len(b) > few and snd_a == len(a) and snd_b == len(b)
    guarded = q.but(min_age=S.MIN_AGE, flags=RELEASED_ONLY)
    for m, snd in ((CM.channel(CS.A), snd_a), (CM.channel(CS.B), snd_b)):
        lst, counts = CM.query(truth, now, guarded, own, m)
        assert 0 < counts[1] < counts[2] == snd, "no sounding slot of a channel is protected: the two counts cannot differ"
    assert not set(a.tolist()) & set(b.tolist()) and len(everybody) > len(a) + len(b) and len(plain) > len(everybody), "untagged candidates exist"
    merged = [h for h in everybody.tolist() if h in set(a.tolist())]
    assert merged == a.tolist(), "a channel's victims keep the victim order"
    ms = CS.matches(own, K)
    assert CM.query(truth, now, q, own, ms[3])[1][1] <= 1 and CM.query(truth, now, q, own, ms[5])[1] == [0, 0, 0] and CM.query(truth, now, q, own, ms[6])[1] == [0, 0, 0]
    # a kernel that read the owner word of a member (junk: channel A) instead of the first voice's would see more of channel A
    if K > 1:
        wrong = own.copy()
        wrong[::K] = own[1::K][:len(own[::K])]
        assert len(CM.victim_slots(truth, now, q, wrong, CM.channel(CS.A))[0]) > len(a)


def test_burst_script_shows_every_kind():
    """On the oracle alone: the six kinds, each at least once, for both patches of tests/test_chan.py."""
    for patch, members, voices in (("3sk", (0, 1, 2), (0, 1, 2, 3)), ("18sk", (0, 10), (0, 1, 2, 10))):
        seen, log = run_burst_script(patch, members, voices, None)
        assert seen >= CS.KINDS, (patch, seen, log)


def run_burst_script(patch, members, voices, on_burst):
    """The bursts of chan_scenes.BURSTS on the oracle; on_burst(step, state, args, want, now) runs the device's side: step -1 before the
    first burst, then per burst once with its arguments and the model's (d_assigned, d_result), and once per block ("block", the
    oracle's render) behind it."""
    from test_slots import slot_notes
    bank, tables, g, K, own = CS.burst_bank(patch, members)
    mmask, vmask = sum(1 << l for l in members), sum(1 << l for l in voices)
    truth, gl = bank.copy(), g.copy()
    for _ in range(4):
        cpuref.render(truth, gl, tables, CS.F, 0)
    seen, log = set(), []
    state = dict(bank=bank, tables=tables, g=g, K=K, own=own, truth=truth, gl=gl, mmask=mmask, vmask=vmask)
    if on_burst:
        on_burst(-1, state, None, None, None)
    for step in range(len(CS.BURSTS)):
        now = int(gl.synth_sample_count)
        iq, sq, match, cap, n, tags = CS.burst_args(step, truth, now, own, K, mmask, bank.n)
        want, res, n_idle = CM.burst(truth, now, own, iq, sq, match, cap, n)
        kind = CM.kind(n, n_idle, res, cap)
        seen.add(kind)
        log.append((CS.BURSTS[step][0], n, cap, n_idle, res, kind))
        before = own.copy()
        heads, snd_all, _, _ = CM.terms(truth, now, M.SlotQuery(0, bank.n, K, mmask, exclude_idle=iq.which, settle_level=float(iq.settle_level)), before, (0, 0))
        other = heads[snd_all & ~CM.matches(before[heads], match)]                # the sounding slots of the other channels
        notes = slot_notes(n, K, vmask, step, [SM.SET_PHASE, SM.SET_PHASE | SM.SET_PAN])
        if on_burst:
            on_burst(step, state, (iq, sq, match, cap, n, tags, notes), (want, res), now)
        SM.store_notes((truth,), truth, notes, K, vmask, want, now)
        CM.tag(own, want, tags, K)
        # victims come from the channel only (the others keep their tags), and the channel never exceeds a cap it was under
        stolen = want[res[0] - res[2]:res[0]]
        assert CM.matches(before[stolen], match).all() and (own[other] == before[other]).all()
        after = CM.victim_slots(truth, now, sq.but(exclude_idle=iq.which, settle_level=float(iq.settle_level), min_age=0, flags=0), own, match)[1]
        if CS.BURSTS[step][5] is None:                                           # (the steal range is the whole bank: S is the channel's count)
            assert after <= max(cap, res[3]), (step, after, cap, res)
        for _ in range(2):
            ref = cpuref.render(truth, gl, tables, CS.F, 0, want_stems=on_burst is not None)
            if on_burst:
                on_burst(step, state, "block", ref, None)
    return seen, log
