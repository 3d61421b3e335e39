"""Pedals without a GPU: the symbols against the header, the model (tests/pedal_model.py) against a brute-force loop over every slot,
every refusal and the flag packing (through tests/c_pedal_host.c, a program of its own on a bank that is nothing but its size), and the
scenes (a) .. (f) of tests/test_pedal.py on the oracle alone -- envelope clocks and rendered state through oracle.cpuref with
slot_model's stamps.  Scene (b) must FAIL on a model without the clear behind the tag launch: that is what shows it bites.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import chan_model as CM
import owner_scenes as OS
import pedal_model as PM
import slot_model as SM
from skred_amd import banks, device

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
SYMBOLS = ("skred_bank_stamp_owned_pedal", "skred_bank_release_tags_pedal", "skred_bank_pedal_latch", "skred_bank_pedal_up",
           "skred_bank_pedal_clear", "skred_bank_download_pedals")


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    L = device.load()
    for s in SYMBOLS + ("skred_pedal_check",):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in device.ABI_SYMBOLS + device.HOST_ABI_SYMBOLS
    for name, value in (("PENDING", 0), ("LATCHED", 1), ("LIFT_SUSTAIN", 0), ("LIFT_SOSTENUTO", 1), ("SUSTAIN_DOWN", 2)):
        assert re.search(r"SKRED_PEDAL_%s = 1u << %d\b" % (name, value), text), name
        assert getattr(device, "PEDAL_" + name) == getattr(PM, name) == 1 << value
    calls = re.search(r"enum \{ (SKRED_PEDAL_CALL_STAMP_OWNED = 0, SKRED_PEDAL_CALL_RELEASE_TAGS, SKRED_PEDAL_CALL_LATCH, SKRED_PEDAL_CALL_UP) \}", text)
    assert calls and (device.PEDAL_CALL_STAMP_OWNED, device.PEDAL_CALL_RELEASE_TAGS, device.PEDAL_CALL_LATCH, device.PEDAL_CALL_UP) == (0, 1, 2, 3)


# ---------------------------------------------------------------------------------------------- the model

def random_state(rng, n, K):
    bank, _, g = banks.bank_c2(n)
    e = bank["voice_amp_envelope"]
    now = int(g.synth_sample_count)
    e["sample_release"][:] = rng.choice([0, 0, 0, now - 3, 9, 1 << 40], n).astype(np.uint64)
    e["is_active"][:] = rng.integers(0, 4, n) != 0
    bank["voice_use_amp_envelope"][:] = rng.integers(0, 5, n) != 0
    owner = rng.choice(np.array([0, PM.tag_of(3, 1), PM.tag_of(3, 2), PM.tag_of(5, 1), 0xFFFFFFFF, 0x00FFFFFF], np.uint32), n)
    pedal = rng.choice(np.array([0, 0, PM.PENDING, PM.LATCHED, PM.PENDING | PM.LATCHED], np.uint32), n)
    return bank, now, owner, pedal


def brute_latch(owner, pedal, bank, first, count, K, vmask, match):
    e = bank["voice_amp_envelope"]
    value, mask = match
    res = [0, 0]
    for h in range(first, first + count, K):
        o = int(owner[h])
        if o == 0 or (o & mask) != value:
            res[1] += 1
            continue
        some = any(bank["voice_use_amp_envelope"][h + l] != 0 and e["is_active"][h + l] != 0 and int(e["sample_release"][h + l]) == 0
                   for l in range(K) if (vmask >> l) & 1)
        if some and not int(pedal[h]) & PM.PENDING:
            pedal[h] = int(pedal[h]) | PM.LATCHED
            res[0] += 1
    return res


def brute_up(owner, pedal, bank, first, count, K, vmask, match, flags, now):
    e = bank["voice_amp_envelope"]
    value, mask = match
    res = [0, 0, 0]
    for h in range(first, first + count, K):
        o = int(owner[h])
        if o == 0 or (o & mask) != value:
            res[2] += 1
            continue
        w = int(pedal[h])
        if flags & PM.LIFT_SOSTENUTO:
            w &= ~PM.LATCHED
        if (w & PM.PENDING) and not (w & PM.LATCHED) and not (flags & PM.SUSTAIN_DOWN):
            w &= ~PM.PENDING
            res[0] += 1
            for l in range(K):
                if (vmask >> l) & 1 and e["is_active"][h + l] != 0:
                    e["sample_release"][h + l] = now
        res[1] += bool(w & PM.PENDING)
        pedal[h] = w
    return res


def brute_off(owner, pedal, bank, entries, tags, count, K, vmask, hold_all, now):
    e = bank["voice_amp_envelope"]
    res = [0, 0, 0, 0]
    m = len(tags) if count is None else min(len(tags), count)
    for k in range(m):
        h = int(entries[k])
        if h < 0 or h % K or h + K > len(owner):
            res[2] += 1
        elif int(owner[h]) != int(tags[k]):
            res[1] += 1
        elif hold_all or int(pedal[h]) & PM.LATCHED:
            pedal[h] = int(pedal[h]) | PM.PENDING
            res[3] += 1
        else:
            res[0] += 1
            for l in range(K):
                if (vmask >> l) & 1 and e["is_active"][h + l] != 0:
                    e["sample_release"][h + l] = now
    return res


def same_state(a, b, pa, pb):
    ea, eb = a["voice_amp_envelope"], b["voice_amp_envelope"]
    return np.array_equal(pa, pb) and np.array_equal(ea["sample_release"], eb["sample_release"]) and np.array_equal(ea["is_active"], eb["is_active"])


@pytest.mark.parametrize("K", [1, 2, 8, 64])
def test_model_against_brute_force(K):
    rng = np.random.default_rng(6400 + K)
    n = max(256, 16 * K)
    slots = n // K
    seen = dict(latched=0, released=0, kept=0, held=0, stamped=0)
    for trial in range(20):
        bank, now, owner, pedal = random_state(rng, n, K)
        first = int(rng.integers(0, slots)) * K if trial % 3 else 0
        count = int(rng.integers(1, slots - first // K + 1)) * K if trial % 3 else n
        vmask = (1 << K) - 1 if trial % 2 or K == 1 else int(rng.integers(1, 1 << min(K, 62)))
        for match in ((0, 0), CM.channel(3), (PM.tag_of(3, 2), 0xFFFFFFFF)):
            a, b, pa, pb = bank.copy(), bank.copy(), pedal.copy(), pedal.copy()
            got, want = PM.latch(owner, pa, a, first, count, K, vmask, match), brute_latch(owner, pb, b, first, count, K, vmask, match)
            assert got == want and same_state(a, b, pa, pb), (K, trial, match, got, want)
            seen["latched"] += got[0]
            for flags in (PM.LIFT_SUSTAIN, PM.LIFT_SOSTENUTO, PM.LIFT_SUSTAIN | PM.LIFT_SOSTENUTO, PM.LIFT_SOSTENUTO | PM.SUSTAIN_DOWN):
                a, b, qa, qb = bank.copy(), bank.copy(), pa.copy(), pa.copy()
                got = PM.up(owner, qa, a, first, count, K, vmask, match, flags, now)[0]
                want = brute_up(owner, qb, b, first, count, K, vmask, match, flags, now)
                assert got == want and same_state(a, b, qa, qb), (K, trial, match, flags, got, want)
                seen["released"] += got[0]
                seen["kept"] += got[1]
        heads = np.arange(0, n, K)
        entries = np.concatenate([rng.choice(heads, 12), [-1, n, 3 if K > 1 else -2]]).astype(np.int32)
        tags = np.where(rng.integers(0, 3, len(entries)) == 0, 77, owner[np.clip(entries, 0, n - 1)]).astype(np.uint32)
        tags[tags == 0] = 78
        for hold_all in (False, True):
            for cnt in (None, 9):
                a, b, pa, pb = bank.copy(), bank.copy(), pedal.copy(), pedal.copy()
                got = PM.stamp_owned_pedal(owner, pa, a, entries, tags, cnt, K, vmask, hold_all, now)[0]
                want = brute_off(owner, pb, b, entries, tags, cnt, K, vmask, hold_all, now)
                assert got == want and same_state(a, b, pa, pb), (K, trial, hold_all, cnt, got, want)
                seen["held"] += got[3]
                seen["stamped"] += got[0]
    assert all(v > 10 for v in seen.values()), seen


def test_hold_nothing_is_the_owner_model():
    """hold_all = 0 with nothing latched: words 0 .. 2 and the clocks of owner_model.stamp_owned / release_tags."""
    import owner_model as OM
    rng = np.random.default_rng(11)
    n, K, vmask = 256, 4, 0b1011
    bank, now, owner, pedal = random_state(rng, n, K)
    pedal[:] = rng.choice(np.array([0, PM.PENDING], np.uint32), n)
    entries = np.concatenate([np.arange(0, n, K)[::3], [-1, 2, n]]).astype(np.int32)
    tags = np.where(owner[np.clip(entries, 0, n - 1)] == 0, 5, owner[np.clip(entries, 0, n - 1)]).astype(np.uint32)
    a, b, before = bank.copy(), bank.copy(), pedal.copy()
    got, _ = PM.stamp_owned_pedal(owner, pedal, a, entries, tags, None, K, vmask, False, now)
    want, _ = OM.stamp_owned(owner, b, entries, tags, None, K, vmask, SM.STAMP_RELEASE, now)
    assert got[:3] == want and got[3] == 0 and np.array_equal(pedal, before)
    assert np.array_equal(a["voice_amp_envelope"]["sample_release"], b["voice_amp_envelope"]["sample_release"])


# ---------------------------------------------------------------------------------------------- the entry points' host checks

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pedal") / "c_pedal_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_pedal_host.c"), os.path.join(CSRC, "skred_bank_pedal.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"),
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
    assert host_lines[-1] == "OK" and len(host_lines) > 80
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "check", "flags", "stamp", "release", "latch", "up", "clear", "download", "untouched"}, groups


def test_check_through_ctypes():
    m = device.owner_match(*CM.channel(3))
    P = device
    assert P.pedal_check(P.PEDAL_CALL_UP, 1024, 0, 1024, 8, 0x55, m, P.PEDAL_LIFT_SUSTAIN) == 0
    for flags in range(16):
        assert P.pedal_check(P.PEDAL_CALL_UP, 1024, 0, 1024, 8, 0x55, m, flags) == PM.up_flags_check(flags), flags
    assert P.pedal_check(P.PEDAL_CALL_UP, 1024, 0, 1024, 8, 0x55, m, 5) == BAD and b"stays down" in device.load().skred_amd_last_error()
    assert P.pedal_check(P.PEDAL_CALL_LATCH, 1024, 0, 1024, 8, 0x55, m, 99) == 0              # (flags are not the latch's)
    assert P.pedal_check(P.PEDAL_CALL_LATCH, 1024, 0, 1024, 8, 0x55, None) == BAD
    assert P.pedal_check(P.PEDAL_CALL_LATCH, 1000, 0, 1024, 8, 0x55, m) == RANGE
    assert P.pedal_check(P.PEDAL_CALL_LATCH, 1024, 4, 8, 8, 0x55, m) == RANGE
    assert P.pedal_check(P.PEDAL_CALL_RELEASE_TAGS, 1024, 0, 1024, 8, 0x55, tags=[5, 6]) == 0
    assert P.pedal_check(P.PEDAL_CALL_RELEASE_TAGS, 1024, 0, 1024, 8, 0x55, tags=[5, 5]) == BAD
    assert P.pedal_check(P.PEDAL_CALL_STAMP_OWNED, 1024, slot_voices=8, voice_mask=0x55, tags=[5, 5]) == 0
    assert P.pedal_check(P.PEDAL_CALL_STAMP_OWNED, 1024, slot_voices=8, voice_mask=0x55, tags=[5, 0]) == BAD
    assert P.pedal_check(P.PEDAL_CALL_STAMP_OWNED, 1024, slot_voices=8, voice_mask=0x155, tags=[5]) == BAD
    assert P.pedal_check(P.PEDAL_CALL_STAMP_OWNED, 1024, slot_voices=12, voice_mask=0x55, tags=[5]) == RANGE
    assert P.pedal_check(7, 1024, 0, 1024, 8, 0x55, m, 1) == BAD


# ---------------------------------------------------------------------------------------------- the scenes

def scene_stage(clear_rule=True):
    """tests/owner_scenes.py's bank: 3.sk tiled over 256 voices, K = 4, every slot but A_SLOTS sustaining since long ago."""
    bank, tables, g = OS.bank()
    slots = [int(x) for x in OS.others()[:8]]
    return PM.Stage(bank, tables, g, OS.K, OS.VMASK, clear_rule), slots


@pytest.mark.parametrize("name", PM.SCENES)
def test_scene_on_the_oracle(name):
    st, slots = scene_stage()
    PM.run_scene(name, st, slots)
    others = np.setdiff1d(np.arange(st.n), np.concatenate([np.arange(s, s + st.K) for s in slots]))
    assert not st.pedal[others].any() and not st.owner[others].any(), "a scene touched a slot outside its own"


def test_scene_b_bites_without_the_clear_rule():
    st, slots = scene_stage(clear_rule=False)
    with pytest.raises(AssertionError, match="still down"):
        PM.run_scene("b", st, slots)


def test_documented_behaviour_of_the_plain_calls():
    """release_tags on a pending slot stamps at once and leaves the bit: a later pedal_up stamps again."""
    st, slots = scene_stage()
    t = [PM.tag_of(3, 60)]
    st.strike(slots[:1], t)
    st.block()
    assert st.off(t, True) == [0, 0, 0, 1]
    t1 = st.now()
    assert st.plain_off(t) == [1, 0, 0] and st.release_clock(slots[0]) == t1 and st.word(slots[0]) == PM.PENDING
    st.block()
    assert st.up(CM.channel(3), PM.LIFT_SUSTAIN)[:2] == [1, 0]
    assert st.release_clock(slots[0]) == st.now() > t1
