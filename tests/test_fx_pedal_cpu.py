"""Pedals on the fixed-point bank without a GPU: the symbols against the header, the model (tests/fx_pedal_model.py) against a
brute-force loop over every voice, every refusal and the tags' packing (through tests/c_fx_pedal_host.c, a program of its own on a bank
that is nothing but its size), and the float bank's scenes (a) .. (f) (tests/pedal_model.py, unchanged, one voice per slot) on the
oracle alone -- envelope clocks and rendered state through oracle.cpuref.fx_render with fx_live_model's stamps.  Scenes (b) and (c)
must FAIL on a model without the clear behind the tag launch: that is what shows they bite.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import chan_model as CM
import fx_owner_model as om
import fx_pedal_model as FP
import pedal_model as PM
from skred_amd import device, fxbank as fxb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
SYMBOLS = ("skred_fxbank_stamp_owned_pedal", "skred_fxbank_release_tags_pedal", "skred_fxbank_pedal_latch", "skred_fxbank_pedal_up",
           "skred_fxbank_pedal_clear", "skred_fxbank_download_pedals")
N_SCENE = 600
SCENE_VOICES = [5, 63, 64, 255, 256, 300, 511, 599]            # wave and workgroup edges of the range kernels among them


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd_fxpt.h")).read()
    L = device.load()
    for s in SYMBOLS + ("skred_fx_pedal_check",):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in fxb.FX_ABI_SYMBOLS + fxb.FX_HOST_ABI_SYMBOLS
    assert "SKRED_PEDAL_PENDING =" not in text, "the bits are include/skred_amd.h's: no copies"
    for name in ("PENDING", "LATCHED", "LIFT_SUSTAIN", "LIFT_SOSTENUTO", "SUSTAIN_DOWN"):
        assert getattr(fxb, "PEDAL_" + name) == getattr(PM, name) == getattr(FP, name)
    assert "Not built here: the fixed-point bank's twin" not in open(os.path.join(ROOT, "include", "skred_amd.h")).read()


# ---------------------------------------------------------------------------------------------- the model

def random_state(rng, n):
    bank, _, now = fxb.bank_fx(n)
    bank["sample_release"] = rng.choice([0, 0, 0, now - 3, 9, 1 << 40], n).astype(np.uint64)
    bank["is_active"] = (rng.integers(0, 4, n) != 0).astype(bank["is_active"].dtype)
    bank["use_envelope"] = (rng.integers(0, 5, n) != 0).astype(bank["use_envelope"].dtype)
    owner = rng.choice(np.array([0, PM.tag_of(3, 1), PM.tag_of(3, 2), PM.tag_of(5, 1), 0xFFFFFFFF, 0x00FFFFFF], np.uint32), n)
    pedal = rng.choice(np.array([0, 0, FP.PENDING, FP.LATCHED, FP.PENDING | FP.LATCHED], np.uint32), n)
    return bank, now, owner, pedal


def hit(o, match):
    value, mask = match
    return o != 0 and (o & mask) == value


def brute_release(bank, v, now):
    if bank["is_active"][v]:                                   # (this bank: no release clock on an envelope that is not active)
        bank["sample_release"][v] = now


def brute_latch(owner, pedal, bank, first, count, match):
    res = [0, 0]
    for v in range(first, first + count):
        if not hit(int(owner[v]), match):
            res[1] += 1
            continue
        is_held = bank["use_envelope"][v] != 0 and bank["is_active"][v] != 0 and int(bank["sample_release"][v]) == 0
        if not int(pedal[v]) & FP.PENDING and is_held:
            pedal[v] = int(pedal[v]) | FP.LATCHED
            res[0] += 1
    return res


def brute_up(owner, pedal, bank, first, count, match, flags, now):
    res = [0, 0, 0]
    for v in range(first, first + count):
        if not hit(int(owner[v]), match):
            res[2] += 1
            continue
        w = int(pedal[v])
        if flags & FP.LIFT_SOSTENUTO:
            w &= ~FP.LATCHED
        if w & FP.PENDING and not w & FP.LATCHED and not flags & FP.SUSTAIN_DOWN:
            w &= ~FP.PENDING
            brute_release(bank, v, now)
            res[0] += 1
        if w & FP.PENDING:
            res[1] += 1
        pedal[v] = w
    return res


def brute_stamps(owner, pedal, bank, entries, tags, count, hold_all, now):
    res = [0, 0, 0, 0]
    m = len(tags) if count is None else min(len(tags), count)
    for k in range(m):
        v = int(entries[k])
        if v < 0 or v >= len(owner):
            res[2] += 1
        elif int(owner[v]) != int(tags[k]):
            res[1] += 1
        elif hold_all or int(pedal[v]) & FP.LATCHED:
            pedal[v] = int(pedal[v]) | FP.PENDING
            res[3] += 1
        else:
            brute_release(bank, v, now)
            res[0] += 1
    return res


def same(a, b):
    owner_a, pedal_a, bank_a = a
    owner_b, pedal_b, bank_b = b
    assert np.array_equal(owner_a, owner_b) and np.array_equal(pedal_a, pedal_b)
    for name, _, _ in fxb.FX_FIELDS:
        assert np.array_equal(bank_a[name], bank_b[name]), name


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_brute_force(seed):
    rng = np.random.default_rng(6400 + seed)
    n = 600
    seen = {"latched": 0, "released": 0, "pending": 0, "held_back": 0, "stamped": 0, "stolen": 0, "inactive_released": 0}
    for trial in range(12):
        bank, now, owner, pedal = random_state(rng, n)
        a, b = (owner.copy(), pedal.copy(), bank.copy()), (owner.copy(), pedal.copy(), bank.copy())
        first = int(rng.integers(0, 100))
        count = int(rng.integers(1, n - first + 1))
        match = [CM.channel(3), CM.channel(5), (0, 0), (PM.tag_of(3, 2), 0xFFFFFFFF), CM.channel(9)][trial % 5]
        got, want = FP.latch(a[0], a[1], a[2], first, count, match), brute_latch(b[0], b[1], b[2], first, count, match)
        assert got == want
        same(a, b)
        seen["latched"] += got[0]
        entries = rng.integers(-2, n + 3, 80)
        entries[5] = entries[3]                                  # an entry named twice
        tags = np.where(rng.integers(0, 4, 80) == 0, 7, owner[np.clip(entries, 0, n - 1)]).astype(np.uint32)
        tags[tags == 0] = 9
        cnt = [None, 80, 33, 0, 200][trial % 5]
        hold = trial % 3 == 0
        got, _ = FP.stamp_owned_pedal(a[0], a[1], a[2], entries, tags, cnt, hold, now)
        assert got == brute_stamps(b[0], b[1], b[2], entries, tags, cnt, hold, now)
        same(a, b)
        seen["stamped"] += got[0]
        seen["stolen"] += got[1]
        seen["held_back"] += got[3]
        for flags in (FP.LIFT_SOSTENUTO | FP.SUSTAIN_DOWN, FP.LIFT_SUSTAIN, FP.LIFT_SUSTAIN | FP.LIFT_SOSTENUTO)[trial % 3:]:
            before = a[1].copy()
            got, voices = FP.up(a[0], a[1], a[2], first, count, match, flags, now + 64)
            assert got == brute_up(b[0], b[1], b[2], first, count, match, flags, now + 64)
            same(a, b)
            assert got[0] == len(voices) and ((before[voices] & FP.PENDING) != 0).all()
            seen["released"] += got[0]
            seen["pending"] += got[1]
            seen["inactive_released"] += int((a[2]["is_active"][voices] == 0).sum())
        uniq = np.unique(owner[owner != 0])[:3].tolist() + [0x12345678]
        got, _, lst = FP.release_tags_pedal(a[0], a[1], a[2], first, count, uniq, hold, now + 128)
        want_lst = [next((v for v in range(first, first + count) if int(owner[v]) == t), -1) for t in uniq]
        assert lst.tolist() == want_lst and got == brute_stamps(b[0], b[1], b[2], want_lst, uniq, None, hold, now + 128)
        same(a, b)
        FP.clear(a[1], first, count)
        assert not a[1][first:first + count].any() and np.array_equal(a[1][:first], b[1][:first])
    assert all(v > 10 for v in seen.values()), seen


def test_hold_nothing_is_the_owner_model():
    """hold_all = 0 with nothing latched: words 0 .. 2 and the bank of fx_owner_model.stamp_owned / release_tags."""
    rng = np.random.default_rng(11)
    bank, now, owner, pedal = random_state(rng, 600)
    pedal &= np.uint32(FP.PENDING)                              # pending words do not hold anything back by themselves
    entries = rng.integers(-2, 603, 90)
    tags = np.where(rng.integers(0, 3, 90) == 0, 7, owner[np.clip(entries, 0, 599)]).astype(np.uint32)
    tags[tags == 0] = 9
    a, b, p = bank.copy(), bank.copy(), pedal.copy()
    got, voices = FP.stamp_owned_pedal(owner, p, a, entries, tags, 77, False, now)
    want, wv = om.stamp_owned(owner, b, entries, tags, 77, FP.REL, now)
    assert got == want + [0] and np.array_equal(voices, wv) and np.array_equal(p, pedal) and want[0] > 10
    uniq = np.unique(owner[owner != 0]).tolist()
    got, _, lst = FP.release_tags_pedal(owner, p, a, 37, 500, uniq, False, now + 5)
    want, _, wl = om.release_tags(owner, b, 37, 500, uniq, FP.REL, now + 5)
    assert got == want + [0] and np.array_equal(lst, wl)
    for name, _, _ in fxb.FX_FIELDS:
        assert np.array_equal(a[name], b[name]), name


def test_tag_list_clears_only_what_it_tags():
    owner, pedal = om.new(16), FP.new(16)
    pedal[:] = 3
    assert FP.tag_list(owner, pedal, [3, -1, 16, 5, 7], [9, 9, 9, 8, 7], count=4) == [2, 2]
    assert pedal.tolist() == [3, 3, 3, 0, 3, 0] + [3] * 10 and owner[7] == 0
    pedal[:] = 3
    FP.tag_list(owner, pedal, [3, 5], [9, 8], clear_rule=False)
    assert (pedal == 3).all()
    FP.tag_list(owner, None, [3, 5], [9, 8])                     # a bank without the array


# ---------------------------------------------------------------------------------------------- the host program

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fxpedal") / "c_fx_pedal_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_fx_pedal_host.c"), os.path.join(CSRC, "skred_fx_pedal.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"),
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
    assert host_lines[-1] == "OK" and len(host_lines) > 100
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "check", "flags", "pack", "stamp", "release", "latch", "up", "clear", "download", "untouched"}, groups


def test_check_through_ctypes():
    m = device.owner_match(*CM.channel(3))
    P = fxb
    assert P.fx_pedal_check(P.PEDAL_CALL_UP, 600, 37, 500, m, P.PEDAL_LIFT_SUSTAIN) == 0
    for flags in range(16):
        assert P.fx_pedal_check(P.PEDAL_CALL_UP, 600, 37, 500, m, flags) == FP.up_flags_check(flags) == PM.up_flags_check(flags), flags
    assert P.fx_pedal_check(P.PEDAL_CALL_UP, 600, 0, 600, m, 5) == BAD and b"stays down" in device.load().skred_amd_last_error()
    assert P.fx_pedal_check(P.PEDAL_CALL_LATCH, 600, 0, 600, m, 99) == 0                        # (flags are not the latch's)
    assert P.fx_pedal_check(P.PEDAL_CALL_LATCH, 600, 0, 600, None) == BAD
    assert P.fx_pedal_check(P.PEDAL_CALL_LATCH, 600, 37, 564, m) == RANGE
    assert P.fx_pedal_check(P.PEDAL_CALL_LATCH, 600, 599, 1, m) == 0
    assert P.fx_pedal_check(P.PEDAL_CALL_RELEASE_TAGS, 600, 0, 600, tags=[5, 6]) == 0
    assert P.fx_pedal_check(P.PEDAL_CALL_RELEASE_TAGS, 600, 0, 600, tags=[5, 5]) == BAD
    assert P.fx_pedal_check(P.PEDAL_CALL_RELEASE_TAGS, 600, 0, 0, tags=[5, 6]) == RANGE
    assert P.fx_pedal_check(P.PEDAL_CALL_STAMP_OWNED, 600, tags=[5, 5]) == 0
    assert P.fx_pedal_check(P.PEDAL_CALL_STAMP_OWNED, 600, tags=[5, 0]) == BAD
    assert P.fx_pedal_check(P.PEDAL_CALL_STAMP_OWNED, 600, tags=None, n=2) == BAD
    assert P.fx_pedal_check(7, 600, 0, 600, m, 1) == BAD
    # the same verdicts as the float bank's check at one voice per slot
    for call, first, count, flags, tags in ((0, 0, 0, 0, [5]), (1, 0, 601, 0, [5]), (2, 0, 600, 0, None), (3, 0, 600, 4, None), (3, 1, 600, 1, None)):
        assert P.fx_pedal_check(call, 600, first, count, m, flags, tags) == device.pedal_check(call, 600, first, count, 1, 1, m, flags, tags)


# ---------------------------------------------------------------------------------------------- the scenes

def scene_stage(clear_rule=True):
    """600 voices of the bank_fx recipe, every one sustaining since long ago and tagged by nobody."""
    bank, pool, c0 = fxb.bank_fx(N_SCENE)
    return FP.FxStage(bank, pool, c0, clear_rule), SCENE_VOICES


@pytest.mark.parametrize("name", PM.SCENES)
def test_scene_on_the_oracle(name):
    st, voices = scene_stage()
    PM.run_scene(name, st, voices)
    others = np.setdiff1d(np.arange(st.n), voices)
    assert not st.pedal[others].any() and not st.owner[others].any(), "a scene touched a voice outside its own"


@pytest.mark.parametrize("name", ["b", "c"])
def test_scenes_b_and_c_bite_without_the_clear_rule(name):
    st, voices = scene_stage(clear_rule=False)
    with pytest.raises(AssertionError):
        PM.run_scene(name, st, voices)


def test_documented_behaviour_of_the_plain_calls():
    """release_tags on a pending voice stamps at once and leaves the bit: a later pedal_up stamps again.  And this bank's own point:
    a pending voice whose envelope is no longer active is counted as released, its clock stays."""
    st, voices = scene_stage()
    t = [PM.tag_of(3, 60), PM.tag_of(3, 61)]
    st.strike(voices[:2], t)
    st.block()
    assert st.off(t, True) == [0, 0, 0, 2]
    t1 = st.now()
    assert st.plain_off(t[:1]) == [1, 0, 0] and st.release_clock(voices[0]) == t1 and st.word(voices[0]) == FP.PENDING
    st.truth["is_active"][voices[1]] = 0
    st.block()
    assert st.up(CM.channel(3), FP.LIFT_SUSTAIN)[:2] == [2, 0]
    assert st.release_clock(voices[0]) == st.now() > t1 and st.release_clock(voices[1]) == 0 and not st.pedal.any()
