"""Patch controllers without a GPU: every refusal of skred_ctl_check, the entry points' host checks and the record packing (through
tests/c_ctl_host.c, a program of its own on a bank that is nothing but its size), the ctypes image of skred_ctl_t, and the model's
self-checks (tests/ctl_model.py is what tests/test_ctl.py holds the device to)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ctl_model as M
from skred_amd import banks, device
from skred_amd.device import CtlC, ctl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
NAN, INF = float("nan"), float("inf")

VALUES = dict(phase_inc=0.37, inc_scale=1.0594631, amp=0.8, pan_left=0.25, pan_right=0.75, b0=0.2, b1=0.4, b2=0.2, a1=-0.3, a2=0.1,
              attack_time=30.0, decay_time=60.0, sustain_level=0.5, release_time=400.0, velocity=0.9, smoothing=0.25,
              fm_depth=0.3, freq_scale=2.0, am_depth=0.2, pan_depth=0.1, cz_depth=0.4, cz_dist=0.6)
NAMES = {M.PHASE_INC: ("phase_inc",), M.INC_SCALE: ("inc_scale",), M.AMP: ("amp",), M.PAN: ("pan_left", "pan_right"),
         M.FILTER: ("b0", "b1", "b2", "a1", "a2"), M.ENV_TIMES: ("attack_time", "decay_time", "sustain_level", "release_time"),
         M.VELOCITY: ("velocity",), M.SMOOTHING: ("smoothing",), M.FM_DEPTH: ("fm_depth",), M.FREQ_SCALE: ("freq_scale",),
         M.AM_DEPTH: ("am_depth",), M.PAN_DEPTH: ("pan_depth",), M.CZ_DEPTH: ("cz_depth",), M.CZ_DIST: ("cz_dist",)}


def full(set_bits, **over):
    v = dict(VALUES)
    v.update(over)
    return ctl(set_bits, **v)


def junk():
    """A record skred_ctl_check would refuse in every way: it must not be looked at where the mask has no bit."""
    c = ctl(0xFFFFFFFF, **{k: NAN for k in VALUES})
    c.reserved = 7
    return c


# ---------------------------------------------------------------------------------------------- the struct and the symbols

def test_struct_matches_the_header():
    assert C.sizeof(CtlC) == 96
    text = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    body = re.search(r"typedef struct skred_ctl \{(.*?)\} skred_ctl_t;", text, re.S).group(1)
    names = re.findall(r"\b([a-z_0-9]+)\s*[,;]", body)
    assert names == [f[0] for f in CtlC._fields_]
    for i, (name, _) in enumerate(CtlC._fields_):
        assert getattr(CtlC, name).offset == 4 * i, name
    for name, bit in re.findall(r"SKRED_CTL_(\w+)\s*=\s*1u<<(\d+)", text):
        assert getattr(device, "CTL_" + name) == getattr(M, name) == 1 << int(bit), name
    assert device.CTL_ALL == M.ALL == sum(M.BITS) and set(NAMES) == set(M.BITS)
    # the device record (skred_launch.h: the SK_CTL_W_* enumerators) in the same order, word for word
    launch = open(os.path.join(CSRC, "skred_launch.h")).read()
    enum = re.search(r"enum \{ SK_CTL_SET = 0,(.*?)SK_CTL_WORDS \};", launch, re.S).group(1)
    words = [w.strip() for w in enum.split(",") if w.strip()]
    assert len(words) == 23 and words[-1] == "SK_CTL_W_RESERVED"
    short = {"SK_CTL_W_ATTACK": "attack_time", "SK_CTL_W_DECAY": "decay_time", "SK_CTL_W_SUSTAIN": "sustain_level", "SK_CTL_W_RELEASE": "release_time"}
    assert [short.get(w, w[len("SK_CTL_W_"):].lower()) for w in words] == [f[0] for f in CtlC._fields_[1:]]


def test_symbols_exported():
    L = device.load()
    for s in ("skred_bank_ctl_range", "skred_bank_ctl_slots", "skred_bank_download_ctl"):
        assert hasattr(L, s) and s in device.ABI_SYMBOLS, s
    assert hasattr(L, "skred_ctl_check") and "skred_ctl_check" in device.HOST_ABI_SYMBOLS


# ---------------------------------------------------------------------------------------------- skred_ctl_check

def test_check_accepts_the_edges():
    assert device.ctl_check([full(M.ALL & ~M.INC_SCALE)], 1) == 0
    assert device.ctl_check([full(M.ALL & ~M.PHASE_INC)], 1) == 0
    for bit in M.BITS:
        assert device.ctl_check([full(bit)], 1) == 0, bit
    assert device.ctl_check([full(M.AMP, amp=-0.5)], 1) == 0                                   # negative amp
    assert device.ctl_check([full(M.FM_DEPTH | M.AM_DEPTH | M.PAN_DEPTH | M.CZ_DEPTH | M.CZ_DIST, fm_depth=0.0, am_depth=-0.0, pan_depth=0.0,
                                  cz_depth=0.0, cz_dist=0.0)], 1) == 0                         # zero depths
    assert device.ctl_check([full(M.ENV_TIMES, attack_time=0.0, decay_time=0.0, sustain_level=0.0, release_time=0.0)], 1) == 0   # zero times
    assert device.ctl_check([full(M.PHASE_INC, phase_inc=0.0)], 1) == 0 and device.ctl_check([full(M.INC_SCALE, inc_scale=-2.0)], 1) == 0
    assert device.ctl_check([full(M.AMP, amp=1e-40)], 1) == 0                                  # a subnormal is not 0
    # values the record does not name are not looked at
    assert device.ctl_check([full(M.PAN, amp=0.0, b0=NAN, inc_scale=INF)], 1) == 0
    for K in (1, 2, 4, 8, 16, 32, 64):
        recs = [junk() for _ in range(K)]
        recs[K - 1] = full(M.FILTER)
        assert device.ctl_check(recs, 1 << (K - 1)) == 0, K                                     # the single high bit
        assert device.ctl_check([full(M.PAN)] * K, (1 << K) - 1) == 0, K


@pytest.mark.parametrize("bit", M.BITS)
def test_check_refuses_values_that_are_not_finite(bit):
    for name in NAMES[bit]:
        for bad in (NAN, INF, -INF):
            assert device.ctl_check([full(bit, **{name: bad})], 1) == BAD, (name, bad)
            other = M.PAN if bit != M.PAN else M.FILTER
            assert device.ctl_check([full(other, **{name: bad})], 1) == 0, (name, bad)          # ... only where the field is named


def test_check_refuses():
    ok = full(M.FILTER)
    L = device.load()
    assert L.skred_ctl_check(None, 1, 1) == BAD
    assert device.ctl_check([full(1 << 14)], 1) == BAD and device.ctl_check([full(M.PAN | (1 << 31))], 1) == BAD   # unknown bits
    assert device.ctl_check([full(0)], 1) == BAD                                                # set == 0 under a mask bit
    r = full(M.PAN)
    r.reserved = 1
    assert device.ctl_check([r], 1) == BAD
    assert device.ctl_check([full(M.PHASE_INC | M.INC_SCALE)], 1) == BAD
    assert device.ctl_check([full(M.AMP, amp=0.0)], 1) == BAD and device.ctl_check([full(M.AMP | M.PAN, amp=-0.0)], 1) == BAD
    for K in (0, -1, 3, 12, 65, 128):
        assert device.ctl_check([ok] * 64, 1, slot_voices=K) == RANGE, K
    assert device.ctl_check([ok] * 8, 0) == BAD and device.ctl_check([ok] * 8, 0x100) == BAD and device.ctl_check([ok], 2) == BAD
    assert device.ctl_check([ok] * 32, 1 << 32) == BAD and device.ctl_check([ok] * 64, (1 << 64) - 1) == 0
    # a bad record is seen exactly when its voice's bit is set
    recs = [ok, ok, junk(), ok]
    assert device.ctl_check(recs, 0b1011) == 0 and device.ctl_check(recs, 0b0100) == BAD and device.ctl_check(recs, 0b1111) == BAD
    assert b"record 2" in L.skred_amd_last_error()


def test_entry_points_refuse_a_null_bank():
    L = device.load()
    arr = device.ctl_array([full(M.FILTER)] * 8)
    p, word = C.cast(arr, C.c_void_p), C.c_void_p(16)       # (a refused call never reads through the device pointers)
    assert L.skred_bank_ctl_range(None, p, 0, 8, 8, 0xFF, word, None) == BAD
    assert L.skred_bank_ctl_slots(None, p, 8, 0xFF, word, 2, None, word, None) == BAD
    assert L.skred_bank_download_ctl(None, None, 0, 0, 0) == BAD


# ---------------------------------------------------------------------------------------------- the entry points' host checks, the packing

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ctl") / "c_ctl_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_ctl_host.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"), "-lskred_amd", "-lm", "-lpthread",
           "-Wl,-rpath," + os.path.join(ROOT, "skred_amd")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return out.stdout.strip().splitlines()


@pytest.mark.parametrize("group", ["check", "pack", "range", "slots", "download", "bank"])
def test_host_cases(host_lines, group):
    mine = [l for l in host_lines if l.startswith(group + "/")]
    assert mine, f"no case of group {group} ran"
    bad = [l for l in mine if not l.endswith(" ok")]
    assert not bad, "\n".join(bad)


def test_every_host_case_passed(host_lines):
    assert host_lines[-1] == "OK", "\n".join(l for l in host_lines if not l.endswith(" ok"))


# ---------------------------------------------------------------------------------------------- the model

def small_bank(n=64):
    bank, tables, g = banks.bank_c2(n)
    bank["voice_amp"][5::8] = 0.0
    bank["voice_amp"][6::16] = np.float32(-0.0)
    return bank


def test_model_one_voice_slots_are_a_per_voice_loop():
    bank = small_bank()
    a, b = bank.copy(), bank.copy()
    rec = full(M.ALL & ~M.INC_SCALE)
    res, touched = M.ctl_range((a,), [rec], 8, 40, 1)
    wh = sum(M.store_voice(b, v, rec) for v in range(8, 48))
    assert res == [40, wh] and np.array_equal(touched, np.arange(8, 48)) and wh == int((bank["voice_amp"][8:48] == 0).sum()) > 0
    assert not M.words_differ(a, b) and M.words_differ(a, bank)
    outside = np.r_[0:8, 48:64]
    for field, sub in M.CTL_WORDS:
        assert (M.word(a, field, sub)[outside].view("<u4") == M.word(bank, field, sub)[outside].view("<u4")).all(), (field, sub)
    # nothing but the named words: every other field of the view keeps its bytes
    for name in bank.a:
        if name not in {f for f, _ in M.CTL_WORDS}:
            assert a[name].tobytes() == bank[name].tobytes(), name
    e, e0 = a["voice_amp_envelope"], bank["voice_amp_envelope"]
    for sub in ("a", "d", "s", "r", "sample_start", "sample_release", "is_active"):
        assert e[sub].tobytes() == e0[sub].tobytes(), sub
    f, f0 = a["voice_filter"], bank["voice_filter"]
    for sub in ("x1", "x2", "y1", "y2", "last_freq", "last_resonance", "last_mode"):
        assert f[sub].tobytes() == f0[sub].tobytes(), sub


def test_model_masks_and_records():
    bank = small_bank()
    a = bank.copy()
    recs = [full(M.PAN, pan_left=0.1 * l, pan_right=1.0 - 0.1 * l) for l in range(4)]
    recs[1] = junk()
    res, touched = M.ctl_range((a,), recs, 16, 32, 0b1101)
    assert res == [24, 0] and np.array_equal(touched, [v for v in range(16, 48) if v % 4 != 1])
    assert (a["voice_pan_left"][16:48:4] == np.float32(0.0)).all() and (a["voice_pan_left"][19:48:4] == np.float32(0.1 * 3)).all()
    assert a["voice_pan_left"][17:48:4].tobytes() == bank["voice_pan_left"][17:48:4].tobytes()
    assert M.listed(recs, 0b1101) == 0 and M.listed([full(M.AMP), full(M.FILTER), full(M.FILTER | M.SMOOTHING), full(M.VELOCITY)], 0b0111) == 0b0101


def test_model_list_rules_duplicates_and_counts():
    n, K = 64, 4
    bank = small_bank(n)
    recs = [full(M.AMP | M.FILTER, amp=0.3 + 0.1 * l) for l in range(K)]
    entries = np.array([8, -1, 6, 64, 8, 60, -4, 2**31 - 4, 12, 20], np.int32)
    a, b = bank.copy(), bank.copy()
    res, touched = M.ctl_slots((a,), recs, 0b1111, entries, len(entries), 9, n)          # the count cuts the last entry off
    assert np.array_equal(touched, np.r_[8:16, 60:64])                                   # 8 (twice), 60, 12; not 20
    res1, touched1 = M.ctl_slots((b,), recs, 0b1111, np.array([8, 60, 12], np.int32), 3, None, n)
    assert not M.words_differ(a, b) and np.array_equal(touched, touched1)                # a duplicate slot equals a single one
    zero = int((bank["voice_amp"][touched] == 0).sum())
    dup_zero = int((bank["voice_amp"][8:12] == 0).sum())
    assert res1 == [12, zero] and res == [16, zero + dup_zero] and zero > 0
    assert (a["voice_amp"][touched][bank["voice_amp"][touched] == 0] == 0).all()         # zero stays zero (and -0.0 keeps its sign)
    assert a["voice_amp"].view("<u4")[14] == bank["voice_amp"].view("<u4")[14] if bank["voice_amp"][14] == 0 else True
    res2, _ = M.ctl_slots((bank.copy(),), recs, 0b1111, entries, 3, None, n)
    assert res2[0] == 4                                                                  # n smaller than the list: entry 8 only


def test_model_inc_scale_guard():
    bank = small_bank()
    bank["voice_phase_inc"][3] = np.float32(3e38)
    bank["voice_phase_inc"][4] = np.float32(-3e38)
    a = bank.copy()
    res, _ = M.ctl_range((a,), [full(M.INC_SCALE, inc_scale=2.0)], 0, 8, 1)
    assert res == [8, 2]
    assert a["voice_phase_inc"][3] == np.float32(3e38) and a["voice_phase_inc"][4] == np.float32(-3e38)
    want = (bank["voice_phase_inc"][[0, 1, 2, 5, 6, 7]] * np.float32(2.0)).astype(np.float32)
    assert a["voice_phase_inc"][[0, 1, 2, 5, 6, 7]].tobytes() == want.tobytes()
    # one fp32 multiply, rounded once: not the double-precision product rounded
    x, s = np.float32(0.1234567), np.float32(1.0594631)
    c = bank.copy()
    c["voice_phase_inc"][0] = x
    M.ctl_range((c,), [full(M.INC_SCALE, inc_scale=float(s))], 0, 1, 1)
    assert c["voice_phase_inc"][0] == np.float32(x * s) and np.isfinite(c["voice_phase_inc"]).all()
    assert np.float32(x * s) >= np.finfo(np.float32).tiny                                # (a normal product: no denormal mode involved)


def test_model_views_must_agree():
    bank = small_bank()
    stale = bank.copy()
    stale["voice_amp"][0] = 0.0
    assert bank["voice_amp"][0] != 0
    with pytest.raises(AssertionError):
        M.ctl_range((bank.copy(), stale), [full(M.AMP)], 0, 8, 1)
