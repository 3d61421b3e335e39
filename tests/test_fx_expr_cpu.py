"""Channels and per-note expression on the fixed-point bank without a GPU: the per-entry record and the symbols against the header,
skred_fx_ctl_each_check against the model on every refusal beside the accepted edge, the entries' packing, the sort-plus-permutation
of skred_fxbank_ctl_tags_each and every entry point's refusals (through tests/c_fx_expr_host.c), the model's own edges
(tests/fx_expr_model.py is what tests/test_fx_expr.py holds the device to) against plain Python integers, and the channel scene on
the oracle alone."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import fx_ctl_model as cm
import fx_expr_model as em
import fx_owner_model as om
from oracle import cpuref
from skred_amd import device, fxbank as fxb
from skred_amd.fxbank import fx_ctl, fx_each

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BAD = -2
EXPR_CALLS = ("skred_fxbank_find_match", "skred_fxbank_find_match_host", "skred_fxbank_stamp_match", "skred_fxbank_ctl_match",
              "skred_fxbank_ctl_owned_each", "skred_fxbank_ctl_tags_each")
CHANNEL = 0xFF000000


# ---------------------------------------------------------------------------------------------- the header, the symbols

def test_fx_expr_record_and_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd_fxpt.h")).read()
    float_header = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    assert C.sizeof(fxb.FxCtlEachC) == 32 and C.sizeof(device.OwnerMatchC) == 8
    body = re.search(r"typedef struct skred_fx_ctl_each \{(.*?)\} skred_fx_ctl_each_t;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in fxb.FxCtlEachC._fields_], names
    bits = dict(re.findall(r"SKRED_EACH_(INC_SCALE|AMP_SCALE|VELOCITY|PAN)\s*=\s*1u << (\d)", float_header))
    assert [1 << int(bits[k]) for k in ("INC_SCALE", "AMP_SCALE", "VELOCITY", "PAN")] == \
        [fxb.EACH_INC_SCALE, fxb.EACH_AMP_SCALE, fxb.EACH_VELOCITY, fxb.EACH_PAN]
    assert "SKRED_EACH_INC_SCALE =" not in text, "the bits are the float bank's: reused, not redefined"
    L = device.load()
    for s in EXPR_CALLS:
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s) and s in fxb.FX_ABI_SYMBOLS, s
    assert hasattr(L, "skred_fx_ctl_each_check") and "skred_fx_ctl_each_check" in fxb.FX_HOST_ABI_SYMBOLS
    section = float_header[float_header.index("---- channels and per-note expression"):float_header.index("---- voices sharded")]
    assert "skred_fxbank_find_match" in section and "Out of scope: the fixed-point bank" not in section


def test_fx_each_check_is_the_models():
    amp = fx_ctl(fxb.CTL_AMP, amp_q15=30000)
    pan = fx_ctl(fxb.CTL_PAN, pan_left_q15=1, pan_right_q15=2)
    inc = fx_ctl(fxb.CTL_PHASE_INC, phase_inc=1000)
    scale = fx_ctl(fxb.CTL_INC_SCALE, inc_scale_q16=65536)
    bad = fx_ctl(fxb.CTL_PAN | 1 << 8)
    everything = dict(inc_scale_q16=69433, amp_scale_q16=32768, velocity_q15=65535, pan_left_q15=0, pan_right_q15=65535)
    cases = [(fx_each(fxb.EACH_ALL, **everything), amp), (fx_each(fxb.EACH_ALL, **everything), None),
             (fx_each(fxb.EACH_ALL, **everything), pan), (fx_each(fxb.EACH_ALL, **everything), bad),
             (fx_each(0, **everything), amp), (fx_each(16, **everything), amp),
             (fx_each(fxb.EACH_VELOCITY, velocity_q15=65536), None), (fx_each(fxb.EACH_VELOCITY, velocity_q15=-1), None),
             (fx_each(fxb.EACH_VELOCITY, velocity_q15=0), None), (fx_each(fxb.EACH_PAN, velocity_q15=-1), None),
             (fx_each(fxb.EACH_PAN, pan_left_q15=65536), None), (fx_each(fxb.EACH_PAN, pan_right_q15=-1), None),
             (fx_each(fxb.EACH_AMP_SCALE, amp_scale_q16=0), amp), (fx_each(fxb.EACH_AMP_SCALE, amp_scale_q16=1), amp),
             (fx_each(fxb.EACH_AMP_SCALE, amp_scale_q16=0xFFFFFFFF), amp), (fx_each(fxb.EACH_AMP_SCALE, amp_scale_q16=65536), pan),
             (fx_each(fxb.EACH_VELOCITY, amp_scale_q16=0), pan),
             (fx_each(fxb.EACH_INC_SCALE, inc_scale_q16=0), None), (fx_each(fxb.EACH_INC_SCALE, inc_scale_q16=0xFFFFFFFF), pan),
             (fx_each(fxb.EACH_INC_SCALE, inc_scale_q16=65536), inc), (fx_each(fxb.EACH_INC_SCALE, inc_scale_q16=65536), scale),
             (fx_each(fxb.EACH_PAN), scale)]
    verdicts = [fxb.fx_ctl_each_check([e], c) for e, c in cases]
    assert verdicts == [em.each_check([e], c) for e, c in cases]
    assert verdicts.count(0) == 9 and verdicts.count(BAD) == len(cases) - 9, verdicts
    for k in range(2):
        e = fx_each(fxb.EACH_PAN)
        e.reserved[k] = 1
        assert fxb.fx_ctl_each_check([e]) == em.each_check([e], None) == BAD
    good, worse = fx_each(fxb.EACH_PAN), fx_each(0)
    assert fxb.fx_ctl_each_check([good, worse]) == em.each_check([good, worse], None) == BAD
    assert fxb.fx_ctl_each_check([good, worse], None, 1) == em.each_check([good, worse], None, 1) == 0
    assert fxb.fx_ctl_each_check(None) == em.each_check(None, None) == BAD
    assert fxb.fx_ctl_each_check([good], None, -1) == em.each_check([good], None, -1) == BAD
    assert fxb.fx_ctl_each_check([], None) == 0


def test_fx_expr_entry_points_refuse_a_null_bank():
    L = fxb._bind(device.load())
    m, c, e = device.OwnerMatchC(0x03000000, CHANNEL), fx_ctl(fxb.CTL_PAN), fx_each(fxb.EACH_PAN)
    tags, word = np.array([1, 2], np.uint32), C.c_void_p(16)
    total = C.c_int(0)
    assert L.skred_fxbank_find_match(None, 0, 8, C.byref(m), 0, None, word, None) == BAD
    assert L.skred_fxbank_find_match_host(None, 0, 8, C.byref(m), 0, None, C.byref(total), None) == BAD
    assert L.skred_fxbank_stamp_match(None, 0, 8, C.byref(m), fxb.STAMP_RELEASE, word, None) == BAD
    assert L.skred_fxbank_ctl_match(None, C.byref(c), 0, 8, C.byref(m), None, None) == BAD
    assert L.skred_fxbank_ctl_owned_each(None, None, C.byref(e), word, tags.ctypes.data, 1, None, None, None) == BAD
    assert L.skred_fxbank_ctl_tags_each(None, None, C.byref(e), 0, 8, tags.ctypes.data, 1, None, None) == BAD


@functools.lru_cache(maxsize=1)
def host_lines():
    """Builds and runs tests/c_fx_expr_host.c once, as tests/fx_host_cases.py builds tests/c_fx_ctl_host.c: the program's lines."""
    exe = os.path.join(tempfile.mkdtemp(prefix="fx_expr_host"), "c_fx_expr_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "skred_amd", "csrc"),
           "-I" + os.path.join(rocm, "include"), os.path.join(HERE, "c_fx_expr_host.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"),
           "-lskred_amd", "-lm", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "skred_amd")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return tuple(out.stdout.strip().splitlines())


@pytest.mark.parametrize("group", ["const", "check", "pack", "perm", "find", "find_host", "stamp", "ctlmatch", "each", "tags", "bank"])
def test_fx_expr_host_cases(group):
    mine = [l for l in host_lines() if l.startswith(group + "/")]
    assert mine, f"no case of group {group} ran"
    bad = [l for l in mine if not l.endswith(" ok")]
    assert not bad, "\n".join(bad)
    assert host_lines()[-1] == "OK"


# ---------------------------------------------------------------------------------------------- the model's edges

def tagged_bank(n=8):
    b, pool, c0 = fxb.bank_fx(n)
    owner = om.new(n)
    om.tag_list(owner, np.arange(n), 100 + np.arange(n))
    return b, pool, c0, owner


def test_fx_model_match_predicate_and_list():
    owner = np.array([0, 0x03000001, 0x03000002, 0x04000001, 0, 0x03FFFFFF, 0xFFFFFFFF, 0x00000007], np.uint32)
    assert em.matches(owner, 0, 0).tolist() == [False, True, True, True, False, True, True, True]            # every tagged voice
    assert em.matches(owner, 0x03000000, CHANNEL).tolist() == [False, True, True, False, False, True, False, False]
    assert em.matches(owner, 0, CHANNEL).tolist() == [False] * 7 + [True]                                   # channel 0: the untagged do not match
    assert em.matches(owner, 0xFFFFFFFF, 0xFFFFFFFF).tolist() == [False] * 6 + [True, False]
    assert em.match_check(0x03000001, CHANNEL) == BAD and em.match_check(1, 0) == BAD and em.match_check(0, 0) == 0
    lst, total = em.find_match(owner, 1, 6, 0x03000000, CHANNEL)
    assert lst.tolist() == [1, 2, 5] and total == 3 and lst.dtype == np.int32
    lst, total = em.find_match(owner, 1, 6, 0x03000000, CHANNEL, 2)
    assert lst.tolist() == [1, 2] and total == 3
    lst, total = em.find_match(owner, 0, 8, 0x03000000, CHANNEL, 0)
    assert lst.tolist() == [] and total == 3
    assert em.find_match(owner, 3, 2, 0x03000000, CHANNEL) == (pytest.approx([]), 0)


def test_fx_model_increment_products_against_python_integers():
    """An increment product that is exactly 0xFFFFFFFF is stored, 0x100000000 is withheld (SKRED_CTL_INC_SCALE's rule)."""
    b, _, _, owner = tagged_bank()
    b["phase_inc"][:4] = [0x10000, 0x10001, 0x80000000, 0xFFFFFFFF]
    want = b["phase_inc"].copy()
    entries = [fx_each(fxb.EACH_INC_SCALE, inc_scale_q16=s) for s in (0xFFFFFFFF, 0xFFFFFFFF, 131072, 65536)]
    prods = [(0x10000 * 0xFFFFFFFF) >> 16, (0x10001 * 0xFFFFFFFF) >> 16, (0x80000000 * 131072) >> 16, (0xFFFFFFFF * 65536) >> 16]
    assert prods[0] == 0xFFFFFFFF and prods[1] > 0xFFFFFFFF and prods[2] == 0x100000000 and prods[3] == 0xFFFFFFFF
    res = em.ctl_owned_each(owner, b, None, entries, [0, 1, 2, 3], [100, 101, 102, 103])
    want[0], want[3] = 0xFFFFFFFF, 0xFFFFFFFF
    assert res == [4, 2, 0] and b["phase_inc"].tolist() == want.tolist()


def test_fx_model_amp_products_against_python_integers():
    """An amp product of exactly 1 or exactly 65535 is stored; 0 and 65536 are withheld and the amp is left alone; a voice whose
    device amp is 0 has its amp withheld ONCE -- by the product or by the amp guard, never by both."""
    b, _, _, owner = tagged_bank()
    before = b["amp_q15"].copy()
    one = fx_ctl(fxb.CTL_AMP, amp_q15=1)
    full = fx_ctl(fxb.CTL_AMP, amp_q15=65535)
    cases = [(one, 65536, 1), (one, 0x7FFF, None), (one, 0xFFFF, None), (one, 0xFFFFFFFF, 65535), (full, 65536, 65535), (full, 65538, None),
             (full, 1, None), (full, 2, 1)]
    for v, (c, scale, stored) in enumerate(cases):
        prod = (c.amp_q15 * scale) >> 16
        assert (stored is None) == (prod == 0 or prod > 65535) and (stored is None or prod == stored), (c.amp_q15, scale, prod)
        res = em.ctl_owned_each(owner, b, c, [fx_each(fxb.EACH_AMP_SCALE, amp_scale_q16=scale)], [v], [100 + v])
        assert res == [1, 0 if stored else 1, 0] and b["amp_q15"][v] == (stored if stored else before[v]), (v, res)
    assert (1 * 0x7FFF) >> 16 == 0 and (65535 * 65538) >> 16 == 65536
    # ---- a silent voice (device amp 0): once by the guard when the product is fine, once by the product when it is not
    b["amp_q15"][:2] = 0
    res = em.ctl_owned_each(owner, b, full, [fx_each(fxb.EACH_AMP_SCALE, amp_scale_q16=32768), fx_each(fxb.EACH_AMP_SCALE, amp_scale_q16=1)],
                            [0, 1], [100, 101])
    assert res == [2, 2, 0] and b["amp_q15"][:2].tolist() == [0, 0]
    # ---- both withheld stores on one voice: the increment and the amp, 2 at the most
    b["phase_inc"][2] = 0xFFFFFFFF
    e = fx_each(fxb.EACH_AMP_SCALE | fxb.EACH_INC_SCALE | fxb.EACH_VELOCITY, amp_scale_q16=1, inc_scale_q16=65537, velocity_q15=777)
    assert em.ctl_owned_each(owner, b, full, [e], [2], [102]) == [1, 2, 0]
    assert b["phase_inc"][2] == 0xFFFFFFFF and b["velocity_q15"][2] == 777


def test_fx_model_overlay_replaces_and_supplies():
    b, _, _, owner = tagged_bank()
    base = fx_ctl(fxb.CTL_VELOCITY | fxb.CTL_SMOOTHING, velocity_q15=1000, smoother_k_q15=55)
    entries = [fx_each(fxb.EACH_VELOCITY, velocity_q15=2000), fx_each(fxb.EACH_PAN, pan_left_q15=3, pan_right_q15=4)]
    before = b.copy()
    res = em.ctl_owned_each(owner, b, base, entries + entries, [0, 1, -1, 8], [100, 101, 102, 103])
    assert res == [2, 0, 0]                                                                   # holes and out-of-bank entries are skipped
    assert b["velocity_q15"][:2].tolist() == [2000, 1000] and b["smoother_k_q15"][:2].tolist() == [55, 55]
    assert b["pan_left_q15"][:2].tolist() == [before["pan_left_q15"][0], 3] and b["pan_right_q15"][1] == 4
    res = em.ctl_owned_each(owner, b, None, entries, [2, 3], [102, 999])                      # a stale tag: counted, the voice untouched
    assert res == [1, 0, 1] and b["velocity_q15"][2] == 2000 and b["pan_left_q15"][3] == before["pan_left_q15"][3]
    res = em.ctl_owned_each(owner, b, None, entries + entries, [4, 5, 6, 7], [104, 105, 106, 107], d_count=1)
    assert res == [1, 0, 0] and b["velocity_q15"][4] == 2000 and b["pan_left_q15"][5] == before["pan_left_q15"][5]
    res, lst = em.ctl_tags_each(owner, b, None, entries, 0, 8, [107, 555])
    assert res == [1, 0, 0] and lst.tolist() == [7, -1] and b["velocity_q15"][7] == 2000
    changed = [k for k in b.a if not np.array_equal(b[k], before[k])]
    assert sorted(changed) == ["pan_left_q15", "pan_right_q15", "smoother_k_q15", "velocity_q15"]
    with pytest.raises(AssertionError):
        em.ctl_owned_each(owner, b, None, [fx_each(fxb.EACH_INC_SCALE, inc_scale_q16=70000)] * 2, [0, 0], [100, 100])


def test_fx_model_match_calls_count_every_voice_of_the_range():
    b, _, c0, owner = tagged_bank(16)
    owner[:] = 0
    om.tag_list(owner, np.arange(2, 14), (np.arange(12) % 3 + 1) << 24 | np.arange(12) + 1)
    b["amp_q15"][6] = 0
    res = em.ctl_match(owner, b, fx_ctl(fxb.CTL_AMP | fxb.CTL_PAN, amp_q15=9, pan_left_q15=1, pan_right_q15=2), 1, 14, 2 << 24, CHANNEL)
    assert res == [4, 1, 10] and b["amp_q15"][[3, 6, 9, 12]].tolist() == [9, 0, 9, 9]             # the silent voice keeps its 0 ...
    assert b["pan_left_q15"][[3, 6, 9, 12]].tolist() == [1] * 4 and b["pan_left_q15"][5] != 1     # ... and still gets the pan
    res, voices = em.stamp_match(owner, b, 0, 16, 0, 0, fxb.STAMP_RELEASE, c0 + 5)
    assert res == [12, 4] and voices.tolist() == list(range(2, 14))
    assert (b["sample_release"][2:14] == c0 + 5).all() and (b["sample_release"][[0, 1, 14, 15]] == 0).all()


# ---------------------------------------------------------------------------------------------- the channel scene, on the oracle alone

def test_fx_channel_scene_all_notes_off_spares_the_thief():
    """Two channels share a range; channel B steals some of A's voices (a thief's tags overwrite its victims'); an all-notes-off on A,
    by the model's match, releases exactly A's surviving voices, and B's voices keep sounding in fx_render's mix."""
    n, a_chan, b_chan = 48, 1 << 24, 2 << 24
    b, pool, c0 = fxb.bank_fx(n)
    b["smoother_enable"] = 0
    b["attack_frames"], b["decay_frames"], b["release_frames"] = 0, 0, 32                       # held at sustain: a release acts at once
    owner = om.new(n)
    a_voices, b_own = np.arange(0, 32), np.arange(32, 44)                                       # 44..47 stay untagged
    om.tag_list(owner, a_voices, a_chan | (1 + a_voices))
    om.tag_list(owner, b_own, b_chan | (1 + b_own))
    stolen = np.array([3, 8, 21, 31])
    om.tag_list(owner, stolen, b_chan | (100 + stolen))
    live_bank, twin = b.copy(), b.copy()                                                        # the twin gets no note-off
    _, _, cnt = cpuref.fx_render(live_bank, pool, c0, 64, 1)
    cpuref.fx_render(twin, pool, c0, 64, 1)
    res, released = em.stamp_match(owner, live_bank, 0, n, a_chan, CHANNEL, fxb.STAMP_RELEASE, cnt)
    survivors = np.setdiff1d(a_voices, stolen)
    assert released.tolist() == survivors.tolist() and res == [len(survivors), n - len(survivors)]
    assert (live_bank["sample_release"][survivors] == cnt).all()
    others = np.setdiff1d(np.arange(n), survivors)
    assert (live_bank["sample_release"][others] == twin["sample_release"][others]).all()
    assert em.find_match(owner, 0, n, b_chan, CHANNEL)[0].tolist() == sorted(stolen.tolist() + b_own.tolist())
    mix, stems, _ = cpuref.fx_render(live_bank, pool, cnt, 96, 1, want_stems=True)
    twin_mix, twin_stems, _ = cpuref.fx_render(twin, pool, cnt, 96, 1, want_stems=True)
    assert (live_bank["is_active"][survivors] == 0).all() and (live_bank["is_active"][others] == 1).all()
    assert (stems[40:, survivors] == 0).all(), "A's surviving voices end with their release"
    assert np.abs(twin_stems[40:, survivors]).sum() > 0
    assert np.array_equal(stems[:, others], twin_stems[:, others]), "B's voices and the untagged ones render as if nothing had happened"
    b_all = np.concatenate([stolen, b_own])
    assert (np.abs(stems[40:, b_all]).sum(axis=(0, 2)) > 0).all(), "every voice of B keeps sounding"
    assert np.array_equal(mix, stems.astype(np.int64).sum(axis=1)) and not np.array_equal(mix, twin_mix)
    assert np.array_equal(mix[40:], stems[40:, others].astype(np.int64).sum(axis=1))
