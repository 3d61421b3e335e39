"""Channels and per-note expression without a GPU: the constants and symbols against the header, the two check functions against the
model, every refusal and the packing and permutation of the per-entry records (through tests/c_expr_host.c, a program of its own on a
bank that is nothing but its size), the model against hand-written cases (tests/expr_model.py is what tests/test_expr.py holds the
device to), and the channel scene of the GPU tests on the oracle's state alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ctl_model as CM
import expr_model as EM
import expr_scenes as XS
import owner_model as OM
import owner_scenes as S
import slot_model as SM
from skred_amd import banks, device
from skred_amd.device import ctl, ctl_each, owner_match

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
REL = SM.STAMP_RELEASE
EXPR_CALLS = ("skred_bank_find_match", "skred_bank_find_match_host", "skred_bank_stamp_match", "skred_bank_ctl_match",
              "skred_bank_ctl_owned_each", "skred_bank_ctl_tags_each")


# ---------------------------------------------------------------------------------------------- the header, the symbols

def test_constants_and_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    bits = dict(re.findall(r"SKRED_EACH_(INC_SCALE|AMP_SCALE|VELOCITY|PAN)\s*=\s*1u << (\d)", text))
    assert [1 << int(bits[k]) for k in ("INC_SCALE", "AMP_SCALE", "VELOCITY", "PAN")] == \
        [device.EACH_INC_SCALE, device.EACH_AMP_SCALE, device.EACH_VELOCITY, device.EACH_PAN] == \
        [EM.EACH_INC_SCALE, EM.EACH_AMP_SCALE, EM.EACH_VELOCITY, EM.EACH_PAN]
    assert C.sizeof(device.CtlEachC) == 32 and C.sizeof(device.OwnerMatchC) == 8
    L = device.load()
    for s in EXPR_CALLS:
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s) and s in device.ABI_SYMBOLS, s
    for s in ("skred_owner_match_check", "skred_ctl_each_check"):
        assert hasattr(L, s) and s in device.HOST_ABI_SYMBOLS, s
    # what the section promises to stay out of
    section = text[text.index("---- channels and per-note expression"):text.index("---- voices sharded")]
    for word in ("fixed-point bank", "drop-in mode", "deferred items and pattern steps", "skred_shard_bank()", "per-entry filter"):
        assert word in section, word


def test_match_check_is_the_models():
    for value, mask in ((0, 0), (0x03000000, 0xFF000000), (0xFFFFFFFF, 0xFFFFFFFF), (1, 0), (0x03000001, 0xFF000000), (0, 0xFFFFFFFF),
                        (0x80000000, 0x7FFFFFFF)):
        assert device.owner_match_check(owner_match(value, mask)) == EM.match_check(value, mask), (hex(value), hex(mask))
    assert device.owner_match_check(None) == BAD


def test_each_check_is_the_models():
    K = 4
    plain = [ctl(CM.FILTER, b0=0.5) for _ in range(K)]
    amp = [ctl(CM.FILTER | CM.AMP, b0=0.5, amp=0.5) for _ in range(K)]
    amp3 = amp[:3] + [plain[3]]
    inc = plain[:2] + [ctl(CM.INC_SCALE, inc_scale=1.5)] + plain[3:]
    pinc = plain[:2] + [ctl(CM.PHASE_INC, phase_inc=0.1)] + plain[3:]
    ok = ctl_each(EM.EACH_PAN | EM.EACH_VELOCITY, pan_left=0.1, pan_right=0.2, velocity=0.3)
    cases = [([ok], plain, 0xF), ([ok], None, 0xF), ([ok], None, 0), ([ok], None, 0x10),
             ([ctl_each(16)], plain, 0xF), ([ctl_each(0)], plain, 0xF), ([ok, ctl_each(0)], plain, 0xF),
             ([ctl_each(EM.EACH_INC_SCALE, inc_scale=float("inf"))], plain, 0xF), ([ctl_each(EM.EACH_VELOCITY, velocity=float("nan"))], plain, 0xF),
             ([ctl_each(EM.EACH_PAN, pan_left=0.5, pan_right=float("-inf"))], plain, 0xF),
             ([ctl_each(EM.EACH_PAN, pan_left=0.5, pan_right=0.5, inc_scale=float("nan"))], plain, 0xF),
             ([ctl_each(EM.EACH_AMP_SCALE, amp_scale=0.5)], amp, 0xF), ([ctl_each(EM.EACH_AMP_SCALE, amp_scale=0.5)], plain, 0xF),
             ([ctl_each(EM.EACH_AMP_SCALE, amp_scale=0.5)], None, 0xF), ([ctl_each(EM.EACH_AMP_SCALE, amp_scale=0.5)], amp3, 0xF),
             ([ctl_each(EM.EACH_AMP_SCALE, amp_scale=0.5)], amp3, 0x7), ([ctl_each(EM.EACH_AMP_SCALE, amp_scale=0.0)], amp, 0xF),
             ([ctl_each(EM.EACH_AMP_SCALE, amp_scale=-0.0)], amp, 0xF),
             ([ctl_each(EM.EACH_INC_SCALE, inc_scale=1.01)], inc, 0xF), ([ctl_each(EM.EACH_INC_SCALE, inc_scale=1.01)], inc, 0xB),
             ([ctl_each(EM.EACH_INC_SCALE, inc_scale=1.01)], pinc, 0xF), ([ctl_each(EM.EACH_ALL, inc_scale=1.0, amp_scale=1.0)], amp, 0xF)]
    seen = set()
    for each, ctls, mask in cases:
        want = EM.each_check(each, ctls, K, mask)
        assert device.ctl_each_check(each, ctls, mask, K) == want, ([hex(e.set) for e in each], mask)
        seen.add(want)
    assert seen == {0, BAD}
    r = ctl_each(EM.EACH_PAN, pan_left=0.5, pan_right=0.5)
    r.reserved[1] = 7
    assert device.ctl_each_check([r], plain, 0xF) == EM.each_check([r], plain, K, 0xF) == BAD
    assert device.ctl_each_check([ok], None, 0x7, 3) == EM.each_check([ok], None, 3, 0x7) == RANGE
    assert device.ctl_each_check([ok], plain[:3] + [ctl(0)], 0xF) == BAD             # what skred_ctl_check refuses about the records
    assert device.load().skred_ctl_each_check(None, 1, None, 4, 0xF) == BAD


def test_entry_points_refuse_a_null_bank():
    L = device.load()
    tags = device.tag_array([1, 2])
    arr = device.ctl_array([ctl(device.CTL_PAN, pan_left=0.5, pan_right=0.5)] * 8)
    each = device.ctl_each_array([ctl_each(device.EACH_PAN, pan_left=0.5, pan_right=0.5)] * 2)
    m = owner_match(0x03000000, 0xFF000000)
    word = C.c_void_p(16)                                    # (a refused call never reads through the device pointers)
    p, e = C.cast(arr, C.c_void_p), C.cast(each, C.c_void_p)
    assert L.skred_bank_find_match(None, 0, 64, 8, C.byref(m), 4, word, word, None) == BAD
    assert L.skred_bank_find_match_host(None, 0, 64, 8, C.byref(m), 0, None, None, None) == BAD
    assert L.skred_bank_stamp_match(None, 0, 64, 8, 0xFF, C.byref(m), REL, word, None) == BAD
    assert L.skred_bank_ctl_match(None, p, 0, 64, 8, 0xFF, C.byref(m), None, None) == BAD
    assert L.skred_bank_ctl_owned_each(None, p, e, 8, 0xFF, word, tags.ctypes.data, 2, None, None, None) == BAD
    assert L.skred_bank_ctl_tags_each(None, p, e, 0, 64, 8, 0xFF, tags.ctypes.data, 2, None, None) == BAD


# ---------------------------------------------------------------------------------------------- the entry points' host checks, the packing

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("expr") / "c_expr_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_expr_host.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"), "-lskred_amd", "-lm", "-lpthread",
           "-Wl,-rpath," + os.path.join(ROOT, "skred_amd")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return out.stdout.strip().splitlines()


@pytest.mark.parametrize("group", ["const", "match", "each", "pack", "perm", "find", "find_host", "stamp", "ctl", "owned", "tags", "bank"])
def test_host_cases(host_lines, group):
    mine = [l for l in host_lines if l.startswith(group + "/")]
    assert mine, f"no case of group {group} ran"
    bad = [l for l in mine if not l.endswith(" ok")]
    assert not bad, "\n".join(bad)


def test_every_host_case_passed(host_lines):
    assert host_lines[-1] == "OK", "\n".join(l for l in host_lines if not l.endswith(" ok"))


# ---------------------------------------------------------------------------------------------- the model

def tagged_owner():
    """128 voices, K = 4: slots 0, 20, 60 on channel 3, slot 100 on channel 4, slot 124 with every bit set, the rest untagged."""
    owner = OM.new(128)
    OM.tag_slots(owner, [0, 20, 60, 100, 124], [0x03000001, 0x03000002, 0x03FFFFFF, 0x04000001, 0xFFFFFFFF], None, 4)
    return owner


def test_model_matches_and_the_list():
    owner = tagged_owner()
    ch = lambda c: (c << 24, 0xFF000000)   # noqa: E731
    lst, total = EM.find_match(owner, 0, 128, 4, *ch(3), 8)
    assert lst.tolist() == [0, 20, 60] and total == 3
    lst, total = EM.find_match(owner, 0, 128, 4, *ch(3), 2)
    assert lst.tolist() == [0, 20] and total == 3                                         # cut short: the count is still the total
    assert EM.find_match(owner, 0, 128, 4, *ch(3), 0)[1] == 3 and len(EM.find_match(owner, 0, 128, 4, *ch(3), 0)[0]) == 0
    assert EM.find_match(owner, 0, 128, 4, 0, 0, 99)[0].tolist() == [0, 20, 60, 100, 124]     # mask 0: every TAGGED slot, no untagged one
    assert EM.find_match(owner, 0, 128, 4, 0xFFFFFFFF, 0xFFFFFFFF, 9)[0].tolist() == [124]
    assert EM.find_match(owner, 0, 128, 4, *ch(0xFF), 9)[0].tolist() == [124]
    assert EM.find_match(owner, 0, 128, 4, *ch(5), 9) [1] == 0                            # a value nobody carries
    assert EM.find_match(owner, 0, 128, 4, 0, 0xFF000000, 9)[1] == 0                      # channel 0: untagged slots do not match
    assert EM.find_match(owner, 24, 80, 4, *ch(3), 9)[0].tolist() == [60]                 # a range inside the bank
    owner[1] = 0x03000009                                                                 # a word that is no slot's first voice
    assert EM.find_match(owner, 0, 128, 4, *ch(3), 9)[1] == 3 and EM.find_match(owner, 0, 128, 1, *ch(3), 9)[0].tolist() == [0, 1, 20, 60]
    with pytest.raises(AssertionError):
        EM.find_match(owner, 0, 128, 4, 1, 0, 9)


def test_model_stamp_match_is_all_notes_off_on_one_channel():
    owner = tagged_owner()
    truth, _, _ = banks.bank_c2(128)
    e = truth["voice_amp_envelope"]
    e["is_active"][:] = 1
    e["sample_release"][:] = 0
    res, voices = EM.stamp_match(owner, truth, 0, 128, 4, 0b0101, 0x03000000, 0xFF000000, REL, 777)
    assert res == [3, 29] and voices.tolist() == [0, 2, 20, 22, 60, 62]
    assert (e["sample_release"][voices] == 777).all() and int((e["sample_release"] != 0).sum()) == 6
    res, voices = EM.stamp_match(owner, truth, 64, 64, 4, 0b1111, 0, 0, REL, 778)
    assert res == [2, 14] and voices.tolist() == list(range(100, 104)) + list(range(124, 128))


def test_model_ctl_match_and_the_bound():
    owner = tagged_owner()
    bank, _, _ = banks.bank_c2(128)
    bank["voice_amp"][22] = 0.0
    a = bank.copy()
    recs = [ctl(CM.PAN | CM.AMP, pan_left=0.1 * l, pan_right=0.9, amp=0.5) for l in range(4)]
    res, touched = EM.ctl_match(owner, (a,), recs, 0, 128, 0b0110, 0x03000000, 0xFF000000)
    assert res == [6, 1, 29] and touched.tolist() == [1, 2, 21, 22, 61, 62]
    assert a["voice_amp"][22] == 0 and a["voice_amp"][21] == np.float32(0.5) and a["voice_pan_right"][100] == bank["voice_pan_right"][100]
    assert EM.lists_range(recs, 0b0110, 0, 128) == 32 * 2
    filt = [ctl(CM.FILTER, b0=0.5) for _ in range(4)]
    assert EM.lists_range(filt, 0b1111, 0, 128) == 0                                      # a filter sweep lists nobody


def test_model_per_entry_values():
    owner = tagged_owner()
    bank, _, _ = banks.bank_c2(128)
    bank["voice_amp"][:] = np.float32(0.8)
    bank["voice_amp"][21] = 0.0
    bank["voice_phase_inc"][60:64] = np.float32(3e38)
    a = bank.copy()
    recs = [ctl(CM.AMP | CM.VELOCITY | CM.FILTER, amp=0.5 + 0.1 * l, velocity=0.9, b0=0.25) for l in range(4)]
    each = [ctl_each(EM.EACH_AMP_SCALE | EM.EACH_INC_SCALE, amp_scale=0.5, inc_scale=1.5),
            ctl_each(EM.EACH_VELOCITY | EM.EACH_PAN, velocity=0.1, pan_left=0.2, pan_right=0.3),
            ctl_each(EM.EACH_AMP_SCALE | EM.EACH_INC_SCALE, amp_scale=1e-45, inc_scale=2.0),
            ctl_each(EM.EACH_PAN, pan_left=0.7, pan_right=0.7), ctl_each(EM.EACH_PAN, pan_left=0.7, pan_right=0.7)]
    entries, tags = [0, 20, 60, 100, -1], [0x03000001, 0x03000002, 0x03FFFFFF, 0x04000009, 5]
    res, touched = EM.ctl_owned_each(owner, (a,), recs, each, 4, 0b0011, entries, tags, None)
    # entry 0: both voices written; entry 1: voice 21 has amp 0 (withheld); entry 2: 3e38 * 2 overflows on both voices, 0.5 * 1e-45
    # rounds to 0 on voice 60 (withheld) and 0.6 * 1e-45 to the smallest subnormal on voice 61 (stored); entry 3: the owner
    # differs; entry 4: no slot
    assert res == [6, 1 + 3, 1] and touched.tolist() == [0, 1, 20, 21, 60, 61]
    assert a["voice_amp"][61] == np.float32(1e-45) and a["voice_amp"][61] != 0
    assert a["voice_amp"][0] == np.float32(0.5) * np.float32(0.5) and a["voice_amp"][1] == np.float32(0.6) * np.float32(0.5)
    assert a["voice_phase_inc"][0] == bank["voice_phase_inc"][0] * np.float32(1.5)
    assert a["voice_amp_envelope"]["velocity"][0] == np.float32(0.9) and a["voice_amp_envelope"]["velocity"][20] == np.float32(0.1)
    assert a["voice_pan_left"][20] == np.float32(0.2) and a["voice_pan_left"][0] == bank["voice_pan_left"][0]
    assert a["voice_amp"][20] == np.float32(0.5) and a["voice_amp"][21] == 0
    assert a["voice_amp"][60] == np.float32(0.8) and a["voice_phase_inc"][60] == np.float32(3e38)     # withheld: both kept
    assert a["voice_filter"]["b0"][60] == np.float32(0.25) and a["voice_filter"]["b0"][100] == bank["voice_filter"]["b0"][100]
    assert a["voice_amp"][2:4].tobytes() == bank["voice_amp"][2:4].tobytes()                          # outside voice_mask
    # no base records: the entries supply everything
    b = bank.copy()
    res, touched = EM.ctl_owned_each(owner, (b,), None, each[1:2], 4, 0b1000, [20], [0x03000002], None)
    assert res == [1, 0, 0] and touched.tolist() == [23] and b["voice_amp_envelope"]["velocity"][23] == np.float32(0.1)
    assert EM.lists_each(None, each[3:], 4, 0b0011, 2) == 0 and EM.lists_each(None, each[1:2], 4, 0b0011, 1) == 2
    assert EM.lists_each(recs, each[3:], 4, 0b0011, 2) == 4


def test_model_tags_each_keeps_each_entry_with_its_tag():
    owner = tagged_owner()
    bank, _, _ = banks.bank_c2(128)
    tags = np.array([0xFFFFFFFF, 0x03000002, 0x55, 0x03000001], np.uint32)
    each = [ctl_each(EM.EACH_VELOCITY, velocity=0.1 * (k + 1)) for k in range(4)]
    srt, permuted, perm = EM.pack(tags, each)
    assert srt.tolist() == [0x55, 0x03000001, 0x03000002, 0xFFFFFFFF] and perm.tolist() == [2, 3, 1, 0]
    assert [round(float(e.velocity), 1) for e in permuted] == [0.3, 0.4, 0.2, 0.1]
    a, b = bank.copy(), bank.copy()
    res, touched, lst = EM.ctl_tags_each(owner, (a,), None, each, 0, 128, 4, 0b0001, tags)
    assert res == [3, 0, 0] and lst.tolist() == [124, 20, -1, 0] and touched.tolist() == [0, 20, 124]
    v = a["voice_amp_envelope"]["velocity"]
    assert v[124] == np.float32(0.1) and v[20] == np.float32(0.2) and v[0] == np.float32(0.4)
    # the sorted route stores the same bytes
    res2, _, _ = EM.ctl_tags_each(owner, (b,), None, permuted, 0, 128, 4, 0b0001, srt)
    assert res2 == res and b["voice_amp_envelope"].tobytes() == a["voice_amp_envelope"].tobytes()


# ---------------------------------------------------------------------------------------------- the channel scene

def test_the_channel_scene_on_the_oracle():
    """Channels A and B share the range; the bank fills and B steals six of A's slots.  All notes off on A then releases exactly A's two
    survivors and none of B's notes; B's sweep and B's bends land on B alone."""
    st = XS.Story()
    a_assigned, tagged = st.chord_a()
    assert tagged == [8, 0]
    st.block()
    assert st.fill_up() == [56, 0]
    st.block()
    assert len(SM.idle_slots(st.truth, 0, XS.N, XS.K, S.MMASK, S.WHICH, S.SETTLE)) == 0     # the bank is full
    b_assigned, counts, tagged = st.chord_b()
    assert counts == (S.B_COUNT, 0, S.B_COUNT) and tagged == [S.B_COUNT, 0]
    stolen = set(b_assigned.tolist()) & set(a_assigned.tolist())
    assert len(stolen) == S.B_COUNT
    survivors = sorted(set(a_assigned.tolist()) - stolen)
    assert st.count(XS.CH_A)[0].tolist() == survivors and st.count(XS.CH_A)[1] == 2
    assert st.count(XS.CH_B)[0].tolist() == sorted(b_assigned.tolist()) and st.count(XS.CH_C)[1] == 56 and st.count(0x0D)[1] == 0
    before = st.truth["voice_amp_envelope"]["sample_release"].copy()
    res, voices = st.a_all_notes_off()
    assert res == [2, 62] and sorted(voices.tolist()) == [s + l for s in survivors for l in range(XS.K)]
    rel = st.truth["voice_amp_envelope"]["sample_release"]
    b_voices = np.concatenate([np.arange(s, s + XS.K) for s in b_assigned])
    assert (rel[b_voices] == 0).all() and set(np.flatnonzero(rel != before).tolist()) <= set(voices.tolist())
    st.block()
    snap = st.truth.copy()
    res, touched = st.b_sweep()
    assert res == [S.B_COUNT * 3, 0, 64 - S.B_COUNT] and set(touched.tolist()) <= set(b_voices.tolist())
    res, touched, lst = st.b_bends()
    assert res == [S.B_COUNT * 3, 0, 0] and np.array_equal(lst, b_assigned) and set(touched.tolist()) <= set(b_voices.tolist())
    others = np.setdiff1d(np.arange(XS.N), b_voices)
    for field, sub in CM.CTL_WORDS:
        assert CM.word(st.truth, field, sub)[others].tobytes() == CM.word(snap, field, sub)[others].tobytes(), (field, sub)
    # every note of B got ITS bend: the entry stayed with its tag although the tags travel sorted
    for k, s in enumerate(b_assigned):
        want = snap["voice_phase_inc"][s] * np.float32(XS.bends()[k].inc_scale)
        assert st.truth["voice_phase_inc"][s] == want and st.truth["voice_amp_envelope"]["velocity"][s] == np.float32(0.4 + 0.1 * k)
    st.block()
