"""Note owners without a GPU: the constants and symbols against the header, every refusal beside the accepted edge and the
sort-plus-permutation packing (through tests/c_owner_host.c, a program of its own on a bank that is nothing but its size), the model's
self-checks (tests/owner_model.py is what tests/test_owner.py holds the device to), and the theft scene of the GPU tests on the
oracle's state: it really steals, and the reference placement alone drops no note of chord B."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import owner_model as OM
import owner_scenes as S
import slot_model as SM
from skred_amd import banks, device
from skred_amd.device import ctl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
REL, TRIG = SM.STAMP_RELEASE, SM.STAMP_TRIGGER
OWNER_CALLS = ("skred_bank_tag_slots", "skred_bank_find_owned", "skred_bank_stamp_owned", "skred_bank_release_tags",
               "skred_bank_ctl_owned", "skred_bank_owner_clear", "skred_bank_download_owners", "skred_bank_download_env_clocks")


# ---------------------------------------------------------------------------------------------- the header, the symbols

def test_constants_and_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    assert int(re.search(r"#define\s+SKRED_OWNER_MAX_TAGS\s+(\d+)", text).group(1)) == device.OWNER_MAX_TAGS == OM.MAX_TAGS == 1024
    flags = dict(re.findall(r"SKRED_OWNER_(ALLOW_ZERO|UNIQUE)\s*=\s*1u << (\d)", text))
    assert 1 << int(flags["ALLOW_ZERO"]) == device.OWNER_ALLOW_ZERO == OM.ALLOW_ZERO
    assert 1 << int(flags["UNIQUE"]) == device.OWNER_UNIQUE == OM.UNIQUE
    launch = open(os.path.join(CSRC, "skred_launch.h")).read()
    assert int(re.search(r"#define\s+SK_OWNER_MAX_TAGS\s+(\d+)", launch).group(1)) == 1024
    L = device.load()
    for s in OWNER_CALLS:
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s) and s in device.ABI_SYMBOLS, s
    assert hasattr(L, "skred_owner_tags_check") and "skred_owner_tags_check" in device.HOST_ABI_SYMBOLS
    # what the section promises to stay out of
    section = text[text.index("---- note owners"):text.index("---- voices sharded")]
    for word in ("fixed-point bank", "drop-in mode", "deferred items and pattern steps", "skred_shard_bank()"):
        assert word in section, word


def test_tags_check_is_the_models():
    big = list(range(1, 1026))
    cases = [([5, 2**31], 0), ([5, 0], 0), ([5, 0], OM.ALLOW_ZERO), ([9, 5, 9], OM.UNIQUE), ([9, 5, 9], 0), ([0xFFFFFFFF, 1], OM.UNIQUE),
             (big[:1024], OM.UNIQUE), (big, OM.UNIQUE), (big, 0), ([], OM.UNIQUE), ([1], 4), ([0, 0], OM.ALLOW_ZERO | OM.UNIQUE),
             ([0, 7], OM.ALLOW_ZERO | OM.UNIQUE)]
    for tags, flags in cases:
        assert device.owner_tags_check(tags, flags) == OM.tags_check(tags, flags), (tags[:4], flags)
    assert device.load().skred_owner_tags_check(None, 1, 0) == BAD


def test_entry_points_refuse_a_null_bank():
    L = device.load()
    tags = device.tag_array([1, 2])
    arr = device.ctl_array([ctl(device.CTL_PAN, pan_left=0.5, pan_right=0.5)] * 8)
    word = C.c_void_p(16)                                    # (a refused call never reads through the device pointers)
    assert L.skred_bank_tag_slots(None, word, tags.ctypes.data, 2, None, 8, None, None) == BAD
    assert L.skred_bank_find_owned(None, 0, 64, 8, tags.ctypes.data, 2, word, None) == BAD
    assert L.skred_bank_stamp_owned(None, word, tags.ctypes.data, 2, None, 8, 0xFF, REL, word, None) == BAD
    assert L.skred_bank_release_tags(None, 0, 64, 8, 0xFF, tags.ctypes.data, 2, REL, word, None) == BAD
    assert L.skred_bank_ctl_owned(None, C.cast(arr, C.c_void_p), 8, 0xFF, word, tags.ctypes.data, 2, None, None, None) == BAD
    assert L.skred_bank_owner_clear(None, 0, 8, None) == BAD
    assert L.skred_bank_download_owners(None, word, 0, 8) == BAD
    assert L.skred_bank_download_env_clocks(None, None, None, 0, 8) == BAD


# ---------------------------------------------------------------------------------------------- the entry points' host checks, the packing

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("owner") / "c_owner_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_owner_host.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"), "-lskred_amd", "-lm", "-lpthread",
           "-Wl,-rpath," + os.path.join(ROOT, "skred_amd")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return out.stdout.strip().splitlines()


@pytest.mark.parametrize("group", ["const", "check", "pack", "tag", "find", "stamp", "release", "ctl", "clear", "download", "bank"])
def test_host_cases(host_lines, group):
    mine = [l for l in host_lines if l.startswith(group + "/")]
    assert mine, f"no case of group {group} ran"
    bad = [l for l in mine if not l.endswith(" ok")]
    assert not bad, "\n".join(bad)


def test_every_host_case_passed(host_lines):
    assert host_lines[-1] == "OK", "\n".join(l for l in host_lines if not l.endswith(" ok"))


# ---------------------------------------------------------------------------------------------- the model

def test_model_pack_sorts_unsigned():
    for n in (1, 2, 1023, 1024):
        rng = np.random.default_rng(n)
        tags = rng.choice(np.arange(1, 2**32, 65537, dtype=np.uint64), n, replace=False).astype(np.uint32)
        tags[0] = 0xFFFFFFFF
        srt, perm = OM.pack(tags)
        assert (np.diff(srt.astype(np.int64)) > 0).all() and np.array_equal(tags[perm], srt) and sorted(perm.tolist()) == list(range(n))
        assert srt[-1] == 0xFFFFFFFF and perm[-1] == 0 and (n == 1 or (srt >= 2**31).any())


def test_model_owner_array_is_a_function_of_the_calls():
    n, K = 64, 8
    owner = OM.new(n)
    entries = np.array([8, -1, 12, 64, 56, 0, 2**31 - 8], np.int32)
    tags = [11, 12, 13, 14, 0x80000005, 16, 17]
    assert OM.tag_slots(owner, entries, tags, None, K) == [3, 4]
    want = np.zeros(n, np.uint32)
    want[[8, 56, 0]] = [11, 0x80000005, 16]
    assert np.array_equal(owner, want)
    assert OM.tag_slots(owner, entries, [21, 22, 23, 24, 25, 26, 27], 1, K) == [1, 0] and owner[8] == 21 and owner[56] == 0x80000005
    assert OM.tag_slots(owner, entries, [0], None, K) == [1, 0] and owner[8] == 0           # tag 0 clears
    with pytest.raises(AssertionError):
        OM.tag_slots(owner, [8, 8], [1, 2], None, K)
    OM.clear(owner, 0, 8)
    assert owner[0] == 0 and owner[56] == 0x80000005
    # ranges of different K in one bank: the word at a slot's FIRST voice, whatever K
    OM.tag_slots(owner, [16, 17, 18], [5, 6, 7], None, 1)
    assert OM.find_owned(owner, 16, 8, 1, [7, 6, 5]).tolist() == [18, 17, 16] and OM.find_owned(owner, 16, 8, 8, [5, 6]).tolist() == [16, -1]


def test_model_lowest_match_and_the_range():
    n, K = 128, 4
    owner = OM.new(n)
    OM.tag_slots(owner, [100, 20, 60, 124, 0], [9, 9, 0xFFFFFFFF, 3, 4], None, K)          # (two slots carry tag 9)
    assert OM.find_owned(owner, 0, n, K, [9, 0xFFFFFFFF, 3, 4, 77]).tolist() == [20, 60, 124, 0, -1]
    assert OM.find_owned(owner, 24, 80, K, [9, 4, 3]).tolist() == [100, -1, -1]            # carried only outside the range: -1
    assert OM.find_owned(owner, 20, 4, K, [9]).tolist() == [20]
    truth, _, _ = banks.bank_c2(n)
    e = truth["voice_amp_envelope"]
    e["is_active"][:] = 1
    e["sample_release"][:] = 0
    res, voices, lst = OM.release_tags(owner, truth, 0, n, K, 0b0101, [9, 5, 3], REL, 777)
    assert res == [2, 0, 1] and lst.tolist() == [20, -1, 124] and voices.tolist() == [20, 22, 124, 126]
    rel = e["sample_release"]
    assert (rel[[20, 22, 124, 126]] == 777).all() and int((rel != 0).sum()) == 4           # the higher slot with tag 9 is not stamped


def test_model_guard_and_counts():
    n, K = 64, 8
    owner = OM.new(n)
    OM.tag_slots(owner, [0, 8, 16], [1, 2, 3], None, K)
    truth, _, _ = banks.bank_c2(n)
    e = truth["voice_amp_envelope"]
    e["is_active"][:] = 1
    e["sample_release"][:] = 0
    entries = np.array([0, 8, -1, 16, 24, 12, 64, 16], np.int32)
    tags = [1, 9, 5, 3, 4, 6, 7, 3]
    res, voices = OM.stamp_owned(owner, truth.copy(), entries, tags, None, K, 0x81, REL, 5)
    assert res == [3, 2, 3] and voices.tolist() == [0, 7, 16, 23, 16, 23]                  # 24 is untagged: a miss, never a match
    res, voices = OM.stamp_owned(owner, truth.copy(), entries, tags, 2, K, 0x81, REL, 5)
    assert res == [1, 1, 0] and sum(res) == 2                                              # a count shorter than n
    OM.tag_slots(owner, [0], [0], None, K)
    res, voices = OM.stamp_owned(owner, truth, entries, tags, 1, K, 0x81, REL, 5)
    assert res == [0, 1, 0] and len(voices) == 0 and int((e["sample_release"] != 0).sum()) == 0
    with pytest.raises(AssertionError):
        OM.stamp_owned(owner, truth, entries, [0] * 8, None, K, 0x81, REL, 5)              # tags are non-zero


def test_model_ctl_owned_leaves_a_stolen_slot_alone():
    n, K = 64, 4
    bank, _, _ = banks.bank_c2(n)
    owner = OM.new(n)
    OM.tag_slots(owner, [0, 4, 8], [1, 2, 3], None, K)
    OM.tag_slots(owner, [4], [99], None, K)                                                # slot 4 is stolen
    a = bank.copy()
    recs = [ctl(device.CTL_PAN | device.CTL_AMP, pan_left=0.1 * l, pan_right=0.9, amp=0.5) for l in range(K)]
    res, touched = OM.ctl_owned(owner, (a,), recs, 0b1011, [0, 4, 8, -1], [1, 2, 3, 4], None)
    zero = int((bank["voice_amp"][touched] == 0).sum())
    assert res == [6, zero, 1] and touched.tolist() == [0, 1, 3, 8, 9, 11]
    assert a["voice_pan_left"][4:8].tobytes() == bank["voice_pan_left"][4:8].tobytes()
    assert a["voice_pan_right"][0] == np.float32(0.9) and a["voice_pan_right"][2] == bank["voice_pan_right"][2]


# ---------------------------------------------------------------------------------------------- the theft scene

def test_the_theft_scene_really_steals():
    """On the oracle alone: chord A fills the idle slots, the rest is played again, chord B finds no idle slot, steals A's six oldest
    slots and DROPS NOTHING; A's note-off then misses exactly those six, and B's release by tag stamps exactly B."""
    st = S.Story()
    a_assigned, tagged = st.chord_a()
    assert sorted(a_assigned.tolist()) == sorted(S.A_SLOTS.tolist()) and tagged == [8, 0]
    assert len(SM.idle_slots(st.truth, 0, S.N, S.K, S.MMASK, S.WHICH, S.SETTLE)) == 0       # the bank is full
    st.block()
    assert st.fill_up() == [56, 0]
    st.block()
    assert len(SM.idle_slots(st.truth, 0, S.N, S.K, S.MMASK, S.WHICH, S.SETTLE)) == 0
    b_assigned, counts, tagged = st.chord_b()
    assert counts == (S.B_COUNT, 0, S.B_COUNT) and tagged == [S.B_COUNT, 0]                # every note placed, every one on a victim
    assert set(b_assigned.tolist()) <= set(a_assigned.tolist()) and (b_assigned >= 0).all()
    stolen = len(set(b_assigned.tolist()) & set(a_assigned.tolist()))
    assert stolen == S.B_COUNT
    before = st.truth["voice_amp_envelope"]["sample_release"].copy()
    res, voices = st.a_off()
    assert res == [len(a_assigned) - stolen, stolen, 0]
    rel = st.truth["voice_amp_envelope"]["sample_release"]
    b_voices = np.concatenate([np.arange(s, s + S.K) for s in b_assigned])
    assert (rel[b_voices] == 0).all() and len(voices) == (len(a_assigned) - stolen) * 4
    changed = np.flatnonzero(rel != before)
    assert len(changed) >= (len(a_assigned) - stolen) * 3 and set(changed.tolist()) <= set(voices.tolist())   # A's two survivors only
    st.block()
    res, voices, lst = st.b_off()
    assert res == [S.B_COUNT, 0, 0] and np.array_equal(lst, b_assigned) and sorted(voices.tolist()) == sorted(b_voices.tolist())
    # an unguarded note-off of A would have released B: that is the hole
    assert set(SM.stamp_voices(a_assigned, len(a_assigned), None, S.K, S.VMASK, S.N).tolist()) >= set(b_voices.tolist())
