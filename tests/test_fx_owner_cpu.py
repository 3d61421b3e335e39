"""Note owners of the fixed-point bank without a GPU: the symbols against the header, every refusal beside the accepted edge and the
sort-plus-permutation of the tags (through tests/c_fx_ctl_host.c, a program of its own on a bank that is nothing but its size), the
model's self-checks (tests/fx_owner_model.py is what tests/test_fx_owner.py holds the device to), and the theft scene of the GPU
tests on the oracle's state: it really steals, the unguarded note-off really releases the thieves, the guarded ones nobody."""
import os
import re

import numpy as np
import pytest

import fx_host_cases
import fx_owner_model as om
import fx_owner_scenes as sc
from skred_amd import device, fxbank as fxb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = -2
REL, TRIG = fxb.STAMP_RELEASE, fxb.STAMP_TRIGGER
OWNER_CALLS = ("skred_fxbank_tag_list", "skred_fxbank_find_owned", "skred_fxbank_stamp_owned", "skred_fxbank_release_tags",
               "skred_fxbank_owner_clear", "skred_fxbank_download_owners", "skred_fxbank_download_params")


def test_fx_owner_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd_fxpt.h")).read()
    L = device.load()
    for s in OWNER_CALLS:
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s) and s in fxb.FX_ABI_SYMBOLS, s
    assert (fxb.OWNER_MAX_TAGS, fxb.OWNER_ALLOW_ZERO, fxb.OWNER_UNIQUE) == (device.OWNER_MAX_TAGS, device.OWNER_ALLOW_ZERO, device.OWNER_UNIQUE)
    section = text[text.index("---- note owners and controllers"):text.index("Same on host buffers")]
    for word in ("NO SLOTS", "K > 1", "skred_fxshard_bank()", "sk_fx_render_kernel never reads it", "skred_owner_tags_check"):
        assert word in section, word
    float_header = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    owners = float_header[float_header.index("---- note owners"):float_header.index("---- voices sharded")]
    assert "skred_fxbank_tag_list" in owners and "Not in the fixed-point bank" not in owners


def test_fx_owner_entry_points_refuse_a_null_bank():
    import ctypes as C
    L = fxb._bind(device.load())
    tags = np.array([1, 2], np.uint32)
    word = C.c_void_p(16)                                    # (a refused call never reads through the device pointers)
    assert L.skred_fxbank_tag_list(None, word, tags.ctypes.data, 2, None, None, None) == BAD
    assert L.skred_fxbank_find_owned(None, 0, 64, tags.ctypes.data, 2, word, None) == BAD
    assert L.skred_fxbank_stamp_owned(None, word, tags.ctypes.data, 2, None, REL, word, None) == BAD
    assert L.skred_fxbank_release_tags(None, 0, 64, tags.ctypes.data, 2, REL, word, None) == BAD
    assert L.skred_fxbank_owner_clear(None, 0, 8, None) == BAD
    assert L.skred_fxbank_download_owners(None, word, 0, 8) == BAD
    assert L.skred_fxbank_download_params(None, None, None, 0, 0, 8) == BAD


@pytest.mark.parametrize("group", ["sort", "tag", "find", "stamp", "release", "clear", "download", "bank"])
def test_fx_owner_host_cases(group):
    fx_host_cases.group(group)


def test_fx_every_host_case_passed():
    lines = fx_host_cases.lines()
    assert lines[-1] == "OK", "\n".join(l for l in lines if not l.endswith(" ok"))


# ---------------------------------------------------------------------------------------------- the model

def test_fx_model_tags_check_is_the_librarys():
    big = list(range(1, 1026))
    cases = [([5, 2**31], 0), ([5, 0], 0), ([5, 0], om.ALLOW_ZERO), ([9, 5, 9], om.UNIQUE), ([9, 5, 9], 0), ([0xFFFFFFFF, 1], om.UNIQUE),
             (big[:1024], om.UNIQUE), (big, om.UNIQUE), (big, 0), ([], om.UNIQUE), ([1], 4), ([0, 7], om.ALLOW_ZERO | om.UNIQUE)]
    for tags, flags in cases:
        assert device.owner_tags_check(tags, flags) == om.tags_check(tags, flags), (tags[:4], flags)


def test_fx_model_pack_sorts_unsigned():
    for n in (1, 2, 3, 1023, 1024):
        rng = np.random.default_rng(n)
        tags = rng.choice(np.arange(1, 2**32, 65537, dtype=np.uint64), n, replace=False).astype(np.uint32)
        tags[0] = 0xFFFFFFFF
        srt, perm = om.pack(tags)
        assert (np.diff(srt.astype(np.int64)) > 0).all() and np.array_equal(tags[perm], srt) and sorted(perm.tolist()) == list(range(n))
        assert srt[-1] == 0xFFFFFFFF and perm[-1] == 0


def test_fx_model_owner_array_is_a_function_of_the_calls():
    n = 64
    owner = om.new(n)
    entries = np.array([8, -1, 12, 64, 56, 0, 2**31 - 8], np.int32)
    tags = [11, 12, 13, 14, 0x80000005, 16, 17]
    assert om.tag_list(owner, entries, tags) == [4, 3]
    want = np.zeros(n, np.uint32)
    want[[8, 12, 56, 0]] = [11, 13, 0x80000005, 16]
    assert np.array_equal(owner, want)
    assert om.tag_list(owner, entries, [21, 22, 23, 24, 25, 26, 27], 1) == [1, 0] and owner[8] == 21 and owner[12] == 13
    assert om.tag_list(owner, entries, [0]) == [1, 0] and owner[8] == 0                    # tag 0 clears
    with pytest.raises(AssertionError):
        om.tag_list(owner, [8, 8], [1, 2])
    om.clear(owner, 0, 8)
    assert owner[0] == 0 and owner[56] == 0x80000005


def test_fx_model_lowest_match_guard_and_counts():
    n = 128
    owner = om.new(n)
    om.tag_list(owner, [100, 20, 60, 124, 0], [9, 9, 0xFFFFFFFF, 3, 4])                     # (two voices carry tag 9)
    assert om.find_owned(owner, 0, n, [9, 0xFFFFFFFF, 3, 4, 77]).tolist() == [20, 60, 124, 0, -1]
    assert om.find_owned(owner, 21, 80, [9, 4, 3]).tolist() == [100, -1, -1]               # carried only outside the range: -1
    assert om.find_owned(owner, 20, 1, [9]).tolist() == [20]
    bank = fxb.FxVoiceBank(n)
    bank["is_active"] = 1
    res, voices, lst = om.release_tags(owner, bank, 0, n, [9, 5, 3], REL, 777)
    assert res == [2, 0, 1] and lst.tolist() == [20, -1, 124] and voices.tolist() == [20, 124]
    assert (bank["sample_release"][[20, 124]] == 777).all() and int((bank["sample_release"] != 0).sum()) == 2
    entries = np.array([0, 20, -1, 60, 24, 128, 60], np.int32)
    tags = [4, 5, 5, 0xFFFFFFFF, 4, 7, 0xFFFFFFFF]
    fresh = fxb.FxVoiceBank(n)
    fresh["is_active"][0] = 1                                                               # (60 is inactive: stamped, no release stored)
    res, voices = om.stamp_owned(owner, fresh, entries, tags, None, REL, 5)
    assert res == [3, 2, 2] and voices.tolist() == [0, 60, 60]                              # 24 is untagged: a miss, never a match
    assert fresh["sample_release"][0] == 5 and fresh["sample_release"][60] == 0
    res, _ = om.stamp_owned(owner, fresh, entries, tags, 2, TRIG, 9)
    assert res == [1, 1, 0] and fresh["sample_start"][0] == 9 and fresh["sample_release"][0] == 0
    with pytest.raises(AssertionError):
        om.stamp_owned(owner, fresh, entries, [0] * 7, None, REL, 5)                        # tags are non-zero


# ---------------------------------------------------------------------------------------------- the theft scene

def reach_the_theft():
    st = sc.Story()
    st.block(sc.WARM)
    a_assigned, counts, tagged = st.chord_a()
    assert sorted(a_assigned.tolist()) == sc.IDLE.tolist() and counts == (sc.CHORD, 0) and tagged == [sc.CHORD, 0]
    st.block()
    b_assigned, counts, tagged = st.chord_b()
    assert counts == (sc.CHORD, 0, sc.CHORD) and tagged == [sc.CHORD, 0]                    # every note placed, every one on a victim
    st.block()
    return st, a_assigned, b_assigned


def test_fx_theft_scene_really_steals():
    """64 voices sounding, chord A's eight tagged voices stolen by chord B: at least one -- here every -- tagged voice is stolen."""
    st, a_assigned, b_assigned = reach_the_theft()
    stolen = set(a_assigned.tolist()) & set(b_assigned.tolist())
    assert len(stolen) >= 1 and len(stolen) == sc.CHORD
    assert sorted(st.owner[sorted(stolen)].tolist()) == sorted(sc.B_TAGS) and not set(sc.A_TAGS) & set(st.owner.tolist())
    assert (st.truth["is_active"] != 0).all() and (st.truth["sample_release"] == 0).all()   # 64 voices sounding, nobody released


def test_fx_theft_unguarded_note_off_releases_the_thieves():
    st, a_assigned, b_assigned = reach_the_theft()
    hit = st.a_off_unguarded(a_assigned)
    assert set(hit.tolist()) == set(b_assigned.tolist())
    assert (st.truth["sample_release"][b_assigned] == st.cnt).all(), "stamp_list on the old d_assigned did not release chord B"


def test_fx_theft_guarded_note_offs_release_nobody():
    st, a_assigned, b_assigned = reach_the_theft()
    before = st.truth.copy()
    res, voices, lst = st.a_off_by_tag()
    assert res == [0, 0, sc.CHORD] and len(voices) == 0 and (lst == -1).all()
    res, voices = st.a_off_guarded(a_assigned)
    assert res == [0, sc.CHORD, 0] and len(voices) == 0
    assert all(np.array_equal(st.truth[k], before[k]) for k in before.a), "a guarded note-off of chord A changed the bank"
    # ... while B's own note-off by id releases exactly B, in B's order
    res, voices, lst = om.release_tags(st.owner, st.truth, 0, sc.N, sc.B_TAGS, REL, st.cnt)
    assert res == [sc.CHORD, 0, 0] and np.array_equal(lst, b_assigned) and np.array_equal(voices, b_assigned)
    assert int((st.truth["sample_release"] != 0).sum()) == sc.CHORD
