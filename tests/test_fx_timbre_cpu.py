"""Per-note timbre on the fixed-point bank without a GPU: the record and the symbols against the header,
skred_fx_filter_each_check against the model, the fixed-point groups of tests/c_timbre_host.c (every refusal with its return code,
the packing, the permutation with the sorted tags for n = 1, 2, 1023 and 1024), the model (tests/fx_timbre_model.py is what
tests/test_fx_timbre.py holds the device to) against a brute-force loop over every voice, and three notes with three cutoffs on
oracle.cpuref.fx_render alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fx_ctl_model as cm
import fx_expr_model as em
import fx_owner_model as om
import fx_timbre_model as tm
from oracle import cpuref
from skred_amd import device, fxbank as fxb
from skred_amd.fxbank import fx_ctl, fx_each, fx_filter_each
from test_timbre_cpu import group_passed, host_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = -2
CALLS = ("skred_fxbank_ctl_owned_each_filter", "skred_fxbank_ctl_tags_each_filter")


def test_fx_filter_record_and_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd_fxpt.h")).read()
    assert C.sizeof(fxb.FxFilterEachC) == 32
    body = re.search(r"typedef struct skred_fx_filter_each \{(.*?)\} skred_fx_filter_each_t;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in fxb.FxFilterEachC._fields_], names
    L = device.load()
    for s in CALLS:
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s) and s in fxb.FX_ABI_SYMBOLS, s
    assert hasattr(L, "skred_fx_filter_each_check") and "skred_fx_filter_each_check" in fxb.FX_HOST_ABI_SYMBOLS


def test_fx_filter_check_is_the_models():
    pan, names, bad = fx_ctl(fxb.CTL_PAN, pan_left_q15=1, pan_right_q15=2), fx_ctl(fxb.CTL_PAN | fxb.CTL_FILTER), fx_ctl(0)
    ok = [fx_filter_each(1, -2, 3, -(1 << 31), (1 << 31) - 1)]
    resv = fx_filter_each(1, 2, 3, 4, 5)
    resv.reserved[2] = 1
    cases = [(ok, pan, None), (ok, None, None), (ok, names, None), (ok, bad, None), ([resv], None, None), (ok + [resv], pan, None),
             (ok + [resv], pan, 1), (None, pan, None), (ok, pan, -1), ([], None, None)]
    verdicts = [fxb.fx_filter_each_check(f, c, n) for f, c, n in cases]
    assert verdicts == [tm.filter_check(f, c, n) for f, c, n in cases]
    assert verdicts == [0, 0, BAD, BAD, BAD, BAD, 0, BAD, BAD, 0]


def test_fx_timbre_entry_points_refuse_a_null_bank():
    L = fxb._bind(device.load())
    f = C.cast(fxb.fx_filter_each_array([fx_filter_each(1, 2, 3, 4, 5)]), C.c_void_p)
    tags, word = np.array([1, 2], np.uint32), C.c_void_p(16)
    assert L.skred_fxbank_ctl_owned_each_filter(None, None, None, f, word, tags.ctypes.data, 1, None, None, None) == BAD
    assert L.skred_fxbank_ctl_tags_each_filter(None, None, None, f, 0, 8, tags.ctypes.data, 1, None, None) == BAD


@pytest.mark.parametrize("group", ["fxcheck", "pack", "perm", "fxowned", "fxtags", "fxplain", "fxbank"])
def test_fx_timbre_host_cases(group):
    group_passed(group)
    assert host_lines()[-1] == "OK"


def tagged_bank(n=24):
    b, pool, c0 = fxb.bank_fx(n)
    b["amp_q15"][[2, 9]] = 0
    owner = om.new(n)
    om.tag_list(owner, np.arange(n), 100 + np.arange(n))
    return b, pool, c0, owner


def test_fx_model_equals_a_loop_over_every_voice():
    b, _, _, owner = tagged_bank()
    voices = np.array([3, 9, -1, 17, 24, 2, 11, 5], np.int32)
    tags = np.array([103, 109, 7, 117, 124, 999, 111, 105], np.uint32)                            # voice 2's tag is stale
    filt = [fx_filter_each(1000 + k, -2000 - k, 3000 + k, -(1 << 31) + k, (1 << 31) - 1 - k) for k in range(8)]
    base = fx_ctl(fxb.CTL_AMP | fxb.CTL_SMOOTHING, amp_q15=20000, smoother_k_q15=77)
    entries = [fx_each((fxb.EACH_INC_SCALE, fxb.EACH_AMP_SCALE, fxb.EACH_VELOCITY, fxb.EACH_PAN)[k % 4], inc_scale_q16=65536 + k,
                       amp_scale_q16=1 if k == 1 else 40000, velocity_q15=k, pan_left_q15=k, pan_right_q15=2 * k) for k in range(8)]
    for c, ee, count in ((base, entries, None), (None, None, None), (None, None, 4), (base, None, 6)):
        model = b.copy()
        res = tm.ctl_owned_each_filter(owner, model, c, ee, filt, voices, tags, count)
        want, written, withheld, differs = b.copy(), 0, 0, 0
        m = len(tags) if count is None else count
        for v in range(b.n):                                                                      # every voice of the bank in turn
            for k in range(m):
                if int(voices[k]) != v:
                    continue
                if owner[v] != tags[k]:
                    differs += 1
                    continue
                written += 1
                if ee is not None or c is not None:
                    r, w = em.overlay(c, ee[k]) if ee is not None else (c, 0)
                    withheld += w + (cm.store(want, r, v) if r is not None else 0)
                for name in tm.COEFFS:
                    want[name][v] = getattr(filt[k], name)
        assert res == [written, withheld, differs], (res, written, withheld, differs)
        assert all(np.array_equal(model[k], want[k]) for k in b.a), [k for k in b.a if not np.array_equal(model[k], want[k])]
        if c is None and ee is None:
            changed = sorted(k for k in b.a if not np.array_equal(model[k], b[k]))
            assert changed == sorted(tm.COEFFS) and res == ([5, 0, 1] if count is None else [3, 0, 0])
        assert all(np.array_equal(model[k], b[k]) for k in ("x1", "x2", "y1", "y2", "filter_mode"))
    # by note id: each set stays beside its tag through the sort
    model = b.copy()
    res, lst = tm.ctl_tags_each_filter(owner, model, None, None, filt[:3], 0, b.n, np.array([120, 555, 101], np.uint32))
    assert res == [2, 0, 0] and lst.tolist() == [20, -1, 1] and model["b0_q30"][20] == 1000 and model["b0_q30"][1] == 1002


def test_fx_three_notes_three_cutoffs_on_the_oracle():
    """Three voices in the same state render the same stems; three cutoffs by note id through the model: three different stems, each
    equal to a bank whose host view was given those words directly."""
    b, pool, c0 = fxb.bank_fx(8)
    for k in b.a:
        b[k][1], b[k][2] = b[k][0], b[k][0]                                                       # voices 0, 1, 2: one voice three times
    assert b["filter_mode"][0] != 0
    owner = om.new(8)
    om.tag_list(owner, [0, 1, 2], [0x03000043, 0x0300003C, 0x03000040])
    filt = [fx_filter_each(*[tm.q30(x) for x in device.filter_coeffs(1, f, 0.9, 48000.0)]) for f in (400.0, 1600.0, 6400.0)]
    plain, through_model, direct = b.copy(), b.copy(), b.copy()
    res, lst = tm.ctl_tags_each_filter(owner, through_model, None, None, filt, 0, 8, np.array([0x03000043, 0x0300003C, 0x03000040], np.uint32))
    assert res == [3, 0, 0] and lst.tolist() == [0, 1, 2]
    for v in range(3):
        for name in tm.COEFFS:
            direct[name][v] = getattr(filt[v], name)

    def stems_of(bank):
        _, st, cnt = cpuref.fx_render(bank, pool, c0, 64, 1, want_stems=True)
        _, st2, _ = cpuref.fx_render(bank, pool, cnt, 64, 1, want_stems=True)
        return np.concatenate([st, st2])

    s0, sa, sb = stems_of(plain), stems_of(through_model), stems_of(direct)
    assert np.array_equal(s0[:, 0], s0[:, 1]) and np.array_equal(s0[:, 0], s0[:, 2]) and np.abs(s0[:, 0]).sum() > 0
    assert np.array_equal(sa, sb)
    assert len({sa[:, v].tobytes() for v in range(3)}) == 3 and all(not np.array_equal(sa[:, v], s0[:, v]) for v in range(3))
    assert np.array_equal(sa[:, 3:], s0[:, 3:]), "the other voices heard nothing"
