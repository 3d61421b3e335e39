"""Controllers of the fixed-point bank without a GPU: the record and the symbols against the header, skred_fx_ctl_check against the
model on every refusal beside the accepted edge, the record's packing and every entry point's refusals (through
tests/c_fx_ctl_host.c), and the model's own edges (tests/fx_ctl_model.py is what tests/test_fx_ctl.py holds the device to): the
INC_SCALE overflow boundary, AMP on an amp of 0, ENV_TIMES with a zero-length stage rendered by the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fx_ctl_model as cm
import fx_host_cases
import fx_owner_model as om
from oracle import cpuref
from skred_amd import device, fxbank as fxb
from skred_amd.fxbank import fx_ctl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = -2
CTL_CALLS = ("skred_fxbank_ctl_range", "skred_fxbank_ctl_list", "skred_fxbank_ctl_owned")


def everything(**kw):
    v = dict(phase_inc=0xDEADBEEF, inc_scale_q16=65536, amp_q15=65535, pan_left_q15=0, pan_right_q15=65535, b0_q30=-(1 << 31),
             b1_q30=(1 << 31) - 1, b2_q30=-1, a1_q30=7, a2_q30=-7, attack_frames=0, decay_frames=1, release_frames=3, sustain_q15=32768,
             velocity_q15=0, smoother_k_q15=32768)
    which = kw.pop("which", fxb.CTL_ALL)
    v.update(kw)
    return fx_ctl(which, **v)


def test_fx_ctl_record_and_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd_fxpt.h")).read()
    float_header = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    assert C.sizeof(fxb.FxCtlC) == 80
    body = re.search(r"typedef struct skred_fx_ctl \{(.*?)\} skred_fx_ctl_t;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in fxb.FxCtlC._fields_], names
    for name, bit in (("PHASE_INC", fxb.CTL_PHASE_INC), ("INC_SCALE", fxb.CTL_INC_SCALE), ("AMP", fxb.CTL_AMP), ("PAN", fxb.CTL_PAN),
                      ("FILTER", fxb.CTL_FILTER), ("ENV_TIMES", fxb.CTL_ENV_TIMES), ("VELOCITY", fxb.CTL_VELOCITY),
                      ("SMOOTHING", fxb.CTL_SMOOTHING)):
        assert 1 << int(re.search(r"SKRED_CTL_%s\s*=\s*1u<<(\d+)" % name, float_header).group(1)) == bit == getattr(device, "CTL_" + name)
    assert fxb.CTL_REFUSED == sum(1 << int(b) for b in re.findall(r"SKRED_CTL_(?:\w+_DEPTH|FREQ_SCALE|CZ_DIST)\s*=\s*1u<<(\d+)", float_header))
    L = device.load()
    for s in CTL_CALLS:
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s) and s in fxb.FX_ABI_SYMBOLS, s
    assert hasattr(L, "skred_fx_ctl_check") and "skred_fx_ctl_check" in fxb.FX_HOST_ABI_SYMBOLS
    ctl_section = float_header[float_header.index("---- patch controllers"):float_header.index("---- note owners")]
    assert "skred_fxbank_ctl_range" in ctl_section and "Not in the fixed-point" not in ctl_section


def test_fx_ctl_check_is_the_models():
    cases = [everything(), everything(which=0), everything(which=1 << 14), everything(which=fxb.CTL_PAN | 1 << 8),
             everything(which=fxb.CTL_PAN | 1 << 13), everything(amp_q15=0), everything(amp_q15=0, which=fxb.CTL_ALL & ~fxb.CTL_AMP),
             everything(amp_q15=1), everything(amp_q15=65536), everything(amp_q15=-1), everything(pan_left_q15=65536),
             everything(pan_right_q15=-1), everything(pan_right_q15=-1, which=fxb.CTL_VELOCITY), everything(sustain_q15=32769),
             everything(sustain_q15=-1), everything(attack_frames=0, decay_frames=0, release_frames=0, sustain_q15=0),
             everything(velocity_q15=65535), everything(velocity_q15=65536), everything(velocity_q15=-1),
             everything(smoother_k_q15=32769), everything(smoother_k_q15=-1), everything(smoother_k_q15=0),
             everything(which=fxb.CTL_PHASE_INC | fxb.CTL_INC_SCALE, inc_scale_q16=0xFFFFFFFF),
             everything(which=fxb.CTL_FILTER, amp_q15=0, velocity_q15=-5)]
    verdicts = [fxb.fx_ctl_check(c) for c in cases]
    assert verdicts == [cm.check(c) for c in cases]
    assert verdicts.count(0) == 9 and verdicts.count(BAD) == len(cases) - 9
    for k in range(3):
        c = everything()
        c.reserved[k] = 1
        assert fxb.fx_ctl_check(c) == cm.check(c) == BAD
    assert fxb.fx_ctl_check(None) == BAD


def test_fx_ctl_entry_points_refuse_a_null_bank():
    L = fxb._bind(device.load())
    c, tags, word = everything(), np.array([1, 2], np.uint32), C.c_void_p(16)
    assert L.skred_fxbank_ctl_range(None, C.byref(c), 0, 8, None, None) == BAD
    assert L.skred_fxbank_ctl_list(None, C.byref(c), word, 2, None, None, None) == BAD
    assert L.skred_fxbank_ctl_owned(None, C.byref(c), word, tags.ctypes.data, 2, None, None, None) == BAD


@pytest.mark.parametrize("group", ["const", "check", "pack", "range", "list", "owned"])
def test_fx_ctl_host_cases(group):
    fx_host_cases.group(group)


# ---------------------------------------------------------------------------------------------- the model's edges

def small_bank(n=8):
    b, pool, c0 = fxb.bank_fx(n)
    return b, pool, c0


def test_fx_model_inc_scale_overflow_boundary():
    """scale 2.0 (131072): 0x7FFFFFFF is the largest increment that still stores (-> 0xFFFFFFFE), 0x80000000 the first that does not;
    scale 0xFFFFFFFF: 0x10000 stores 0xFFFFFFFF exactly, 0x10001 does not; a withheld product leaves a PHASE_INC of the same record in."""
    b, _, _ = small_bank()
    b["phase_inc"][:4] = [0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 1]
    assert cm.ctl_range(b, fx_ctl(fxb.CTL_INC_SCALE, inc_scale_q16=131072), 0, 4) == [4, 2]
    assert b["phase_inc"][:4].tolist() == [0xFFFFFFFE, 0x80000000, 0xFFFFFFFF, 2]
    b["phase_inc"][:2] = [0x10000, 0x10001]
    assert cm.ctl_range(b, fx_ctl(fxb.CTL_INC_SCALE, inc_scale_q16=0xFFFFFFFF), 0, 2) == [2, 1]
    assert b["phase_inc"][:2].tolist() == [0xFFFFFFFF, 0x10001]
    assert cm.ctl_range(b, fx_ctl(fxb.CTL_INC_SCALE, inc_scale_q16=65536), 0, 8)[1] == 0      # 1.0 never overflows
    assert cm.ctl_range(b, fx_ctl(fxb.CTL_INC_SCALE | fxb.CTL_PHASE_INC, phase_inc=0x80000000, inc_scale_q16=131072), 0, 2) == [2, 2]
    assert b["phase_inc"][:2].tolist() == [0x80000000, 0x80000000]
    assert cm.ctl_range(b, fx_ctl(fxb.CTL_INC_SCALE | fxb.CTL_PHASE_INC, phase_inc=1000, inc_scale_q16=32768), 0, 2) == [2, 0]
    assert b["phase_inc"][:2].tolist() == [500, 500]


def test_fx_model_amp_keeps_a_zero_and_names_only_its_fields():
    b, _, _ = small_bank()
    b["amp_q15"][[1, 5]] = 0
    before = b.copy()
    res = cm.ctl_list(b, fx_ctl(fxb.CTL_AMP | fxb.CTL_PAN, amp_q15=777, pan_left_q15=1, pan_right_q15=2), [1, -1, 2, 8, 5, 2], 6)
    assert res == [4, 2] and b["amp_q15"].tolist() == [32768, 0, 777, 32768, 32768, 0, 32768, 32768]
    assert b["pan_left_q15"][[1, 2, 5]].tolist() == [1, 1, 1] and b["pan_left_q15"][0] == before["pan_left_q15"][0]
    changed = [k for k in b.a if not np.array_equal(b[k], before[k])]
    assert sorted(changed) == ["amp_q15", "pan_left_q15", "pan_right_q15"]
    owner = om.new(8)
    om.tag_list(owner, [2, 5], [9, 9])
    res = cm.ctl_list(b, fx_ctl(fxb.CTL_VELOCITY, velocity_q15=5), [2, 3, 5, -1], 4, None, owner, [9, 9, 8, 7])
    assert res == [1, 0, 2] and b["velocity_q15"][2] == 5 and b["velocity_q15"][5] == before["velocity_q15"][5]
    with pytest.raises(AssertionError):
        cm.ctl_list(b, fx_ctl(fxb.CTL_INC_SCALE, inc_scale_q16=70000), [2, 2], 2)


def test_fx_model_env_times_with_a_zero_length_stage():
    """attack 0 and decay 0: the oracle renders the voice at its sustain level from the first frame; release 0: a released voice
    ends in the first frame.  The reciprocals of zero-length stages are 0."""
    b, pool, c0 = small_bank()
    b["smoother_enable"] = 0
    b["sample_start"] = c0                                  # every voice at the very start of its attack
    c = fx_ctl(fxb.CTL_ENV_TIMES, attack_frames=0, decay_frames=0, release_frames=0, sustain_q15=12345)
    assert cm.check(c) == 0 and cm.ctl_range(b, c, 0, 4) == [4, 0]
    assert cm.recips(b)[:4].tolist() == [[0, 0, 0]] * 4 and cm.recips(b)[4].tolist() == [(1 << 32) // 480, (1 << 32) // 4800, (1 << 32) // 9600]
    b["sample_release"][[2, 3]] = c0
    plain = b.copy()
    for k in ("attack_frames", "decay_frames", "release_frames", "sustain_q15"):
        plain[k][:4] = plain[k][4]                          # the same voices without the controller
    _, stems, _ = cpuref.fx_render(b, pool, c0, 4, 1, want_stems=True)
    _, plain_stems, _ = cpuref.fx_render(plain, pool, c0, 4, 1, want_stems=True)
    assert b["is_active"].tolist() == [1, 1, 0, 0, 1, 1, 1, 1] and plain["is_active"].tolist() == [1] * 8
    assert (stems[:, 2:4] == 0).all() and np.array_equal(stems[:, 4:], plain_stems[:, 4:])
    # held at sustain (12345) from the first frame; with the recipe's times the envelope is at most 4 / 480 * 32768 = 273 by then:
    # more than ten times louder
    loud, quiet = np.abs(stems[:, :2]).sum(axis=(0, 2)), np.abs(plain_stems[:, :2]).sum(axis=(0, 2))
    assert (loud > 10 * np.maximum(quiet, 1)).all(), (loud, quiet)
