"""Fixed-point voice bank: numpy mirror + ctypes binding of include/skred_amd_fxpt.h.

The fixed-point path is defined by this project (oracle/cpu_ref_fxpt.c), not by the reference,
which has none."""
from __future__ import annotations

import ctypes as C
import json
from typing import Dict, Optional, Tuple

import numpy as np

from . import banks
from .device import OwnerMatchC, SkredAmdError, _check, load
from .device import (PEDAL_PENDING, PEDAL_LATCHED, PEDAL_LIFT_SUSTAIN, PEDAL_LIFT_SOSTENUTO, PEDAL_SUSTAIN_DOWN,   # noqa: F401
                     PEDAL_CALL_STAMP_OWNED, PEDAL_CALL_RELEASE_TAGS, PEDAL_CALL_LATCH, PEDAL_CALL_UP)             # (SKRED_PEDAL_*: the float bank's, as they are)

U32, I32, U64 = np.dtype("<u4"), np.dtype("<i4"), np.dtype("<u8")
FX_FIELDS = [
    ("phase", U32, True), ("phase_inc", U32, False), ("table_offset", I32, False), ("log2_size", I32, False),
    ("amp_q15", I32, False), ("pan_left_q15", I32, False), ("pan_right_q15", I32, False),
    ("disconnect", I32, False), ("use_envelope", I32, False),
    ("attack_frames", U32, False), ("decay_frames", U32, False), ("release_frames", U32, False),
    ("sustain_q15", I32, False), ("velocity_q15", I32, False),
    ("sample_start", U64, False), ("sample_release", U64, False),
    ("is_active", I32, True), ("smoother_enable", I32, False), ("smoother_k_q15", I32, False),
    ("smoother_gain_q15", I32, True), ("voice_sample", I32, True),
    ("one_shot", I32, False), ("finished", I32, True), ("filter_mode", I32, False),
    ("b0_q30", I32, False), ("b1_q30", I32, False), ("b2_q30", I32, False), ("a1_q30", I32, False), ("a2_q30", I32, False),
    ("x1", I32, True), ("x2", I32, True), ("y1", I32, True), ("y2", I32, True),
]
FX_RW = [f[0] for f in FX_FIELDS if f[2]]
FX_ABI_SYMBOLS = ["skred_fxbank_create", "skred_fxbank_destroy", "skred_fxbank_set_tables_i16",
                  "skred_fxbank_upload", "skred_fxbank_download", "skred_fxbank_set_sample_count",
                  "skred_fxbank_get_sample_count", "skred_fxbank_render", "skred_fxbank_render_host",
                  "skred_fxbank_last_render_ms", "skred_fxbank_render_mix", "skred_fxbank_master", "skred_fxbank_set_master",
                  "skred_fxbank_get_master_gain", "skred_fxbank_stamp",
                  "skred_fxbank_update", "skred_fxbank_find_idle", "skred_fxbank_find_idle_host",
                  "skred_fxbank_notes_on_list", "skred_fxbank_note_on_idle", "skred_fxbank_stamp_list",
                  "skred_fxbank_find_steal", "skred_fxbank_find_steal_host", "skred_fxbank_note_on_steal",
                  "skred_fxbank_tag_list", "skred_fxbank_find_owned", "skred_fxbank_stamp_owned", "skred_fxbank_release_tags",
                  "skred_fxbank_owner_clear", "skred_fxbank_download_owners", "skred_fxbank_ctl_range", "skred_fxbank_ctl_list",
                  "skred_fxbank_ctl_owned", "skred_fxbank_download_params",
                  "skred_fxbank_find_match", "skred_fxbank_find_match_host", "skred_fxbank_stamp_match", "skred_fxbank_ctl_match",
                  "skred_fxbank_ctl_owned_each", "skred_fxbank_ctl_tags_each",
                  "skred_fxbank_ctl_owned_each_filter", "skred_fxbank_ctl_tags_each_filter",
                  "skred_fxbank_find_steal_match", "skred_fxbank_find_steal_match_host", "skred_fxbank_note_on_channel",
                  "skred_fxbank_stamp_owned_pedal", "skred_fxbank_release_tags_pedal", "skred_fxbank_pedal_latch",
                  "skred_fxbank_pedal_up", "skred_fxbank_pedal_clear", "skred_fxbank_download_pedals",
                  "skred_fxbank_glide_owned", "skred_fxbank_glide_tags", "skred_fxbank_glide_advance", "skred_fxbank_glide_stop",
                  "skred_fxbank_download_glide",
                  "skred_fxbank_bend_match", "skred_fxbank_bend_owned_each", "skred_fxbank_bend_tags_each", "skred_fxbank_bend_clear",
                  "skred_fxbank_download_bend",
                  "skred_fxbank_cutoff_match", "skred_fxbank_cutoff_owned_each", "skred_fxbank_cutoff_tags_each",
                  "skred_fxbank_cutoff_advance", "skred_fxbank_cutoff_stop", "skred_fxbank_download_cutoff",
                  "skred_fxbank_fenv_match", "skred_fxbank_fenv_owned_each", "skred_fxbank_fenv_tags_each", "skred_fxbank_download_fenv",
                  "skred_fxshard_create", "skred_fxshard_bank", "skred_fxshard_upload"]
FX_HOST_ABI_SYMBOLS = ["skred_fx_idle_check", "skred_fx_notes_check", "skred_fx_steal_check", "skred_fx_ctl_check",
                       "skred_fx_ctl_each_check", "skred_fx_filter_each_check", "skred_fx_chan_check", "skred_fx_pedal_check",
                       "skred_fx_glide_check", "skred_fx_bend_check", "skred_fx_cutoff_check", "skred_fx_filter_coeffs_w", "skred_fx_fenv_check"]                                                                     # pure host: no bank, no device
FX_STAMP_TRIGGER, FX_STAMP_RELEASE = 1, 2
# live control: the float bank's vocabulary (include/skred_amd.h: SKRED_DIRTY_* / SKRED_STAMP_* / SKRED_IDLE_* / SKRED_NOTE_*)
DIRTY_PARAMS, DIRTY_PHASE, DIRTY_ENV_STATE, DIRTY_PAN, DIRTY_FILTER_STATE = 1, 2, 4, 8, 16
DIRTY_SMOOTHER, DIRTY_HOLD, DIRTY_SAMPLE, STAMP_TRIGGER, STAMP_RELEASE, DIRTY_ENV_CLOCK = 32, 64, 128, 256, 512, 1024
IDLE_FINISHED, IDLE_ENV_DONE, IDLE_AMP_ZERO, IDLE_UNNAMED = 1, 2, 4, 256
NOTE_SET_PHASE, NOTE_SET_PAN = 1, 2
STEAL_OLDEST, STEAL_QUIETEST = 0, 1               # SKRED_STEAL_*: policy; flags; the longest list
STEAL_RELEASED_FIRST, STEAL_RELEASED_ONLY, STEAL_UNNAMED = 1, 2, 256
STEAL_MAX = 1024
# note owners and controllers: SKRED_OWNER_* and the SKRED_CTL_* bits this path has (FM_DEPTH .. CZ_DIST, 1 << 8 .. 1 << 13, are refused)
OWNER_MAX_TAGS, OWNER_ALLOW_ZERO, OWNER_UNIQUE = 1024, 1, 2
CTL_PHASE_INC, CTL_INC_SCALE, CTL_AMP, CTL_PAN, CTL_FILTER, CTL_ENV_TIMES, CTL_VELOCITY, CTL_SMOOTHING = 1, 2, 4, 8, 16, 32, 64, 128
CTL_ALL = 255
CTL_REFUSED = 0x3F00
# channels and per-note expression: the float bank's SKRED_EACH_* bits
EACH_INC_SCALE, EACH_AMP_SCALE, EACH_VELOCITY, EACH_PAN = 1, 2, 4, 8
EACH_ALL = 15
CHAN_NO_CAP = 0xFFFFFFFF                          # SKRED_CHAN_NO_CAP: a cap that never limits
FX_GLIDE_FROM_SCALE, FX_GLIDE_TO_SCALE, FX_GLIDE_TO_INC = 1, 2, 4   # SKRED_FX_GLIDE_*: exactly one per entry
FX_BEND_ONE = 1 << 24                             # SKRED_FX_BEND_ONE: the wheel at centre, as a Q24 ratio
# filter cutoff: SKRED_FX_CUTOFF_* -- the set bits and the integer boxes (w_q29: Q29 radians per frame; q_q16)
FX_CUTOFF_ABS, FX_CUTOFF_TRACK, FX_CUTOFF_GLIDE, FX_CUTOFF_Q, FX_CUTOFF_MODE = 1, 2, 4, 8, 16
FX_CUTOFF_W_MIN, FX_CUTOFF_W_MAX, FX_CUTOFF_Q_MIN, FX_CUTOFF_Q_MAX = 1 << 19, 3 << 29, 1 << 10, 1 << 26
# filter envelope: SKRED_FX_FENV_* -- the set bits; the stage values of the first fenv word
FX_FENV_ABS, FX_FENV_REL, FX_FENV_START = 1, 2, 4
FX_FENV_OFF, FX_FENV_ATTACK, FX_FENV_DECAY, FX_FENV_SUSTAIN, FX_FENV_RELEASE = 0, 1, 2, 3, 4
FX_CTL_SPAN = 256                                 # voices or entries per workgroup of the controller and guarded-stamp kernels
FX_RING_SLOTS = 8                                 # SKRED_FX_RING_SLOTS: staging slots of the control ring
FX_NOTE_SPAN = 256                                # notes per workgroup of the placement kernel
MASTER_TARGET_Q31 = int(0.025 * 2147483648.0)     # the library's default: volume_user 1 x AMY_FACTOR
MASTER_K_Q15 = 66                                 # 0.002


class FxBankC(C.Structure):
    _fields_ = [("n_voices", C.c_int32)] + [(n, C.c_void_p) for n, _, _ in FX_FIELDS]


class FxIdleQueryC(C.Structure):
    """ctypes image of ``skred_fx_idle_query_t``."""
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("which", C.c_uint32), ("settle_q15", C.c_int32),
                ("start", C.c_int32), ("max_out", C.c_int32)]          # `start`: the header's `from`


class FxStealQueryC(C.Structure):
    """ctypes image of ``skred_fx_steal_query_t`` (40 bytes)."""
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("policy", C.c_uint32), ("flags", C.c_uint32), ("min_age", C.c_uint64),
                ("exclude_idle", C.c_uint32), ("settle_q15", C.c_int32), ("max_out", C.c_int32), ("reserved", C.c_int32)]


def fx_steal_query(first, count, policy=STEAL_OLDEST, flags=0, min_age=0, exclude_idle=0, settle_q15=0, max_out=0) -> FxStealQueryC:
    return FxStealQueryC(int(first), int(count), int(policy), int(flags), int(min_age), int(exclude_idle), int(settle_q15), int(max_out), 0)


def fx_steal_check(q: "FxStealQueryC", n_voices: int) -> int:
    """skred_fx_steal_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4).  Pure host, no device."""
    return int(_bind(load()).skred_fx_steal_check(C.byref(q) if q is not None else None, int(n_voices)))


class FxCtlC(C.Structure):
    """ctypes image of ``skred_fx_ctl_t`` (80 bytes)."""
    _fields_ = [("which", C.c_uint32), ("phase_inc", C.c_uint32), ("inc_scale_q16", C.c_uint32), ("amp_q15", C.c_int32),
                ("pan_left_q15", C.c_int32), ("pan_right_q15", C.c_int32), ("b0_q30", C.c_int32), ("b1_q30", C.c_int32),
                ("b2_q30", C.c_int32), ("a1_q30", C.c_int32), ("a2_q30", C.c_int32), ("attack_frames", C.c_uint32),
                ("decay_frames", C.c_uint32), ("release_frames", C.c_uint32), ("sustain_q15", C.c_int32), ("velocity_q15", C.c_int32),
                ("smoother_k_q15", C.c_int32), ("reserved", C.c_uint32 * 3)]


def fx_ctl(which: int, **values) -> FxCtlC:
    """One controller record: ``which`` (CTL_*) and the named fields; everything else 0."""
    c = FxCtlC()
    c.which = int(which)
    for k, v in values.items():
        setattr(c, k, int(v))
    return c


def fx_ctl_check(ctl: Optional[FxCtlC]) -> int:
    """skred_fx_ctl_check: 0, or SKRED_E_BAD_ARG (-2).  Pure host, no device."""
    return int(_bind(load()).skred_fx_ctl_check(C.byref(ctl) if ctl is not None else None))


class FxCtlEachC(C.Structure):
    """ctypes image of ``skred_fx_ctl_each_t`` (32 bytes)."""
    _fields_ = [("set", C.c_uint32), ("inc_scale_q16", C.c_uint32), ("amp_scale_q16", C.c_uint32), ("velocity_q15", C.c_int32),
                ("pan_left_q15", C.c_int32), ("pan_right_q15", C.c_int32), ("reserved", C.c_uint32 * 2)]


def fx_each(set: int, **values) -> FxCtlEachC:
    """One per-entry record: ``set`` (EACH_*) and the named values; everything else 0."""
    e = FxCtlEachC()
    e.set = int(set)
    for k, v in values.items():
        setattr(e, k, int(v))
    return e


def fx_each_array(entries):
    """A contiguous ``FxCtlEachC`` array from a sequence of FxCtlEachC (a ctypes array of FxCtlEachC passes through)."""
    if isinstance(entries, C.Array) and entries._type_ is FxCtlEachC:
        return entries
    entries = list(entries)
    return (FxCtlEachC * len(entries))(*entries)


def fx_ctl_each_check(entries, ctl: Optional[FxCtlC] = None, n: Optional[int] = None) -> int:
    """skred_fx_ctl_each_check: 0, or SKRED_E_BAD_ARG (-2).  Pure host, no device.  ``entries`` None: a NULL array."""
    arr = fx_each_array(entries) if entries is not None else None
    n = (len(arr) if arr is not None else 0) if n is None else n
    return int(_bind(load()).skred_fx_ctl_each_check(C.cast(arr, C.c_void_p) if arr is not None else None, int(n),
                                                      C.byref(ctl) if ctl is not None else None))


class FxFilterEachC(C.Structure):
    """ctypes image of ``skred_fx_filter_each_t`` (32 bytes): the five Q2.30 coefficients entry k brings."""
    _fields_ = [("b0_q30", C.c_int32), ("b1_q30", C.c_int32), ("b2_q30", C.c_int32), ("a1_q30", C.c_int32), ("a2_q30", C.c_int32),
                ("reserved", C.c_uint32 * 3)]


def fx_filter_each(b0_q30: int = 0, b1_q30: int = 0, b2_q30: int = 0, a1_q30: int = 0, a2_q30: int = 0) -> FxFilterEachC:
    """One set of per-entry coefficients (Q2.30, any int32)."""
    return FxFilterEachC(int(b0_q30), int(b1_q30), int(b2_q30), int(a1_q30), int(a2_q30))


def fx_filter_each_array(filt):
    """A contiguous ``FxFilterEachC`` array from a sequence of FxFilterEachC (a ctypes array of FxFilterEachC passes through)."""
    if isinstance(filt, C.Array) and filt._type_ is FxFilterEachC:
        return filt
    filt = list(filt)
    return (FxFilterEachC * len(filt))(*filt)


def fx_filter_each_check(filt, ctl: Optional[FxCtlC] = None, n: Optional[int] = None) -> int:
    """skred_fx_filter_each_check: 0, or SKRED_E_BAD_ARG (-2).  Pure host, no device.  ``filt`` None: a NULL array."""
    arr = fx_filter_each_array(filt) if filt is not None else None
    n = (len(arr) if arr is not None else 0) if n is None else n
    return int(_bind(load()).skred_fx_filter_each_check(C.cast(arr, C.c_void_p) if arr is not None else None, int(n),
                                                         C.byref(ctl) if ctl is not None else None))


def _tags(tags) -> np.ndarray:
    return np.ascontiguousarray(tags, np.uint32)


def fx_chan_check(idle_q: Optional[FxIdleQueryC], steal_q: Optional[FxStealQueryC], m: Optional[OwnerMatchC], cap: int, tags,
                  n_voices: int, n: Optional[int] = None) -> int:
    """skred_fx_chan_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4).  Pure host, no device.  ``tags`` None: a NULL array."""
    t = _tags(tags) if tags is not None else None
    n = (len(t) if t is not None else 0) if n is None else n
    return int(_bind(load()).skred_fx_chan_check(C.byref(idle_q) if idle_q is not None else None,
                                                 C.byref(steal_q) if steal_q is not None else None,
                                                 C.byref(m) if m is not None else None, int(cap),
                                                 t.ctypes.data if t is not None else None, int(n), int(n_voices)))


def fx_pedal_check(call: int, n_voices: int, first: int = 0, count: int = 0, m: Optional[OwnerMatchC] = None, flags: int = 0, tags=None,
                   n: Optional[int] = None) -> int:
    """skred_fx_pedal_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4) for what the pedal entry point PEDAL_CALL_* would refuse.
    Pure host, no device.  ``tags`` None: a NULL array."""
    t = _tags(tags) if tags is not None else None
    n = (len(t) if t is not None else 0) if n is None else n
    return int(_bind(load()).skred_fx_pedal_check(int(call), int(n_voices), int(first), int(count), C.byref(m) if m is not None else None,
                                                  int(flags), t.ctypes.data if t is not None else None, int(n)))


class FxGlideC(C.Structure):
    """ctypes image of ``skred_fx_glide_t`` (32 bytes): `set` is exactly one of FX_GLIDE_FROM_SCALE, _TO_SCALE and _TO_INC."""
    _fields_ = [("set", C.c_uint32), ("up_q32", C.c_uint32), ("down_q32", C.c_uint32), ("scale_q16", C.c_uint32),
                ("target_inc", C.c_uint32), ("reserved", C.c_uint32 * 3)]


def glide(set: int, up_q32: int, down_q32: int, scale_q16: int = 0, target_inc: int = 0) -> FxGlideC:
    """One glide: ``glide(FX_GLIDE_FROM_SCALE, 31000000, 31000000, 43740)`` slides up a fifth into the note."""
    return FxGlideC(int(set), int(up_q32), int(down_q32), int(scale_q16), int(target_inc))


def glide_array(glides):
    """A contiguous ``FxGlideC`` array from a sequence of FxGlideC (a ctypes array of FxGlideC passes through)."""
    if isinstance(glides, C.Array) and glides._type_ is FxGlideC:
        return glides
    glides = list(glides)
    return (FxGlideC * len(glides))(*glides)


def bend_ratios(ratios_q24) -> np.ndarray:
    """Q24 ratios as the calls take them: a contiguous uint32 array (FX_BEND_ONE = 1 << 24 is the centre)."""
    return np.ascontiguousarray(np.asarray(ratios_q24, np.uint32).reshape(-1))


def bend_ratio_q24(semitones: float) -> int:
    """The wheel at `semitones` as a Q24 ratio; 0 semitones is exactly FX_BEND_ONE."""
    return max(1, min(0xFFFFFFFF, int(round(2.0 ** (float(semitones) / 12.0) * (1 << 24)))))


def fx_bend_check(ratios_q24, n: Optional[int] = None) -> int:
    """skred_fx_bend_check: 0, or SKRED_E_BAD_ARG (-2).  Pure host, no device.  ``ratios_q24`` None: a NULL array."""
    r = bend_ratios(ratios_q24) if ratios_q24 is not None else None
    n = (len(r) if r is not None else 0) if n is None else n
    return int(_bind(load()).skred_fx_bend_check(r.ctypes.data if r is not None else None, int(n)))


class FxCutoffC(C.Structure):
    """ctypes image of ``skred_fx_cutoff_t`` (32 bytes): `set` holds exactly one of FX_CUTOFF_ABS and FX_CUTOFF_TRACK."""
    _fields_ = [("set", C.c_uint32), ("value", C.c_uint32), ("q_q16", C.c_uint32), ("mode", C.c_uint32), ("up_q32", C.c_uint32),
                ("down_q32", C.c_uint32), ("reserved", C.c_uint32 * 2)]


def fx_cutoff(set: int, value: int, q_q16: int = 0, mode: int = 0, up_q32: int = 0, down_q32: int = 0) -> FxCutoffC:
    """One record: ``fx_cutoff(FX_CUTOFF_TRACK | FX_CUTOFF_Q | FX_CUTOFF_MODE, track_q24, 2 << 16, 1)`` is a low-pass that follows the key."""
    return FxCutoffC(int(set), int(value), int(q_q16), int(mode), int(up_q32), int(down_q32))


def fx_cutoff_array(recs):
    """A contiguous ``FxCutoffC`` array from a sequence of FxCutoffC (a ctypes array of FxCutoffC passes through)."""
    if isinstance(recs, C.Array) and recs._type_ is FxCutoffC:
        return recs
    recs = list(recs)
    return (FxCutoffC * len(recs))(*recs)


def fx_cutoff_check(recs, n: Optional[int] = None, first_time: bool = False) -> int:
    """skred_fx_cutoff_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4).  Pure host, no device.  ``recs`` None: a NULL array."""
    arr = fx_cutoff_array(recs) if recs is not None else None
    n = (len(arr) if arr is not None else 0) if n is None else n
    return int(_bind(load()).skred_fx_cutoff_check(C.cast(arr, C.c_void_p) if arr is not None else None, int(n), int(bool(first_time))))


class FxFenvC(C.Structure):
    """ctypes image of ``skred_fx_fenv_t`` (32 bytes): `set` holds exactly one of FX_FENV_ABS and FX_FENV_REL, and FX_FENV_START or not."""
    _fields_ = [("set", C.c_uint32), ("start", C.c_uint32), ("peak", C.c_uint32), ("sustain", C.c_uint32), ("end", C.c_uint32),
                ("rate_attack_q32", C.c_uint32), ("rate_decay_q32", C.c_uint32), ("rate_release_q32", C.c_uint32)]


def fx_fenv(set: int, peak: int, sustain: int, end: int, rate_attack_q32: int, rate_decay_q32: int, rate_release_q32: int,
            start: int = 0) -> FxFenvC:
    """One record: ``fx_fenv(FX_FENV_REL, 8 << 16, 2 << 16, 1 << 15, ra, rd, rr)`` opens to 8 x the present cutoff, falls to 2 x while the
    key is held and closes to half of it after the note-off."""
    return FxFenvC(int(set), int(start), int(peak), int(sustain), int(end), int(rate_attack_q32), int(rate_decay_q32), int(rate_release_q32))


def fx_fenv_array(recs):
    """A contiguous ``FxFenvC`` array from a sequence of FxFenvC (a ctypes array of FxFenvC passes through)."""
    if isinstance(recs, C.Array) and recs._type_ is FxFenvC:
        return recs
    recs = list(recs)
    return (FxFenvC * len(recs))(*recs)


def fx_fenv_check(recs, n: Optional[int] = None) -> int:
    """skred_fx_fenv_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4).  Pure host, no device.  ``recs`` None: a NULL array."""
    arr = fx_fenv_array(recs) if recs is not None else None
    n = (len(arr) if arr is not None else 0) if n is None else n
    return int(_bind(load()).skred_fx_fenv_check(C.cast(arr, C.c_void_p) if arr is not None else None, int(n)))


def fx_filter_coeffs_w(mode: int, w_q29: int, q_q16: int):
    """skred_fx_filter_coeffs_w: (return code, the five Q2.30 words b0 b1 b2 a1 a2 as an int32 array).  Pure host, no device."""
    out = np.zeros(5, np.int32)
    rc = int(_bind(load()).skred_fx_filter_coeffs_w(int(mode), int(w_q29), int(q_q16), out.ctypes.data))
    return rc, out


def fx_glide_check(glides, n: Optional[int] = None) -> int:
    """skred_fx_glide_check: 0, or SKRED_E_BAD_ARG (-2).  Pure host, no device.  ``glides`` None: a NULL array."""
    arr = glide_array(glides) if glides is not None else None
    n = (len(arr) if arr is not None else 0) if n is None else n
    return int(_bind(load()).skred_fx_glide_check(C.cast(arr, C.c_void_p) if arr is not None else None, int(n)))


class FxNoteC(C.Structure):
    """ctypes image of ``skred_fx_note_t`` (32 bytes)."""
    _fields_ = [("phase_inc", C.c_uint32), ("velocity_q15", C.c_int32), ("phase", C.c_uint32), ("pan_left_q15", C.c_int32),
                ("pan_right_q15", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


def fx_note_array(notes):
    """A contiguous ``FxNoteC`` array from a sequence of FxNoteC (a ctypes array of FxNoteC passes through)."""
    if isinstance(notes, C.Array) and notes._type_ is FxNoteC:
        return notes
    notes = list(notes)
    return (FxNoteC * len(notes))(*notes)


def fx_notes_check(notes) -> int:
    """skred_fx_notes_check: 0, or SKRED_E_BAD_ARG (-2).  Pure host, no device."""
    arr = fx_note_array(notes)
    return int(_bind(load()).skred_fx_notes_check(C.cast(arr, C.c_void_p), len(arr)))


def fx_idle_check(q: "FxIdleQueryC", n_voices: int) -> int:
    """skred_fx_idle_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4).  Pure host, no device."""
    return int(_bind(load()).skred_fx_idle_check(C.byref(q) if q is not None else None, int(n_voices)))


class FxVoiceBank:
    def __init__(self, n: int):
        self.n = int(n)
        self.a: Dict[str, np.ndarray] = {name: np.zeros(self.n, dt) for name, dt, _ in FX_FIELDS}
        self.a["log2_size"][:] = 3
        self.a["pan_left_q15"][:] = 16384
        self.a["pan_right_q15"][:] = 16384
        self.a["velocity_q15"][:] = 32768
        self.a["sustain_q15"][:] = 32768

    def __getitem__(self, k):
        return self.a[k]

    def __setitem__(self, k, v):
        self.a[k][...] = v

    def as_c(self) -> FxBankC:
        c = FxBankC()
        c.n_voices = self.n
        for name, dt, _ in FX_FIELDS:
            arr = self.a[name]
            assert arr.dtype == dt and arr.flags["C_CONTIGUOUS"] and arr.shape == (self.n,), name
            setattr(c, name, arr.ctypes.data)
        return c

    def copy(self) -> "FxVoiceBank":
        o = FxVoiceBank.__new__(FxVoiceBank)
        o.n, o.a = self.n, {k: v.copy() for k, v in self.a.items()}
        return o

    def take(self, index) -> "FxVoiceBank":
        idx = np.arange(self.n)[index]
        o = FxVoiceBank.__new__(FxVoiceBank)
        o.n, o.a = int(idx.size), {k: np.ascontiguousarray(v[idx]) for k, v in self.a.items()}
        return o

    def rw_mismatch(self, other: "FxVoiceBank") -> Dict[str, int]:
        return {k: int((self.a[k] != other.a[k]).sum()) for k in FX_RW if (self.a[k] != other.a[k]).any()}


def _bind(L):
    vp, i32 = C.c_void_p, C.c_int
    L.skred_fxbank_create.argtypes = [i32, i32, C.POINTER(vp)]
    L.skred_fxbank_destroy.argtypes = [vp]
    L.skred_fxbank_destroy.restype = None
    L.skred_fxbank_set_tables_i16.argtypes = [vp, vp, C.c_size_t]
    L.skred_fxbank_upload.argtypes = [vp, C.POINTER(FxBankC), i32, i32, i32]
    L.skred_fxbank_download.argtypes = [vp, C.POINTER(FxBankC), i32, i32, i32]
    L.skred_fxbank_set_sample_count.argtypes = [vp, C.c_uint64]
    L.skred_fxbank_get_sample_count.argtypes = [vp]
    L.skred_fxbank_get_sample_count.restype = C.c_uint64
    L.skred_fxbank_render.argtypes = [vp, i32, i32, vp, vp, vp]
    L.skred_fxbank_render_host.argtypes = [vp, i32, i32, vp, vp]
    L.skred_fxbank_last_render_ms.argtypes = [vp]
    L.skred_fxbank_last_render_ms.restype = C.c_float
    L.skred_fxbank_render_mix.argtypes = [vp, i32, i32, vp, vp, vp]
    L.skred_fxbank_master.argtypes = [vp, vp, i32, vp, vp]
    L.skred_fxbank_set_master.argtypes = [vp, C.c_int64, C.c_int32, C.c_int64]
    L.skred_fxbank_get_master_gain.argtypes = [vp]
    L.skred_fxbank_get_master_gain.restype = C.c_int64
    L.skred_fxbank_stamp.argtypes = [vp, vp, i32, i32, vp]
    L.skred_fxbank_update.argtypes = [vp, C.POINTER(FxBankC), vp, i32, C.c_uint32, vp]
    L.skred_fx_idle_check.argtypes = [vp, i32]
    L.skred_fxbank_find_idle.argtypes = [vp, vp, vp, vp, vp]
    L.skred_fxbank_find_idle_host.argtypes = [vp, vp, vp, C.POINTER(C.c_int), vp]
    L.skred_fx_notes_check.argtypes = [vp, i32]
    L.skred_fxbank_notes_on_list.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_note_on_idle.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_stamp_list.argtypes = [vp, vp, i32, vp, C.c_uint32, vp]
    L.skred_fx_steal_check.argtypes = [vp, i32]
    L.skred_fxbank_find_steal.argtypes = [vp, vp, vp, vp, vp]
    L.skred_fxbank_find_steal_host.argtypes = [vp, vp, vp, C.POINTER(C.c_int), vp]
    L.skred_fxbank_note_on_steal.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_tag_list.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_find_owned.argtypes = [vp, i32, i32, vp, i32, vp, vp]
    L.skred_fxbank_stamp_owned.argtypes = [vp, vp, vp, i32, vp, C.c_uint32, vp, vp]
    L.skred_fxbank_release_tags.argtypes = [vp, i32, i32, vp, i32, C.c_uint32, vp, vp]
    L.skred_fxbank_owner_clear.argtypes = [vp, i32, i32, vp]
    L.skred_fxbank_download_owners.argtypes = [vp, vp, i32, i32]
    L.skred_fx_ctl_check.argtypes = [vp]
    L.skred_fxbank_ctl_range.argtypes = [vp, vp, i32, i32, vp, vp]
    L.skred_fxbank_ctl_list.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_ctl_owned.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_download_params.argtypes = [vp, C.POINTER(FxBankC), vp, i32, i32, i32]
    L.skred_fxbank_find_match.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp]
    L.skred_fxbank_find_match_host.argtypes = [vp, i32, i32, vp, i32, vp, C.POINTER(C.c_int), vp]
    L.skred_fxbank_stamp_match.argtypes = [vp, i32, i32, vp, C.c_uint32, vp, vp]
    L.skred_fxbank_ctl_match.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.skred_fx_ctl_each_check.argtypes = [vp, i32, vp]
    L.skred_fxbank_ctl_owned_each.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_ctl_tags_each.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp]
    L.skred_fx_filter_each_check.argtypes = [vp, i32, vp]
    L.skred_fxbank_ctl_owned_each_filter.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_ctl_tags_each_filter.argtypes = [vp, vp, vp, vp, i32, i32, vp, i32, vp, vp]
    L.skred_fxbank_find_steal_match.argtypes = [vp, vp, vp, vp, vp, vp]
    L.skred_fxbank_find_steal_match_host.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), vp]
    L.skred_fx_chan_check.argtypes = [vp, vp, vp, C.c_uint32, vp, i32, i32]
    L.skred_fxbank_note_on_channel.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp, i32, vp, vp, vp]
    L.skred_fx_pedal_check.argtypes = [i32, i32, i32, i32, vp, C.c_uint32, vp, i32]
    L.skred_fxbank_stamp_owned_pedal.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp]
    L.skred_fxbank_release_tags_pedal.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp]
    L.skred_fxbank_pedal_latch.argtypes = [vp, i32, i32, vp, vp, vp]
    L.skred_fxbank_pedal_up.argtypes = [vp, i32, i32, vp, C.c_uint32, vp, vp]
    L.skred_fxbank_pedal_clear.argtypes = [vp, i32, i32, vp]
    L.skred_fxbank_download_pedals.argtypes = [vp, vp, i32, i32]
    L.skred_fx_glide_check.argtypes = [vp, i32]
    L.skred_fxbank_glide_owned.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_glide_tags.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp]
    L.skred_fxbank_glide_advance.argtypes = [vp, i32, i32, i32, vp, vp]
    L.skred_fxbank_glide_stop.argtypes = [vp, i32, i32, i32, vp]
    L.skred_fxbank_download_glide.argtypes = [vp, vp, i32, i32]
    L.skred_fx_bend_check.argtypes = [vp, i32]
    L.skred_fxbank_bend_match.argtypes = [vp, i32, i32, vp, C.c_uint32, vp, vp]
    L.skred_fxbank_bend_owned_each.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_bend_tags_each.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp]
    L.skred_fxbank_bend_clear.argtypes = [vp, i32, i32, i32, vp]
    L.skred_fxbank_download_bend.argtypes = [vp, vp, i32, i32]
    L.skred_fx_cutoff_check.argtypes = [vp, i32, i32]
    L.skred_fx_filter_coeffs_w.argtypes = [i32, C.c_uint32, C.c_uint32, vp]
    L.skred_fxbank_cutoff_match.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.skred_fxbank_cutoff_owned_each.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_cutoff_tags_each.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp]
    L.skred_fxbank_cutoff_advance.argtypes = [vp, i32, i32, i32, vp, vp]
    L.skred_fxbank_cutoff_stop.argtypes = [vp, i32, i32, i32, vp]
    L.skred_fxbank_download_cutoff.argtypes = [vp, vp, i32, i32]
    L.skred_fx_fenv_check.argtypes = [vp, i32]
    L.skred_fxbank_fenv_match.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.skred_fxbank_fenv_owned_each.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.skred_fxbank_fenv_tags_each.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp]
    L.skred_fxbank_download_fenv.argtypes = [vp, vp, i32, i32]
    L.skred_fxshard_create.argtypes = [i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.skred_fxshard_bank.argtypes = [vp]
    L.skred_fxshard_bank.restype = vp
    L.skred_fxshard_upload.argtypes = [vp, C.POINTER(FxBankC)]
    return L


class DeviceFxBank:
    def __init__(self, n_voices: int, device: int = 0):
        self.L = _bind(load())
        self.n = int(n_voices)
        h = C.c_void_p()
        _check(self.L.skred_fxbank_create(device, self.n, C.byref(h)), "skred_fxbank_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.skred_fxbank_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tables(self, pool: np.ndarray):
        pool = np.ascontiguousarray(pool, np.int16)
        _check(self.L.skred_fxbank_set_tables_i16(self.h, pool.ctypes.data, pool.size), "skred_fxbank_set_tables_i16")

    @classmethod
    def borrowed(cls, handle, n_voices: int) -> "DeviceFxBank":
        """A view of a bank a shard owns (skred_fxshard_bank): close() does not destroy it."""
        self = cls.__new__(cls)
        self.L = _bind(load())
        self.n = int(n_voices)
        self.h = C.c_void_p(handle)
        self.close = lambda: None
        return self

    def upload(self, bank: FxVoiceBank):
        cb = bank.as_c()
        _check(self.L.skred_fxbank_upload(self.h, C.byref(cb), 0, 0, bank.n), "skred_fxbank_upload")

    def download(self, bank: FxVoiceBank):
        cb = bank.as_c()
        _check(self.L.skred_fxbank_download(self.h, C.byref(cb), 0, 0, bank.n), "skred_fxbank_download")

    def set_sample_count(self, c: int):
        _check(self.L.skred_fxbank_set_sample_count(self.h, c), "skred_fxbank_set_sample_count")

    def sample_count(self) -> int:
        return int(self.L.skred_fxbank_get_sample_count(self.h))

    def render(self, frames: int, d_mix: int, interp: int = 0, d_stems: int = 0, stream: int = 0):
        _check(self.L.skred_fxbank_render(self.h, frames, interp, d_mix, d_stems or None, stream or None), "skred_fxbank_render")

    def render_host(self, frames: int, interp: int = 0, want_stems: bool = False):
        mix = np.zeros((frames, 2), np.int64)
        stems = np.zeros((frames, self.n, 2), np.int32) if want_stems else None
        _check(self.L.skred_fxbank_render_host(self.h, frames, interp, mix.ctypes.data,
                                               stems.ctypes.data if want_stems else None), "skred_fxbank_render_host")
        return mix, stems

    def last_render_ms(self) -> float:
        return float(self.L.skred_fxbank_last_render_ms(self.h))

    def render_mix(self, frames: int, d_out: int, interp: int = 0, d_stems: int = 0, stream: int = 0):
        """Render + mix-down + master stage in one launch; d_out: device int64 [frames][2]."""
        _check(self.L.skred_fxbank_render_mix(self.h, frames, interp, d_out, d_stems or None, stream or None), "skred_fxbank_render_mix")

    def master(self, d_sum: int, frames: int, d_out: int, stream: int = 0):
        _check(self.L.skred_fxbank_master(self.h, d_sum, frames, d_out, stream or None), "skred_fxbank_master")

    def set_master(self, target_q31: int = MASTER_TARGET_Q31, k_q15: int = MASTER_K_Q15, gain_q31: int = 0):
        _check(self.L.skred_fxbank_set_master(self.h, target_q31, k_q15, gain_q31), "skred_fxbank_set_master")

    def master_gain(self) -> int:
        return int(self.L.skred_fxbank_get_master_gain(self.h))

    def stamp(self, voices, which: int, stream: int = 0):
        v = np.ascontiguousarray(voices, np.int32)
        _check(self.L.skred_fxbank_stamp(self.h, v.ctypes.data, len(v), which, stream or None), "skred_fxbank_stamp")

    # ---- live control (include/skred_amd_fxpt.h): asynchronous on `stream`, nothing waits for the device ----
    def update(self, bank: FxVoiceBank, voices, dirty: int, stream: int = 0):
        """Push the `dirty` parts (DIRTY_* | STAMP_*) of the listed voices from the host view."""
        v = np.ascontiguousarray(voices, np.int32)
        cb = bank.as_c()
        _check(self.L.skred_fxbank_update(self.h, C.byref(cb), v.ctypes.data, len(v), dirty, stream or None), "skred_fxbank_update")

    @staticmethod
    def _query(first, count, which, settle_q15, start, max_out) -> FxIdleQueryC:
        return FxIdleQueryC(int(first), int(count), int(which), int(settle_q15), int(first if start is None else start), int(max_out))

    def find_idle(self, first: int, count: int, which: int, settle_q15: int = 0, start: Optional[int] = None,
                  max_out: int = 0, d_voices: int = 0, d_count: int = 0, stream: int = 0):
        """The idle voices of [first, first + count) in ascending order from `start` (default `first`), wrapping, into
        d_voices[0 .. written) (int32, device memory); d_count[0] = written, d_count[1] = total (uint32)."""
        q = self._query(first, count, which, settle_q15, start, max_out)
        _check(self.L.skred_fxbank_find_idle(self.h, C.byref(q), d_voices or None, d_count or None, stream or None),
               "skred_fxbank_find_idle")

    def find_idle_host(self, first: int, count: int, which: int, settle_q15: int = 0, start: Optional[int] = None,
                       max_out: Optional[int] = None, stream: int = 0):
        """The same into host memory, waiting for `stream` only.  Returns (np.int32 array of the listed voices, total)."""
        max_out = count if max_out is None else max_out
        q = self._query(first, count, which, settle_q15, start, max_out)
        out = np.empty(max(max_out, 0), np.int32)
        total = C.c_int(0)
        n = self.L.skred_fxbank_find_idle_host(self.h, C.byref(q), out.ctypes.data if max_out > 0 else None, C.byref(total),
                                               stream or None)
        if n < 0:
            _check(n, "skred_fxbank_find_idle_host")
        return out[:n].copy(), int(total.value)

    def notes_on_list(self, notes, d_voices: int, d_count: int, first_entry: int = 0, d_assigned: int = 0, d_result: int = 0,
                      stream: int = 0):
        """Note k goes to voice d_voices[first_entry + k] while that entry is below d_count[0] and names a voice of the bank, else
        it is dropped.  d_assigned[k] (int32, may be 0) = the voice or -1; d_result[0] = placed, d_result[1] = dropped (uint32)."""
        arr = fx_note_array(notes)
        _check(self.L.skred_fxbank_notes_on_list(self.h, C.cast(arr, C.c_void_p), len(arr), d_voices or None, d_count or None,
                                                 int(first_entry), d_assigned or None, d_result or None, stream or None),
               "skred_fxbank_notes_on_list")

    def note_on_idle(self, notes, first: int, count: int, which: int, settle_q15: int = 0, start: Optional[int] = None,
                     d_assigned: int = 0, d_result: int = 0, stream: int = 0):
        """find_idle (room for len(notes) voices, in scratch the bank owns) and the placement on its list, in one call."""
        arr = fx_note_array(notes)
        q = self._query(first, count, which, settle_q15, start, 0)
        _check(self.L.skred_fxbank_note_on_idle(self.h, C.byref(q), C.cast(arr, C.c_void_p), len(arr), d_assigned or None,
                                                d_result or None, stream or None), "skred_fxbank_note_on_idle")

    def stamp_list(self, d_voices: int, n: int, stamps: int, d_count: int = 0, stream: int = 0):
        """STAMP_TRIGGER / STAMP_RELEASE on the first min(n, d_count[0]) entries of a list in device memory (d_count 0: n entries);
        entries outside the bank are skipped."""
        _check(self.L.skred_fxbank_stamp_list(self.h, d_voices or None, int(n), d_count or None, int(stamps), stream or None),
               "skred_fxbank_stamp_list")

    # ---- voice stealing (include/skred_amd_fxpt.h: skred_fxbank_find_steal / _find_steal_host / _note_on_steal) ----
    def find_steal(self, q: FxStealQueryC, d_voices: int = 0, d_count: int = 0, stream: int = 0):
        """The q.max_out least important sounding voices of the range into d_voices (int32, device memory), most stealable first;
        d_count[0] = written, d_count[1] = total candidates (uint32)."""
        _check(self.L.skred_fxbank_find_steal(self.h, C.byref(q), d_voices or None, d_count or None, stream or None),
               "skred_fxbank_find_steal")

    def find_steal_host(self, q: FxStealQueryC, stream: int = 0):
        """The same into host memory, waiting for `stream` only.  Returns (np.int32 array of the victims, total)."""
        out = np.empty(max(q.max_out, 0), np.int32)
        total = C.c_int(0)
        n = self.L.skred_fxbank_find_steal_host(self.h, C.byref(q), out.ctypes.data if q.max_out > 0 else None, C.byref(total),
                                                stream or None)
        if n < 0:
            _check(n, "skred_fxbank_find_steal_host")
        return out[:n].copy(), int(total.value)

    def note_on_steal(self, notes, idle_q: FxIdleQueryC, steal_q: FxStealQueryC, d_assigned: int = 0, d_result: int = 0,
                      stream: int = 0):
        """Idle voices take the first notes, the victims of steal_q the next ones; d_result[0..2] = placed, dropped, placed on
        stolen voices (uint32)."""
        arr = fx_note_array(notes)
        _check(self.L.skred_fxbank_note_on_steal(self.h, C.byref(idle_q), C.byref(steal_q), C.cast(arr, C.c_void_p), len(arr),
                                                 d_assigned or None, d_result or None, stream or None), "skred_fxbank_note_on_steal")

    # ---- note owners (include/skred_amd_fxpt.h): one uint32 tag per voice on the device, 0 nobody ----
    def tag_list(self, d_voices: int, tags, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """owner[d_voices[k]] = tags[k] for the first min(len(tags), d_count[0]) entries that are voices; d_result[0..1] = tagged,
        entries that are no voice (uint32, may be 0)."""
        t = _tags(tags)
        _check(self.L.skred_fxbank_tag_list(self.h, d_voices or None, t.ctypes.data, len(t), d_count or None, d_result or None,
                                            stream or None), "skred_fxbank_tag_list")

    def find_owned(self, first: int, count: int, tags, d_voices_out: int, stream: int = 0):
        """d_voices_out[k] (int32) = the lowest voice of the range whose owner is tags[k], or -1."""
        t = _tags(tags)
        _check(self.L.skred_fxbank_find_owned(self.h, int(first), int(count), t.ctypes.data, len(t), d_voices_out or None,
                                              stream or None), "skred_fxbank_find_owned")

    def stamp_owned(self, d_voices: int, tags, stamps: int, d_result: int, d_count: int = 0, stream: int = 0):
        """stamp_list under the guard owner[voice] == tags[k]; d_result[0..2] = stamped, owner differs, no voice (uint32)."""
        t = _tags(tags)
        _check(self.L.skred_fxbank_stamp_owned(self.h, d_voices or None, t.ctypes.data, len(t), d_count or None, int(stamps),
                                               d_result or None, stream or None), "skred_fxbank_stamp_owned")

    def release_tags(self, first: int, count: int, tags, stamps: int, d_result: int, stream: int = 0):
        """Note-off by id: each tag stamps the lowest voice of the range that carries it; d_result as stamp_owned's, [1] is 0."""
        t = _tags(tags)
        _check(self.L.skred_fxbank_release_tags(self.h, int(first), int(count), t.ctypes.data, len(t), int(stamps), d_result or None,
                                                stream or None), "skred_fxbank_release_tags")

    def owner_clear(self, first: int, count: int, stream: int = 0):
        _check(self.L.skred_fxbank_owner_clear(self.h, int(first), int(count), stream or None), "skred_fxbank_owner_clear")

    def download_owners(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        count = self.n - first if count is None else count
        out = np.full(max(count, 0), 0xABABABAB, np.uint32)
        _check(self.L.skred_fxbank_download_owners(self.h, out.ctypes.data, int(first), int(count)), "skred_fxbank_download_owners")
        return out

    # ---- controllers: a few parameter words of resident voices, stored by a kernel ----
    def ctl_range(self, ctl: FxCtlC, first: int, count: int, d_result: int = 0, stream: int = 0):
        """The record on every voice of [first, first + count); d_result[0..1] = voices written, stores withheld (uint32, may be 0)."""
        _check(self.L.skred_fxbank_ctl_range(self.h, C.byref(ctl), int(first), int(count), d_result or None, stream or None),
               "skred_fxbank_ctl_range")

    def ctl_list(self, ctl: FxCtlC, d_voices: int, n: int, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """The record on the first min(n, d_count[0]) entries of a device list that are voices of the bank."""
        _check(self.L.skred_fxbank_ctl_list(self.h, C.byref(ctl), d_voices or None, int(n), d_count or None, d_result or None,
                                            stream or None), "skred_fxbank_ctl_list")

    def ctl_owned(self, ctl: FxCtlC, d_voices: int, tags, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """ctl_list under the guard owner[voice] == tags[k]; d_result[0..2] = written, withheld, owner differs."""
        t = _tags(tags)
        _check(self.L.skred_fxbank_ctl_owned(self.h, C.byref(ctl), d_voices or None, t.ctypes.data, len(t), d_count or None,
                                             d_result or None, stream or None), "skred_fxbank_ctl_owned")

    def download_params(self, bank: FxVoiceBank) -> np.ndarray:
        """Every parameter field skred_fxbank_download leaves out, as the device holds it, into `bank` (the flags as 0 / 1);
        returns the reciprocals of the three frame counts, uint32 [n][3]."""
        cb = bank.as_c()
        recip = np.zeros((bank.n, 3), np.uint32)
        _check(self.L.skred_fxbank_download_params(self.h, C.byref(cb), recip.ctypes.data, 0, 0, bank.n), "skred_fxbank_download_params")
        return recip

    # ---- channels and per-note expression: masked owner matches, per-entry controller values ----
    def find_match(self, first: int, count: int, value: int, mask: int, max_out: int = 0, d_voices: int = 0, d_count: int = 0,
                   stream: int = 0):
        """The voices of the range with owner != 0 and (owner & mask) == value, ascending, into d_voices[0 .. min(total, max_out))
        (int32, device memory); d_count[0] = the total (uint32)."""
        m = OwnerMatchC(int(value), int(mask))
        _check(self.L.skred_fxbank_find_match(self.h, int(first), int(count), C.byref(m), int(max_out), d_voices or None,
                                              d_count or None, stream or None), "skred_fxbank_find_match")

    def find_match_host(self, first: int, count: int, value: int, mask: int, max_out: Optional[int] = None, stream: int = 0):
        """The same into host memory, waiting for `stream` only.  Returns (np.int32 array of the listed voices, total)."""
        max_out = count if max_out is None else max_out
        m = OwnerMatchC(int(value), int(mask))
        out = np.empty(max(max_out, 0), np.int32)
        total = C.c_int(0)
        n = self.L.skred_fxbank_find_match_host(self.h, int(first), int(count), C.byref(m), int(max_out),
                                                out.ctypes.data if max_out > 0 else None, C.byref(total), stream or None)
        if n < 0:
            _check(n, "skred_fxbank_find_match_host")
        return out[:n].copy(), int(total.value)

    def stamp_match(self, first: int, count: int, value: int, mask: int, stamps: int, d_result: int, stream: int = 0):
        """stamp_list's stores on every matching voice of the range; d_result[0..1] = stamped, did not match (uint32)."""
        m = OwnerMatchC(int(value), int(mask))
        _check(self.L.skred_fxbank_stamp_match(self.h, int(first), int(count), C.byref(m), int(stamps), d_result or None,
                                               stream or None), "skred_fxbank_stamp_match")

    def ctl_match(self, ctl: FxCtlC, first: int, count: int, value: int, mask: int, d_result: int = 0, stream: int = 0):
        """ctl_range under the match guard; d_result[0..2] = written, withheld, did not match (uint32, may be 0)."""
        m = OwnerMatchC(int(value), int(mask))
        _check(self.L.skred_fxbank_ctl_match(self.h, C.byref(ctl), int(first), int(count), C.byref(m), d_result or None,
                                             stream or None), "skred_fxbank_ctl_match")

    def ctl_owned_each(self, ctl: Optional[FxCtlC], entries, d_voices: int, tags, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """ctl_owned with entry k's record laid over `ctl` (may be None); d_result[0..2] = written, withheld, owner differs."""
        t, arr = _tags(tags), fx_each_array(entries)
        _check(self.L.skred_fxbank_ctl_owned_each(self.h, C.byref(ctl) if ctl is not None else None, C.cast(arr, C.c_void_p),
                                                  d_voices or None, t.ctypes.data, len(t), d_count or None, d_result or None,
                                                  stream or None), "skred_fxbank_ctl_owned_each")

    def ctl_tags_each(self, ctl: Optional[FxCtlC], entries, first: int, count: int, tags, d_result: int = 0, stream: int = 0):
        """Expression by note id: entries[k] on the lowest voice of the range that carries tags[k]; d_result as ctl_owned_each's."""
        t, arr = _tags(tags), fx_each_array(entries)
        _check(self.L.skred_fxbank_ctl_tags_each(self.h, C.byref(ctl) if ctl is not None else None, C.cast(arr, C.c_void_p),
                                                 int(first), int(count), t.ctypes.data, len(t), d_result or None, stream or None),
               "skred_fxbank_ctl_tags_each")

    # ---- per-note timbre (include/skred_amd_fxpt.h: skred_fxbank_ctl_owned_each_filter / _ctl_tags_each_filter) ----
    def ctl_owned_each_filter(self, ctl: Optional[FxCtlC], entries, filt, d_voices: int, tags, d_count: int = 0, d_result: int = 0,
                              stream: int = 0):
        """ctl_owned_each with entry k's five coefficients filt[k] (entries None: the coefficients only); d_result as there."""
        t, f = _tags(tags), fx_filter_each_array(filt)
        arr = fx_each_array(entries) if entries is not None else None
        assert len(f) == len(t) and (arr is None or len(arr) == len(t)), "one entry per tag"
        _check(self.L.skred_fxbank_ctl_owned_each_filter(self.h, C.byref(ctl) if ctl is not None else None,
                                                         C.cast(arr, C.c_void_p) if arr is not None else None, C.cast(f, C.c_void_p),
                                                         d_voices or None, t.ctypes.data, len(t), d_count or None, d_result or None,
                                                         stream or None), "skred_fxbank_ctl_owned_each_filter")

    def ctl_tags_each_filter(self, ctl: Optional[FxCtlC], entries, filt, first: int, count: int, tags, d_result: int = 0, stream: int = 0):
        """Timbre by note id: filt[k] (and entries[k]) on the lowest voice of the range that carries tags[k]."""
        t, f = _tags(tags), fx_filter_each_array(filt)
        arr = fx_each_array(entries) if entries is not None else None
        assert len(f) == len(t) and (arr is None or len(arr) == len(t)), "one entry per tag"
        _check(self.L.skred_fxbank_ctl_tags_each_filter(self.h, C.byref(ctl) if ctl is not None else None,
                                                        C.cast(arr, C.c_void_p) if arr is not None else None, C.cast(f, C.c_void_p),
                                                        int(first), int(count), t.ctypes.data, len(t), d_result or None, stream or None),
               "skred_fxbank_ctl_tags_each_filter")

    # ---- channel polyphony (include/skred_amd_fxpt.h: skred_fxbank_find_steal_match / _find_steal_match_host / _note_on_channel) ----
    def find_steal_match(self, q: FxStealQueryC, value: int, mask: int, d_voices: int = 0, d_count: int = 0, stream: int = 0):
        """find_steal among the voices with owner != 0 and (owner & mask) == value; d_count[0..2] = written, total candidates, the
        sounding voices of the match in the range (uint32)."""
        m = OwnerMatchC(int(value), int(mask))
        _check(self.L.skred_fxbank_find_steal_match(self.h, C.byref(q), C.byref(m), d_voices or None, d_count or None, stream or None),
               "skred_fxbank_find_steal_match")

    def find_steal_match_host(self, q: FxStealQueryC, value: int, mask: int, stream: int = 0):
        """The same into host memory, waiting for `stream` only.  Returns (np.int32 array of the victims, total, sounding)."""
        m = OwnerMatchC(int(value), int(mask))
        out = np.empty(max(q.max_out, 0), np.int32)
        total, sounding = C.c_int(0), C.c_int(0)
        n = self.L.skred_fxbank_find_steal_match_host(self.h, C.byref(q), C.byref(m), out.ctypes.data if q.max_out > 0 else None,
                                                      C.byref(total), C.byref(sounding), stream or None)
        if n < 0:
            _check(n, "skred_fxbank_find_steal_match_host")
        return out[:n].copy(), int(total.value), int(sounding.value)

    def note_on_channel(self, notes, idle_q: FxIdleQueryC, steal_q: FxStealQueryC, value: int, mask: int, cap: int, tags,
                        d_assigned: int = 0, d_result: int = 0, stream: int = 0):
        """A burst of one channel under a polyphony cap: idle voices as far as the cap allows, then the channel's own victims; every
        placed note k is tagged tags[k]; d_result[0..3] = placed, dropped, stolen, the channel's sounding count before (uint32)."""
        arr, t, m = fx_note_array(notes), _tags(tags), OwnerMatchC(int(value), int(mask))
        _check(self.L.skred_fxbank_note_on_channel(self.h, C.byref(idle_q), C.byref(steal_q), C.byref(m), int(cap),
                                                   C.cast(arr, C.c_void_p), t.ctypes.data, len(arr), d_assigned or None,
                                                   d_result or None, stream or None), "skred_fxbank_note_on_channel")

    # ---- pedals (include/skred_amd_fxpt.h: skred_fxbank_stamp_owned_pedal / _release_tags_pedal / _pedal_latch / _pedal_up) ----
    def stamp_owned_pedal(self, d_voices: int, tags, hold_all: bool, d_result: int, d_count: int = 0, stream: int = 0):
        """stamp_owned's release, held back (PEDAL_PENDING) where hold_all is set or the voice is PEDAL_LATCHED; d_result[0..3] =
        stamped, owner differs, no voice, held back (uint32)."""
        t = _tags(tags)
        _check(self.L.skred_fxbank_stamp_owned_pedal(self.h, d_voices or None, t.ctypes.data, len(t), d_count or None, int(bool(hold_all)),
                                                     d_result or None, stream or None), "skred_fxbank_stamp_owned_pedal")

    def release_tags_pedal(self, first: int, count: int, tags, hold_all: bool, d_result: int, stream: int = 0):
        """Note-off by note id under the pedals: every tag reaches the lowest voice of the range that carries it.  d_result as for
        stamp_owned_pedal; [2] counts the tags nobody carries."""
        t = _tags(tags)
        _check(self.L.skred_fxbank_release_tags_pedal(self.h, int(first), int(count), t.ctypes.data, len(t), int(bool(hold_all)),
                                                      d_result or None, stream or None), "skred_fxbank_release_tags_pedal")

    def pedal_latch(self, first: int, count: int, value: int, mask: int, d_result: int, stream: int = 0):
        """Sostenuto down: PEDAL_LATCHED on the matching voices that are held and not pending; d_result[0..1] = voices that satisfy
        the rule, voices that did not match (uint32)."""
        m = OwnerMatchC(int(value), int(mask))
        _check(self.L.skred_fxbank_pedal_latch(self.h, int(first), int(count), C.byref(m), d_result or None, stream or None),
               "skred_fxbank_pedal_latch")

    def pedal_up(self, first: int, count: int, value: int, mask: int, flags: int, d_result: int, stream: int = 0):
        """A pedal goes up (PEDAL_LIFT_* / PEDAL_SUSTAIN_DOWN): the held-back note-offs of the matching voices are stamped now.
        d_result[0..2] = released, still pending, did not match (uint32)."""
        m = OwnerMatchC(int(value), int(mask))
        _check(self.L.skred_fxbank_pedal_up(self.h, int(first), int(count), C.byref(m), int(flags), d_result or None, stream or None),
               "skred_fxbank_pedal_up")

    def pedal_clear(self, first: int = 0, count: Optional[int] = None, stream: int = 0):
        count = self.n - first if count is None else count
        _check(self.L.skred_fxbank_pedal_clear(self.h, int(first), int(count), stream or None), "skred_fxbank_pedal_clear")

    def download_pedals(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The pedal words of [first, first + count) (uint32); waits for the device.  Zeros on a bank without a pedal array."""
        count = self.n - first if count is None else count
        out = np.full(max(count, 0), 0xABABABAB, np.uint32)
        _check(self.L.skred_fxbank_download_pedals(self.h, out.ctypes.data, int(first), int(count)), "skred_fxbank_download_pedals")
        return out

    # ---- portamento (include/skred_amd_fxpt.h: skred_fxbank_glide_owned / _glide_tags / _glide_advance / _glide_stop) ----
    def glide_owned(self, glides, d_voices: int, tags, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """Entry k starts glides[k] on d_voices[k] where that voice's owner is tags[k].  d_result (uint32[3], may be 0) = voices set
        gliding, starts withheld, voices whose owner differs."""
        arr, t = glide_array(glides), _tags(tags)
        assert len(arr) == len(t), "one glide per tag"
        _check(self.L.skred_fxbank_glide_owned(self.h, C.cast(arr, C.c_void_p), d_voices or None, t.ctypes.data, len(t), d_count or None,
                                               d_result or None, stream or None), "skred_fxbank_glide_owned")

    def glide_tags(self, glides, first: int, count: int, tags, d_result: int = 0, stream: int = 0):
        """Glides by note id: glides[k] starts on the lowest voice of the range that carries tags[k]."""
        arr, t = glide_array(glides), _tags(tags)
        assert len(arr) == len(t), "one glide per tag"
        _check(self.L.skred_fxbank_glide_tags(self.h, C.cast(arr, C.c_void_p), int(first), int(count), t.ctypes.data, len(t),
                                              d_result or None, stream or None), "skred_fxbank_glide_tags")

    def glide_advance(self, first: int, count: int, frames: int, d_result: int = 0, stream: int = 0):
        """Every gliding voice of the range moves on by `frames` frames (one step per 64) or lands on its target.  d_result
        (uint32[2], may be 0) = still gliding, arrived."""
        _check(self.L.skred_fxbank_glide_advance(self.h, int(first), int(count), int(frames), d_result or None, stream or None),
               "skred_fxbank_glide_advance")

    def glide_stop(self, first: int = 0, count: Optional[int] = None, snap: bool = False, stream: int = 0):
        count = self.n - first if count is None else count
        _check(self.L.skred_fxbank_glide_stop(self.h, int(first), int(count), int(bool(snap)), stream or None), "skred_fxbank_glide_stop")

    def download_glide(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The glide words of [first, first + count) as a (count, 4) uint32 array: target, up_q32, down_q32, carry; waits for the
        device.  Zeros on a bank that never started a glide."""
        count = self.n - first if count is None else count
        out = np.full((max(count, 0), 4), 0xABABABAB, np.uint32)
        _check(self.L.skred_fxbank_download_glide(self.h, out.ctypes.data, int(first), int(count)), "skred_fxbank_download_glide")
        return out

    # ---- pitch wheel (include/skred_amd_fxpt.h: skred_fxbank_bend_match / _bend_owned_each / _bend_tags_each / _bend_clear) ----
    def bend_match(self, first: int, count: int, value: int, mask: int, ratio_q24: int, d_result: int = 0, stream: int = 0):
        """The channel wheel: the absolute bend to ratio_q24 (FX_BEND_ONE: the centre, which gives the key's bits back) on every
        matching voice of the range.  d_result (uint32[3], may be 0) = stored or restored, withheld, did not match."""
        m = OwnerMatchC(int(value), int(mask))
        _check(self.L.skred_fxbank_bend_match(self.h, int(first), int(count), C.byref(m), int(ratio_q24), d_result or None, stream or None),
               "skred_fxbank_bend_match")

    def bend_owned_each(self, ratios_q24, d_voices: int, tags, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """Entry k bends d_voices[k] to ratios_q24[k] where that voice's owner is tags[k].  d_result (uint32[3], may be 0) = stored or
        restored, withheld, voices whose owner differs."""
        r, t = bend_ratios(ratios_q24), _tags(tags)
        assert len(r) == len(t), "one ratio per tag"
        _check(self.L.skred_fxbank_bend_owned_each(self.h, r.ctypes.data, d_voices or None, t.ctypes.data, len(t), d_count or None,
                                                   d_result or None, stream or None), "skred_fxbank_bend_owned_each")

    def bend_tags_each(self, ratios_q24, first: int, count: int, tags, d_result: int = 0, stream: int = 0):
        """Bends by note id: ratios_q24[k] on the lowest voice of the range that carries tags[k]."""
        r, t = bend_ratios(ratios_q24), _tags(tags)
        assert len(r) == len(t), "one ratio per tag"
        _check(self.L.skred_fxbank_bend_tags_each(self.h, r.ctypes.data, int(first), int(count), t.ctypes.data, len(t), d_result or None,
                                                  stream or None), "skred_fxbank_bend_tags_each")

    def bend_clear(self, first: int = 0, count: Optional[int] = None, snap: bool = False, stream: int = 0):
        count = self.n - first if count is None else count
        _check(self.L.skred_fxbank_bend_clear(self.h, int(first), int(count), int(bool(snap)), stream or None), "skred_fxbank_bend_clear")

    def download_bend(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The bend words of [first, first + count) as a (count, 2) uint32 array: key, ratio_q24; waits for the device.  Zeros on a
        bank that never bent."""
        count = self.n - first if count is None else count
        out = np.full((max(count, 0), 2), 0xABABABAB, np.uint32)
        _check(self.L.skred_fxbank_download_bend(self.h, out.ctypes.data, int(first), int(count)), "skred_fxbank_download_bend")
        return out

    # ---- filter cutoff (include/skred_amd_fxpt.h: skred_fxbank_cutoff_match / _cutoff_owned_each / _cutoff_tags_each / _cutoff_advance /
    # _cutoff_stop) ----
    def cutoff_match(self, first: int, count: int, value: int, mask: int, rec: FxCutoffC, d_result: int = 0, stream: int = 0):
        """The channel sweep: the record on every matching voice of the range.  d_result (uint32[4], may be 0) = set or started,
        withheld, did not match, clamped."""
        m = OwnerMatchC(int(value), int(mask))
        _check(self.L.skred_fxbank_cutoff_match(self.h, int(first), int(count), C.byref(m), C.byref(rec), d_result or None, stream or None),
               "skred_fxbank_cutoff_match")

    def cutoff_owned_each(self, recs, d_voices: int, tags, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """Entry k brings recs[k] to d_voices[k] where that voice's owner is tags[k].  d_result (uint32[4], may be 0) = set or started,
        withheld, voices whose owner differs, clamped."""
        arr, t = fx_cutoff_array(recs), _tags(tags)
        assert len(arr) == len(t), "one record per tag"
        _check(self.L.skred_fxbank_cutoff_owned_each(self.h, C.cast(arr, C.c_void_p), d_voices or None, t.ctypes.data, len(t), d_count or None,
                                                     d_result or None, stream or None), "skred_fxbank_cutoff_owned_each")

    def cutoff_tags_each(self, recs, first: int, count: int, tags, d_result: int = 0, stream: int = 0):
        """By note id: recs[k] on the lowest voice of the range that carries tags[k]."""
        arr, t = fx_cutoff_array(recs), _tags(tags)
        assert len(arr) == len(t), "one record per tag"
        _check(self.L.skred_fxbank_cutoff_tags_each(self.h, C.cast(arr, C.c_void_p), int(first), int(count), t.ctypes.data, len(t),
                                                    d_result or None, stream or None), "skred_fxbank_cutoff_tags_each")

    def cutoff_advance(self, first: int, count: int, frames: int, d_result: int = 0, stream: int = 0):
        """The advance pass by `frames`: d_result (uint32[2], may be 0) = still moving, arrived."""
        _check(self.L.skred_fxbank_cutoff_advance(self.h, int(first), int(count), int(frames), d_result or None, stream or None),
               "skred_fxbank_cutoff_advance")

    def cutoff_stop(self, first: int = 0, count: Optional[int] = None, snap: bool = False, stream: int = 0):
        count = self.n - first if count is None else count
        _check(self.L.skred_fxbank_cutoff_stop(self.h, int(first), int(count), int(bool(snap)), stream or None), "skred_fxbank_cutoff_stop")

    def download_cutoff(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The cutoff words of [first, first + count) as a (count, 8) uint32 array: w_q29, target_q29, up_q32, down_q32, carry, q_q16,
        mode, 0; waits for the device.  Zeros on a bank that never set a cutoff."""
        count = self.n - first if count is None else count
        out = np.full((max(count, 0), 8), 0xABABABAB, np.uint32)
        _check(self.L.skred_fxbank_download_cutoff(self.h, out.ctypes.data, int(first), int(count)), "skred_fxbank_download_cutoff")
        return out

    # ---- filter envelope (include/skred_amd_fxpt.h: skred_fxbank_fenv_match / _fenv_owned_each / _fenv_tags_each / _download_fenv; the
    # contour is stepped by cutoff_advance above) ----
    def fenv_match(self, first: int, count: int, value: int, mask: int, rec: FxFenvC, d_result: int = 0, stream: int = 0):
        """The channel sweep: the record on every matching voice of the range.  d_result (uint32[4], may be 0) = started, withheld, did
        not match, clamped."""
        m = OwnerMatchC(int(value), int(mask))
        _check(self.L.skred_fxbank_fenv_match(self.h, int(first), int(count), C.byref(m), C.byref(rec), d_result or None, stream or None),
               "skred_fxbank_fenv_match")

    def fenv_owned_each(self, recs, d_voices: int, tags, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """Entry k brings recs[k] to d_voices[k] where that voice's owner is tags[k].  d_result (uint32[4], may be 0) = started, withheld,
        voices whose owner differs, clamped."""
        arr, t = fx_fenv_array(recs), _tags(tags)
        assert len(arr) == len(t), "one record per tag"
        _check(self.L.skred_fxbank_fenv_owned_each(self.h, C.cast(arr, C.c_void_p), d_voices or None, t.ctypes.data, len(t), d_count or None,
                                                   d_result or None, stream or None), "skred_fxbank_fenv_owned_each")

    def fenv_tags_each(self, recs, first: int, count: int, tags, d_result: int = 0, stream: int = 0):
        """By note id: recs[k] on the lowest voice of the range that carries tags[k]."""
        arr, t = fx_fenv_array(recs), _tags(tags)
        assert len(arr) == len(t), "one record per tag"
        _check(self.L.skred_fxbank_fenv_tags_each(self.h, C.cast(arr, C.c_void_p), int(first), int(count), t.ctypes.data, len(t),
                                                  d_result or None, stream or None), "skred_fxbank_fenv_tags_each")

    def download_fenv(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The fenv words of [first, first + count) as a (count, 8) uint32 array: stage, w_peak, w_sustain, w_end, rate_attack_q32,
        rate_decay_q32, rate_release_q32, 0; waits for the device.  Zeros on a bank without the array."""
        count = self.n - first if count is None else count
        out = np.full((max(count, 0), 8), 0xABABABAB, np.uint32)
        _check(self.L.skred_fxbank_download_fenv(self.h, out.ctypes.data, int(first), int(count)), "skred_fxbank_download_fenv")
        return out


# ------------------------------------------------------------------ synthetic fixed-point bank

def fx_lut_pool() -> Tuple[np.ndarray, dict]:
    """All notamy int16 LUTs concatenated; returns (pool, {name: (offset, log2_size, highest_harmonic)})."""
    z, names, meta = banks.load_luts()
    info, pos, parts = {}, 0, []
    for nm in names:
        t = z["i16_" + nm]
        info[nm] = (pos, meta[nm]["log2_size"], meta[nm]["highest_harmonic"])
        parts.append(t)
        pos += len(t)
    return np.concatenate(parts).astype(np.int16), info


# what bench.py's `fixed_point` leg says about itself
DTYPE_NOTE = "q15 gains / u32 phase / q2.30 x q12 biquad / i64 mix"
WORKLOAD_NOTE = ("fixed-point analogue of the C2 recipe (fxbank.bank_fx): int16 LUT pyramids, linear interpolation, "
                 "per-voice biquad (modes 1-4), ADSR, amp smoother")


def q30_coeffs(mode, freq, q, sample_rate) -> Dict[str, np.ndarray]:
    """RBJ coefficients (banks.biquad_coeffs == mmf_set_params, synth.c:929-1008) rounded to Q2.30."""
    co = banks.biquad_coeffs(mode, freq, q, sample_rate)
    return {k + "_q30": np.clip(np.round(co[k].astype(np.float64) * (1 << 30)), -(1 << 31), (1 << 31) - 1).astype(np.int32)
            for k in ("b0", "b1", "b2", "a1", "a2")}


def bank_fx(n: int = 65536, sample_rate: int = 48000, seed: int = banks.SEED, with_filter: bool = True):
    """Fixed-point analogue of the C2 recipe: v mod 3 -> sine / triangle / impulse int16 pyramids (level by frequency),
    biquad mode 1 + v mod 4 with K ~ logU[100, 8000] Hz and Q ~ U[0.5, 4] (the float recipe's draws), ADSR
    0.01/0.1/0.7/0.2 s, staggered note-ons, smoother k=0.02."""
    pool, info = fx_lut_pool()
    u5 = banks.lcg_uniform(5 * n, seed).reshape(5, n)
    u = u5[:3]
    freq = (np.float32(27.5) * np.exp2(np.float32(7.0) * u[0])).astype(np.float64)
    b = FxVoiceBank(n)
    fam = np.arange(n) % 3
    off = np.zeros(n, np.int32)
    lg = np.zeros(n, np.int32)
    for f_id, family in enumerate(("sine", "triangle", "impulse")):
        levels = [k for k in info if k.startswith(family + "_")]
        hh = np.array([info[k][2] for k in levels], np.float64)
        sel = np.where(fam == f_id)[0]
        ok = hh[None, :] * freq[sel, None] <= sample_rate / 2.0
        lvl = np.where(ok.any(1), ok.argmax(1), len(levels) - 1)
        off[sel] = np.array([info[levels[k]][0] for k in lvl], np.int32)
        lg[sel] = np.array([info[levels[k]][1] for k in lvl], np.int32)
    b["table_offset"], b["log2_size"] = off, lg
    b["phase_inc"] = np.round(freq / sample_rate * 4294967296.0).astype(np.uint64).astype(np.uint32)
    b["phase"] = (u[2].astype(np.float64) * 4294967295.0).astype(np.uint64).astype(np.uint32)
    b["amp_q15"] = 32768
    pan = u[1].astype(np.float64) * 2.0 - 1.0
    b["pan_left_q15"] = np.round((1.0 - pan) / 2.0 * 32768).astype(np.int32)
    b["pan_right_q15"] = np.round((1.0 + pan) / 2.0 * 32768).astype(np.int32)
    b["use_envelope"] = 1
    b["attack_frames"] = int(0.01 * sample_rate)
    b["decay_frames"] = int(0.1 * sample_rate)
    b["release_frames"] = int(0.2 * sample_rate)
    b["sustain_q15"] = int(0.7 * 32768)
    count0 = 2 * sample_rate
    stagger = np.minimum((u[2] * np.float32(sample_rate)).astype(np.int64), sample_rate - 1)
    b["sample_start"] = (count0 - stagger).astype(np.uint64)
    b["is_active"] = 1
    b["smoother_enable"] = 1
    b["smoother_k_q15"] = int(round(0.02 * 32768))
    if with_filter:
        mode = (1 + np.arange(n) % 4).astype(np.int32)
        cutoff = (np.float32(100.0) * np.power(np.float32(80.0), u5[3])).astype(np.float32)
        q = (np.float32(0.5) + np.float32(3.5) * u5[4]).astype(np.float32)
        for k, v in q30_coeffs(mode, cutoff, q, sample_rate).items():
            b[k] = v
        b["filter_mode"] = mode
    return b, pool, count0
