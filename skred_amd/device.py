"""ctypes binding of libskred_amd.so (the C ABI in include/skred_amd.h).

This is plumbing for tests and bench.py; the product is the shared library.  There is no
fallback of any kind: a missing library or a machine without a usable GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from .bank import GlobalsC, SlotQueryC, SlotStealQueryC, VoiceBank, VoiceBankC, slot_query, slot_steal_query  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SKRED_AMD_LIB", os.path.join(_HERE, "libskred_amd.so"))   # override: A/B builds

# every symbol include/skred_amd.h declares
ABI_SYMBOLS = [
    "skred_amd_abi_version", "skred_amd_device_count", "skred_amd_last_error",
    "skred_bank_create", "skred_bank_destroy", "skred_bank_n_voices",
    "skred_bank_set_tables_f32", "skred_bank_upload", "skred_bank_download",
    "skred_bank_set_globals", "skred_bank_get_globals",
    "skred_bank_render", "skred_bank_master", "skred_bank_render_mix", "skred_bank_render_host",
    "skred_bank_last_render_ms", "skred_bank_timing_reset", "skred_bank_timing_summary",
    "skred_bank_set_option", "skred_bank_last_kernel", "skred_bank_last_in_place", "skred_bank_last_split", "skred_bank_last_pack", "skred_bank_last_cz", "skred_bank_list_violations", "skred_bank_set_probe",
    "skred_bank_set_taps", "skred_bank_last_taps",
    "skred_bank_set_form_counter", "skred_bank_last_cross_group",
    "skred_bank_update", "skred_bank_defer", "skred_bank_run_queue", "skred_bank_queue_pending",
    "skred_shard_partition", "skred_shard_cut_ok", "skred_shard_create", "skred_shard_create_custom", "skred_shard_destroy",
    "skred_shard_bank", "skred_shard_range", "skred_shard_upload", "skred_shard_set_ops", "skred_shard_rccl_unique_id",
    "skred_shard_init_rccl", "skred_shard_render_mix", "skred_shard_render_mix_pipelined", "skred_shard_flush",
    "skred_seq_create", "skred_seq_destroy", "skred_seq_tempo_set", "skred_seq_time_per_step", "skred_seq_step_set",
    "skred_seq_mute_set", "skred_seq_modulo_set", "skred_seq_state_set", "skred_seq_pattern_reset", "skred_seq_pointer",
    "skred_seq_counter", "skred_seq_tick",
    "skred_bank_seq", "skred_bank_set_sample_rate", "skred_bank_pattern_step_set", "skred_bank_pattern_step_clear",
    "skred_bank_find_idle", "skred_bank_find_idle_host",
    "skred_bank_notes_on_list", "skred_bank_note_on_idle", "skred_bank_stamp_list",
    "skred_bank_find_steal", "skred_bank_find_steal_host", "skred_bank_note_on_steal",
    "skred_bank_find_idle_slots", "skred_bank_find_idle_slots_host", "skred_bank_notes_on_slots", "skred_bank_note_on_idle_slots",
    "skred_bank_stamp_slots",
    "skred_bank_find_steal_slots", "skred_bank_find_steal_slots_host", "skred_bank_note_on_steal_slots",
    "skred_bank_ctl_range", "skred_bank_ctl_slots", "skred_bank_download_ctl",
    "skred_bank_tag_slots", "skred_bank_find_owned", "skred_bank_stamp_owned", "skred_bank_release_tags", "skred_bank_ctl_owned",
    "skred_bank_owner_clear", "skred_bank_download_owners", "skred_bank_download_env_clocks",
    "skred_bank_find_match", "skred_bank_find_match_host", "skred_bank_stamp_match", "skred_bank_ctl_match",
    "skred_bank_ctl_owned_each", "skred_bank_ctl_tags_each",
    "skred_bank_ctl_owned_each_filter", "skred_bank_ctl_tags_each_filter",
    "skred_bank_find_steal_slots_match", "skred_bank_find_steal_slots_match_host", "skred_bank_note_on_channel",
    "skred_bank_stamp_owned_pedal", "skred_bank_release_tags_pedal", "skred_bank_pedal_latch", "skred_bank_pedal_up",
    "skred_bank_pedal_clear", "skred_bank_download_pedals",
    "skred_bank_glide_owned", "skred_bank_glide_tags", "skred_bank_glide_advance", "skred_bank_glide_stop", "skred_bank_download_glide",
    "skred_bank_bend_match", "skred_bank_bend_owned_each", "skred_bank_bend_tags_each", "skred_bank_bend_clear", "skred_bank_download_bend",
    "skred_bank_cutoff_match", "skred_bank_cutoff_owned_each", "skred_bank_cutoff_tags_each", "skred_bank_cutoff_advance",
    "skred_bank_cutoff_stop", "skred_bank_download_cutoff",
    "skred_bank_fenv_match", "skred_bank_fenv_owned_each", "skred_bank_fenv_tags_each", "skred_bank_download_fenv",
]
# ... and the one it declares outside the skred_amd_ / skred_bank_ / skred_shard_ / skred_seq_ families (pure host, no handle)
HOST_ABI_SYMBOLS = ["skred_notes_check", "skred_steal_check", "skred_slot_query_check", "skred_slot_notes_check", "skred_slot_steal_check",
                    "skred_ctl_check", "skred_owner_tags_check", "skred_owner_match_check", "skred_ctl_each_check",
                    "skred_filter_each_check", "skred_filter_coeffs",
                    "skred_chan_check", "skred_pedal_check", "skred_glide_check", "skred_bend_check",
                    "skred_cutoff_check", "skred_filter_coeffs_w", "skred_fenv_check"]

# SKRED_DIRTY_* / SKRED_STAMP_* of include/skred_amd.h
DIRTY_PARAMS, DIRTY_PHASE, DIRTY_ENV_STATE, DIRTY_PAN = 1, 2, 4, 8
DIRTY_FILTER_STATE, DIRTY_SMOOTHER, DIRTY_HOLD, DIRTY_SAMPLE = 16, 32, 64, 128
STAMP_TRIGGER, STAMP_RELEASE, DIRTY_ENV_CLOCK = 256, 512, 1024
# SKRED_IDLE_* (skred_bank_find_idle)
IDLE_FINISHED, IDLE_ENV_DONE, IDLE_AMP_ZERO, IDLE_UNNAMED = 1, 2, 4, 256


class IdleQueryC(C.Structure):
    """ctypes image of ``skred_idle_query_t``."""
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("which", C.c_uint32), ("settle_level", C.c_float),
                ("start", C.c_int32), ("max_out", C.c_int32)]          # `start`: the header's `from`

# SKRED_STEAL_* (skred_bank_find_steal)
STEAL_MAX = 1024
STEAL_OLDEST, STEAL_QUIETEST = 0, 1
STEAL_RELEASED_FIRST, STEAL_RELEASED_ONLY, STEAL_UNNAMED = 1, 2, 256


class StealQueryC(C.Structure):
    """ctypes image of ``skred_steal_query_t`` (40 bytes)."""
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("policy", C.c_uint32), ("flags", C.c_uint32),
                ("min_age", C.c_uint64), ("exclude_idle", C.c_uint32), ("settle_level", C.c_float),
                ("max_out", C.c_int32), ("reserved", C.c_int32)]


def steal_query(first: int, count: int, policy: int = STEAL_OLDEST, flags: int = 0, min_age: int = 0, exclude_idle: int = 0,
                settle_level: float = 0.0, max_out: int = 0) -> StealQueryC:
    return StealQueryC(int(first), int(count), int(policy), int(flags), int(min_age), int(exclude_idle), float(settle_level),
                       int(max_out), 0)

# SKRED_NOTE_* (skred_bank_notes_on_list)
NOTE_SET_PHASE, NOTE_SET_PAN = 1, 2


class NoteC(C.Structure):
    """ctypes image of ``skred_note_t`` (32 bytes)."""
    _fields_ = [("phase_inc", C.c_float), ("velocity", C.c_float), ("phase", C.c_float), ("pan_left", C.c_float),
                ("pan_right", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


def note_array(notes):
    """A contiguous ``NoteC`` array from a sequence of NoteC (a ctypes array of NoteC passes through)."""
    if isinstance(notes, C.Array) and notes._type_ is NoteC:
        return notes
    notes = list(notes)
    return (NoteC * len(notes))(*notes)


# SKRED_CTL_* (skred_bank_ctl_range / _ctl_slots)
CTL_PHASE_INC, CTL_INC_SCALE, CTL_AMP, CTL_PAN, CTL_FILTER, CTL_ENV_TIMES, CTL_VELOCITY, CTL_SMOOTHING = (1 << i for i in range(8))
CTL_FM_DEPTH, CTL_FREQ_SCALE, CTL_AM_DEPTH, CTL_PAN_DEPTH, CTL_CZ_DEPTH, CTL_CZ_DIST = (1 << i for i in range(8, 14))
CTL_ALL = (1 << 14) - 1


class CtlC(C.Structure):
    """ctypes image of ``skred_ctl_t`` (96 bytes): `set` names the fields the record stores."""
    _fields_ = [("set", C.c_uint32)] + [(name, C.c_float) for name in (
        "phase_inc", "inc_scale", "amp", "pan_left", "pan_right", "b0", "b1", "b2", "a1", "a2",
        "attack_time", "decay_time", "sustain_level", "release_time", "velocity", "smoothing",
        "fm_depth", "freq_scale", "am_depth", "pan_depth", "cz_depth", "cz_dist")] + [("reserved", C.c_uint32)]


def ctl(set: int = 0, **values) -> CtlC:
    """A controller record: ``ctl(CTL_AMP | CTL_PAN, amp=0.5, pan_left=0.2, pan_right=0.8)``."""
    c = CtlC()
    c.set = int(set)
    for k, v in values.items():
        setattr(c, k, v)
    return c


def ctl_array(ctls):
    """A contiguous ``CtlC`` array from a sequence of CtlC (a ctypes array of CtlC passes through)."""
    if isinstance(ctls, C.Array) and ctls._type_ is CtlC:
        return ctls
    ctls = list(ctls)
    return (CtlC * len(ctls))(*ctls)


# SKRED_OWNER_* (skred_bank_tag_slots / _find_owned / _stamp_owned / _release_tags / _ctl_owned)
OWNER_MAX_TAGS = 1024
OWNER_ALLOW_ZERO, OWNER_UNIQUE = 1, 2


def tag_array(tags) -> np.ndarray:
    """A contiguous uint32 array of note tags."""
    return np.ascontiguousarray(tags, dtype=np.uint32)


# SKRED_EACH_* (skred_bank_ctl_owned_each / _ctl_tags_each)
EACH_INC_SCALE, EACH_AMP_SCALE, EACH_VELOCITY, EACH_PAN = 1, 2, 4, 8
EACH_ALL = 15


class OwnerMatchC(C.Structure):
    """ctypes image of ``skred_owner_match_t``: a slot matches when owner != 0 and (owner & mask) == value."""
    _fields_ = [("value", C.c_uint32), ("mask", C.c_uint32)]


def owner_match(value: int = 0, mask: int = 0) -> OwnerMatchC:
    return OwnerMatchC(int(value) & 0xFFFFFFFF, int(mask) & 0xFFFFFFFF)


class CtlEachC(C.Structure):
    """ctypes image of ``skred_ctl_each_t`` (32 bytes): `set` names the values entry k brings."""
    _fields_ = [("set", C.c_uint32), ("inc_scale", C.c_float), ("amp_scale", C.c_float), ("velocity", C.c_float),
                ("pan_left", C.c_float), ("pan_right", C.c_float), ("reserved", C.c_uint32 * 2)]


def ctl_each(set: int = 0, **values) -> CtlEachC:
    """A per-entry record: ``ctl_each(EACH_INC_SCALE | EACH_PAN, inc_scale=1.01, pan_left=0.2, pan_right=0.8)``."""
    e = CtlEachC()
    e.set = int(set)
    for k, v in values.items():
        setattr(e, k, v)
    return e


def ctl_each_array(each):
    """A contiguous ``CtlEachC`` array from a sequence of CtlEachC (a ctypes array of CtlEachC passes through)."""
    if isinstance(each, C.Array) and each._type_ is CtlEachC:
        return each
    each = list(each)
    return (CtlEachC * len(each))(*each)


class FilterEachC(C.Structure):
    """ctypes image of ``skred_filter_each_t`` (32 bytes): the five biquad coefficients entry k brings."""
    _fields_ = [("b0", C.c_float), ("b1", C.c_float), ("b2", C.c_float), ("a1", C.c_float), ("a2", C.c_float), ("reserved", C.c_uint32 * 3)]


def filter_each(b0: float = 0.0, b1: float = 0.0, b2: float = 0.0, a1: float = 0.0, a2: float = 0.0) -> FilterEachC:
    """One set of per-entry coefficients: ``filter_each(*filter_coeffs(1, 880.0, 0.9, 44100.0))``."""
    return FilterEachC(b0, b1, b2, a1, a2)


def filter_each_array(filt):
    """A contiguous ``FilterEachC`` array from a sequence of FilterEachC (a ctypes array of FilterEachC passes through)."""
    if isinstance(filt, C.Array) and filt._type_ is FilterEachC:
        return filt
    filt = list(filt)
    return (FilterEachC * len(filt))(*filt)


# SKRED_PEDAL_* (skred_bank_stamp_owned_pedal / _release_tags_pedal / _pedal_latch / _pedal_up)
PEDAL_PENDING, PEDAL_LATCHED = 1, 2
PEDAL_LIFT_SUSTAIN, PEDAL_LIFT_SOSTENUTO, PEDAL_SUSTAIN_DOWN = 1, 2, 4
PEDAL_CALL_STAMP_OWNED, PEDAL_CALL_RELEASE_TAGS, PEDAL_CALL_LATCH, PEDAL_CALL_UP = 0, 1, 2, 3


# SKRED_GLIDE_* (skred_bank_glide_owned / _glide_tags)
GLIDE_FROM_SCALE, GLIDE_TO_SCALE = 1, 2


class GlideC(C.Structure):
    """ctypes image of ``skred_glide_t`` (32 bytes): `set` is exactly one of GLIDE_FROM_SCALE and GLIDE_TO_SCALE."""
    _fields_ = [("set", C.c_uint32), ("rate_up", C.c_float), ("rate_down", C.c_float), ("scale", C.c_float), ("reserved", C.c_uint32 * 4)]


def glide(set: int, rate_up: float, rate_down: float, scale: float) -> GlideC:
    """One glide: ``glide(GLIDE_FROM_SCALE, 2 ** (1 / 96), 2 ** (-1 / 96), 2 ** (-7 / 12))`` slides up a fifth into the note."""
    return GlideC(int(set), rate_up, rate_down, scale)


def glide_array(glides):
    """A contiguous ``GlideC`` array from a sequence of GlideC (a ctypes array of GlideC passes through)."""
    if isinstance(glides, C.Array) and glides._type_ is GlideC:
        return glides
    glides = list(glides)
    return (GlideC * len(glides))(*glides)


# SKRED_CUTOFF_* (skred_bank_cutoff_match / _cutoff_owned_each / _cutoff_tags_each)
CUTOFF_ABS, CUTOFF_TRACK, CUTOFF_GLIDE, CUTOFF_Q, CUTOFF_MODE = 1, 2, 4, 8, 16
CUTOFF_W_MIN, CUTOFF_W_MAX, CUTOFF_Q_MIN, CUTOFF_Q_MAX = 2.0 ** -10, 3.0, 2.0 ** -6, 2.0 ** 10
CUTOFF_RATE_MIN, CUTOFF_RATE_MAX = 2.0 ** -4, 2.0 ** 4


class CutoffC(C.Structure):
    """ctypes image of ``skred_cutoff_t`` (32 bytes): `set` names ABS or TRACK, and GLIDE, Q, MODE as the record brings them."""
    _fields_ = [("set", C.c_uint32), ("value", C.c_float), ("q", C.c_float), ("mode", C.c_uint32), ("rate_up", C.c_float),
                ("rate_down", C.c_float), ("reserved", C.c_uint32 * 2)]


def cutoff(set: int, value: float, q: float = 0.0, mode: int = 0, rate_up: float = 0.0, rate_down: float = 0.0) -> CutoffC:
    """One cutoff record: ``cutoff(CUTOFF_TRACK | CUTOFF_Q | CUTOFF_MODE, 4 * 2 * pi / table_size, 0.9, 1)`` is a low-pass at four
    times each note's own frequency."""
    return CutoffC(int(set), value, q, int(mode), rate_up, rate_down)


def cutoff_array(recs):
    """A contiguous ``CutoffC`` array from a sequence of CutoffC (a ctypes array of CutoffC passes through)."""
    if isinstance(recs, C.Array) and recs._type_ is CutoffC:
        return recs
    recs = list(recs)
    return (CutoffC * len(recs))(*recs)


# SKRED_FENV_* (skred_bank_fenv_match / _fenv_owned_each / _fenv_tags_each)
FENV_ABS, FENV_REL, FENV_START = 1, 2, 4
FENV_OFF, FENV_ATTACK, FENV_DECAY, FENV_SUSTAIN, FENV_RELEASE = range(5)


class FenvC(C.Structure):
    """ctypes image of ``skred_fenv_t`` (32 bytes): `set` names ABS or REL, and START if the contour begins at `start`."""
    _fields_ = [("set", C.c_uint32), ("start", C.c_float), ("peak", C.c_float), ("sustain", C.c_float), ("end", C.c_float),
                ("rate_attack", C.c_float), ("rate_decay", C.c_float), ("rate_release", C.c_float)]


def fenv(set: int, peak: float, sustain: float, end: float, rate_attack: float, rate_decay: float, rate_release: float,
         start: float = 0.0) -> FenvC:
    """One filter-envelope record: ``fenv(FENV_REL, 8.0, 2.0, 1.0, 1.5, 0.9, 0.8)`` opens each note's cutoff to eight times its base,
    falls to twice the base while the key is held and closes to the base after the note-off (rates per 64 frames)."""
    return FenvC(int(set), start, peak, sustain, end, rate_attack, rate_decay, rate_release)


def fenv_array(recs):
    """A contiguous ``FenvC`` array from a sequence of FenvC (a ctypes array of FenvC passes through)."""
    if isinstance(recs, C.Array) and recs._type_ is FenvC:
        return recs
    recs = list(recs)
    return (FenvC * len(recs))(*recs)


_lib: Optional[C.CDLL] = None


class SkredAmdError(RuntimeError):
    pass


def load() -> C.CDLL:
    """dlopen the HIP library; raise loudly when it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process.  PyTorch bundles its own libamdhip64 and asks for it by the unversioned name,
    # which the loader does not match against an already loaded /opt/rocm copy (same SONAME, different request):
    # if this library came first, torch would bring a second runtime that finds no GPU.  Loading torch first makes
    # this library resolve its libamdhip64.so.7 to the copy torch loaded.  (C hosts link one runtime and never see this.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise SkredAmdError(f"{LIB_PATH} is missing: build it with `make -C skred_amd/csrc` "
                            "(there is no CPU fallback for the render path)")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.skred_amd_abi_version.restype = i32
    L.skred_amd_device_count.restype = i32
    L.skred_amd_last_error.restype = C.c_char_p
    L.skred_bank_create.argtypes = [i32, i32, C.POINTER(vp)]
    L.skred_bank_destroy.argtypes = [vp]
    L.skred_bank_destroy.restype = None
    L.skred_bank_n_voices.argtypes = [vp]
    L.skred_bank_set_tables_f32.argtypes = [vp, vp, C.c_size_t]
    L.skred_bank_upload.argtypes = [vp, C.POINTER(VoiceBankC), i32, i32, i32]
    L.skred_bank_download.argtypes = [vp, C.POINTER(VoiceBankC), i32, i32, i32]
    L.skred_bank_set_globals.argtypes = [vp, C.POINTER(GlobalsC)]
    L.skred_bank_get_globals.argtypes = [vp, C.POINTER(GlobalsC)]
    L.skred_bank_render.argtypes = [vp, i32, i32, vp, vp, vp]
    L.skred_bank_master.argtypes = [vp, vp, i32, i32, vp, vp]
    L.skred_bank_render_mix.argtypes = [vp, i32, i32, vp, i32, vp, vp]
    L.skred_bank_render_host.argtypes = [vp, vp, i32, i32, i32, vp]
    L.skred_bank_last_render_ms.argtypes = [vp]
    L.skred_bank_last_render_ms.restype = C.c_float
    L.skred_bank_set_option.argtypes = [vp, i32, i32]
    L.skred_bank_last_kernel.argtypes = [vp]
    L.skred_bank_last_in_place.argtypes = [vp]
    L.skred_bank_last_split.argtypes = [vp]
    L.skred_bank_last_pack.argtypes = [vp]
    L.skred_bank_last_cz.argtypes = [vp]
    L.skred_bank_set_probe.argtypes = [vp, vp, i32, vp]
    L.skred_bank_set_taps.argtypes = [vp, vp, i32, vp]
    L.skred_bank_last_taps.argtypes = [vp]
    L.skred_bank_set_form_counter.argtypes = [vp, vp]
    L.skred_bank_last_cross_group.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.skred_bank_list_violations.argtypes = [vp]
    L.skred_bank_list_violations.restype = C.c_uint
    L.skred_bank_timing_reset.argtypes = [vp]
    L.skred_bank_timing_reset.restype = None
    L.skred_bank_timing_summary.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(i32)]
    L.skred_bank_update.argtypes = [vp, C.POINTER(VoiceBankC), vp, i32, C.c_uint32, vp]
    L.skred_bank_defer.argtypes = [vp, C.c_uint64, C.POINTER(VoiceBankC), vp, i32, C.c_uint32]
    L.skred_bank_run_queue.argtypes = [vp, i32, vp]
    L.skred_bank_queue_pending.argtypes = [vp]
    L.skred_seq_create.argtypes = [C.POINTER(vp)]
    L.skred_seq_destroy.argtypes = [vp]
    L.skred_seq_destroy.restype = None
    L.skred_seq_tempo_set.argtypes = [vp, C.c_float]
    L.skred_seq_time_per_step.argtypes = [vp]
    L.skred_seq_time_per_step.restype = C.c_float
    for name in ("skred_seq_step_set", "skred_seq_mute_set"):
        getattr(L, name).argtypes = [vp, i32, i32, i32]
    for name in ("skred_seq_modulo_set", "skred_seq_state_set"):
        getattr(L, name).argtypes = [vp, i32, i32]
    for name in ("skred_seq_pattern_reset", "skred_seq_pointer", "skred_seq_counter"):
        getattr(L, name).argtypes = [vp, i32]
    L.skred_seq_tick.argtypes = [vp, i32, C.c_float, vp, i32]
    L.skred_bank_seq.argtypes = [vp]
    L.skred_bank_seq.restype = vp
    L.skred_bank_set_sample_rate.argtypes = [vp, C.c_float]
    L.skred_bank_pattern_step_set.argtypes = [vp, i32, i32, C.POINTER(VoiceBankC), vp, i32, C.c_uint32]
    L.skred_bank_pattern_step_clear.argtypes = [vp, i32, i32]
    L.skred_bank_find_idle.argtypes = [vp, C.POINTER(IdleQueryC), vp, vp, vp]
    L.skred_bank_find_idle_host.argtypes = [vp, C.POINTER(IdleQueryC), vp, C.POINTER(i32), vp]
    L.skred_notes_check.argtypes = [vp, i32]
    L.skred_bank_notes_on_list.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp]
    L.skred_bank_note_on_idle.argtypes = [vp, C.POINTER(IdleQueryC), vp, i32, vp, vp, vp]
    L.skred_bank_stamp_list.argtypes = [vp, vp, i32, vp, C.c_uint32, vp]
    L.skred_steal_check.argtypes = [C.POINTER(StealQueryC), i32]
    L.skred_bank_find_steal.argtypes = [vp, C.POINTER(StealQueryC), vp, vp, vp]
    L.skred_bank_find_steal_host.argtypes = [vp, C.POINTER(StealQueryC), vp, C.POINTER(i32), vp]
    L.skred_bank_note_on_steal.argtypes = [vp, C.POINTER(IdleQueryC), C.POINTER(StealQueryC), vp, i32, vp, vp, vp]
    L.skred_slot_query_check.argtypes = [C.POINTER(SlotQueryC), i32]
    L.skred_slot_notes_check.argtypes = [vp, i32, i32, C.c_uint64]
    L.skred_bank_find_idle_slots.argtypes = [vp, C.POINTER(SlotQueryC), vp, vp, vp]
    L.skred_bank_find_idle_slots_host.argtypes = [vp, C.POINTER(SlotQueryC), vp, C.POINTER(i32), vp]
    L.skred_bank_notes_on_slots.argtypes = [vp, vp, i32, i32, C.c_uint64, vp, vp, i32, vp, vp, vp]
    L.skred_bank_note_on_idle_slots.argtypes = [vp, C.POINTER(SlotQueryC), vp, i32, C.c_uint64, vp, vp, vp]
    L.skred_bank_stamp_slots.argtypes = [vp, vp, i32, vp, i32, C.c_uint64, C.c_uint32, vp]
    L.skred_slot_steal_check.argtypes = [C.POINTER(SlotStealQueryC), i32]
    L.skred_bank_find_steal_slots.argtypes = [vp, C.POINTER(SlotStealQueryC), vp, vp, vp]
    L.skred_bank_find_steal_slots_host.argtypes = [vp, C.POINTER(SlotStealQueryC), vp, C.POINTER(i32), vp]
    L.skred_bank_note_on_steal_slots.argtypes = [vp, C.POINTER(SlotQueryC), C.POINTER(SlotStealQueryC), vp, i32, C.c_uint64, vp, vp, vp]
    L.skred_ctl_check.argtypes = [vp, i32, C.c_uint64]
    L.skred_bank_ctl_range.argtypes = [vp, vp, i32, i32, i32, C.c_uint64, vp, vp]
    L.skred_bank_ctl_slots.argtypes = [vp, vp, i32, C.c_uint64, vp, i32, vp, vp, vp]
    L.skred_bank_download_ctl.argtypes = [vp, C.POINTER(VoiceBankC), i32, i32, i32]
    L.skred_owner_tags_check.argtypes = [vp, i32, C.c_uint32]
    L.skred_bank_tag_slots.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp]
    L.skred_bank_find_owned.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp]
    L.skred_bank_stamp_owned.argtypes = [vp, vp, vp, i32, vp, i32, C.c_uint64, C.c_uint32, vp, vp]
    L.skred_bank_release_tags.argtypes = [vp, i32, i32, i32, C.c_uint64, vp, i32, C.c_uint32, vp, vp]
    L.skred_bank_ctl_owned.argtypes = [vp, vp, i32, C.c_uint64, vp, vp, i32, vp, vp, vp]
    L.skred_bank_owner_clear.argtypes = [vp, i32, i32, vp]
    L.skred_bank_download_owners.argtypes = [vp, vp, i32, i32]
    L.skred_bank_download_env_clocks.argtypes = [vp, vp, vp, i32, i32]
    L.skred_owner_match_check.argtypes = [C.POINTER(OwnerMatchC)]
    L.skred_ctl_each_check.argtypes = [vp, i32, vp, i32, C.c_uint64]
    L.skred_bank_find_match.argtypes = [vp, i32, i32, i32, C.POINTER(OwnerMatchC), i32, vp, vp, vp]
    L.skred_bank_find_match_host.argtypes = [vp, i32, i32, i32, C.POINTER(OwnerMatchC), i32, vp, C.POINTER(i32), vp]
    L.skred_bank_stamp_match.argtypes = [vp, i32, i32, i32, C.c_uint64, C.POINTER(OwnerMatchC), C.c_uint32, vp, vp]
    L.skred_bank_ctl_match.argtypes = [vp, vp, i32, i32, i32, C.c_uint64, C.POINTER(OwnerMatchC), vp, vp]
    L.skred_bank_ctl_owned_each.argtypes = [vp, vp, vp, i32, C.c_uint64, vp, vp, i32, vp, vp, vp]
    L.skred_bank_ctl_tags_each.argtypes = [vp, vp, vp, i32, i32, i32, C.c_uint64, vp, i32, vp, vp]
    L.skred_filter_each_check.argtypes = [vp, i32, vp, i32, C.c_uint64, C.c_uint64]
    L.skred_filter_coeffs.argtypes = [i32, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float)]
    L.skred_bank_ctl_owned_each_filter.argtypes = [vp, vp, vp, vp, i32, C.c_uint64, C.c_uint64, vp, vp, i32, vp, vp, vp]
    L.skred_bank_ctl_tags_each_filter.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_uint64, C.c_uint64, vp, i32, vp, vp]
    L.skred_chan_check.argtypes = [C.POINTER(SlotQueryC), C.POINTER(SlotStealQueryC), C.POINTER(OwnerMatchC), C.c_uint32, vp, i32, i32]
    L.skred_bank_find_steal_slots_match.argtypes = [vp, C.POINTER(SlotStealQueryC), C.POINTER(OwnerMatchC), vp, vp, vp]
    L.skred_bank_find_steal_slots_match_host.argtypes = [vp, C.POINTER(SlotStealQueryC), C.POINTER(OwnerMatchC), vp, C.POINTER(i32),
                                                         C.POINTER(i32), vp]
    L.skred_bank_note_on_channel.argtypes = [vp, C.POINTER(SlotQueryC), C.POINTER(SlotStealQueryC), C.POINTER(OwnerMatchC), C.c_uint32,
                                             vp, vp, i32, C.c_uint64, vp, vp, vp]
    L.skred_pedal_check.argtypes = [i32, i32, i32, i32, i32, C.c_uint64, C.POINTER(OwnerMatchC), C.c_uint32, vp, i32]
    L.skred_bank_stamp_owned_pedal.argtypes = [vp, vp, vp, i32, vp, i32, C.c_uint64, i32, vp, vp]
    L.skred_bank_release_tags_pedal.argtypes = [vp, i32, i32, i32, C.c_uint64, vp, i32, i32, vp, vp]
    L.skred_bank_pedal_latch.argtypes = [vp, i32, i32, i32, C.c_uint64, C.POINTER(OwnerMatchC), vp, vp]
    L.skred_bank_pedal_up.argtypes = [vp, i32, i32, i32, C.c_uint64, C.POINTER(OwnerMatchC), C.c_uint32, vp, vp]
    L.skred_bank_pedal_clear.argtypes = [vp, i32, i32, vp]
    L.skred_bank_download_pedals.argtypes = [vp, vp, i32, i32]
    L.skred_glide_check.argtypes = [vp, i32, i32, C.c_uint64]
    L.skred_bank_glide_owned.argtypes = [vp, vp, i32, C.c_uint64, vp, vp, i32, vp, vp, vp]
    L.skred_bank_glide_tags.argtypes = [vp, vp, i32, i32, i32, C.c_uint64, vp, i32, vp, vp]
    L.skred_bank_glide_advance.argtypes = [vp, i32, i32, i32, vp, vp]
    L.skred_bank_glide_stop.argtypes = [vp, i32, i32, i32, vp]
    L.skred_bank_download_glide.argtypes = [vp, vp, i32, i32]
    L.skred_bend_check.argtypes = [vp, i32, i32, C.c_uint64]
    L.skred_bank_bend_match.argtypes = [vp, i32, i32, i32, C.c_uint64, vp, C.c_float, vp, vp]
    L.skred_bank_bend_owned_each.argtypes = [vp, vp, i32, C.c_uint64, vp, vp, i32, vp, vp, vp]
    L.skred_bank_bend_tags_each.argtypes = [vp, vp, i32, i32, i32, C.c_uint64, vp, i32, vp, vp]
    L.skred_bank_bend_clear.argtypes = [vp, i32, i32, i32, vp]
    L.skred_bank_download_bend.argtypes = [vp, vp, i32, i32]
    L.skred_filter_coeffs_w.argtypes = [i32, C.c_float, C.c_float, C.POINTER(C.c_float)]
    L.skred_cutoff_check.argtypes = [vp, i32, i32, C.c_uint64, C.c_uint64, i32]
    L.skred_bank_cutoff_match.argtypes = [vp, i32, i32, i32, C.c_uint64, vp, vp, vp, vp]
    L.skred_bank_cutoff_owned_each.argtypes = [vp, vp, i32, C.c_uint64, vp, vp, i32, vp, vp, vp]
    L.skred_bank_cutoff_tags_each.argtypes = [vp, vp, i32, i32, i32, C.c_uint64, vp, i32, vp, vp]
    L.skred_bank_cutoff_advance.argtypes = [vp, i32, i32, i32, vp, vp]
    L.skred_bank_cutoff_stop.argtypes = [vp, i32, i32, i32, vp]
    L.skred_bank_download_cutoff.argtypes = [vp, vp, i32, i32]
    L.skred_fenv_check.argtypes = [vp, i32, i32, C.c_uint64, C.c_uint64]
    L.skred_bank_fenv_match.argtypes = [vp, i32, i32, i32, C.c_uint64, vp, vp, vp, vp]
    L.skred_bank_fenv_owned_each.argtypes = [vp, vp, i32, C.c_uint64, vp, vp, i32, vp, vp, vp]
    L.skred_bank_fenv_tags_each.argtypes = [vp, vp, i32, i32, i32, C.c_uint64, vp, i32, vp, vp]
    L.skred_bank_download_fenv.argtypes = [vp, vp, i32, i32]
    _lib = L
    return L


def _check(rc: int, what: str):
    if rc != 0:
        msg = load().skred_amd_last_error().decode(errors="replace")
        raise SkredAmdError(f"{what} failed (rc={rc}): {msg}")


def notes_check(notes) -> int:
    """skred_notes_check: 0, or SKRED_E_BAD_ARG (-2) for a note the bank entry points would refuse.  Pure host, no device."""
    arr = note_array(notes)
    return int(load().skred_notes_check(C.cast(arr, C.c_void_p), len(arr)))


def steal_check(q: StealQueryC, n_voices: int) -> int:
    """skred_steal_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4) for a query the bank entry points would refuse.  Pure host."""
    return int(load().skred_steal_check(C.byref(q) if q is not None else None, int(n_voices)))


def slot_query_check(q: SlotQueryC, n_voices: int) -> int:
    """skred_slot_query_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4) for a query find_idle_slots would refuse.  Pure host."""
    return int(load().skred_slot_query_check(C.byref(q) if q is not None else None, int(n_voices)))


def slot_steal_check(q: SlotStealQueryC, n_voices: int) -> int:
    """skred_slot_steal_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4) for a query find_steal_slots would refuse.  Pure host."""
    return int(load().skred_slot_steal_check(C.byref(q) if q is not None else None, int(n_voices)))


def slot_notes_check(notes, slot_voices: int, voice_mask: int) -> int:
    """skred_slot_notes_check on len(notes) // slot_voices patch notes (record k * K + l: voice l of note k).  Pure host."""
    arr = note_array(notes)
    return int(load().skred_slot_notes_check(C.cast(arr, C.c_void_p), len(arr) // max(int(slot_voices), 1), int(slot_voices),
                                             int(voice_mask)))


def ctl_check(ctls, voice_mask: int, slot_voices: Optional[int] = None) -> int:
    """skred_ctl_check on the K = len(ctls) records of a controller (record l: voice l of a slot): 0, SKRED_E_BAD_ARG (-2) or
    SKRED_E_RANGE (-4) for one the bank entry points would refuse.  Pure host."""
    arr = ctl_array(ctls)
    return int(load().skred_ctl_check(C.cast(arr, C.c_void_p), len(arr) if slot_voices is None else int(slot_voices), int(voice_mask)))


def owner_tags_check(tags, flags: int = 0) -> int:
    """skred_owner_tags_check: 0, or SKRED_E_BAD_ARG (-2) for tags the owner entry points would refuse.  Pure host."""
    arr = tag_array(tags)
    return int(load().skred_owner_tags_check(arr.ctypes.data, len(arr), int(flags)))


def owner_match_check(m: Optional[OwnerMatchC]) -> int:
    """skred_owner_match_check: 0, or SKRED_E_BAD_ARG (-2) for None or a value with bits outside the mask.  Pure host."""
    return int(load().skred_owner_match_check(C.byref(m) if m is not None else None))


CHAN_NO_CAP = 0xFFFFFFFF          # SKRED_CHAN_NO_CAP


def chan_check(idle_q, steal_q, m, cap: int, tags, n_voices: int) -> int:
    """skred_chan_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4) for a burst note_on_channel would refuse (queries, match, cap
    and the len(tags) tags; None stands for a NULL pointer).  Pure host."""
    arr = tag_array(tags) if tags is not None else None
    ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
    return int(load().skred_chan_check(ref(idle_q), ref(steal_q), ref(m), int(cap) & 0xFFFFFFFF, arr.ctypes.data if arr is not None else None,
                                       len(arr) if arr is not None else 0, int(n_voices)))


def pedal_check(call: int, n_voices: int, first: int = 0, count: int = 0, slot_voices: int = 1, voice_mask: int = 1, m=None, flags: int = 0,
                tags=None) -> int:
    """skred_pedal_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4) for what the pedal entry point PEDAL_CALL_* would refuse (None
    stands for a NULL pointer).  Pure host."""
    arr = tag_array(tags) if tags is not None else None
    return int(load().skred_pedal_check(int(call), int(n_voices), int(first), int(count), int(slot_voices), int(voice_mask),
                                        C.byref(m) if m is not None else None, int(flags) & 0xFFFFFFFF,
                                        arr.ctypes.data if arr is not None else None, len(arr) if arr is not None else 0))


def glide_check(glides, slot_voices: int, voice_mask: int) -> int:
    """skred_glide_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4) for what the two starting calls would refuse about the entries
    (None stands for a NULL array).  Pure host."""
    arr = glide_array(glides) if glides is not None else None
    return int(load().skred_glide_check(C.cast(arr, C.c_void_p) if arr is not None else None, len(arr) if arr is not None else 0,
                                        int(slot_voices), int(voice_mask)))


def ratio_array(ratios) -> np.ndarray:
    """The per-entry ratios of bend_owned_each / bend_tags_each as a contiguous float32 array."""
    return np.ascontiguousarray(ratios, dtype=np.float32).reshape(-1)


def bend_check(ratios, slot_voices: int, voice_mask: int) -> int:
    """skred_bend_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4) for what the bending calls would refuse about K, the mask and
    the ratios (None stands for a NULL array).  Pure host."""
    arr = ratio_array(ratios) if ratios is not None else None
    return int(load().skred_bend_check(arr.ctypes.data if arr is not None else None, len(arr) if arr is not None else 0,
                                       int(slot_voices), int(voice_mask)))


def ctl_each_check(each, ctls, voice_mask: int, slot_voices: Optional[int] = None) -> int:
    """skred_ctl_each_check on the entries `each` over the K records `ctls` (None: no base records, then slot_voices is required):
    0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4).  Pure host."""
    e = ctl_each_array(each)
    arr = ctl_array(ctls) if ctls is not None else None
    K = len(arr) if slot_voices is None else int(slot_voices)
    return int(load().skred_ctl_each_check(C.cast(e, C.c_void_p), len(e), C.cast(arr, C.c_void_p) if arr is not None else None, K,
                                           int(voice_mask)))


def filter_each_check(filt, ctls, voice_mask: int, filter_mask: int, slot_voices: Optional[int] = None) -> int:
    """skred_filter_each_check on the coefficients `filt` over the K records `ctls` (None: no base records, then slot_voices is
    required): 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4).  Pure host."""
    f = filter_each_array(filt) if filt is not None else None
    arr = ctl_array(ctls) if ctls is not None else None
    K = len(arr) if slot_voices is None else int(slot_voices)
    return int(load().skred_filter_each_check(C.cast(f, C.c_void_p) if f is not None else None, len(f) if f is not None else 0,
                                              C.cast(arr, C.c_void_p) if arr is not None else None, K, int(voice_mask), int(filter_mask)))


def filter_coeffs(mode: int, freq: float, resonance: float, sample_rate: float):
    """skred_filter_coeffs: (b0, b1, b2, a1, a2) as np.float32 for one filter setting -- the drop-in mode's mmf_set_params arithmetic
    with the rate as an argument.  None for mode 0 (bypass: nothing is computed).  Pure host."""
    out = (C.c_float * 5)()
    rc = int(load().skred_filter_coeffs(int(mode), float(freq), float(resonance), float(sample_rate), out))
    if rc == 1:
        return None
    _check(rc, "skred_filter_coeffs")
    return tuple(np.float32(x) for x in out)


def filter_coeffs_w(mode: int, w: float, q: float):
    """skred_filter_coeffs_w: (b0, b1, b2, a1, a2) as np.float32 from the normalised angular cutoff w = 2 pi f / rate, by the
    arithmetic the device uses (include/skred_amd.h, "filter cutoff on the device").  None for mode 0.  Pure host."""
    out = (C.c_float * 5)()
    rc = int(load().skred_filter_coeffs_w(int(mode), float(w), float(q), out))
    if rc == 1:
        return None
    _check(rc, "skred_filter_coeffs_w")
    return tuple(np.float32(x) for x in out)


def cutoff_check(recs, slot_voices: int, voice_mask: int, filter_mask: int, first_time: bool = False) -> int:
    """skred_cutoff_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4) for what the record calls would refuse.  Pure host."""
    arr = cutoff_array(recs) if recs is not None else None
    return int(load().skred_cutoff_check(C.cast(arr, C.c_void_p) if arr is not None else None, len(arr) if arr is not None else 0,
                                         int(slot_voices), int(voice_mask), int(filter_mask), int(bool(first_time))))


def fenv_check(recs, slot_voices: int, voice_mask: int, filter_mask: int) -> int:
    """skred_fenv_check: 0, SKRED_E_BAD_ARG (-2) or SKRED_E_RANGE (-4) for what the record calls would refuse.  Pure host."""
    arr = fenv_array(recs) if recs is not None else None
    return int(load().skred_fenv_check(C.cast(arr, C.c_void_p) if arr is not None else None, len(arr) if arr is not None else 0,
                                       int(slot_voices), int(voice_mask), int(filter_mask)))


class DeviceBank:
    """A voice bank resident in one GPU's HBM."""

    def __init__(self, n_voices: int, device: int = 0):
        self.L = load()
        self.n = int(n_voices)
        self.device = device
        h = C.c_void_p()
        _check(self.L.skred_bank_create(device, self.n, C.byref(h)), "skred_bank_create")
        self.h = h

    @classmethod
    def borrowed(cls, handle, n_voices: int, device: int = 0) -> "DeviceBank":
        """A view of a bank somebody else owns (skred_shard_bank): close() does not destroy it."""
        self = cls.__new__(cls)
        self.L = load()
        self.n = int(n_voices)
        self.device = device
        self.h = C.c_void_p(handle)
        self._borrowed = True
        return self

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.L.skred_bank_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tables(self, pool: np.ndarray):
        pool = np.ascontiguousarray(pool, np.float32)
        _check(self.L.skred_bank_set_tables_f32(self.h, pool.ctypes.data, pool.size), "skred_bank_set_tables_f32")

    def upload(self, bank: VoiceBank, src_first: int = 0, dst_first: int = 0, count: Optional[int] = None):
        count = bank.n - src_first if count is None else count
        cb = bank.as_c()
        _check(self.L.skred_bank_upload(self.h, C.byref(cb), src_first, dst_first, count), "skred_bank_upload")

    def download(self, bank: VoiceBank, src_first: int = 0, dst_first: int = 0, count: Optional[int] = None):
        count = bank.n - dst_first if count is None else count
        cb = bank.as_c()
        _check(self.L.skred_bank_download(self.h, C.byref(cb), src_first, dst_first, count), "skred_bank_download")

    def set_globals(self, g: GlobalsC):
        _check(self.L.skred_bank_set_globals(self.h, C.byref(g)), "skred_bank_set_globals")

    def get_globals(self) -> GlobalsC:
        g = GlobalsC()
        _check(self.L.skred_bank_get_globals(self.h, C.byref(g)), "skred_bank_get_globals")
        return g

    def render(self, frames: int, d_partial: int, d_stems: int = 0, interp: int = 0, stream: int = 0):
        """Asynchronous render into device pointers (ints), e.g. torch tensor .data_ptr()."""
        _check(self.L.skred_bank_render(self.h, frames, interp, d_partial, d_stems or None, stream or None),
               "skred_bank_render")

    def render_mix(self, frames: int, d_out: int, channels: int = 2, d_stems: int = 0, interp: int = 0, stream: int = 0):
        """Single-GPU render + mix-down + master volume: one launch."""
        _check(self.L.skred_bank_render_mix(self.h, frames, interp, d_out, channels, d_stems, stream),
               "skred_bank_render_mix")

    def kernel_timing(self, every: int = 1):
        """SKRED_OPT_KERNEL_TIMING: event pair around the render kernels of every n-th launch (0: never)."""
        _check(self.L.skred_bank_set_option(self.h, 4, int(every)), "skred_bank_set_option")

    def master(self, d_sum: int, frames: int, d_out: int, channels: int = 2, stream: int = 0):
        _check(self.L.skred_bank_master(self.h, d_sum, frames, channels, d_out, stream or None), "skred_bank_master")

    def render_host(self, frames: int, channels: int = 2, interp: int = 0, want_stems: bool = False):
        """The synth() contract on host buffers.  Returns (buffer [F][ch], stems [F][N][2] | None)."""
        buf = np.zeros((frames, channels), np.float32)
        stems = np.zeros((frames, self.n, 2), np.float32) if want_stems else None
        _check(self.L.skred_bank_render_host(self.h, buf.ctypes.data, frames, channels, interp,
                                             stems.ctypes.data if want_stems else None), "skred_bank_render_host")
        return buf, stems

    # ---- block-granular updates (include/skred_amd.h: skred_bank_update / _defer / _run_queue) ----
    def update(self, bank: VoiceBank, voices, dirty: int, stream: int = 0):
        """Push the `dirty` parts (DIRTY_* | STAMP_*) of the listed voices from the host view."""
        v = np.ascontiguousarray(voices, np.int32)
        _check(self.L.skred_bank_update(self.h, C.byref(bank.as_c()), v.ctypes.data, len(v), dirty, stream),
               "skred_bank_update")

    def defer(self, when: int, bank: VoiceBank, voices, dirty: int):
        v = np.ascontiguousarray(voices, np.int32)
        _check(self.L.skred_bank_defer(self.h, when, C.byref(bank.as_c()), v.ctypes.data, len(v), dirty),
               "skred_bank_defer")

    def run_queue(self, frame_count: int, stream: int = 0) -> int:
        n = self.L.skred_bank_run_queue(self.h, frame_count, stream)
        if n < 0:
            _check(n, "skred_bank_run_queue")
        return n

    def queue_pending(self) -> int:
        return self.L.skred_bank_queue_pending(self.h)

    # ---- pattern steps on the bank's own step clock (include/skred_amd.h: skred_bank_pattern_* / skred_seq_*) ----
    def seq(self) -> "SeqClock":
        return SeqClock(self.L.skred_bank_seq(self.h), owner=False)

    def set_sample_rate(self, rate: float):
        _check(self.L.skred_bank_set_sample_rate(self.h, rate), "skred_bank_set_sample_rate")

    def pattern_step_set(self, pattern: int, step: int, bank: Optional[VoiceBank] = None, voices=(), dirty: int = 0):
        v = np.ascontiguousarray(voices, np.int32)
        cb = bank.as_c() if bank is not None else None
        _check(self.L.skred_bank_pattern_step_set(self.h, pattern, step, C.byref(cb) if cb is not None else None,
                                                  v.ctypes.data if len(v) else None, len(v), dirty), "skred_bank_pattern_step_set")

    def pattern_step_clear(self, pattern: int, step: int):
        _check(self.L.skred_bank_pattern_step_clear(self.h, pattern, step), "skred_bank_pattern_step_clear")

    # ---- the free-voice query (include/skred_amd.h: skred_bank_find_idle / _find_idle_host) ----
    def find_idle(self, first: int, count: int, which: int, settle_level: float = 0.0, start: Optional[int] = None,
                  max_out: int = 0, d_voices: int = 0, d_count: int = 0, stream: int = 0):
        """Asynchronous on `stream`: the idle voices of [first, first + count) in ascending order from `start` (default `first`),
        wrapping, into d_voices[0 .. written) (int32, device memory); d_count[0] = written, d_count[1] = total (uint32)."""
        q = IdleQueryC(int(first), int(count), int(which), float(settle_level), int(first if start is None else start), int(max_out))
        _check(self.L.skred_bank_find_idle(self.h, C.byref(q), d_voices or None, d_count or None, stream or None),
               "skred_bank_find_idle")

    def find_idle_host(self, first: int, count: int, which: int, settle_level: float = 0.0, start: Optional[int] = None,
                       max_out: Optional[int] = None, stream: int = 0):
        """The same into host memory, waiting for `stream` only.  Returns (np.int32 array of the listed voices, total)."""
        max_out = count if max_out is None else max_out
        q = IdleQueryC(int(first), int(count), int(which), float(settle_level), int(first if start is None else start), int(max_out))
        out = np.empty(max(max_out, 0), np.int32)
        total = C.c_int(0)
        n = self.L.skred_bank_find_idle_host(self.h, C.byref(q), out.ctypes.data if max_out > 0 else None, C.byref(total),
                                             stream or None)
        if n < 0:
            _check(n, "skred_bank_find_idle_host")
        return out[:n].copy(), int(total.value)

    # ---- device-side note-ons (include/skred_amd.h: skred_bank_notes_on_list / _note_on_idle / _stamp_list) ----
    def notes_on_list(self, notes, d_voices: int, d_count: int, first_entry: int = 0, d_assigned: int = 0, d_result: int = 0,
                      stream: int = 0):
        """Asynchronous on `stream`: note k goes to voice d_voices[first_entry + k] while that entry is below d_count[0] (device
        memory, as find_idle leaves them) and names a voice of the bank, else it is dropped.  d_assigned[k] (int32, may be 0) = the
        voice or -1; d_result[0] = placed, d_result[1] = dropped (uint32)."""
        arr = note_array(notes)
        _check(self.L.skred_bank_notes_on_list(self.h, C.cast(arr, C.c_void_p), len(arr), d_voices or None, d_count or None,
                                               int(first_entry), d_assigned or None, d_result or None, stream or None),
               "skred_bank_notes_on_list")

    def note_on_idle(self, notes, first: int, count: int, which: int, settle_level: float = 0.0, start: Optional[int] = None,
                     d_assigned: int = 0, d_result: int = 0, stream: int = 0):
        """The query of find_idle (room for len(notes) voices, in scratch the bank owns) and the placement of the notes on its list,
        in one call; IDLE_AMP_ZERO is refused."""
        arr = note_array(notes)
        q = IdleQueryC(int(first), int(count), int(which), float(settle_level), int(first if start is None else start), 0)
        _check(self.L.skred_bank_note_on_idle(self.h, C.byref(q), C.cast(arr, C.c_void_p), len(arr), d_assigned or None,
                                              d_result or None, stream or None), "skred_bank_note_on_idle")

    def stamp_list(self, d_voices: int, n: int, stamps: int, d_count: int = 0, stream: int = 0):
        """STAMP_TRIGGER / STAMP_RELEASE on the first min(n, d_count[0]) entries of a list in device memory (d_count 0: n entries);
        entries outside the bank -- the -1 of a dropped note -- are skipped."""
        _check(self.L.skred_bank_stamp_list(self.h, d_voices or None, int(n), d_count or None, int(stamps), stream or None),
               "skred_bank_stamp_list")

    # ---- voice stealing (include/skred_amd.h: skred_bank_find_steal / _find_steal_host / skred_bank_note_on_steal) ----
    def find_steal(self, q: StealQueryC, d_voices: int = 0, d_count: int = 0, stream: int = 0):
        """Asynchronous on `stream`: the first q.max_out candidates of the victim order (ascending key, ties by voice index) into
        d_voices[0 .. written) (int32, device memory); d_count[0] = written, d_count[1] = total candidates (uint32)."""
        _check(self.L.skred_bank_find_steal(self.h, C.byref(q), d_voices or None, d_count or None, stream or None),
               "skred_bank_find_steal")

    def find_steal_host(self, q: StealQueryC, stream: int = 0):
        """The same into host memory, waiting for `stream` only.  Returns (np.int32 array of the victims, total candidates)."""
        out = np.empty(max(int(q.max_out), 0), np.int32)
        total = C.c_int(0)
        n = self.L.skred_bank_find_steal_host(self.h, C.byref(q), out.ctypes.data if q.max_out > 0 else None, C.byref(total),
                                              stream or None)
        if n < 0:
            _check(n, "skred_bank_find_steal_host")
        return out[:n].copy(), int(total.value)

    def note_on_steal(self, notes, idle_q: IdleQueryC, steal_q: StealQueryC, d_assigned: int = 0, d_result: int = 0, stream: int = 0):
        """The idle query, the steal query (exclude_idle, settle_level and max_out overridden by the library), the victims appended
        behind the idle entries and the placement of the notes, in one call; d_result[0..3) = placed, dropped, stolen (uint32)."""
        arr = note_array(notes)
        _check(self.L.skred_bank_note_on_steal(self.h, C.byref(idle_q), C.byref(steal_q), C.cast(arr, C.c_void_p), len(arr),
                                               d_assigned or None, d_result or None, stream or None), "skred_bank_note_on_steal")

    # ---- patch notes (include/skred_amd.h: skred_bank_find_idle_slots / _notes_on_slots / _note_on_idle_slots / _stamp_slots) ----
    def find_idle_slots(self, q: SlotQueryC, d_slots: int = 0, d_count: int = 0, stream: int = 0):
        """Asynchronous on `stream`: the first voices of the idle slots of q's range, ascending from q.start and wrapping, into
        d_slots[0 .. written) (int32, device memory); d_count[0] = written, d_count[1] = total (uint32)."""
        _check(self.L.skred_bank_find_idle_slots(self.h, C.byref(q), d_slots or None, d_count or None, stream or None),
               "skred_bank_find_idle_slots")

    def find_idle_slots_host(self, q: SlotQueryC, stream: int = 0):
        """The same into host memory, waiting for `stream` only.  Returns (np.int32 array of the listed slots, total)."""
        out = np.empty(max(int(q.max_out), 0), np.int32)
        total = C.c_int(0)
        n = self.L.skred_bank_find_idle_slots_host(self.h, C.byref(q), out.ctypes.data if q.max_out > 0 else None, C.byref(total),
                                                   stream or None)
        if n < 0:
            _check(n, "skred_bank_find_idle_slots_host")
        return out[:n].copy(), int(total.value)

    def notes_on_slots(self, notes, slot_voices: int, voice_mask: int, d_slots: int, d_count: int, first_entry: int = 0,
                       d_assigned: int = 0, d_result: int = 0, stream: int = 0):
        """Asynchronous on `stream`: patch note k (records notes[k * K : k * K + K]) goes to the slot d_slots[first_entry + k] while
        that entry is below d_count[0] and is a slot of the bank, else it is dropped; only voices with a bit in voice_mask are
        stored to.  d_assigned[k] (int32, may be 0) = the slot or -1; d_result[0] = placed, d_result[1] = dropped notes (uint32)."""
        arr = note_array(notes)
        _check(self.L.skred_bank_notes_on_slots(self.h, C.cast(arr, C.c_void_p), len(arr) // int(slot_voices), int(slot_voices),
                                                int(voice_mask), d_slots or None, d_count or None, int(first_entry),
                                                d_assigned or None, d_result or None, stream or None), "skred_bank_notes_on_slots")

    def note_on_idle_slots(self, notes, q: SlotQueryC, voice_mask: int, d_assigned: int = 0, d_result: int = 0, stream: int = 0):
        """The query of find_idle_slots (room for the batch, in scratch the bank owns) and the placement of the patch notes on its
        list, in one call; IDLE_AMP_ZERO is refused."""
        arr = note_array(notes)
        _check(self.L.skred_bank_note_on_idle_slots(self.h, C.byref(q), C.cast(arr, C.c_void_p), len(arr) // int(q.slot_voices),
                                                    int(voice_mask), d_assigned or None, d_result or None, stream or None),
               "skred_bank_note_on_idle_slots")

    def stamp_slots(self, d_slots: int, n: int, slot_voices: int, voice_mask: int, stamps: int, d_count: int = 0, stream: int = 0):
        """STAMP_TRIGGER / STAMP_RELEASE on the masked voices of the first min(n, d_count[0]) listed slots (d_count 0: n entries);
        entries that are no slot of the bank -- the -1 of a dropped note -- are skipped."""
        _check(self.L.skred_bank_stamp_slots(self.h, d_slots or None, int(n), d_count or None, int(slot_voices), int(voice_mask),
                                             int(stamps), stream or None), "skred_bank_stamp_slots")

    # ---- patch controllers (include/skred_amd.h: skred_bank_ctl_range / _ctl_slots / _download_ctl) ----
    def ctl_range(self, ctls, first: int, count: int, voice_mask: int, d_result: int = 0, stream: int = 0):
        """Asynchronous on `stream`: the controller (K = len(ctls) records, record l for voice l of a slot) on the masked voices of
        every slot of [first, first + count).  d_result (uint32[2], may be 0): voices written, stores withheld by the two guards."""
        arr = ctl_array(ctls)
        _check(self.L.skred_bank_ctl_range(self.h, C.cast(arr, C.c_void_p), int(first), int(count), len(arr), int(voice_mask),
                                           d_result or None, stream or None), "skred_bank_ctl_range")

    def ctl_slots(self, ctls, voice_mask: int, d_slots: int, n: int, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """The same on the first min(n, d_count[0]) listed slots (d_count 0: n entries); entries that are no slot of the bank -- the
        -1 of a dropped note -- are skipped, so an earlier d_assigned is the list for "this chord only"."""
        arr = ctl_array(ctls)
        _check(self.L.skred_bank_ctl_slots(self.h, C.cast(arr, C.c_void_p), len(arr), int(voice_mask), d_slots or None, int(n),
                                           d_count or None, d_result or None, stream or None), "skred_bank_ctl_slots")

    def download_ctl(self, bank: VoiceBank, src_first: int = 0, dst_first: int = 0, count: Optional[int] = None):
        """The words a controller can store, as the device holds them, into `bank` (download() returns the state fields only)."""
        count = bank.n - dst_first if count is None else count
        cb = bank.as_c()
        _check(self.L.skred_bank_download_ctl(self.h, C.byref(cb), src_first, dst_first, count), "skred_bank_download_ctl")

    # ---- note owners (include/skred_amd.h: skred_bank_tag_slots / _find_owned / _stamp_owned / _release_tags / _ctl_owned) ----
    def tag_slots(self, d_slots: int, tags, slot_voices: int, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """Asynchronous on `stream`: owner[d_slots[k]] = tags[k] (0 clears) for the first min(len(tags), d_count[0]) entries that are
        slots of the bank -- a d_assigned, -1 holes and all.  d_result (uint32[2], may be 0): slots tagged, entries that are no slot."""
        arr = tag_array(tags)
        _check(self.L.skred_bank_tag_slots(self.h, d_slots or None, arr.ctypes.data, len(arr), d_count or None, int(slot_voices),
                                           d_result or None, stream or None), "skred_bank_tag_slots")

    def find_owned(self, first: int, count: int, slot_voices: int, tags, d_slots_out: int, stream: int = 0):
        """d_slots_out[k] (int32, device memory) = the lowest slot of [first, first + count) whose owner is tags[k], or -1."""
        arr = tag_array(tags)
        _check(self.L.skred_bank_find_owned(self.h, int(first), int(count), int(slot_voices), arr.ctypes.data, len(arr),
                                            d_slots_out or None, stream or None), "skred_bank_find_owned")

    def stamp_owned(self, d_slots: int, tags, slot_voices: int, voice_mask: int, stamps: int, d_result: int, d_count: int = 0,
                    stream: int = 0):
        """stamp_slots on the entries whose owner is tags[k].  d_result (uint32[3]): slots stamped, slots whose owner differs, entries
        that are no slot."""
        arr = tag_array(tags)
        _check(self.L.skred_bank_stamp_owned(self.h, d_slots or None, arr.ctypes.data, len(arr), d_count or None, int(slot_voices),
                                             int(voice_mask), int(stamps), d_result or None, stream or None), "skred_bank_stamp_owned")

    def release_tags(self, first: int, count: int, slot_voices: int, voice_mask: int, tags, stamps: int, d_result: int, stream: int = 0):
        """Note-off by note id: every tag stamps the lowest slot of the range that carries it.  d_result as for stamp_owned; [2] counts
        the tags nobody carries."""
        arr = tag_array(tags)
        _check(self.L.skred_bank_release_tags(self.h, int(first), int(count), int(slot_voices), int(voice_mask), arr.ctypes.data, len(arr),
                                              int(stamps), d_result or None, stream or None), "skred_bank_release_tags")

    def ctl_owned(self, ctls, voice_mask: int, d_slots: int, tags, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """ctl_slots on the entries whose owner is tags[k].  d_result (uint32[3], may be 0): voices written, stores withheld, slots
        whose owner differs."""
        arr, t = ctl_array(ctls), tag_array(tags)
        _check(self.L.skred_bank_ctl_owned(self.h, C.cast(arr, C.c_void_p), len(arr), int(voice_mask), d_slots or None, t.ctypes.data,
                                           len(t), d_count or None, d_result or None, stream or None), "skred_bank_ctl_owned")

    def owner_clear(self, first: int = 0, count: Optional[int] = None, stream: int = 0):
        count = self.n - first if count is None else count
        _check(self.L.skred_bank_owner_clear(self.h, int(first), int(count), stream or None), "skred_bank_owner_clear")

    def download_owners(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The owner words of [first, first + count) (uint32); waits for the device.  Zeros on a bank that was never tagged."""
        count = self.n - first if count is None else count
        out = np.full(max(count, 0), 0xDEADBEEF, np.uint32)
        _check(self.L.skred_bank_download_owners(self.h, out.ctypes.data, int(first), int(count)), "skred_bank_download_owners")
        return out

    def download_env_clocks(self, first: int = 0, count: Optional[int] = None):
        """(sample_start, sample_release) of [first, first + count) as the device holds them (uint64); waits for the device."""
        count = self.n - first if count is None else count
        start, release = np.zeros(max(count, 0), np.uint64), np.zeros(max(count, 0), np.uint64)
        _check(self.L.skred_bank_download_env_clocks(self.h, start.ctypes.data, release.ctypes.data, int(first), int(count)),
               "skred_bank_download_env_clocks")
        return start, release

    # ---- channels and per-note expression (include/skred_amd.h: skred_bank_find_match / _stamp_match / _ctl_match /
    # _ctl_owned_each / _ctl_tags_each) ----
    def find_match(self, first: int, count: int, slot_voices: int, m: OwnerMatchC, max_out: int = 0, d_slots: int = 0, d_count: int = 0,
                   stream: int = 0):
        """Asynchronous on `stream`: the first voices of the slots of [first, first + count) whose owner matches m, ascending, into
        d_slots[0 .. min(total, max_out)) (int32, device memory); d_count[0] = the TOTAL (uint32)."""
        _check(self.L.skred_bank_find_match(self.h, int(first), int(count), int(slot_voices), C.byref(m), int(max_out), d_slots or None,
                                            d_count or None, stream or None), "skred_bank_find_match")

    def find_match_host(self, first: int, count: int, slot_voices: int, m: OwnerMatchC, max_out: int = 0, stream: int = 0):
        """The same into host memory, waiting for `stream` only.  Returns (np.int32 array of the listed slots, total)."""
        out = np.empty(max(int(max_out), 0), np.int32)
        total = C.c_int(0)
        n = self.L.skred_bank_find_match_host(self.h, int(first), int(count), int(slot_voices), C.byref(m), int(max_out),
                                              out.ctypes.data if max_out > 0 else None, C.byref(total), stream or None)
        if n < 0:
            _check(n, "skred_bank_find_match_host")
        return out[:n].copy(), int(total.value)

    def stamp_match(self, first: int, count: int, slot_voices: int, voice_mask: int, m: OwnerMatchC, stamps: int, d_result: int,
                    stream: int = 0):
        """stamp_slots' stores on every matching slot of the range, in one pass.  d_result (uint32[2]): slots stamped, slots that did
        not match."""
        _check(self.L.skred_bank_stamp_match(self.h, int(first), int(count), int(slot_voices), int(voice_mask), C.byref(m), int(stamps),
                                             d_result or None, stream or None), "skred_bank_stamp_match")

    def ctl_match(self, ctls, first: int, count: int, voice_mask: int, m: OwnerMatchC, d_result: int = 0, stream: int = 0):
        """ctl_range on the matching slots of the range.  d_result (uint32[3], may be 0): voices written, stores withheld, slots that
        did not match."""
        arr = ctl_array(ctls)
        _check(self.L.skred_bank_ctl_match(self.h, C.cast(arr, C.c_void_p), int(first), int(count), len(arr), int(voice_mask), C.byref(m),
                                           d_result or None, stream or None), "skred_bank_ctl_match")

    def ctl_owned_each(self, ctls, each, voice_mask: int, d_slots: int, tags, slot_voices: Optional[int] = None, d_count: int = 0,
                       d_result: int = 0, stream: int = 0):
        """ctl_owned with entry k's record each[k] laid over the K records (ctls None: no base records, slot_voices required).
        d_result (uint32[3], may be 0): voices written, stores withheld, slots whose owner differs."""
        e, t = ctl_each_array(each), tag_array(tags)
        assert len(e) == len(t), "one entry per tag"
        arr = ctl_array(ctls) if ctls is not None else None
        K = len(arr) if slot_voices is None else int(slot_voices)
        _check(self.L.skred_bank_ctl_owned_each(self.h, C.cast(arr, C.c_void_p) if arr is not None else None, C.cast(e, C.c_void_p), K,
                                                int(voice_mask), d_slots or None, t.ctypes.data, len(t), d_count or None,
                                                d_result or None, stream or None), "skred_bank_ctl_owned_each")

    def ctl_tags_each(self, ctls, each, first: int, count: int, voice_mask: int, tags, slot_voices: Optional[int] = None,
                      d_result: int = 0, stream: int = 0):
        """Expression by note id: each[k] on the lowest slot of [first, first + count) that carries tags[k]."""
        e, t = ctl_each_array(each), tag_array(tags)
        assert len(e) == len(t), "one entry per tag"
        arr = ctl_array(ctls) if ctls is not None else None
        K = len(arr) if slot_voices is None else int(slot_voices)
        _check(self.L.skred_bank_ctl_tags_each(self.h, C.cast(arr, C.c_void_p) if arr is not None else None, C.cast(e, C.c_void_p),
                                               int(first), int(count), K, int(voice_mask), t.ctypes.data, len(t), d_result or None,
                                               stream or None), "skred_bank_ctl_tags_each")

    # ---- per-note timbre (include/skred_amd.h: skred_bank_ctl_owned_each_filter / _ctl_tags_each_filter) ----
    def ctl_owned_each_filter(self, ctls, each, filt, voice_mask: int, filter_mask: int, d_slots: int, tags,
                              slot_voices: Optional[int] = None, d_count: int = 0, d_result: int = 0, stream: int = 0):
        """ctl_owned_each with entry k's coefficients filt[k] stored on the voices of filter_mask (each None: the coefficients only;
        ctls None: no base records, slot_voices required).  d_result (uint32[3], may be 0) as for ctl_owned_each."""
        f, t = filter_each_array(filt), tag_array(tags)
        e = ctl_each_array(each) if each is not None else None
        assert len(f) == len(t) and (e is None or len(e) == len(t)), "one entry per tag"
        arr = ctl_array(ctls) if ctls is not None else None
        K = len(arr) if slot_voices is None else int(slot_voices)
        _check(self.L.skred_bank_ctl_owned_each_filter(self.h, C.cast(arr, C.c_void_p) if arr is not None else None,
                                                       C.cast(e, C.c_void_p) if e is not None else None, C.cast(f, C.c_void_p), K,
                                                       int(voice_mask), int(filter_mask), d_slots or None, t.ctypes.data, len(t),
                                                       d_count or None, d_result or None, stream or None),
               "skred_bank_ctl_owned_each_filter")

    def ctl_tags_each_filter(self, ctls, each, filt, first: int, count: int, voice_mask: int, filter_mask: int, tags,
                             slot_voices: Optional[int] = None, d_result: int = 0, stream: int = 0):
        """Timbre by note id: filt[k] (and each[k]) on the lowest slot of [first, first + count) that carries tags[k]."""
        f, t = filter_each_array(filt), tag_array(tags)
        e = ctl_each_array(each) if each is not None else None
        assert len(f) == len(t) and (e is None or len(e) == len(t)), "one entry per tag"
        arr = ctl_array(ctls) if ctls is not None else None
        K = len(arr) if slot_voices is None else int(slot_voices)
        _check(self.L.skred_bank_ctl_tags_each_filter(self.h, C.cast(arr, C.c_void_p) if arr is not None else None,
                                                      C.cast(e, C.c_void_p) if e is not None else None, C.cast(f, C.c_void_p),
                                                      int(first), int(count), K, int(voice_mask), int(filter_mask), t.ctypes.data, len(t),
                                                      d_result or None, stream or None), "skred_bank_ctl_tags_each_filter")

    # ---- slot stealing (include/skred_amd.h: skred_bank_find_steal_slots / _find_steal_slots_host / _note_on_steal_slots) ----
    def find_steal_slots(self, q: SlotStealQueryC, d_slots: int = 0, d_count: int = 0, stream: int = 0):
        """Asynchronous on `stream`: the first voices of the first q.max_out candidate slots of the victim order (ascending key, ties
        by first voice) into d_slots[0 .. written) (int32, device memory); d_count[0] = written, d_count[1] = total (uint32)."""
        _check(self.L.skred_bank_find_steal_slots(self.h, C.byref(q), d_slots or None, d_count or None, stream or None),
               "skred_bank_find_steal_slots")

    def find_steal_slots_host(self, q: SlotStealQueryC, stream: int = 0):
        """The same into host memory, waiting for `stream` only.  Returns (np.int32 array of the victim slots, total candidates)."""
        out = np.empty(max(int(q.max_out), 0), np.int32)
        total = C.c_int(0)
        n = self.L.skred_bank_find_steal_slots_host(self.h, C.byref(q), out.ctypes.data if q.max_out > 0 else None, C.byref(total),
                                                    stream or None)
        if n < 0:
            _check(n, "skred_bank_find_steal_slots_host")
        return out[:n].copy(), int(total.value)

    def note_on_steal_slots(self, notes, idle_q: SlotQueryC, steal_q: SlotStealQueryC, voice_mask: int, d_assigned: int = 0,
                            d_result: int = 0, stream: int = 0):
        """The idle-slot query, the slot steal query (exclude_idle, settle_level and max_out overridden by the library), the victims
        appended behind the idle slots and the placement of the patch notes, in one call; d_result[0..3) = placed, dropped, stolen."""
        arr = note_array(notes)
        _check(self.L.skred_bank_note_on_steal_slots(self.h, C.byref(idle_q), C.byref(steal_q), C.cast(arr, C.c_void_p),
                                                     len(arr) // int(idle_q.slot_voices), int(voice_mask), d_assigned or None,
                                                     d_result or None, stream or None), "skred_bank_note_on_steal_slots")

    # ---- channel polyphony (include/skred_amd.h: skred_bank_find_steal_slots_match / _match_host / _note_on_channel) ----
    def find_steal_slots_match(self, q: SlotStealQueryC, m: OwnerMatchC, d_slots: int = 0, d_count: int = 0, stream: int = 0):
        """find_steal_slots restricted to the slots whose owner word matches `m`; d_count (uint32[3], device memory) = written, total
        candidates, sounding slots of the match in the range."""
        _check(self.L.skred_bank_find_steal_slots_match(self.h, C.byref(q), C.byref(m), d_slots or None, d_count or None, stream or None),
               "skred_bank_find_steal_slots_match")

    def find_steal_slots_match_host(self, q: SlotStealQueryC, m: OwnerMatchC, stream: int = 0):
        """The same into host memory, waiting for `stream` only.  Returns (np.int32 array of the victim slots, total, sounding)."""
        out = np.empty(max(int(q.max_out), 0), np.int32)
        total, sounding = C.c_int(0), C.c_int(0)
        n = self.L.skred_bank_find_steal_slots_match_host(self.h, C.byref(q), C.byref(m), out.ctypes.data if q.max_out > 0 else None,
                                                          C.byref(total), C.byref(sounding), stream or None)
        if n < 0:
            _check(n, "skred_bank_find_steal_slots_match_host")
        return out[:n].copy(), int(total.value), int(sounding.value)

    def note_on_channel(self, notes, tags, idle_q: SlotQueryC, steal_q: SlotStealQueryC, m: OwnerMatchC, cap: int, voice_mask: int,
                        d_assigned: int = 0, d_result: int = 0, stream: int = 0):
        """A burst of len(tags) patch notes of one channel under a polyphony cap: idle slots while the channel's sounding count stays
        below `cap`, then victims of the channel itself, every placed note tagged with its tags[k];
        d_result[0..4) = placed, dropped, stolen, the channel's sounding count before the burst."""
        arr = note_array(notes)
        t = tag_array(tags)
        _check(self.L.skred_bank_note_on_channel(self.h, C.byref(idle_q), C.byref(steal_q), C.byref(m), int(cap) & 0xFFFFFFFF,
                                                 C.cast(arr, C.c_void_p), t.ctypes.data, len(t), int(voice_mask), d_assigned or None,
                                                 d_result or None, stream or None), "skred_bank_note_on_channel")

    # ---- pedals (include/skred_amd.h: skred_bank_stamp_owned_pedal / _release_tags_pedal / _pedal_latch / _pedal_up) ----
    def stamp_owned_pedal(self, d_slots: int, tags, slot_voices: int, voice_mask: int, hold_all: bool, d_result: int, d_count: int = 0,
                          stream: int = 0):
        """stamp_owned's release, except where `hold_all` or the slot is latched: there the note-off is held back (PENDING).
        d_result (uint32[4]): slots stamped, slots whose owner differs, entries that are no slot, slots held back."""
        arr = tag_array(tags)
        _check(self.L.skred_bank_stamp_owned_pedal(self.h, d_slots or None, arr.ctypes.data, len(arr), d_count or None, int(slot_voices),
                                                   int(voice_mask), int(bool(hold_all)), d_result or None, stream or None),
               "skred_bank_stamp_owned_pedal")

    def release_tags_pedal(self, first: int, count: int, slot_voices: int, voice_mask: int, tags, hold_all: bool, d_result: int,
                           stream: int = 0):
        """Note-off by note id under the pedals: every tag reaches the lowest slot of the range that carries it.  d_result as for
        stamp_owned_pedal; [2] counts the tags nobody carries."""
        arr = tag_array(tags)
        _check(self.L.skred_bank_release_tags_pedal(self.h, int(first), int(count), int(slot_voices), int(voice_mask), arr.ctypes.data,
                                                    len(arr), int(bool(hold_all)), d_result or None, stream or None),
               "skred_bank_release_tags_pedal")

    def pedal_latch(self, first: int, count: int, slot_voices: int, voice_mask: int, m: OwnerMatchC, d_result: int, stream: int = 0):
        """Sostenuto down: LATCHED on the matching slots with a held voice and no pending note-off.  d_result (uint32[2]): slots
        latched, slots that did not match."""
        _check(self.L.skred_bank_pedal_latch(self.h, int(first), int(count), int(slot_voices), int(voice_mask), C.byref(m), d_result or None,
                                             stream or None), "skred_bank_pedal_latch")

    def pedal_up(self, first: int, count: int, slot_voices: int, voice_mask: int, m: OwnerMatchC, flags: int, d_result: int,
                 stream: int = 0):
        """A pedal goes up (PEDAL_LIFT_* / PEDAL_SUSTAIN_DOWN): the held-back note-offs of the matching slots are stamped now.
        d_result (uint32[3]): slots released, slots still pending, slots that did not match."""
        _check(self.L.skred_bank_pedal_up(self.h, int(first), int(count), int(slot_voices), int(voice_mask), C.byref(m), int(flags),
                                          d_result or None, stream or None), "skred_bank_pedal_up")

    def pedal_clear(self, first: int = 0, count: Optional[int] = None, stream: int = 0):
        count = self.n - first if count is None else count
        _check(self.L.skred_bank_pedal_clear(self.h, int(first), int(count), stream or None), "skred_bank_pedal_clear")

    def download_pedals(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The pedal words of [first, first + count) (uint32); waits for the device.  Zeros on a bank without a pedal array."""
        count = self.n - first if count is None else count
        out = np.full(max(count, 0), 0xDEADBEEF, np.uint32)
        _check(self.L.skred_bank_download_pedals(self.h, out.ctypes.data, int(first), int(count)), "skred_bank_download_pedals")
        return out

    # ---- portamento (include/skred_amd.h: skred_bank_glide_owned / _glide_tags / _glide_advance / _glide_stop) ----
    def glide_owned(self, glides, slot_voices: int, voice_mask: int, d_slots: int, tags, d_count: int = 0, d_result: int = 0,
                    stream: int = 0):
        """Entry k starts glides[k] on the masked voices of d_slots[k] where that slot's owner is tags[k].  d_result (uint32[3], may
        be 0): voices set gliding, starts withheld, slots whose owner differs."""
        arr, t = glide_array(glides), tag_array(tags)
        assert len(arr) == len(t)
        _check(self.L.skred_bank_glide_owned(self.h, C.cast(arr, C.c_void_p), int(slot_voices), int(voice_mask), d_slots or None,
                                             t.ctypes.data, len(t), d_count or None, d_result or None, stream or None),
               "skred_bank_glide_owned")

    def glide_tags(self, glides, first: int, count: int, slot_voices: int, voice_mask: int, tags, d_result: int = 0, stream: int = 0):
        """Glides by note id: glides[k] starts on the lowest slot of the range that carries tags[k]."""
        arr, t = glide_array(glides), tag_array(tags)
        assert len(arr) == len(t)
        _check(self.L.skred_bank_glide_tags(self.h, C.cast(arr, C.c_void_p), int(first), int(count), int(slot_voices), int(voice_mask),
                                            t.ctypes.data, len(t), d_result or None, stream or None), "skred_bank_glide_tags")

    def glide_advance(self, first: int, count: int, frames: int, d_result: int = 0, stream: int = 0):
        """Every gliding voice of the range moves by `frames` frames: one multiply per 64 of them, the target's bits on arrival.
        d_result (uint32[2], may be 0): voices still gliding, voices that arrived."""
        _check(self.L.skred_bank_glide_advance(self.h, int(first), int(count), int(frames), d_result or None, stream or None),
               "skred_bank_glide_advance")

    def glide_stop(self, first: int = 0, count: Optional[int] = None, snap: bool = False, stream: int = 0):
        count = self.n - first if count is None else count
        _check(self.L.skred_bank_glide_stop(self.h, int(first), int(count), int(bool(snap)), stream or None), "skred_bank_glide_stop")

    def download_glide(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The glide words of [first, first + count) as a (count, 4) uint32 array: target, rate_up, rate_down, carry; waits for the
        device.  Zeros on a bank that never started a glide."""
        count = self.n - first if count is None else count
        out = np.full((max(count, 0), 4), 0xDEADBEEF, np.uint32)
        _check(self.L.skred_bank_download_glide(self.h, out.ctypes.data, int(first), int(count)), "skred_bank_download_glide")
        return out

    # ---- pitch wheel (include/skred_amd.h: skred_bank_bend_match / _bend_owned_each / _bend_tags_each / _bend_clear) ----
    def bend_match(self, first: int, count: int, slot_voices: int, voice_mask: int, m: OwnerMatchC, ratio: float, d_result: int = 0,
                   stream: int = 0):
        """The channel wheel: the masked voices of every matching slot of the range sound at key * ratio; ratio 1.0 restores the key's
        bits.  d_result (uint32[3], may be 0): voices stored or restored, bends withheld, slots that did not match."""
        _check(self.L.skred_bank_bend_match(self.h, int(first), int(count), int(slot_voices), int(voice_mask), C.byref(m), float(ratio),
                                            d_result or None, stream or None), "skred_bank_bend_match")

    def bend_owned_each(self, ratios, slot_voices: int, voice_mask: int, d_slots: int, tags, d_count: int = 0, d_result: int = 0,
                        stream: int = 0):
        """Entry k bends the masked voices of d_slots[k] to ratios[k] where that slot's owner is tags[k].  d_result (uint32[3], may be
        0): voices stored or restored, bends withheld, slots whose owner differs."""
        arr, t = ratio_array(ratios), tag_array(tags)
        assert len(arr) == len(t)
        _check(self.L.skred_bank_bend_owned_each(self.h, arr.ctypes.data, int(slot_voices), int(voice_mask), d_slots or None,
                                                 t.ctypes.data, len(t), d_count or None, d_result or None, stream or None),
               "skred_bank_bend_owned_each")

    def bend_tags_each(self, ratios, first: int, count: int, slot_voices: int, voice_mask: int, tags, d_result: int = 0, stream: int = 0):
        """Per-note bend by note id: ratios[k] reaches the lowest slot of the range that carries tags[k]."""
        arr, t = ratio_array(ratios), tag_array(tags)
        assert len(arr) == len(t)
        _check(self.L.skred_bank_bend_tags_each(self.h, arr.ctypes.data, int(first), int(count), int(slot_voices), int(voice_mask),
                                                t.ctypes.data, len(t), d_result or None, stream or None), "skred_bank_bend_tags_each")

    def bend_clear(self, first: int = 0, count: Optional[int] = None, snap: bool = False, stream: int = 0):
        count = self.n - first if count is None else count
        _check(self.L.skred_bank_bend_clear(self.h, int(first), int(count), int(bool(snap)), stream or None), "skred_bank_bend_clear")

    # ---- filter cutoff on the device (include/skred_amd.h: skred_bank_cutoff_match / _cutoff_owned_each / _cutoff_tags_each / ...) ----
    def cutoff_match(self, first: int, count: int, slot_voices: int, filter_mask: int, m: OwnerMatchC, rec: CutoffC, d_result: int = 0,
                     stream: int = 0):
        """The channel sweep: `rec` on the filter_mask voices of every slot of the range whose owner matches.  d_result (uint32[4], may
        be 0): voices set or started, records withheld, slots that did not match, cutoffs clamped."""
        _check(self.L.skred_bank_cutoff_match(self.h, int(first), int(count), int(slot_voices), int(filter_mask), C.byref(m), C.byref(rec),
                                              d_result or None, stream or None), "skred_bank_cutoff_match")

    def cutoff_owned_each(self, recs, slot_voices: int, filter_mask: int, d_slots: int, tags, d_count: int = 0, d_result: int = 0,
                          stream: int = 0):
        """Entry k applies recs[k] on the masked voices of d_slots[k] where that slot's owner is tags[k]."""
        arr, t = cutoff_array(recs), tag_array(tags)
        assert len(arr) == len(t)
        _check(self.L.skred_bank_cutoff_owned_each(self.h, C.cast(arr, C.c_void_p), int(slot_voices), int(filter_mask), d_slots or None,
                                                   t.ctypes.data, len(t), d_count or None, d_result or None, stream or None),
               "skred_bank_cutoff_owned_each")

    def cutoff_tags_each(self, recs, first: int, count: int, slot_voices: int, filter_mask: int, tags, d_result: int = 0, stream: int = 0):
        """By note id: recs[k] reaches the lowest slot of the range that carries tags[k]."""
        arr, t = cutoff_array(recs), tag_array(tags)
        assert len(arr) == len(t)
        _check(self.L.skred_bank_cutoff_tags_each(self.h, C.cast(arr, C.c_void_p), int(first), int(count), int(slot_voices), int(filter_mask),
                                                  t.ctypes.data, len(t), d_result or None, stream or None), "skred_bank_cutoff_tags_each")

    def cutoff_advance(self, first: int, count: int, frames: int, d_result: int = 0, stream: int = 0):
        """The advance pass by `frames` frames; d_result (uint32[2], may be 0): voices still moving, voices that arrived."""
        _check(self.L.skred_bank_cutoff_advance(self.h, int(first), int(count), int(frames), d_result or None, stream or None),
               "skred_bank_cutoff_advance")

    def cutoff_stop(self, first: int = 0, count: Optional[int] = None, snap: bool = False, stream: int = 0):
        count = self.n - first if count is None else count
        _check(self.L.skred_bank_cutoff_stop(self.h, int(first), int(count), int(bool(snap)), stream or None), "skred_bank_cutoff_stop")

    def download_cutoff(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The cutoff words of [first, first + count) as a (count, 8) uint32 array: w, target, rate_up, rate_down, carry, q, mode, 0;
        waits for the device.  Zeros on a bank that never set a cutoff."""
        count = self.n - first if count is None else count
        out = np.zeros((count, 8), np.uint32)
        _check(self.L.skred_bank_download_cutoff(self.h, out.ctypes.data, int(first), int(count)), "skred_bank_download_cutoff")
        return out

    # ---- filter envelope (include/skred_amd.h: skred_bank_fenv_match / _fenv_owned_each / _fenv_tags_each; cutoff_advance steps it) ----
    def fenv_match(self, first: int, count: int, slot_voices: int, filter_mask: int, m: OwnerMatchC, rec: FenvC, d_result: int = 0,
                   stream: int = 0):
        """The channel sweep: `rec` on the filter_mask voices of every slot of the range whose owner matches.  d_result (uint32[4], may
        be 0): voices started, records withheld, slots that did not match, voices clamped."""
        _check(self.L.skred_bank_fenv_match(self.h, int(first), int(count), int(slot_voices), int(filter_mask), C.byref(m), C.byref(rec),
                                            d_result or None, stream or None), "skred_bank_fenv_match")

    def fenv_owned_each(self, recs, slot_voices: int, filter_mask: int, d_slots: int, tags, d_count: int = 0, d_result: int = 0,
                        stream: int = 0):
        """Entry k applies recs[k] on the masked voices of d_slots[k] where that slot's owner is tags[k]."""
        arr, t = fenv_array(recs), tag_array(tags)
        assert len(arr) == len(t)
        _check(self.L.skred_bank_fenv_owned_each(self.h, C.cast(arr, C.c_void_p), int(slot_voices), int(filter_mask), d_slots or None,
                                                 t.ctypes.data, len(t), d_count or None, d_result or None, stream or None),
               "skred_bank_fenv_owned_each")

    def fenv_tags_each(self, recs, first: int, count: int, slot_voices: int, filter_mask: int, tags, d_result: int = 0, stream: int = 0):
        """By note id: recs[k] reaches the lowest slot of the range that carries tags[k]."""
        arr, t = fenv_array(recs), tag_array(tags)
        assert len(arr) == len(t)
        _check(self.L.skred_bank_fenv_tags_each(self.h, C.cast(arr, C.c_void_p), int(first), int(count), int(slot_voices), int(filter_mask),
                                                t.ctypes.data, len(t), d_result or None, stream or None), "skred_bank_fenv_tags_each")

    def download_fenv(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The fenv words of [first, first + count) as a (count, 8) uint32 array: stage, w_peak, w_sustain, w_end, rate_attack,
        rate_decay, rate_release, 0; waits for the device.  Zeros on a bank without the array."""
        count = self.n - first if count is None else count
        out = np.zeros((count, 8), np.uint32)
        _check(self.L.skred_bank_download_fenv(self.h, out.ctypes.data, int(first), int(count)), "skred_bank_download_fenv")
        return out

    def download_bend(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The bend words of [first, first + count) as a (count, 2) uint32 array: key, ratio; waits for the device.  Zeros on a bank
        that never bent."""
        count = self.n - first if count is None else count
        out = np.full((max(count, 0), 2), 0xDEADBEEF, np.uint32)
        _check(self.L.skred_bank_download_bend(self.h, out.ctypes.data, int(first), int(count)), "skred_bank_download_bend")
        return out

    def force_generic(self, on: bool = True):
        _check(self.L.skred_bank_set_option(self.h, 1, int(on)), "skred_bank_set_option")

    def fast2_min_voices(self, n: int):
        """Bank size from which the two-voices-per-lane kernel is chosen (0 = always when eligible)."""
        _check(self.L.skred_bank_set_option(self.h, 2, int(n)), "skred_bank_set_option")

    def fm2_min_voices(self, n: int):
        """Bank size from which a two-operator FM bank keeps carrier and modulator in one lane (SKRED_OPT_FM2_MIN_VOICES)."""
        _check(self.L.skred_bank_set_option(self.h, 5, int(n)), "skred_bank_set_option")

    def in_place(self, mode=1):
        """SKRED_OPT_IN_PLACE: 1 short motion lists rendered in the steady kernel's lanes where that is faster (default), 0 never
        (always the envelope kernel beside it), 2 whenever the gain rows provably suffice."""
        _check(self.L.skred_bank_set_option(self.h, 6, int(mode)), "skred_bank_set_option")

    def set_split(self, mode: int) -> None:
        """SKRED_OPT_SPLIT: 0 never (default), 1 the oscillator-wave / post-wave form of the one-voice kernel where it is faster,
        2 whenever the bank qualifies."""
        _check(self.L.skred_bank_set_option(self.h, 7, int(mode)), "skred_bank_set_option")

    def set_probe(self, voices, d_probe: int) -> None:
        """skred_bank_set_probe: (L, R) of every frame of the listed voices into d_probe[frame][i][2] (device memory), written from
        inside the kernels' fast paths; an empty list ends it."""
        v = np.ascontiguousarray(voices, np.int32)
        _check(self.L.skred_bank_set_probe(self.h, v.ctypes.data if len(v) else None, len(v), d_probe or None), "skred_bank_set_probe")

    def set_taps(self, voices, d_taps: int) -> None:
        """skred_bank_set_taps: the (L, R) the reference stores into its stem buffer for the listed voices (64 at most), every frame of
        every later block, into d_taps[frame][k][2] (device memory) -- from whichever kernel family renders the block; the layout a
        wav.Recorder(len(voices), ...) appends.  An empty list ends it."""
        v = np.ascontiguousarray(voices, np.int32)
        _check(self.L.skred_bank_set_taps(self.h, v.ctypes.data if len(v) else None, len(v), d_taps or None), "skred_bank_set_taps")

    def last_taps(self) -> int:
        """Taps written by the latest block, 0: none."""
        return int(self.L.skred_bank_last_taps(self.h))

    def set_form_counter(self, d_counts: int) -> None:
        """skred_bank_set_form_counter: per pass of each wavefront of the modulated kernel, +1 in d_counts[0] (uint32, device memory)
        for the frame-lag form, in d_counts[1] for the level loop of a bank with same-frame dependencies; 0 ends it."""
        _check(self.L.skred_bank_set_form_counter(self.h, d_counts or None), "skred_bank_set_form_counter")

    def set_pack(self, mode: int) -> None:
        """SKRED_OPT_PACK: 1 sparse banks rendered with packed lanes where it pays (default), 0 never, 2 whenever a wavefront disappears."""
        _check(self.L.skred_bank_set_option(self.h, 9, int(mode)), "skred_bank_set_option")

    def set_fm_skew(self, on: int) -> None:
        """SKRED_OPT_FM_SKEW: 1 (default) modulator lanes of a frequency-modulated wavefront run a block ahead of their carriers, 0 per-frame exchange."""
        _check(self.L.skred_bank_set_option(self.h, 10, int(on)), "skred_bank_set_option")

    def set_cross_group(self, on: bool) -> None:
        """SKRED_OPT_CROSS_GROUP: 1 modulators in another aligned 64-voice group of the bank are rendered through the source tape,
        0 (default) such banks are refused."""
        _check(self.L.skred_bank_set_option(self.h, 11, int(bool(on))), "skred_bank_set_option")

    def last_cross_group(self):
        """(n_sources, n_levels) of the latest block: tape sources and pre-pass launches; (0, 0) when it read no tape."""
        ns, nl = C.c_int32(0), C.c_int32(0)
        _check(self.L.skred_bank_last_cross_group(self.h, C.byref(ns), C.byref(nl)), "skred_bank_last_cross_group")
        return int(ns.value), int(nl.value)

    def last_pack(self) -> int:
        """Lanes per 64-voice group in the latest block, 0: not packed."""
        return int(self.L.skred_bank_last_pack(self.h))

    def set_cz_fast(self, on: bool) -> None:
        """SKRED_OPT_CZ_FAST: 1 banks whose CZ voices all qualify (mode 1..7, no CZ source or one above the carrier in its 64-voice
        group, other modulators as for the one-voice kernel) render on the one-voice-per-lane kernel, 0 (default) on the modulated one."""
        _check(self.L.skred_bank_set_option(self.h, 12, int(bool(on))), "skred_bank_set_option")

    def last_cz(self) -> bool:
        """The latest block ran a CZ instantiation of the one-voice-per-lane kernel (SKRED_OPT_CZ_FAST)."""
        return bool(self.L.skred_bank_last_cz(self.h))

    def set_split_pairs(self, pairs: int) -> None:
        """SKRED_OPT_SPLIT_PAIRS (tests): 0 the library's choice, 2 / 4 pairs per workgroup forced."""
        _check(self.L.skred_bank_set_option(self.h, 8, int(pairs)), "skred_bank_set_option")

    def last_split(self) -> bool:
        return bool(self.L.skred_bank_last_split(self.h))

    def last_in_place(self) -> bool:
        return bool(self.L.skred_bank_last_in_place(self.h))

    def last_kernel(self) -> int:
        """0 = generic kernel, 1 = specialised fast kernel (SKRED_KERNEL_*)."""
        return int(self.L.skred_bank_last_kernel(self.h))

    def list_violations(self) -> int:
        """Voices the steady two-per-lane kernel found in motion without being on the motion list (cross-check; 0 by construction)."""
        return int(self.L.skred_bank_list_violations(self.h))

    def last_render_ms(self) -> float:
        return float(self.L.skred_bank_last_render_ms(self.h))

    def timing_reset(self):
        self.L.skred_bank_timing_reset(self.h)

    def timing_summary(self):
        """(mean_ms, min_ms, count) of the render kernel over the calls since timing_reset()."""
        mean, mn, cnt = C.c_float(), C.c_float(), C.c_int()
        _check(self.L.skred_bank_timing_summary(self.h, C.byref(mean), C.byref(mn), C.byref(cnt)),
               "skred_bank_timing_summary")
        return float(mean.value), float(mn.value), int(cnt.value)


class SeqClock:
    """skred_seq_t: the reference's pattern step clock (seq.c:179-213) on the host."""

    def __init__(self, handle=None, owner: bool = True):
        self.L = load()
        self.owner = owner
        if handle is None:
            h = C.c_void_p()
            _check(self.L.skred_seq_create(C.byref(h)), "skred_seq_create")
            handle = h
        self.h = C.c_void_p(handle) if isinstance(handle, int) else handle

    def close(self):
        if self.owner and self.h:
            self.L.skred_seq_destroy(self.h)
        self.h = None

    def tempo(self, bpm: float):
        _check(self.L.skred_seq_tempo_set(self.h, bpm), "skred_seq_tempo_set")

    def time_per_step(self) -> float:
        return float(self.L.skred_seq_time_per_step(self.h))

    def step(self, pattern: int, step: int, occupied: bool = True):
        _check(self.L.skred_seq_step_set(self.h, pattern, step, int(occupied)), "skred_seq_step_set")

    def mute(self, pattern: int, step: int, on: bool = True):
        _check(self.L.skred_seq_mute_set(self.h, pattern, step, int(on)), "skred_seq_mute_set")

    def modulo(self, pattern: int, m: int):
        _check(self.L.skred_seq_modulo_set(self.h, pattern, m), "skred_seq_modulo_set")

    def state(self, pattern: int, state: int):
        _check(self.L.skred_seq_state_set(self.h, pattern, state), "skred_seq_state_set")

    def reset(self, pattern: int):
        _check(self.L.skred_seq_pattern_reset(self.h, pattern), "skred_seq_pattern_reset")

    def pointer(self, pattern: int) -> int:
        return int(self.L.skred_seq_pointer(self.h, pattern))

    def counter(self, pattern: int) -> int:
        return int(self.L.skred_seq_counter(self.h, pattern))

    def tick(self, frame_count: int, sample_rate: float = 44100.0):
        """[(pattern, step)] of the steps that fire in this block."""
        out = (C.c_int32 * 16)()
        n = self.L.skred_seq_tick(self.h, frame_count, sample_rate, out, 16)
        if n < 0:
            _check(n, "skred_seq_tick")
        return [(out[i] >> 16, out[i] & 0xFFFF) for i in range(n)]
