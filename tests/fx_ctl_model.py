"""Numpy statement of the fixed-point bank's controllers (include/skred_amd_fxpt.h: skred_fx_ctl_check, skred_fxbank_ctl_range /
_ctl_list / _ctl_owned), on the arrays oracle.cpuref.fx_render works on.  A record is a skred_amd.fxbank.FxCtlC; every store is
exact.  The reciprocals of the frame counts are not part of an FxVoiceBank (the definition derives them): `recips` restates them
for the comparison with skred_fxbank_download_params."""
import numpy as np

from skred_amd import fxbank as fxb

BAD = -2
M32 = 0xFFFFFFFF
FIELDS = {
    fxb.CTL_PHASE_INC: ("phase_inc",), fxb.CTL_INC_SCALE: ("inc_scale_q16",), fxb.CTL_AMP: ("amp_q15",),
    fxb.CTL_PAN: ("pan_left_q15", "pan_right_q15"), fxb.CTL_FILTER: ("b0_q30", "b1_q30", "b2_q30", "a1_q30", "a2_q30"),
    fxb.CTL_ENV_TIMES: ("attack_frames", "decay_frames", "release_frames", "sustain_q15"),
    fxb.CTL_VELOCITY: ("velocity_q15",), fxb.CTL_SMOOTHING: ("smoother_k_q15",),
}
RANGES = {"amp_q15": (1, 65535), "pan_left_q15": (0, 65535), "pan_right_q15": (0, 65535), "sustain_q15": (0, 32768),
          "velocity_q15": (0, 65535), "smoother_k_q15": (0, 32768)}
# what a controller can store (the comparison with the device's download covers every OTHER field too)
STORED = sorted({"phase_inc", *[f for fs in FIELDS.values() for f in fs]} - {"inc_scale_q16"})


def check(c):
    """skred_fx_ctl_check's verdict: 0 or SKRED_E_BAD_ARG."""
    if c is None or c.which == 0 or c.which & ~fxb.CTL_ALL or any(c.reserved):
        return BAD
    for bit, names in FIELDS.items():
        if c.which & bit:
            for name in names:
                lo, hi = RANGES.get(name, (None, None))
                if lo is not None and not lo <= getattr(c, name) <= hi:
                    return BAD
    return 0


def store(bank, c, v):
    """The stores of record c on voice v.  Returns the stores withheld (0, 1 or 2)."""
    withheld = 0
    w = c.which
    if w & fxb.CTL_PHASE_INC:
        bank["phase_inc"][v] = c.phase_inc
    if w & fxb.CTL_INC_SCALE:
        prod = (int(bank["phase_inc"][v]) * int(c.inc_scale_q16)) >> 16
        if prod <= M32:
            bank["phase_inc"][v] = prod
        else:
            withheld += 1
    if w & fxb.CTL_AMP:
        if bank["amp_q15"][v] != 0:
            bank["amp_q15"][v] = c.amp_q15
        else:
            withheld += 1
    for bit in (fxb.CTL_PAN, fxb.CTL_FILTER, fxb.CTL_ENV_TIMES, fxb.CTL_VELOCITY, fxb.CTL_SMOOTHING):
        if w & bit:
            for name in FIELDS[bit]:
                bank[name][v] = getattr(c, name)
    return withheld


def ctl_range(bank, c, first, count):
    """Returns [voices written, stores withheld]."""
    assert check(c) == 0 and 0 <= first and count >= 0 and first + count <= bank.n
    return [count, sum(store(bank, c, v) for v in range(first, first + count))]


def ctl_list(bank, c, entries, n, d_count=None, owner=None, tags=None, scale_once=True):
    """The record on the looked-at entries that are voices (and, with `owner`, whose owner word is the entry's tag), in list order.
    Returns [written, withheld] or, guarded, [written, withheld, owner differs].  A voice listed twice gets the absolute stores
    twice; under INC_SCALE the device's increment is unspecified, so such lists are refused here."""
    assert check(c) == 0
    m = n if d_count is None else min(n, int(d_count))
    e = np.asarray(entries, np.int64)[:m]
    res = [0, 0, 0]
    seen = set()
    for k, v in enumerate(e.tolist()):
        if v < 0 or v >= bank.n:
            continue
        if owner is not None and owner[v] != np.uint32(tags[k]):
            res[2] += 1
            continue
        assert not (c.which & fxb.CTL_INC_SCALE and v in seen), "INC_SCALE on a voice listed twice is unspecified"
        seen.add(v)
        res[0] += 1
        res[1] += store(bank, c, v)
    return res if owner is not None else res[:2]


def recips(bank):
    """uint32 [n][3]: floor(2^32 / X) for the three frame counts as skred_fxbank_upload packs them (0 for X == 0; 2^32 wraps to 0)"""
    out = np.zeros((bank.n, 3), np.uint32)
    for j, name in enumerate(("attack_frames", "decay_frames", "release_frames")):
        x = bank[name].astype(np.uint64)
        out[:, j] = np.where(x > 0, (np.uint64(1 << 32) // np.maximum(x, np.uint64(1))) & np.uint64(M32), 0).astype(np.uint32)
    return out
