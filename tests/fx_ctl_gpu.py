"""What tests/test_fx_owner.py and tests/test_fx_ctl.py share on the GPU: the bank they run on and the comparison of EVERY word the
device holds -- skred_fxbank_download's read-write fields, skred_fxbank_download_params' parameter fields and reciprocals, the owner
words -- with the oracle's state, byte for byte."""
import numpy as np

import fx_ctl_model as cm
from oracle import cpuref
from skred_amd import fxbank as fxb

FLAGS = ("use_envelope", "smoother_enable", "disconnect", "filter_mode", "one_shot")     # one bit each on the device


def ctl_bank(n):
    """The bank_fx recipe with voices without filter, envelope and smoother, muted, silent (amp 0) and released ones mixed in."""
    b, pool, c0 = fxb.bank_fx(n)
    v = np.arange(n)
    b["filter_mode"][v % 5 == 0] = 0
    b["use_envelope"][v % 6 == 1] = 0
    b["smoother_enable"][v % 7 == 2] = 0
    b["disconnect"][v % 9 == 3] = 1
    b["amp_q15"][v % 11 == 4] = 0
    rel = v % 4 == 1
    b["sample_release"][rel] = (c0 - (v[rel] * 13) % 2000).astype(np.uint64)
    b["phase_inc"] = (b["phase_inc"] >> np.uint32(2)) + np.uint32(1 << 20)                # room above for a pitch bend
    return b, pool, c0


def open_fx(b, pool, c0):
    db = fxb.DeviceFxBank(b.n)
    db.set_tables(pool)
    db.upload(b)
    db.set_sample_count(c0)
    return db


def assert_state(db, ref, tag, owner=None):
    got = ref.copy()
    for k in got.a:
        got[k][...] = 0x55                                  # every field must come back from the device
    db.download(got)
    recip = db.download_params(got)
    bad = {}
    for k in ref.a:
        want = (ref[k] != 0).astype(ref[k].dtype) if k in FLAGS or k in ("is_active", "finished") else ref[k]
        if got[k].tobytes() != want.tobytes():
            bad[k] = np.flatnonzero(got[k] != want)[:4].tolist()
    assert not bad, f"{tag}: fields differ from the model's at {bad}"
    assert recip.tobytes() == cm.recips(ref).tobytes(), f"{tag}: reciprocals differ"
    if owner is not None:
        assert db.download_owners().tobytes() == owner.tobytes(), f"{tag}: owner words differ"


def block(db, ref, pool, cnt, frames, interp, tag, stems=True):
    """One block on both sides: mix and stems bit for bit against the oracle."""
    mix, st = db.render_host(frames, interp, want_stems=stems)
    want, want_st, cnt = cpuref.fx_render(ref, pool, cnt, frames, interp, want_stems=stems)
    assert (mix == want).all(), f"{tag}: the mix differs from the oracle's"
    assert not stems or (st == want_st).all(), f"{tag}: the stems differ from the oracle's"
    assert db.sample_count() == cnt
    return cnt


def dev_i32(values):
    import torch
    return torch.tensor(np.asarray(values, np.int32), dtype=torch.int32, device="cuda")


def dev_fill(k, fill=-7):
    import torch
    return torch.full((k,), fill, dtype=torch.int32, device="cuda")


def host_of(t):
    return t.cpu().numpy()


def u32(t):
    return host_of(t).view(np.uint32).tolist()
