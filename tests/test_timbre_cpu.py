"""Per-note timbre without a GPU: the record and the symbols against the header, skred_filter_each_check against the model, every
refusal with its return code and the packing and permutation of the coefficients for n = 1, 2, 1023 and 1024 (through
tests/c_timbre_host.c, a program of its own on banks that are nothing but their size), the model against a brute-force loop over
every voice (tests/timbre_model.py is what tests/test_timbre.py holds the device to), skred_filter_coeffs bit for bit against the
drop-in mode's mmf_set_params, and three notes with three cutoffs on the oracle alone."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import ctl_model as CM
import expr_model as EM
import owner_model as OM
import timbre_model as TM
from oracle import cpuref
from skred_amd import banks, device
from skred_amd.device import ctl, ctl_each, filter_each

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
CALLS = ("skred_bank_ctl_owned_each_filter", "skred_bank_ctl_tags_each_filter")
SYNTH_RATE = 44100.0                                         # SKRED_MAIN_SAMPLE_RATE: the drop-in library's rate


# ---------------------------------------------------------------------------------------------- the header, the symbols

def test_record_and_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    assert C.sizeof(device.FilterEachC) == 32
    body = re.search(r"typedef struct skred_filter_each \{(.*?)\} skred_filter_each_t;", text, re.S).group(1)
    names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in device.FilterEachC._fields_], names
    L = device.load()
    for s in CALLS:
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s) and s in device.ABI_SYMBOLS, s
    for s in ("skred_filter_each_check", "skred_filter_coeffs"):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s) and s in device.HOST_ABI_SYMBOLS, s
    # the axis is no longer out of scope, in either header
    for header in (text, open(os.path.join(ROOT, "include", "skred_amd_fxpt.h")).read()):
        for line in header.splitlines():
            assert not ("Out of scope" in line and "per-entry filter" in line), line
    assert "#define SKRED_MAIN_SAMPLE_RATE 44100" in open(os.path.join(ROOT, "include", "skred_synth_abi.h")).read()


def test_filter_check_is_the_models():
    K = 4
    plain = [ctl(CM.PAN, pan_left=0.5, pan_right=0.5) for _ in range(K)]
    named = plain[:2] + [ctl(CM.FILTER, b0=0.5)] + plain[3:]
    ok = [filter_each(0.1, 0.2, 0.1, -0.5, 0.3)]
    resv = filter_each(0.1, 0.2, 0.1, -0.5, 0.3)
    resv.reserved[1] = 7
    cases = [(ok, plain, K, 0xF, 0xF), (ok, plain, K, 0xF, 0x5), (ok, None, K, 0xF, 0x1), (ok, plain, K, 0xF, 0), (ok, plain, K, 0x3, 0x6),
             (ok, None, K, 0x3, 0x4), (ok, None, K, 0, 0), (ok, None, K, 0x10, 0x10), (ok, None, 3, 0x7, 0x7), (ok, None, 128, 0xF, 0xF),
             (ok, named, K, 0xF, 0x4), (ok, named, K, 0xF, 0xB), (ok, named, K, 0xB, 0xB), ([resv], plain, K, 0xF, 0xF),
             (ok + [resv], plain, K, 0xF, 0xF), ([], plain, K, 0xF, 0xF), (ok, None, 64, (1 << 64) - 1, 1 << 63)]
    for bad in (float("inf"), float("-inf"), float("nan")):
        for c in range(5):
            v = [0.1] * 5
            v[c] = bad
            cases.append(([filter_each(*v)], plain, K, 0xF, 0xF))
    seen = set()
    for filt, ctls, k, vm, fm in cases:
        want = TM.filter_check(filt, ctls, k, vm, fm)
        assert device.filter_each_check(filt, ctls, vm, fm, k) == want, (len(filt), k, hex(vm), hex(fm))
        seen.add(want)
    assert seen == {0, BAD, RANGE}
    assert device.filter_each_check(None, plain, 0xF, 0xF) == TM.filter_check(None, plain, K, 0xF, 0xF) == BAD
    assert device.filter_each_check(ok, plain[:3] + [ctl(0)], 0xF, 0x1) == BAD          # what skred_ctl_check refuses about the records
    assert device.load().skred_filter_each_check(C.cast(device.filter_each_array(ok), C.c_void_p), -1, None, 4, 0xF, 0xF) == BAD


def test_entry_points_refuse_a_null_bank():
    L = device.load()
    tags = device.tag_array([1, 2])
    f = C.cast(device.filter_each_array([filter_each(0.1, 0.2, 0.1, -0.5, 0.3)] * 2), C.c_void_p)
    word = C.c_void_p(16)                                    # (a refused call never reads through the device pointers)
    assert L.skred_bank_ctl_owned_each_filter(None, None, None, f, 8, 0xFF, 0xFF, word, tags.ctypes.data, 2, None, None, None) == BAD
    assert L.skred_bank_ctl_tags_each_filter(None, None, None, f, 0, 64, 8, 0xFF, 0xFF, tags.ctypes.data, 2, None, None) == BAD


# ---------------------------------------------------------------------------------------------- the entry points' host checks, the packing

@functools.lru_cache(maxsize=1)
def host_lines():
    """Builds and runs tests/c_timbre_host.c once (tests/test_fx_timbre_cpu.py reads the fixed-point groups of the same run)."""
    exe = os.path.join(tempfile.mkdtemp(prefix="timbre_host"), "c_timbre_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_timbre_host.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"), "-lskred_amd", "-lm", "-lpthread",
           "-Wl,-rpath," + os.path.join(ROOT, "skred_amd")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return tuple(out.stdout.strip().splitlines())


def group_passed(group):
    mine = [l for l in host_lines() if l.startswith(group + "/")]
    assert mine, f"no case of group {group} ran"
    bad = [l for l in mine if not l.endswith(" ok")]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("group", ["const", "check", "pack", "perm", "coeffs", "owned", "tags", "plain", "bank"])
def test_host_cases(group):
    group_passed(group)


def test_every_host_case_passed():
    assert host_lines()[-1] == "OK", "\n".join(l for l in host_lines() if not l.endswith(" ok"))
    assert {"perm/1 ok", "perm/2 ok", "perm/1023 ok", "perm/1024 ok"} <= set(host_lines())


# ---------------------------------------------------------------------------------------------- the model against a brute-force loop

def brute_force(owner, before, ctls, each, filt, K, vmask, fmask, entries, tags, count):
    """Every voice of the bank in turn: which entry reaches it, and what that entry leaves there -- the five words from filt[k] where
    the voice's lane is in filter_mask, everything else from expr_model's record."""
    after = before.copy()
    m = len(tags) if count is None else min(count, len(tags))
    written = withheld = 0
    for v in range(before.n):
        slot, l = v - v % K, v % K
        hits = [k for k in range(m) if int(entries[k]) == slot and slot + K <= before.n and int(owner[slot]) == int(tags[k])]
        if not hits or not (vmask >> l) & 1:
            continue
        (k,) = hits
        if each is not None or ctls is not None:
            rec, w = EM.lay_over(ctls[l] if ctls is not None else None, each[k]) if each is not None else (EM.Rec(ctls[l]), 0)
            withheld += w + CM.store_voice(after, v, rec)
        if (fmask >> l) & 1:
            for c in TM.COEFFS:
                after["voice_filter"][c][v] = np.float32(getattr(filt[k], c))
        written += 1
    differs = sum(1 for k in range(m) if CM.slot_valid(int(entries[k]), K, before.n) and int(owner[int(entries[k])]) != int(tags[k]))
    return after, [written, withheld, differs]


@pytest.mark.parametrize("K,vmask,fmask", [(1, 1, 1), (4, 0b1111, 0b1111), (4, 0b1011, 0b0010), (8, 0xF1, 0x81)])
def test_model_equals_a_loop_over_every_voice(K, vmask, fmask):
    n = 128
    bank, _, _ = banks.bank_c2(n)
    bank["voice_amp"][5::11] = 0.0
    owner = OM.new(n)
    slots = np.arange(0, n, K)
    OM.tag_slots(owner, slots, (0x03000000 + np.arange(len(slots)) + 1).astype(np.uint32), None, K)
    rng = np.random.default_rng(K)
    entries = rng.permutation(slots)[:12].astype(np.int32)
    tags = owner[entries].copy()
    entries[3] = -1                                          # a hole
    tags[5] ^= 0x100                                         # a stolen slot
    entries[7] = n                                           # past the bank
    filt = [filter_each(0.1 + 0.01 * k, 0.2, 0.1 + 0.02 * k, -0.5 - 0.01 * k, 0.3) for k in range(12)]
    each = [ctl_each((EM.EACH_INC_SCALE, EM.EACH_AMP_SCALE, EM.EACH_VELOCITY, EM.EACH_PAN)[k % 4], inc_scale=1.0 + 0.01 * k, amp_scale=0.5,
                     velocity=0.3, pan_left=0.2, pan_right=0.7) for k in range(12)]
    recs = [ctl(CM.AMP | CM.SMOOTHING | (0 if (fmask >> l) & 1 else CM.FILTER), amp=0.4 + 0.01 * l, smoothing=0.2, b0=0.9, a2=-0.9) for l in range(K)]
    for ctls, ee, count in ((recs, each, None), (None, None, None), (None, None, 6), (recs, None, 9)):
        model = bank.copy()
        res, touched = TM.ctl_owned_each_filter(owner, (model,), ctls, ee, filt, K, vmask, fmask, entries, tags, count)
        want, want_res = brute_force(owner, bank, ctls, ee, filt, K, vmask, fmask, entries, tags, count)
        assert res == want_res, (res, want_res)
        assert not CM.words_differ(model, want) and not model.rw_equal(want), CM.words_differ(model, want)
        if ctls is None and ee is None:
            diff = CM.words_differ(model, bank)
            assert set(diff) == {"voice_filter." + c for c in TM.COEFFS} and res[1] == 0
            changed = np.flatnonzero(model["voice_filter"]["b0"] != bank["voice_filter"]["b0"])
            assert changed.tolist() == touched[np.isin(touched % K, CM.lanes(fmask, K))].tolist()
        for m in ("x1", "x2", "y1", "y2"):
            assert model["voice_filter"][m].tobytes() == bank["voice_filter"][m].tobytes()
    assert TM.lists(None, None, K, vmask, 12) == 0 and TM.lists(recs, None, K, vmask, 12) == 12 * bin(vmask).count("1")


def test_model_tags_route_keeps_each_set_with_its_tag():
    n, K = 64, 4
    bank, _, _ = banks.bank_c2(n)
    owner = OM.new(n)
    OM.tag_slots(owner, [0, 20, 60], [0x03000001, 0x03000002, 0xFFFFFFFF], None, K)
    tags = np.array([0xFFFFFFFF, 0x03000002, 0x55, 0x03000001], np.uint32)
    filt = [filter_each(0.1 * (k + 1), 0, 0, 0, 0) for k in range(4)]
    a = bank.copy()
    res, touched, lst = TM.ctl_tags_each_filter(owner, (a,), None, None, filt, 0, n, K, 0b0011, 0b0001, tags)
    assert res == [6, 0, 0] and lst.tolist() == [60, 20, -1, 0] and touched.tolist() == [0, 1, 20, 21, 60, 61]
    b0 = a["voice_filter"]["b0"]
    assert b0[60] == np.float32(0.1) and b0[20] == np.float32(0.2) and b0[0] == np.float32(0.4) and b0[61] == bank["voice_filter"]["b0"][61]
    srt, permuted, perm = EM.pack(tags, filt)                # what the library ships: sorted tags, filt permuted beside them
    b = bank.copy()
    assert TM.ctl_tags_each_filter(owner, (b,), None, None, permuted, 0, n, K, 0b0011, 0b0001, srt)[0] == res
    assert b["voice_filter"].tobytes() == a["voice_filter"].tobytes()


# ---------------------------------------------------------------------------------------------- the coefficient helper

class MmfC(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("x1", "x2", "y1", "y2", "b0", "b1", "b2", "a1", "a2", "last_freq", "last_resonance")] + [("last_mode", C.c_int32)]


def test_filter_coeffs_are_the_drop_ins_bit_for_bit():
    """The drop-in's mmf_set_params calls skred_filter_coeffs, so this sweep holds the drop-in's cache keys, its rate and its stores to
    the function; the arithmetic itself is held to an independent restatement by tests/c_timbre_host.c (coeffs/sweep_...) and to the
    reference's state by tests/test_dropin.py."""
    S = C.CDLL(os.path.join(ROOT, "skred_amd", "libskred_synth.so"))
    S.mmf_set_params.argtypes = [C.c_int, C.c_float, C.c_float]
    S.mmf_set_params.restype = None
    mode_of = (C.c_int * 64).in_dll(S, "voice_filter_mode")
    filt = (MmfC * 64).in_dll(S, "voice_filter")
    v = 5

    def drop_in(mode, f, res):
        mode_of[v] = mode
        S.mmf_set_params(v, f, res)
        q = filt[v]
        return np.array([q.b0, q.b1, q.b2, q.a1, q.a2], np.float32)

    freqs = np.float32(20.0) * np.exp2(np.arange(64, dtype=np.float32) * np.float32(10.0 / 63.0))       # 20 Hz .. 20.48 kHz
    ress = np.array([0.1, 0.5, 0.707, 1.0, 1.5, 2.5, 4.0, 12.0], np.float32)
    n = 0
    for mode in (1, 2, 3, 4, 5, 9):                          # 9: an unknown mode falls to low-pass
        for f in freqs:
            for res in ress:
                got = np.array(device.filter_coeffs(mode, float(f), float(res), SYNTH_RATE), np.float32)
                want = drop_in(mode, float(f), float(res))
                assert got.tobytes() == want.tobytes(), (mode, float(f), float(res), got, want)
                n += 1
    assert n == 6 * 64 * 8
    low = np.array(device.filter_coeffs(1, 1000.0, 0.7, SYNTH_RATE), np.float32)
    assert np.array(device.filter_coeffs(9, 1000.0, 0.7, SYNTH_RATE), np.float32).tobytes() == low.tobytes()
    assert np.array(device.filter_coeffs(-3, 1000.0, 0.7, SYNTH_RATE), np.float32).tobytes() == low.tobytes()
    # mode 0: bypass -- nothing is computed on either side, the words stay
    kept = drop_in(1, 432.0, 0.9)
    assert drop_in(0, 999.0, 0.8).tobytes() == kept.tobytes()
    assert device.filter_coeffs(0, 999.0, 0.8, SYNTH_RATE) is None
    out = (C.c_float * 5)(7, 7, 7, 7, 7)
    assert device.load().skred_filter_coeffs(0, 999.0, 0.8, SYNTH_RATE, out) == 1 and list(out) == [7.0] * 5
    assert device.load().skred_filter_coeffs(1, 999.0, 0.8, SYNTH_RATE, None) == BAD
    # the rate is an argument: another rate, other coefficients; and what banks.biquad_coeffs states in numpy is the same arithmetic
    assert np.array(device.filter_coeffs(1, 1000.0, 0.7, 48000.0), np.float32).tobytes() != low.tobytes()


# ---------------------------------------------------------------------------------------------- three notes, three cutoffs, on the oracle

def test_three_notes_three_cutoffs_on_the_oracle():
    """3.sk over four copies, its carriers filtered, the three first copies in the SAME state: without the call they render the same
    stems.  Three cutoffs by note id through the model: three different stems, each bit-equal to a bank whose host view was given
    those coefficients directly."""
    n, K, F = 16, 4, 64
    bank, tables, g = banks.bank_patch("3sk", n)
    carriers = (0, 1, 2)
    sel = np.isin(np.arange(n) % K, carriers)
    bank["voice_filter_mode"][sel] = 1
    for c, v in zip(TM.COEFFS, device.filter_coeffs(1, 2000.0, 0.707, SYNTH_RATE)):
        bank["voice_filter"][c][sel] = v
    for s in (4, 8):
        bank["voice_phase"][s:s + K] = bank["voice_phase"][0:K]
    owner = OM.new(n)
    tags = np.array([3 << 24 | 67, 3 << 24 | 60, 3 << 24 | 64], np.uint32)
    OM.tag_slots(owner, [0, 4, 8], tags, None, K)
    filt = [filter_each(*device.filter_coeffs(1, f, 0.9, SYNTH_RATE)) for f in (400.0, 1600.0, 6400.0)]

    def stems_of(b):
        ref = cpuref.render(b, g.copy(), tables, F, 0, want_stems=True)
        ref2 = cpuref.render(b, g.copy(), tables, F, 0, want_stems=True)
        return np.concatenate([ref["stems"], ref2["stems"]])

    untouched = stems_of(bank.copy())
    note = lambda st, s: st[:, s:s + 3, :].tobytes()   # noqa: E731
    assert note(untouched, 0) == note(untouched, 4) == note(untouched, 8) and np.abs(untouched[:, 0:3]).sum() > 0
    through_model, direct = bank.copy(), bank.copy()
    res, touched, lst = TM.ctl_tags_each_filter(owner, (through_model,), None, None, filt, 0, n, K, 0b0111, 0b0111, tags)
    assert res == [9, 0, 0] and lst.tolist() == [0, 4, 8]
    for k, s in enumerate((0, 4, 8)):
        for l in carriers:
            for c in TM.COEFFS:
                direct["voice_filter"][c][s + l] = np.float32(getattr(filt[k], c))
    a, b = stems_of(through_model), stems_of(direct)
    for s in (0, 4, 8):
        assert note(a, s) == note(b, s), f"the stems of slot {s} differ from the directly written bank's"
        assert note(a, s) != note(untouched, s)
    assert len({note(a, 0), note(a, 4), note(a, 8)}) == 3, "three cutoffs, three stems"
    assert a[:, 12:16].tobytes() == untouched[:, 12:16].tobytes(), "the fourth copy heard nothing"
    assert a.tobytes() == b.tobytes() and not through_model.rw_equal(direct)
