"""The pitch wheel without a GPU: the symbols against the header, the model (tests/bend_model.py) against a plain loop over every
voice, the properties the definition promises on the model alone (the wheel returns to the key's bits where the INC_SCALE route does
not; withheld bends; a glide under a bend; the clear rule), every refusal with its return code, the packing and the permutation
(through tests/c_bend_host.c, a program of its own on a bank that is nothing but its size), and a mono line on the oracle alone.

Every increment, key and product chosen here lies in the normal fp32 range (|x| >= 2 ** -126) or is exactly zero, infinite, NaN or the
smallest denormal (whose product with 0.25 is zero on any IEEE multiplier).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import bend_model as BM
import glide_model as GM
import owner_model as OM
import owner_scenes as OS
import slot_model as SM
from oracle import cpuref
from skred_amd import device

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
SYMBOLS = ("skred_bank_bend_match", "skred_bank_bend_owned_each", "skred_bank_bend_tags_each", "skred_bank_bend_clear",
           "skred_bank_download_bend")
SEMI = 2.0 ** (1.0 / 12.0)
ONE = int(BM.ONE)


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    L = device.load()
    for s in SYMBOLS + ("skred_bend_check",):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in device.ABI_SYMBOLS + device.HOST_ABI_SYMBOLS
    assert "pitch wheel" in text and "ABSOLUTE BEND" in text


# ---------------------------------------------------------------------------------------------- the model against a loop

def f32_mul(a, b):
    """the fp32 product by another road: the double product of two fp32 values is exact, one rounding to fp32 follows"""
    x = np.array([a], np.uint32).view(np.float32).astype(np.float64)[0] * np.array([b], np.uint32).view(np.float32).astype(np.float64)[0]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return int(np.array([x], np.float64).astype(np.float32).view(np.uint32)[0])


def ok_bits(x):
    return (x & 0x7F800000) != 0x7F800000 and (x & 0x7FFFFFFF) != 0


def brute_voice(bend, w, v, r):
    """THE RULE on one voice.  Returns 1: stored or restored, 2: withheld, 0: neither."""
    key, cur = int(bend[v, 0]), int(w[v])
    k = key if key else cur
    if r == ONE:
        if key:
            w[v] = key
        bend[v] = 0
        return 1 if key else 0
    p = f32_mul(k, r)
    if not ok_bits(k) or not ok_bits(p):
        return 2
    w[v] = p
    bend[v] = (k, r)
    return 1


def brute_match(owner, bend, inc, first, count, K, vmask, match, ratio):
    w, res = inc.view(np.uint32), [0, 0, 0]
    r = int(BM.bits(np.float32(ratio)))
    for s in range(first, first + count, K):
        o = int(owner[s])
        if o == 0 or (o & match[1]) != match[0]:
            res[2] += 1
            continue
        for l in range(K):
            if (vmask >> l) & 1:
                d = brute_voice(bend, w, s + l, r)
                if d:
                    res[d - 1] += 1
    return res


def brute_owned(owner, bend, inc, ratios, K, vmask, entries, tags, count):
    w, res = inc.view(np.uint32), [0, 0, 0]
    m = len(tags) if count is None else min(len(tags), count)
    for k in range(m):
        e = int(entries[k])
        if e < 0 or e % K or e > len(owner) - K:
            continue
        if int(owner[e]) != int(tags[k]):
            res[2] += 1
            continue
        for l in range(K):
            if (vmask >> l) & 1:
                d = brute_voice(bend, w, e + l, int(BM.bits(np.float32(ratios[k]))))
                if d:
                    res[d - 1] += 1
    return res


def random_bank(rng, n, K):
    inc = (rng.uniform(1e-3, 0.5, n) * rng.choice([1, 1, 1, -1], n)).astype(np.float32)
    inc[rng.integers(0, n, 4)] = 0.0
    inc[rng.integers(0, n, 3)] = np.float32(np.inf)
    inc[rng.integers(0, n, 2)] = np.float32(np.nan)
    inc[rng.integers(0, n, 3)] = np.float32(3e38)
    inc[rng.integers(0, n, 2)] = np.array([1], np.uint32).view(np.float32)[0]
    owner = OM.new(n)
    heads = np.arange(0, n, K)
    owner[heads] = (rng.integers(1, 5, len(heads)).astype(np.uint32) << np.uint32(24)) | (heads // K + 1).astype(np.uint32)
    owner[heads[rng.integers(0, len(heads), 5)]] = 0
    return owner, BM.new(n), inc


WHEEL = [1.5, 1.0, float(SEMI), 2.0, 0.25, 1.0, 3.0, 1.0 / float(SEMI), 0.5, 1.0]


@pytest.mark.parametrize("K", [1, 4, 64])
def test_model_against_a_plain_loop(K):
    rng = np.random.default_rng(900 + K)
    n = 1536
    owner, bend, inc = random_bank(rng, n, K)
    full = (1 << K) - 1
    part = full if K == 1 else (1 << (K - 1)) | 1
    seen = [0, 0, 0]
    for step, ratio in enumerate(WHEEL):
        first = (int(rng.integers(0, n // K // 2)) * K) if step % 2 else 0
        count = (int(rng.integers(1, n // K // 2)) * K) if step % 2 else n
        match = ((int(rng.integers(1, 5)) << 24), 0xFF000000) if step % 3 else (0, 0)
        vmask = part if step % 4 == 3 else full
        a, b, ba, bb = inc.copy(), inc.copy(), bend.copy(), bend.copy()
        got = BM.bend_match(owner, ba, a, first, count, K, vmask, match, ratio)
        want = brute_match(owner, bb, b, first, count, K, vmask, match, ratio)
        assert got == want and a.tobytes() == b.tobytes() and ba.tobytes() == bb.tobytes(), (K, step, got, want)
        # per entry: a list with a hole, a slot past the bank, an entry that is no slot, a stolen slot and a count word
        heads = rng.permutation(np.arange(0, n, K))[:40].astype(np.int32)
        entries = np.r_[heads[:10], [-1, n, 1 if K > 1 else -1], heads[10:]].astype(np.int32)
        tags = np.where(owner[np.clip(entries, 0, n - 1)] != 0, owner[np.clip(entries, 0, n - 1)], 77).astype(np.uint32)
        tags[3] ^= np.uint32(0x00800000)
        ratios = rng.choice(np.array(WHEEL, np.float32), len(entries))
        a2, b2, ba2, bb2 = a.copy(), a.copy(), ba.copy(), ba.copy()
        got2 = BM.bend_owned_each(owner, ba2, a2, ratios, K, vmask, entries, tags, count=len(entries) - 2)
        want2 = brute_owned(owner, bb2, b2, ratios, K, vmask, entries, tags, len(entries) - 2)
        assert got2 == want2 and a2.tobytes() == b2.tobytes() and ba2.tobytes() == bb2.tobytes(), (K, step, got2, want2)
        w = a2.view(np.uint32)
        moved = w != inc.view(np.uint32)
        assert BM.usable(w[moved]).all(), "a store that is zero or not finite"
        seen = [seen[0] + got[0] + got2[0], seen[1] + got[1] + got2[1], seen[2] + got[2] + got2[2]]
        inc, bend = a2, ba2
    assert min(seen) > 10, seen


# ---------------------------------------------------------------------------------------------- the wheel returns to the key

WHEEL_SEED = 2026         # chosen here, on the CPU: the share asserted below is numpy's fp32 multiply and nothing else


def wheel_walk(rng, steps=200):
    """`steps` wheel positions within +-2 semitones, the last at centre"""
    pos = BM.ratio_of(rng.uniform(-2.0, 2.0, steps))
    pos[-1] = np.float32(1.0)
    assert (pos[:-1] != 1.0).all()
    return pos


def test_the_wheel_returns_to_the_keys_bits():
    rng = np.random.default_rng(WHEEL_SEED)
    n = 2048
    inc = (rng.uniform(1e-4, 0.5, n) * rng.choice([1, -1], n)).astype(np.float32)
    original = inc.copy()
    owner, bend = OM.new(n), BM.new(n)
    owner[:] = np.uint32(3 << 24 | 1)
    pos = wheel_walk(rng)
    for r in pos:
        res = BM.bend_match(owner, bend, inc, 0, n, 1, 1, (3 << 24, 0xFF000000), r)
        assert res == [n, 0, 0]
    assert inc.tobytes() == original.tobytes(), "the wheel at centre did not restore the key's bits"
    assert not bend.any(), "the centre left state behind"
    # the same walk through the INC_SCALE route: the ratio of consecutive positions, one unfused multiply each
    scaled, last = original.copy(), np.float32(1.0)
    for r in pos:
        scaled = (scaled * (r / last).astype(np.float32)).astype(np.float32)
        last = r
    off = int((scaled.view(np.uint32) != original.view(np.uint32)).sum())
    print(f"INC_SCALE route: {off} of {n} voices ({100.0 * off / n:.1f} %) do not return to the key's bits after {len(pos)} wheel messages")
    assert off > 0
    # a single up-and-back is enough to part some of them
    r = np.float32(SEMI)
    back = ((original * r).astype(np.float32) * (np.float32(1.0) / r)).astype(np.float32)
    one = int((back.view(np.uint32) != original.view(np.uint32)).sum())
    print(f"INC_SCALE route: {one} of {n} voices do not return after one semitone up and back")
    assert one > 0


def test_bends_are_absolute():
    """the same message twice is the same bits twice, and a bend does not depend on the one before it"""
    rng = np.random.default_rng(5)
    inc = rng.uniform(1e-3, 0.4, 64).astype(np.float32)
    key = inc.copy()
    owner, bend = OM.new(64), BM.new(64)
    owner[:] = 9
    m = (9, 0xFFFFFFFF)
    BM.bend_match(owner, bend, inc, 0, 64, 1, 1, m, 1.25)
    once = inc.copy()
    BM.bend_match(owner, bend, inc, 0, 64, 1, 1, m, 1.25)
    assert inc.tobytes() == once.tobytes() == (key * np.float32(1.25)).astype(np.float32).tobytes()
    BM.bend_match(owner, bend, inc, 0, 64, 1, 1, m, 0.8)
    BM.bend_match(owner, bend, inc, 0, 64, 1, 1, m, 1.25)
    assert inc.tobytes() == once.tobytes() and (bend[:, 0] == key.view(np.uint32)).all() and (bend[:, 1] == BM.bits(np.float32(1.25))).all()
    # the centre on a voice that was never bent stores nothing, counts nothing and leaves no state
    fresh = key.copy()
    b2 = BM.new(64)
    assert BM.bend_match(owner, b2, fresh, 0, 64, 1, 1, m, 1.0) == [0, 0, 0] and fresh.tobytes() == key.tobytes() and not b2.any()


def test_withheld_bends_leave_the_voice_alone():
    tiny = np.array([1], np.uint32).view(np.float32)[0]             # the smallest denormal: times 0.25 it is zero
    inc = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, 3e38, 0.01], np.float32)
    owner, bend = OM.new(8), BM.new(8)
    owner[:] = 5
    before = inc.copy()
    assert BM.bend_match(owner, bend, inc, 0, 8, 1, 1, (5, 0xFFFFFFFF), 0.25) == [2, 6, 0]
    assert inc[:6].tobytes() == before[:6].tobytes() and not bend[:6].any()
    assert inc[6] == np.float32(3e38) * np.float32(0.25) and inc[7] == np.float32(0.0025) and bend[6:, 0].tolist() == before[6:].view(np.uint32).tolist()
    # a ratio that overflows: the bent voice keeps its words and its increment, the unbent one stays unbent
    snap_inc, snap_bend = inc.copy(), bend.copy()
    assert BM.bend_match(owner, bend, inc, 6, 1, 1, 1, (5, 0xFFFFFFFF), 2.0) == [0, 1, 0]
    assert inc.tobytes() == snap_inc.tobytes() and bend.tobytes() == snap_bend.tobytes()
    assert BM.bend_match(owner, bend, inc, 0, 5, 1, 1, (5, 0xFFFFFFFF), 3e38) == [0, 5, 0]
    assert BM.bend_match(owner, bend, inc, 6, 1, 1, 1, (5, 0xFFFFFFFF), 3e38) == [0, 1, 0]     # (the denormal and 0.01 times 3e38 are finite: they stay out)
    assert inc.tobytes() == snap_inc.tobytes() and bend.tobytes() == snap_bend.tobytes()
    # per entry, with the guard: the stolen slot is counted, not bent
    owner[7] = 6
    assert BM.bend_owned_each(owner, bend, inc, [0.5, 0.5], 1, 1, [6, 7], [5, 5]) == [1, 0, 1]
    assert inc[7] == np.float32(0.0025) and inc[6] == np.float32(3e38) * np.float32(0.5)
    # the centre: restores the key's bits
    assert BM.bend_match(owner, bend, inc, 0, 8, 1, 1, (0, 0), 1.0) == [2, 0, 0]
    assert inc.tobytes() == before.tobytes() and not bend.any()


def test_clear_with_and_without_snap():
    inc = np.array([0.01, 0.02, 0.03, 0.04], np.float32)
    key = inc.copy()
    owner, bend = OM.new(4), BM.new(4)
    owner[:] = 5
    BM.bend_match(owner, bend, inc, 0, 4, 1, 1, (0, 0), 1.5)
    bent = inc.copy()
    BM.clear(bend, inc, 0, 2, True)
    BM.clear(bend, inc, 2, 1, False)
    assert inc[:2].tobytes() == key[:2].tobytes() and inc[2:].tobytes() == bent[2:].tobytes()
    assert not bend[:3].any() and bend[3, 0] == key.view(np.uint32)[3]


# ---------------------------------------------------------------------------------------------- a glide under a bend

K4 = 4
RATIOS = np.array([1.0, 2.0, 3.0, 0.5], np.float32)


def patch_slot(base=0.01):
    owner, glide, bend = OM.new(K4), GM.new(K4), BM.new(K4)
    owner[0] = 77
    return owner, glide, bend, (np.float32(base) * RATIOS).astype(np.float32)


@pytest.mark.parametrize("mode", ["from", "to"])
def test_a_glide_under_a_bend_lands_on_target_times_ratio(mode):
    """512 frames cut as 8 x 64, 1 x 512 and 37 + 100 + 27 + 348: the same words at every multiple of 64 frames; on arrival the
    sounding increment is target * ratio bit for bit; the wheel at centre then gives the target's bits."""
    wheel = np.float32(SEMI ** 1.5)
    up, down = GM.per_64(450.0)                                       # 0.65 semitones per step: three semitones take five of the eight steps
    scale = np.float32(SEMI ** -3) if mode == "from" else np.float32(SEMI ** 3)

    def run(cuts):
        owner, glide, bend, inc = patch_slot()
        struck = inc.copy()
        assert BM.bend_owned_each(owner, bend, inc, [wheel], K4, 0xF, [0], [77]) == [4, 0, 0]
        g = GM.Glide(GM.FROM_SCALE if mode == "from" else GM.TO_SCALE, up, down, scale)
        assert BM.glide_start_owned(owner, glide, bend, inc, [g], K4, 0xF, [0], [77]) == [4, 0, 0]
        target = struck if mode == "from" else (struck * scale).astype(np.float32)
        assert (glide[:, 0] == target.view(np.uint32)).all()
        if mode == "from":
            assert (bend[:, 0] == BM.mul(struck.view(np.uint32), BM.bits(scale))).all()
        else:
            assert (bend[:, 0] == struck.view(np.uint32)).all()
        assert (inc.view(np.uint32) == BM.mul(bend[:, 0], bend[:, 1])).all()
        at, seen = 0, {}
        for f in cuts:
            BM.glide_advance(glide, bend, inc, 0, K4, f)
            at += f
            assert (inc.view(np.uint32) == BM.mul(bend[:, 0], bend[:, 1])).all(), "the sounding increment is not key * ratio"
            if at % 64 == 0:
                seen[at] = inc.tobytes() + bend.tobytes() + glide.tobytes()
        assert at == 512 and not glide.any(), "the glide did not arrive within 512 frames"
        assert (bend[:, 0] == target.view(np.uint32)).all()
        assert inc.tobytes() == (target * wheel).astype(np.float32).tobytes(), "not target * ratio"
        assert BM.bend_owned_each(owner, bend, inc, [1.0], K4, 0xF, [0], [77]) == [4, 0, 0]
        assert inc.tobytes() == target.tobytes() and not bend.any(), "the centre did not give the target's bits"
        return seen

    ref = run([64] * 8)
    assert len(set(ref.values())) >= 3
    for cuts in ([512], [37, 100, 27, 348]):
        got = run(cuts)
        assert got and all(ref[at] == b for at, b in got.items()), cuts


def test_an_unbent_voice_glides_as_it_always_did():
    """key == 0: the glide calls under a bend array write what glide_model writes, and the wheel moved mid-glide is carried along"""
    owner, glide, bend, inc = patch_slot()
    o2, g2, _, i2 = patch_slot()
    up, down = GM.per_64(300.0)
    g = GM.Glide(GM.FROM_SCALE, up, down, np.float32(0.5))
    assert BM.glide_start_owned(owner, glide, bend, inc, [g], K4, 0xF, [0], [77]) == GM.start_owned(o2, g2, i2, [g], K4, 0xF, [0], [77])
    for f in (64, 100, 512):
        assert BM.glide_advance(glide, bend, inc, 0, K4, f) == GM.advance(g2, i2, 0, K4, f)
        assert inc.tobytes() == i2.tobytes() and glide.tobytes() == g2.tobytes() and not bend.any()
    # the wheel moves while the glide is under way: the key is the gliding increment, and the glide goes on from it
    assert BM.bend_owned_each(owner, bend, inc, [1.25], K4, 0xF, [0], [77]) == [4, 0, 0]
    assert (bend[:, 0] == i2.view(np.uint32)).all()
    BM.glide_advance(glide, bend, inc, 0, K4, 64)
    GM.advance(g2, i2, 0, K4, 64)
    assert (bend[:, 0] == i2.view(np.uint32)).all() and inc.tobytes() == (i2 * np.float32(1.25)).astype(np.float32).tobytes()
    BM.glide_stop(glide, bend, inc, 0, K4, True)
    GM.stop(g2, i2, 0, K4, True)
    assert (bend[:, 0] == i2.view(np.uint32)).all() and inc.tobytes() == (i2 * np.float32(1.25)).astype(np.float32).tobytes() and not glide.any()


# ---------------------------------------------------------------------------------------------- the clear rule, two scenes

def thief_scene():
    """A bent slot is stolen: the thief's note-on stores its own increments and its tag launch follows.  The thief's first bend must
    bend the THIEF's key.  Returns (the thief's increments after its first bend, what they must be)."""
    owner, glide, bend, inc = patch_slot(0.01)
    BM.bend_owned_each(owner, bend, inc, [1.5], K4, 0xF, [0], [77])
    thief = (np.float32(0.02) * RATIOS).astype(np.float32)
    inc[:] = thief                                                   # the note-on
    OM.tag_slots(owner, [0], [88], None, K4)
    BM.tag_clear(bend, [0], 1, None, K4)
    BM.bend_owned_each(owner, bend, inc, [1.25], K4, 0xF, [0], [88])
    BM.bend_owned_each(owner, bend, inc, [1.0], K4, 0xF, [0], [88])
    return inc, thief


def restrike_scene():
    """Mono mode: a key sounds bent, the same slot is struck again at another key and tagged again, and the wheel returns to centre.
    The new key must sound at its own increments."""
    owner, glide, bend, inc = patch_slot(0.01)
    BM.bend_match(owner, bend, inc, 0, K4, K4, 0xF, (0, 0), 0.8)
    struck = (np.float32(0.015) * RATIOS).astype(np.float32)
    inc[:] = struck
    OM.tag_slots(owner, [0], [77], None, K4)                         # the same tag: the same key of the same channel
    BM.tag_clear(bend, [0], 1, None, K4)
    BM.bend_match(owner, bend, inc, 0, K4, K4, 0xF, (0, 0), 1.0)
    return inc, struck


@pytest.mark.parametrize("scene", [thief_scene, restrike_scene])
def test_a_new_note_clears_the_words(scene, monkeypatch):
    got, want = scene()
    assert got.tobytes() == want.tobytes()                           # CLEAR RULE
    monkeypatch.setattr(BM, "CLEAR_RULE", False)
    got, want = scene()
    assert got.tobytes() != want.tobytes(), "the scene does not tell a model without the clear from one with it"
    assert got.tobytes() == (np.float32(0.01) * RATIOS).astype(np.float32).tobytes(), "without the clear the centre restores the VICTIM's key"


def test_the_tag_launch_clears_the_slot():
    bend = BM.new(16)
    bend[:] = 5
    BM.tag_clear(bend, [4, -1, 16, 6, 8], 5, 4, 4)                   # the first four entries: one slot, a hole, past the bank, no slot
    assert not bend[4:8].any() and bend[:4].all() and bend[8:].all()


# ---------------------------------------------------------------------------------------------- the entry points' host checks

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bend") / "c_bend_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_bend_host.c"), os.path.join(CSRC, "skred_bank_bend.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"),
           "-lskred_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-lm", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "skred_amd"),
           "-Wl,-rpath," + os.path.join(rocm, "lib")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return out.stdout.strip().splitlines()


def test_host_program(host_lines):
    bad = [l for l in host_lines[:-1] if not l.endswith(" ok")]
    assert not bad, bad
    assert host_lines[-1] == "OK" and len(host_lines) >= 90
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "check", "pack", "perm", "match", "owned", "tags", "clear", "download", "untouched"}, groups


def test_check_through_ctypes():
    good = [1.0, 1.5, 0.5]
    assert device.bend_check(good, 8, 0x55) == 0 == BM.check(good, 8, 0x55)
    assert device.bend_check(None, 8, 0x55) == BAD == BM.check(None, 8, 0x55)
    assert device.bend_check(good, 12, 0x55) == RANGE == BM.check(good, 12, 0x55)
    assert device.bend_check(good, 8, 0) == BAD == BM.check(good, 8, 0) and device.bend_check(good, 8, 0x155) == BAD == BM.check(good, 8, 0x155)
    for r in (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert device.bend_check([1.5, r], 8, 0x55) == BAD == BM.check([1.5, r], 8, 0x55), r
        assert b"ratio 1" in device.load().skred_amd_last_error()
    assert device.bend_check([0.0], 3, 1) == RANGE == BM.check([0.0], 3, 1)      # K first


# ---------------------------------------------------------------------------------------------- a mono line on the oracle

def test_a_mono_line_on_the_oracle():
    """tests/owner_scenes.py's bank (3.sk tiled over 256 voices, K = 4), one slot, three keys.  Both lines play the same keys and the
    same legato glide (key one to key two, TO_SCALE); the `bent` line's wheel also moves through key one and the glide and is back at
    centre before the glide arrives.  After centre and arrival the two lines hold the same increments bit for bit -- the target's.
    Their phases parted while the wheel was off centre, so their stems stay different until a note sets the phases again: key three is
    struck on both lines with the oscillators' phases, last samples and filter memory reset, and from the first block in which the slot's read-write state (phase,
    filter memory, ...) agrees -- that block exists, and it is the first block of key three -- the stems of the whole bank are equal
    bit for bit.  Nothing outside the slot ever hears of the wheel."""
    bank, tables, g = OS.bank()
    K, N, F = OS.K, OS.N, OS.F
    slot = int(OS.others()[5])
    vs = np.arange(slot, slot + K)
    rest = np.setdiff1d(np.arange(N), vs)
    plain, bent = bank.copy(), bank.copy()
    gp, gb = g.copy(), g.copy()
    tag = 0x03000030
    owner, glide_p, glide_b, bend = OM.new(N), GM.new(N), GM.new(N), BM.new(N)
    none = BM.new(N)                                                 # the plain line has a bend array too, and never bends
    OM.tag_slots(owner, [slot], [tag], None, K)
    base = bank["voice_phase_inc"][vs].copy()
    assert (np.abs(base) > 1e-6).all() and len(set(base.tolist())) > 1, "the patch's voices sit at different ratios"
    up, down = GM.per_64(700.0)

    def strike(semis, reset_phase):
        note = (base * np.float32(SEMI ** semis)).astype(np.float32)
        now = int(gp.synth_sample_count)
        assert now == int(gb.synth_sample_count)
        for b in (plain, bent):
            b["voice_phase_inc"][vs] = note
            if reset_phase:                                          # the oscillator and everything that remembers its past output
                b["voice_phase"][vs] = np.float32(0.0)
                b["voice_sample"][vs] = np.float32(0.0)
                for sub in ("x1", "x2", "y1", "y2"):
                    b["voice_filter"][sub][vs] = np.float32(0.0)
            SM.stamp(b, vs, SM.STAMP_TRIGGER, now)
        for gl in (glide_p, glide_b):
            GM.tag_clear(gl, [slot], 1, None, K)
        BM.tag_clear(bend, [slot], 1, None, K)
        return note

    def blocks(n, wheel=None):
        """n blocks; ahead of block k the bent line's wheel goes to wheel[k] semitones.  Returns (blocks whose slot stems differ,
        the first block ahead of which the two lines' read-write state and increments agree, or None: from it on the stems must)."""
        differ, agree = 0, None
        for k in range(n):
            if wheel is not None:
                res = BM.bend_tags_each(owner, bend, bent["voice_phase_inc"], [BM.ratio_of(wheel[k])], 0, N, K, OS.VMASK, [tag])[0]
                assert res[1] == 0
            BM.glide_advance(glide_p, none, plain["voice_phase_inc"], 0, N, F)
            BM.glide_advance(glide_b, bend, bent["voice_phase_inc"], 0, N, F)
            same_state = not plain.rw_equal(bent) and plain["voice_phase_inc"].tobytes() == bent["voice_phase_inc"].tobytes()
            a = cpuref.render(plain, gp, tables, F, 0, want_stems=True)["stems"]
            b = cpuref.render(bent, gb, tables, F, 0, want_stems=True)["stems"]
            assert a[:, rest].tobytes() == b[:, rest].tobytes(), "a voice outside the slot changed"
            same = a.tobytes() == b.tobytes()
            differ += not same
            if same_state and agree is None:
                agree = k
            if agree is not None:
                assert same and not plain.rw_equal(bent), f"block {k}: the lines part again after their state agreed in block {agree}"
        return differ, agree

    # key one, the wheel moving
    one = strike(0, False)
    differ, agree = blocks(6, wheel=[0.5, 1.0, 1.5, 2.0, 1.5, 1.0])
    assert differ >= 1 and agree is None
    assert (bend[vs, 0] == one.view(np.uint32)).all() and not np.array_equal(bent["voice_phase_inc"][vs], one)
    # legato onto key two (five semitones up) on both lines, the wheel still off centre on the bent one
    g5 = GM.Glide(GM.TO_SCALE, up, down, np.float32(SEMI ** 5))
    assert BM.glide_start_owned(owner, glide_p, none, plain["voice_phase_inc"], [g5], K, OS.VMASK, [slot], [tag]) == [K, 0, 0]
    assert BM.glide_start_owned(owner, glide_b, bend, bent["voice_phase_inc"], [g5], K, OS.VMASK, [slot], [tag]) == [K, 0, 0]
    two = (one * np.float32(SEMI ** 5)).astype(np.float32)
    assert (glide_p[vs, 0] == two.view(np.uint32)).all() and glide_b.tobytes() == glide_p.tobytes()
    blocks(3, wheel=[0.75, 0.5, 0.0])                                # back at centre while the glide is under way
    assert not bend.any() and glide_b[vs, 0].all(), "centre must come before arrival in this scene"
    assert bent["voice_phase_inc"][vs].tobytes() == plain["voice_phase_inc"][vs].tobytes(), "at centre the gliding increment is the key"
    differ, agree = blocks(12)
    assert not glide_p.any() and not glide_b.any(), "the glide did not arrive"
    assert plain["voice_phase_inc"][vs].tobytes() == bent["voice_phase_inc"][vs].tobytes() == two.tobytes(), "not the target's bits"
    # (the patch plays square waves whose period is some 400 frames: a single 64-frame block may hold no edge and sound the same)
    assert differ >= 6 and agree is None and (plain["voice_phase"][vs] != bent["voice_phase"][vs]).any(), "the phases parted under the wheel"
    # key three, the oscillators' phases set by the note: state and stems agree from its first block on
    strike(-3, True)
    print("ahead of key three's first block the lines differ in", plain.rw_equal(bent))
    differ, agree = blocks(6)
    print(f"key three: the slot's state agrees from block {agree}, {differ} blocks differ")
    assert agree == 0 and differ == 0
