"""Portamento without a GPU: the symbols against the header, the model (tests/glide_model.py) against a brute-force loop over every
voice and every 64-frame step, the properties the definition promises on the model alone, every refusal with its return code, the
32-byte packing and the permutation (through tests/c_glide_host.c, a program of its own on a bank that is nothing but its size), and a
mono line of three keys on the oracle alone.

Every increment, target and product chosen here lies in the normal fp32 range (|x| >= 2 ** -126) or is exactly zero, infinite or NaN:
the one place a host multiply and the device's could part is a denormal, and the definition is not tested there.
"""
import os
import re
import subprocess

import numpy as np
import pytest

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
SYMBOLS = ("skred_bank_glide_owned", "skred_bank_glide_tags", "skred_bank_glide_advance", "skred_bank_glide_stop",
           "skred_bank_download_glide")
SEMI = 2.0 ** (1.0 / 12.0)


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    L = device.load()
    for s in SYMBOLS + ("skred_glide_check",):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in device.ABI_SYMBOLS + device.HOST_ABI_SYMBOLS
    for name, value in (("FROM_SCALE", 0), ("TO_SCALE", 1)):
        assert re.search(r"SKRED_GLIDE_%s = 1u << %d\b" % (name, value), text), name
        assert getattr(device, "GLIDE_" + name) == getattr(GM, name) == 1 << value
    assert re.search(r"uint32_t set; float rate_up, rate_down, scale; uint32_t reserved\[4\];", text)
    import ctypes
    assert ctypes.sizeof(device.GlideC) == 32 and device.GlideC.scale.offset == 12 and device.GlideC.reserved.offset == 16


# ---------------------------------------------------------------------------------------------- the model against a loop

def f32_mul(a, b):
    """the fp32 product by another road: the double product of two fp32 values is exact, one rounding to fp32 follows"""
    x = np.array([a], np.uint32).view(np.float32).astype(np.float64)[0] * np.array([b], np.uint32).view(np.float32).astype(np.float64)[0]
    with np.errstate(over="ignore", invalid="ignore"):
        return int(np.array([x], np.float64).astype(np.float32).view(np.uint32)[0])


def fin(x):
    return (x & 0x7F800000) != 0x7F800000


def brute_advance(glide, inc, first, count, frames):
    w = inc.view(np.uint32)
    res = [0, 0]
    for v in range(first, first + count):
        tgt = int(glide[v, 0])
        if tgt == 0:
            continue
        cur, t = int(w[v]), tgt & 0x7FFFFFFF
        there = (cur & 0x7FFFFFFF) == 0 or not fin(cur) or bool((cur ^ tgt) >> 31)
        c = int(glide[v, 3]) + frames
        for _ in range(c >> 6):                                   # every 64-frame step, one by one
            if there:
                break
            a = cur & 0x7FFFFFFF
            if a < t:
                cur = f32_mul(cur, int(glide[v, 1]))
                there = not fin(cur) or (cur & 0x7FFFFFFF) >= t
            elif a > t:
                cur = f32_mul(cur, int(glide[v, 2]))
                there = not fin(cur) or (cur & 0x7FFFFFFF) <= t
            else:
                there = True
        if there:
            w[v] = tgt
            glide[v] = 0
            res[1] += 1
        else:
            w[v] = cur
            glide[v, 3] = c & 63
            res[0] += 1
    return res


def random_state(rng, n):
    inc = (rng.uniform(1e-3, 0.5, n) * rng.choice([1, 1, 1, -1], n)).astype(np.float32)
    inc[rng.integers(0, n, 4)] = 0.0
    inc[rng.integers(0, n, 3)] = np.float32(np.inf)
    inc[rng.integers(0, n, 2)] = np.float32(np.nan)
    inc[rng.integers(0, n, 3)] = np.float32(3e38)
    glide = GM.new(n)
    on = rng.integers(0, 3, n) != 0
    ratio = 2.0 ** rng.uniform(-2, 2, n)
    with np.errstate(over="ignore", invalid="ignore"):
        target = (np.where(np.isfinite(inc) & (inc != 0), inc, np.float32(0.25)) * ratio * rng.choice([1, 1, 1, 1, -1], n)).astype(np.float32)
    target[~np.isfinite(target)] = np.float32(3.3e38)
    target[rng.integers(0, n, 6)] = inc[rng.integers(0, n, 6)]    # some level with an increment somewhere, some anything
    target[~np.isfinite(target) | (target == 0)] = np.float32(0.125)
    glide[:, 0] = np.where(on, GM.bits(target), 0)
    glide[:, 1] = np.where(on, GM.bits(rng.choice([SEMI, 1.001, 2.0, 1.0 + 2.0 ** -23], n).astype(np.float32)), 0)
    glide[:, 2] = np.where(on, GM.bits(rng.choice([1 / SEMI, 0.999, 0.5, 1.0 - 2.0 ** -24], n).astype(np.float32)), 0)
    glide[:, 3] = np.where(on, rng.integers(0, 64, n), 0)
    return inc, glide


@pytest.mark.parametrize("frames", [1, 63, 64, 100, 512, 4096])
def test_model_against_brute_force(frames):
    rng = np.random.default_rng(500 + frames)
    seen = [0, 0]
    for trial in range(6):
        n = 300
        inc, glide = random_state(rng, n)
        first, count = (0, n) if trial == 0 else (int(rng.integers(0, 100)), int(rng.integers(1, 200)))
        for _ in range(3):
            a, b, ga, gb = inc.copy(), inc.copy(), glide.copy(), glide.copy()
            got, want = GM.advance(ga, a, first, count, frames), brute_advance(gb, b, first, count, frames)
            assert got == want and a.tobytes() == b.tobytes() and ga.tobytes() == gb.tobytes(), (frames, trial, got, want)
            out = np.ones(n, bool)
            out[first:first + count] = False
            assert a[out].tobytes() == inc[out].tobytes() and ga[out].tobytes() == glide[out].tobytes(), "a voice outside the range moved"
            w = a.view(np.uint32)
            moved = w != inc.view(np.uint32)
            assert (GM.finite(w[moved]) | (w[moved] == glide[moved, 0])).all(), "a store that is neither finite nor the target"
            seen = [seen[0] + got[0], seen[1] + got[1]]
            inc, glide = a, ga
    assert seen[1] > 20 and (frames >= 4096 or seen[0] > 20), seen


def test_one_long_block_against_the_loop():
    """num_frames = 65536: 1024 steps in one call, the bound of the loop."""
    rng = np.random.default_rng(65536)
    inc, glide = random_state(rng, 40)
    glide[:, 1] = np.where(glide[:, 0] != 0, GM.bits(np.float32(1.0 + 2.0 ** -12)), 0)
    glide[:, 2] = np.where(glide[:, 0] != 0, GM.bits(np.float32(1.0 - 2.0 ** -12)), 0)
    a, b, ga, gb = inc.copy(), inc.copy(), glide.copy(), glide.copy()
    assert GM.advance(ga, a, 0, 40, 65536) == brute_advance(gb, b, 0, 40, 65536)
    assert a.tobytes() == b.tobytes() and ga.tobytes() == gb.tobytes()


# ---------------------------------------------------------------------------------------------- properties on the model alone

K4 = 4
RATIOS = np.array([1.0, 2.0, 3.0, 0.5], np.float32)               # a patch slot whose four voices sit at different ratios


def patch_slot(base=0.01):
    """(owner, glide, inc) of one tagged slot of four voices, as a note-on of the key `base` stores them"""
    owner, glide = OM.new(K4), GM.new(K4)
    owner[0] = 77
    return owner, glide, (np.float32(base) * RATIOS).astype(np.float32)


@pytest.mark.parametrize("semitones", [7, -7, 12, -19])
def test_a_glide_lands_on_the_note_ons_increments(semitones):
    """FROM_SCALE: the slot slides from the previous key into the note-on's pitch and ends on the note-on's bits, every voice."""
    owner, glide, inc = patch_slot()
    struck = inc.copy()
    up, down = GM.per_64(400.0)
    g = GM.Glide(GM.FROM_SCALE, up, down, np.float32(2.0 ** (-semitones / 12.0)))
    assert GM.start_owned(owner, glide, inc, [g], K4, 0xF, [0], [77]) == [4, 0, 0]
    assert (glide[:, 0] == struck.view(np.uint32)).all() and not np.array_equal(inc, struck) and not glide[:, 3].any()
    assert ((np.abs(inc) < np.abs(struck)) == (semitones > 0)).all()
    blocks = 0
    while glide[:, 0].any():
        before = np.abs(inc.copy())
        still, arrived = GM.advance(glide, inc, 0, K4, 64)
        moving = glide[:, 0] != 0
        assert ((np.abs(inc) > before) == (semitones > 0))[moving].all(), "a glide moved away from its target"
        blocks += 1
        assert blocks < 1000
    assert inc.tobytes() == struck.tobytes() and not glide.any() and blocks > 10


def test_the_curve_does_not_depend_on_the_block_size():
    """The same glide cut into blocks of 64, 100, 512, 1 and 63 + 1 frames: the same increments at every multiple of 64 frames."""
    up, down = GM.per_64(100.0)                                       # 5 semitones in some 35 steps of 64 frames
    total = 64 * 100

    def run(cuts):
        owner, glide, inc = patch_slot()
        GM.start_owned(owner, glide, inc, [GM.Glide(GM.FROM_SCALE, up, down, np.float32(2.0 ** (-5 / 12.0)))], K4, 0xF, [0], [77])
        at, k, seen = 0, 0, {0: inc.tobytes()}
        while at < total:
            f = cuts[k % len(cuts)]
            k += 1
            GM.advance(glide, inc, 0, K4, f)
            at += f
            if at % 64 == 0:
                seen[at] = inc.tobytes()
        return seen

    ref = run([64])
    assert len(set(ref.values())) > 20 and ref[total] == patch_slot()[2].tobytes()
    for cuts in ([100], [512], [1], [63, 1], [64, 100, 512, 1, 63, 1]):
        got = run(cuts)
        assert len(got) >= 2 and all(ref[at] == b for at, b in got.items() if at in ref), cuts
        assert set(got) <= set(range(0, total + 64 * 9, 64))


def test_an_overshooting_product_stores_the_target():
    owner, glide, inc = patch_slot()
    struck = inc.copy()
    g = GM.Glide(GM.FROM_SCALE, np.float32(1.5), np.float32(0.5), np.float32(0.4))     # 0.4 * 1.5 * 1.5 * 1.5 > 1: the third product overshoots
    GM.start_owned(owner, glide, inc, [g], K4, 0xF, [0], [77])
    assert GM.advance(glide, inc, 0, K4, 128) == [4, 0] and (np.abs(inc) < np.abs(struck)).all()
    last = (inc * np.float32(1.5)).astype(np.float32)
    assert (np.abs(last) > np.abs(struck)).all()
    assert GM.advance(glide, inc, 0, K4, 64) == [0, 4] and inc.tobytes() == struck.tobytes() and not glide.any()
    # ... and a product that overflows does too
    owner, glide, inc = patch_slot(1e38)
    inc[:] = np.float32(1e38)
    glide[:] = (GM.bits(np.float32(3.3e38)), GM.bits(np.float32(2.0)), GM.bits(np.float32(0.5)), 0)
    assert GM.advance(glide, inc, 0, K4, 128) == [0, 4] and (inc == np.float32(3.3e38)).all()


def test_a_sign_mismatch_or_a_zero_increment_arrives_at_once():
    glide, inc = GM.new(4), np.array([0.0, -0.01, 0.01, np.inf], np.float32)
    glide[:] = (GM.bits(np.float32(0.02)), GM.bits(np.float32(1.01)), GM.bits(np.float32(0.99)), 5)
    glide[2, 0] = GM.bits(np.float32(-0.02))
    assert GM.advance(glide, inc, 0, 4, 1) == [0, 4]                # one frame: no 64-frame step is due, they arrive all the same
    assert inc.tolist() == [np.float32(0.02), np.float32(0.02), np.float32(-0.02), np.float32(0.02)] and not glide.any()
    # a start from such an increment is withheld and leaves the voice as it was
    owner, glide, inc = patch_slot()
    inc[1], inc[2] = 0.0, np.nan
    before = inc.copy()
    g = GM.Glide(GM.FROM_SCALE, 1.01, 0.99, 0.5)
    assert GM.start_owned(owner, glide, inc, [g], K4, 0xF, [0], [77]) == [2, 2, 0]
    assert inc[[1, 2]].tobytes() == before[[1, 2]].tobytes() and not glide[[1, 2]].any() and glide[[0, 3], 0].all()
    assert GM.start_owned(owner, glide, inc, [GM.Glide(GM.TO_SCALE, 1.01, 0.99, 1e30)], K4, 0xF, [0], [77])[1] == 2     # 0 * s = 0, NaN * s
    owner, glide, inc = patch_slot(1e30)
    assert GM.start_owned(owner, glide, inc, [GM.Glide(GM.TO_SCALE, 1.01, 0.99, 1e30)], K4, 0xF, [0], [77]) == [0, 4, 0]  # the target overflows
    assert not glide.any()
    assert GM.start_owned(owner, glide, inc, [g], K4, 0xF, [0], [78]) == [0, 0, 1]                                        # a stolen slot


def test_a_chain_of_to_scale_composes_on_the_targets():
    """Legato C -> E -> G while the first glide is still under way: the targets are those of the intended notes, not of wherever the
    increment happened to be."""
    owner, glide, inc = patch_slot()
    c = inc.copy()
    up, down = GM.per_64(200.0)
    third, minor = np.float32(SEMI ** 4), np.float32(SEMI ** 3)
    assert GM.start_owned(owner, glide, inc, [GM.Glide(GM.TO_SCALE, up, down, third)], K4, 0xF, [0], [77]) == [4, 0, 0]
    e = (c * third).astype(np.float32)
    assert inc.tobytes() == c.tobytes() and (glide[:, 0] == GM.bits(e)).all()
    GM.advance(glide, inc, 0, K4, 512)
    assert glide[:, 0].all() and (inc > c).all() and (inc < e).all()
    glide[:, 3] = 17                                                # a start resets the carry
    assert GM.start_owned(owner, glide, inc, [GM.Glide(GM.TO_SCALE, up, down, minor)], K4, 0xF, [0], [77]) == [4, 0, 0]
    g = (e * minor).astype(np.float32)
    assert (glide[:, 0] == GM.bits(g)).all() and not glide[:, 3].any()
    for _ in range(200):
        GM.advance(glide, inc, 0, K4, 512)
    assert inc.tobytes() == g.tobytes() and not glide.any()


def test_the_tag_launch_clears_the_slot():
    glide = GM.new(16)
    glide[:] = 5
    GM.tag_clear(glide, [4, -1, 16, 6, 8], 5, 4, 4)                  # the first four entries: one slot, a hole, past the bank, no slot
    assert not glide[4:8].any() and glide[:4].all() and glide[8:].all()


# ---------------------------------------------------------------------------------------------- the entry points' host checks

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("glide") / "c_glide_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_glide_host.c"), os.path.join(CSRC, "skred_bank_glide.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"),
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
    assert host_lines[-1] == "OK" and len(host_lines) > 90
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "check", "pack", "perm", "owned", "tags", "advance", "stop", "download", "untouched"}, groups


def test_check_through_ctypes():
    G = device.glide
    good = [G(GM.FROM_SCALE, 1.01, 0.99, 0.5), G(GM.TO_SCALE, 2.0, 0.5, 3.0)]
    assert device.glide_check(good, 8, 0x55) == 0 == GM.check([GM.Glide(1, 1.01, 0.99, 0.5), GM.Glide(2, 2.0, 0.5, 3.0)], 8, 0x55)
    assert device.glide_check(None, 8, 0x55) == BAD == GM.check(None, 8, 0x55)
    assert device.glide_check(good, 12, 0x55) == RANGE and device.glide_check(good, 8, 0) == BAD and device.glide_check(good, 8, 0x155) == BAD
    for entry in ((0, 1.01, 0.99, 0.5), (3, 1.01, 0.99, 0.5), (4, 1.01, 0.99, 0.5), (1, 1.0, 0.99, 0.5), (1, 1.01, 1.0, 0.5), (1, 1.01, 0.0, 0.5),
                  (1, 1.01, -0.1, 0.5), (2, 1.01, 0.99, 0.0), (2, 1.01, 0.99, -1.0), (1, float("nan"), 0.99, 0.5), (1, 1.01, 0.99, float("inf"))):
        assert device.glide_check([good[0], G(*entry)], 8, 0x55) == BAD == GM.check([GM.Glide(*entry)], 8, 0x55), entry
    assert device.glide_check([G(0, 1.0, 1.0, 0.0)], 3, 1) == RANGE == GM.check([GM.Glide(0, 1.0, 1.0, 0.0)], 3, 1)   # K first
    bad = G(1, 1.01, 0.99, 0.5)
    bad.reserved[2] = 1
    assert device.glide_check([bad], 8, 0x55) == BAD and b"reserved" in device.load().skred_amd_last_error()


# ---------------------------------------------------------------------------------------------- a mono line on the oracle

def test_a_mono_line_of_three_keys_on_the_oracle():
    """tests/owner_scenes.py's bank (3.sk tiled over 256 voices, K = 4), one slot, three keys: C, the F above it, the A below that F.
    One bank is struck at each key's increments at once; the other slides into keys two and three (FROM_SCALE), the model's increments
    written into its host view ahead of every block.  While a glide is under way the slot's phases and stems part from the struck line's; it
    ends on exactly the struck line's increments (its phases have parted by then, so the stems stay different: the increments are
    what lands).  Nothing outside the slot hears of it."""
    bank, tables, g = OS.bank()
    K, N, F = OS.K, OS.N, OS.F
    slot = int(OS.others()[5])
    vs = np.arange(slot, slot + K)
    struck, glided = bank.copy(), bank.copy()
    gs, gg = g.copy(), g.copy()
    owner, glide = OM.new(N), GM.new(N)
    OM.tag_slots(owner, [slot], [0x03000030], None, K)
    base = bank["voice_phase_inc"][vs].copy()
    assert (np.abs(base) > 1e-6).all() and len(set(base.tolist())) > 1, "the patch's voices sit at different ratios"
    up, down = GM.per_64(700.0)                                       # about a semitone per 64-frame block: a handful of blocks per glide
    keys = [(0, None), (5, np.float32(SEMI ** -5)), (-3, np.float32(SEMI ** 8))]
    glide_blocks = []
    for semis, scale in keys:
        note = (base * np.float32(SEMI ** semis)).astype(np.float32)
        now = int(gs.synth_sample_count)
        assert now == int(gg.synth_sample_count)
        for b in (struck, glided):
            b["voice_phase_inc"][vs] = note
            SM.stamp(b, vs, SM.STAMP_TRIGGER, now)
        GM.tag_clear(glide, [slot], 1, None, K)                       # the key's tag launch
        if scale is not None:
            res = GM.start_owned(owner, glide, glided["voice_phase_inc"], [GM.Glide(GM.FROM_SCALE, up, down, scale)], K, OS.VMASK, [slot], [0x03000030])
            assert res == [K, 0, 0] and (glide[vs, 0] == GM.bits(note)).all()
        under_way = heard = 0
        for k in range(40):
            still, arrived = GM.advance(glide, glided["voice_phase_inc"], 0, N, F)
            assert still + arrived <= K
            a = cpuref.render(struck, gs, tables, F, 0, want_stems=True)["stems"]
            b = cpuref.render(glided, gg, tables, F, 0, want_stems=True)["stems"]
            rest = np.setdiff1d(np.arange(N), vs)
            assert a[:, rest].tobytes() == b[:, rest].tobytes(), "a voice outside the slot changed"
            if still:
                under_way += 1
                heard += a[:, vs].tobytes() != b[:, vs].tobytes()
                assert not np.array_equal(glided["voice_phase_inc"][vs], note)
                assert (glided["voice_phase"][vs] != struck["voice_phase"][vs]).any(), f"key {semis}, block {k}: the phases did not part"
            if scale is None:
                assert a.tobytes() == b.tobytes(), "no glide was started: the two lines are one"
        glide_blocks.append(under_way)
        # (the patch plays square waves whose period is some 400 frames: a single 64-frame block may hold no edge)
        assert scale is None or heard >= 1, f"key {semis}: a glide of {under_way} blocks that cannot be heard"
        assert glided["voice_phase_inc"][vs].tobytes() == struck["voice_phase_inc"][vs].tobytes() == note.tobytes(), f"key {semis} did not land"
        assert not glide.any()
    assert glide_blocks[0] == 0 and glide_blocks[1] >= 3 and glide_blocks[2] >= 3, glide_blocks
