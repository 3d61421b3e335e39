"""Portamento on the fixed-point bank without a GPU: the symbols against the header, the model (tests/fx_glide_model.py, numpy on
uint64) against a plain Python-integer loop over every voice and every 64-frame step, the properties the integer definition promises
-- an exact landing from above and from below, increments that do not depend on how the host cuts its blocks, progress at every
increment where the Q16 route stalls, the edges of the 32-bit range --, every refusal and the packing (through
tests/c_fx_glide_host.c, a program of its own on a bank that is nothing but its size), the clear rule's two scenes, which must FAIL
on a model without the clear behind the tag launch, and a mono line of three keys on oracle.cpuref.fx_render alone.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import fx_glide_model as GM
import fx_owner_model as om
from oracle import cpuref
from skred_amd import device, fxbank as fxb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
TOP = 0xFFFFFFFF
SYMBOLS = ("skred_fxbank_glide_owned", "skred_fxbank_glide_tags", "skred_fxbank_glide_advance", "skred_fxbank_glide_stop",
           "skred_fxbank_download_glide")
CUTS = ([64] * 8, [512], [37, 100, 27, 348])                    # 512 frames, three ways
G = GM.Glide


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd_fxpt.h")).read()
    L = device.load()
    for s in SYMBOLS + ("skred_fx_glide_check",):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in fxb.FX_ABI_SYMBOLS + fxb.FX_HOST_ABI_SYMBOLS
    for name, bit in (("FROM_SCALE", 0), ("TO_SCALE", 1), ("TO_INC", 2)):
        assert re.search(r"#define SKRED_FX_GLIDE_%s\s+\(1u << %d\)" % (name, bit), text) and getattr(fxb, "FX_GLIDE_" + name) == 1 << bit
    import ctypes as C
    assert C.sizeof(fxb.FxGlideC) == 32 and fxb.FxGlideC.target_inc.offset == 16
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "the fixed-point twin, the drop-in mode" not in readme and "**Portamento on the fixed-point bank**" in readme


# ---------------------------------------------------------------------------------------------- the model against plain integers

def brute_advance(glide, inc, first, count, frames):
    """The definition, one voice and one step at a time, on Python integers."""
    res = [0, 0]
    for v in range(first, first + count):
        target, up, down, carry = (int(w) for w in glide[v])
        if not target:
            continue
        cur = int(inc[v])
        c = carry + frames
        there = cur == 0 or cur == target
        for _ in range(c >> 6):
            if there:
                break
            if cur < target:
                cur += max(1, (cur * up) >> 32)
                there = cur >= target
            else:
                d = max(1, (cur * down) >> 32)
                assert d <= cur
                cur -= d
                there = cur <= target
        if there:
            inc[v], glide[v] = target, 0
            res[1] += 1
        else:
            assert 0 < cur <= TOP
            inc[v], glide[v, GM.CARRY] = cur, c & 63
            res[0] += 1
    return res


def random_state(rng, n):
    pick = [1, 2, 3, 1000, 65535, 65536, 70000, 1 << 24, 0x7FFFFFFF, 0x80000000, TOP - 1, TOP]
    inc = np.where(rng.integers(0, 3, n) == 0, rng.choice(pick, n), rng.integers(1, 1 << 32, n)).astype(np.uint32)
    inc[rng.integers(0, n, 4)] = 0                             # voices without pitch
    glide = GM.new(n)
    on = rng.integers(0, 3, n) != 0
    near = (inc.astype(np.int64) + rng.integers(-3000, 3000, n)).clip(1, TOP)
    glide[:, GM.TARGET] = np.where(on, np.where(rng.integers(0, 2, n) == 0, near, rng.choice(pick, n)), 0)
    glide[:, GM.UP] = np.where(on, rng.choice([1, 1 << 10, 1 << 20, 1 << 26, 1 << 31, TOP], n), 0)
    glide[:, GM.DOWN] = np.where(on, rng.choice([1, 1 << 10, 1 << 20, 1 << 26, 1 << 31, TOP], n), 0)
    glide[:, GM.CARRY] = np.where(on, rng.integers(0, 64, n), 0)
    same = on & (rng.integers(0, 20, n) == 0)
    inc[same] = glide[same, GM.TARGET]                         # inc == target
    return inc, glide


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_plain_integers(seed):
    rng = np.random.default_rng(9100 + seed)
    n = 600
    seen = {"still": 0, "arrived": 0}
    for trial in range(10):
        inc, glide = random_state(rng, n)
        a, b = (inc.copy(), glide.copy()), (inc.copy(), glide.copy())
        first = int(rng.integers(0, 100))
        count = int(rng.integers(1, n - first + 1))
        for frames in (1, 63, 64, 65, int(rng.integers(1, 3000)), 65536 if trial == 0 else 700):
            got, want = GM.advance(a[1], a[0], first, count, frames), brute_advance(b[1], b[0], first, count, frames)
            assert got == want and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (trial, frames)
            seen["still"] += got[0]
            seen["arrived"] += got[1]
        outside = np.r_[0:first, first + count:n]
        assert np.array_equal(a[0][outside], inc[outside]) and np.array_equal(a[1][outside], glide[outside])
        GM.stop(a[1], a[0], first, count, snap=trial % 2 == 0)
        on = b[1][first:first + count, GM.TARGET] != 0
        want = np.where(on & (trial % 2 == 0), b[1][first:first + count, GM.TARGET], b[0][first:first + count])
        assert not a[1][first:first + count].any() and np.array_equal(a[0][first:first + count], want)
    assert all(v > 100 for v in seen.values()), seen


# ---------------------------------------------------------------------------------------------- what the definition promises

def run_to_arrival(inc0, target, up, down, limit=200000):
    inc, glide = np.array([inc0], np.uint32), GM.new(1)
    glide[0] = (target, up, down, 0)
    trail = [inc0]
    for k in range(limit):
        if GM.advance(glide, inc, 0, 1, 64) == [0, 1]:
            return int(inc[0]), k + 1, trail
        trail.append(int(inc[0]))
    raise AssertionError(f"{inc0} -> {target} did not arrive in {limit} steps")


@pytest.mark.parametrize("lo, hi", [(1000, 1001), (3000017, 4000037), (44739243, 89478485), (1, TOP), (0x7FFFFFFF, 0x80000001)])
def test_landing_is_bit_for_bit_from_above_and_from_below(lo, hi):
    up, down = GM.per_64(900.0)
    for a, b in ((lo, hi), (hi, lo)):
        end, steps, trail = run_to_arrival(a, b, up, down)
        assert end == b and steps >= 1
        assert all((x < y) == (a < b) for x, y in zip(trail, trail[1:])), "the way there is monotone"
        assert all(min(a, b) <= x <= max(a, b) for x in trail), "and never leaves the interval"


def test_block_cutting_does_not_change_the_increments():
    """512 frames as 8 x 64, as 1 x 512 and as 37 + 100 + 27 + 348: the same increments and words."""
    rng = np.random.default_rng(5)
    n = 600
    inc, glide = random_state(rng, n)
    glide[:, GM.CARRY] = 0
    glide[::3, GM.UP], glide[::3, GM.DOWN] = 1 << 22, 1 << 22  # slow enough that many are still on the way after 512 frames
    ends = []
    for cut in CUTS:
        a, g = inc.copy(), glide.copy()
        res = [GM.advance(g, a, 0, n, f) for f in cut]
        ends.append((a, g, sum(r[1] for r in res), res[-1][0]))
    for a, g, arrived, still in ends[1:]:
        assert np.array_equal(a, ends[0][0]) and np.array_equal(g, ends[0][1]) and (arrived, still) == ends[0][2:]
    assert ends[0][3] > 50 and ends[0][2] > 50 and not ends[0][1][:, GM.CARRY].any()
    # ... and at a point that is no multiple of 64 the carries differ by design but the sums of frames agree
    a, g = inc.copy(), glide.copy()
    GM.advance(g, a, 0, n, 37)
    assert (g[g[:, GM.TARGET] != 0, GM.CARRY] == 37).all() and np.array_equal(a[g[:, GM.TARGET] != 0], inc[g[:, GM.TARGET] != 0])


def test_progress_at_every_small_increment_where_the_q16_route_stalls():
    """inc = 1 .. 70000 with the smallest rates: every step moves by at least one.  The parent's route -- one INC_SCALE of 65542 / 65536
    (a sixth of a semitone per thousand... the finest Q16 step worth the name) per block -- stands still below 65536 / 6."""
    inc = np.arange(1, 70001, dtype=np.uint32)
    for target, field in ((TOP, GM.UP), (1, GM.DOWN)):
        a, g = inc.copy(), GM.new(len(inc))
        g[:, GM.TARGET], g[:, GM.UP], g[:, GM.DOWN] = target, 1, 1
        g[inc == target] = 0
        for k in range(1, 4):
            GM.advance(g, a, 0, len(inc), 64)
            moved = a.astype(np.int64) - inc.astype(np.int64)
            on = inc != target
            want = k if target == TOP else -np.minimum(k, inc.astype(np.int64) - 1)
            assert (moved[on] == (want if target == TOP else want[on])).all()
    stalled = [i for i in range(1, 70001) if GM.q16_route(i, 65542) == i]
    assert stalled == list(range(1, 10923)), "the Q16 route stalls exactly below 65536 / 6"
    assert GM.q16_route(10923, 65542) == 10924 and GM.q16_route(5000, 65530) == 4999   # (down it creeps: the floor of a product)


def test_edges_of_the_range():
    one = lambda inc, words: (np.array([inc], np.uint32), np.array([words], np.uint32))
    # the top of the range glides up to the top: inc == target arrives at once
    a, g = one(TOP, (TOP, TOP, TOP, 5))
    assert GM.advance(g, a, 0, 1, 1) == [0, 1] and a[0] == TOP and not g.any()
    # overshoot past 2^32 in the 64-bit sum: lands on the target, does not wrap
    a, g = one(0xF0000000, (TOP, TOP, 1, 0))
    assert GM.advance(g, a, 0, 1, 64) == [0, 1] and a[0] == TOP and not g.any()
    a, g = one(0xF0000000, (0xF8000000, 1 << 31, 1, 0))
    assert GM.advance(g, a, 0, 1, 64) == [0, 1] and a[0] == 0xF8000000
    # the fastest way down at the bottom: the subtrahend is max(1, 0) = 1 and never exceeds inc
    a, g = one(2, (1, 1, TOP, 0))
    assert GM.advance(g, a, 0, 1, 64) == [0, 1] and a[0] == 1
    a, g = one(3, (1, 1, TOP, 0))
    assert GM.advance(g, a, 0, 1, 64) == [0, 1] and a[0] == 1                    # 3 - max(1, 2) = 1
    a, g = one(1, (1, 1, TOP, 0))
    assert GM.advance(g, a, 0, 1, 1) == [0, 1] and a[0] == 1                     # inc == target
    a, g = one(TOP, (1, 1, TOP, 0))
    assert GM.advance(g, a, 0, 1, 64) == [0, 1] and a[0] == 1                    # TOP - (TOP - 1) = 1 <= 1
    # a voice without pitch arrives at once, whatever the frames
    a, g = one(0, (5000, 9, 9, 63))
    assert GM.advance(g, a, 0, 1, 1) == [0, 1] and a[0] == 5000 and not g.any()
    # fewer than 64 frames: no step, the carry alone moves
    a, g = one(1000, (2000, 1 << 30, 1 << 30, 10))
    assert GM.advance(g, a, 0, 1, 53) == [1, 0] and a[0] == 1000 and g[0].tolist() == [2000, 1 << 30, 1 << 30, 63]
    assert GM.advance(g, a, 0, 1, 1) == [1, 0] and a[0] == 1250 and g[0, GM.CARRY] == 0
    # the longest advance: 65536 frames are 1024 steps, and a carry of 63 does not make a 1025th
    a, g = one(1000, (TOP, 1, 1, 63))
    assert GM.advance(g, a, 0, 1, 65536) == [1, 0] and a[0] == 2024 and g[0, GM.CARRY] == 63
    assert GM.advance(g, a, 0, 1, 1) == [1, 0] and a[0] == 2025 and g[0, GM.CARRY] == 0


def one_voice(inc, tag=7):
    owner, glide = om.new(4), GM.new(4)
    owner[2] = tag
    return owner, glide, np.array([1, 1, inc, 1], np.uint32)


def test_to_scale_chains_compose_on_the_old_target():
    owner, glide, inc = one_voice(1 << 24)
    up = G(GM.TO_SCALE, 1 << 20, 1 << 20, GM.scale_q16(7))
    assert GM.start_owned(owner, glide, inc, [up], [2], [7]) == [1, 0, 0]
    t1 = ((1 << 24) * up.scale) >> 16
    assert glide[2].tolist() == [t1, 1 << 20, 1 << 20, 0] and inc[2] == 1 << 24
    GM.advance(glide, inc, 0, 4, 200)
    assert glide[2, GM.CARRY] == 8 and (1 << 24) < inc[2] < t1
    assert GM.start_owned(owner, glide, inc, [up], [2], [7]) == [1, 0, 0]
    assert glide[2, GM.TARGET] == (t1 * up.scale) >> 16, "the second bend starts from the first one's target, not from where the glide is"
    assert glide[2, GM.CARRY] == 0, "a start that stores sets carry = 0"
    # FROM_SCALE replaces a glide: the target is the increment as it stands
    at = int(inc[2])
    assert GM.start_owned(owner, glide, inc, [G(GM.FROM_SCALE, 3, 4, 32768)], [2], [7]) == [1, 0, 0]
    assert glide[2].tolist() == [at, 3, 4, 0] and inc[2] == at >> 1


def test_to_inc_lands_on_the_struck_notes_bits_and_to_scale_need_not():
    key_a, key_b = 39370534, 44189901                           # A3 and B3 at 48 kHz: round(f / 48000 * 2^32), two semitones apart
    up, down = GM.per_64(600.0)
    owner, glide, inc = one_voice(key_a)
    assert GM.start_owned(owner, glide, inc, [G(GM.TO_INC, up, down, target_inc=key_b)], [2], [7]) == [1, 0, 0]
    for _ in range(1000):
        if GM.advance(glide, inc, 0, 4, 64) == [0, 1]:
            break
    assert inc[2] == key_b, "legato lands on the struck key's bits"
    owner, glide, inc = one_voice(key_a)
    GM.start_owned(owner, glide, inc, [G(GM.TO_SCALE, up, down, GM.scale_q16(2))], [2], [7])
    for _ in range(1000):
        if GM.advance(glide, inc, 0, 4, 64) == [0, 1]:
            break
    assert inc[2] != key_b and abs(int(inc[2]) - key_b) < key_b >> 14, "Q16 cannot promise the landing: close, not equal"
    # FROM_SCALE lands on the bits the voice was struck with
    owner, glide, inc = one_voice(key_b)
    GM.start_owned(owner, glide, inc, [G(GM.FROM_SCALE, up, down, GM.scale_q16(-2))], [2], [7])
    assert inc[2] != key_b
    for _ in range(1000):
        if GM.advance(glide, inc, 0, 4, 64) == [0, 1]:
            break
    assert inc[2] == key_b


def test_every_withheld_start_leaves_all_words_as_they_were():
    cases = [(0, G(GM.FROM_SCALE, 1, 1, 65536)),                # a voice without pitch
             (0, G(GM.TO_INC, 1, 1, target_inc=5)),
             (0, G(GM.TO_SCALE, 1, 1, 65536)),
             (1, G(GM.FROM_SCALE, 1, 1, 65535)),                # the new inc would be 0
             (70000, G(GM.FROM_SCALE, 1, 1, TOP)),              # the new inc would be above 32 bits
             (1, G(GM.TO_SCALE, 1, 1, 65535)),                  # the target would be 0
             (70000, G(GM.TO_SCALE, 1, 1, TOP))]                # the target would be above 32 bits
    for inc0, g in cases:
        for words in ((0, 0, 0, 0), (12345, 6, 7, 8)):
            owner, glide, inc = one_voice(inc0)
            glide[2] = words
            if g.set == GM.TO_SCALE and words[0] and inc0:
                continue                                        # (a gliding voice scales its old target: another product)
            assert GM.start_owned(owner, glide, inc, [g], [2], [7]) == [0, 1, 0], (inc0, g.set)
            assert inc[2] == inc0 and glide[2].tolist() == list(words)
    # the old target's product is the one that counts on a gliding voice
    owner, glide, inc = one_voice(5)
    glide[2] = (0x80000000, 1, 1, 9)
    assert GM.start_owned(owner, glide, inc, [G(GM.TO_SCALE, 1, 1, 1 << 17)], [2], [7]) == [0, 1, 0] and glide[2, GM.CARRY] == 9
    # the edge that still starts: exactly 0xFFFFFFFF, exactly 1
    owner, glide, inc = one_voice(0xFFFF)
    assert GM.start_owned(owner, glide, inc, [G(GM.FROM_SCALE, 1, 1, 0x10001 << 0)], [2], [7]) == [1, 0, 0] and inc[2] == 0x10000 - 1 + 0  # 0xFFFF * 0x10001 >> 16
    owner, glide, inc = one_voice(0x10000)
    assert GM.start_owned(owner, glide, inc, [G(GM.TO_SCALE, 1, 1, 1)], [2], [7]) == [1, 0, 0] and glide[2, GM.TARGET] == 1
    # the guard and the list rule: a wrong tag, a hole, an entry beyond the bank, a count below n
    owner, glide, inc = one_voice(1000)
    gs = [G(GM.TO_INC, 1, 1, target_inc=9)] * 4
    assert GM.start_owned(owner, glide, inc, gs, [2, -1, 4, 2], [8, 7, 7, 7], count=3) == [0, 0, 1] and not glide.any()
    assert GM.start_owned(owner, glide, inc, gs, [1, -1, 4, 2], [8, 7, 7, 7]) == [1, 0, 1] and glide[2, GM.TARGET] == 9


def test_check_through_ctypes():
    good = [G(GM.FROM_SCALE, 1, TOP, 1), G(GM.TO_SCALE, TOP, 1, TOP), G(GM.TO_INC, 5, 6, target_inc=1)]
    assert fxb.fx_glide_check([g.c() for g in good]) == 0 == GM.check(good)
    assert fxb.fx_glide_check(None) == BAD == GM.check(None)
    assert fxb.fx_glide_check([g.c() for g in good], n=-1) == BAD == GM.check(good, -1)
    for entry in ((0, 1, 1, 1, 1), (3, 1, 1, 1, 1), (5, 1, 1, 1, 1), (8, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1),
                  (2, 1, 1, 0, 1), (4, 1, 1, 1, 0)):
        assert fxb.fx_glide_check([good[0].c(), G(*entry).c()]) == BAD == GM.check([good[0], G(*entry)]), entry
        assert fxb.fx_glide_check([good[0].c(), G(*entry).c()], n=1) == 0
    assert fxb.fx_glide_check([G(4, 1, 1, 0, 1).c(), G(1, 1, 1, 1, 0).c()]) == 0      # values the form does not use
    bad = G(1, 1, 1, 1, reserved=(0, 0, 1))
    assert fxb.fx_glide_check([bad.c()]) == BAD == GM.check([bad]) and b"reserved" in device.load().skred_amd_last_error()


# ---------------------------------------------------------------------------------------------- the host program

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fxglide") / "c_fx_glide_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_fx_glide_host.c"), os.path.join(CSRC, "skred_fx_glide.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"),
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
    assert host_lines[-1] == "OK" and len(host_lines) > 70
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "check", "pack", "owned", "tags", "advance", "stop", "download", "untouched"}, groups


# ---------------------------------------------------------------------------------------------- the clear rule

N_SCENE = 600


def scene_stage(clear_rule=True):
    bank, pool, c0 = fxb.bank_fx(N_SCENE)
    return GM.FxStage(bank, pool, c0, clear_rule)


@pytest.mark.parametrize("name", GM.SCENES)
def test_scene_on_the_oracle(name):
    st = scene_stage()
    GM.run_scene(name, st)
    assert not st.glide.any()


@pytest.mark.parametrize("name", GM.SCENES)
def test_the_scenes_bite_without_the_clear_rule(name):
    st = scene_stage(clear_rule=False)
    with pytest.raises(AssertionError):
        GM.run_scene(name, st)


def test_tag_list_clears_only_what_it_tags():
    owner, glide = om.new(16), GM.new(16)
    glide[:] = 3
    assert GM.tag_list(owner, glide, [3, -1, 16, 5, 7], [9, 9, 9, 8, 7], count=4) == [2, 2]
    assert [int(g.any()) for g in glide] == [1, 1, 1, 0, 1, 0] + [1] * 10 and owner[7] == 0
    glide[:] = 3
    GM.tag_list(owner, glide, [3, 5], [9, 8], clear_rule=False)
    assert (glide == 3).all()
    GM.tag_list(owner, None, [3, 5], [9, 8])                     # a bank without the array


# ---------------------------------------------------------------------------------------------- a mono line on the oracle

def test_a_mono_line_of_three_keys_on_the_oracle():
    """One voice of the bank_fx recipe plays C, the F above it and the A below that F, legato.  The struck line gets each key's increment
    at once; the glided line slides there (TO_INC, so it lands on the key's bits), the model's advance ahead of every block.  While a
    glide is under way the voice's stems part from the struck line's.  The phase a voice has run through is part of its state, so
    the struck line takes over the glided line's running state -- phase, filter memory, smoother -- in the block of arrival: from
    then on the two lines hold the same increment bits and their stems are bit-equal until the next key.  Nothing outside the voice
    hears of it."""
    bank, pool, c0 = fxb.bank_fx(N_SCENE)
    v, F = 301, 64
    st = GM.FxStage(bank, pool, c0)
    struck, cnt = bank.copy(), c0
    st.tag([v], [0x03000030])
    base = int(bank["phase_inc"][v])
    keys = [base, (base * GM.scale_q16(5)) >> 16, (base * GM.scale_q16(2)) >> 16]
    up, down = GM.per_64(400.0)                                      # about half a semitone per 64-frame block
    rest = np.setdiff1d(np.arange(N_SCENE), [v])
    glide_blocks = []
    for k, key in enumerate(keys):
        struck["phase_inc"][v] = key
        if k == 0:
            st.truth["phase_inc"][v] = key
        else:
            assert st.start([G(GM.TO_INC, up, down, target_inc=key)], [0x03000030]) == [1, 0, 0]
        under_way = heard = 0
        landed = k == 0
        for blk in range(30):
            still, arrived = st.advance(F)
            assert still + arrived <= 1
            if arrived:
                for name in fxb.FX_RW:
                    struck[name][v] = st.truth[name][v]
                landed = True
            a, sa, cnt = cpuref.fx_render(struck, pool, cnt, F, 1, want_stems=True)
            b, sb = st.block(F)
            assert cnt == st.now()
            assert sa[:, rest].tobytes() == sb[:, rest].tobytes(), "a voice outside the line changed"
            if still:
                under_way += 1
                heard += sa[:, v].tobytes() != sb[:, v].tobytes()
                assert st.inc[v] != key
            if landed:
                assert st.inc[v] == key == struck["phase_inc"][v] and not st.glide.any()
                assert sa.tobytes() == sb.tobytes() and a.tobytes() == b.tobytes(), f"key {k}, block {blk}: the lines differ after arrival"
        assert landed and (k == 0 or heard >= 1), f"key {k}: {under_way} blocks of glide, {heard} heard"
        glide_blocks.append(under_way)
    assert glide_blocks[0] == 0 and glide_blocks[1] >= 3 and glide_blocks[2] >= 3, glide_blocks
