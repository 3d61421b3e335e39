"""The pitch wheel of the fixed-point bank without a GPU: the symbols against the header, the model (tests/fx_bend_model.py, numpy on
uint64) against a plain Python-integer loop voice by voice, the properties the integer definition promises -- any sweep followed by
the centre gives the key's bits where the INC_SCALE route does not, the same message twice gives the same bits, a withheld bend leaves
every word alone, a glide under a bend lands on (target * ratio) >> 24 and the centre then gives the target's bits, whatever the block
cutting --, every refusal and the packing (through tests/c_fx_bend_host.c, a program of its own on a bank that is nothing but its
size), the clear rule's two scenes, which must FAIL on a model without the clear behind the tag launch, and a mono line under a held
wheel on oracle.cpuref.fx_render alone.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import fx_bend_model as BM
import fx_glide_model as GM
import fx_owner_model as om
from oracle import cpuref
from skred_amd import device, fxbank as fxb
from test_fx_glide_cpu import CUTS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")
BAD, RANGE = -2, -4
TOP, ONE = 0xFFFFFFFF, 1 << 24
KEY, RATIO = BM.KEY, BM.RATIO
SYMBOLS = ("skred_fxbank_bend_match", "skred_fxbank_bend_owned_each", "skred_fxbank_bend_tags_each", "skred_fxbank_bend_clear",
           "skred_fxbank_download_bend")
INCS = [0, 1, 2, 65535, 65536, 1 << 24, 0x7FFFFFFF, 0x80000000, TOP - 1, TOP]
RATIOS = [1, ONE - 1, ONE, ONE + 1, 1 << 31, TOP]
G = GM.Glide


def test_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "skred_amd_fxpt.h")).read()
    L = device.load()
    for s in SYMBOLS + ("skred_fx_bend_check",):
        assert re.search(r"\b%s\(" % s, text) and hasattr(L, s), s
        assert s in fxb.FX_ABI_SYMBOLS + fxb.FX_HOST_ABI_SYMBOLS
    assert "skred_fx_bend_check" in fxb.FX_HOST_ABI_SYMBOLS and all(s in fxb.FX_ABI_SYMBOLS for s in SYMBOLS)
    assert re.search(r"#define SKRED_FX_BEND_ONE\s+\(1u << 24\)", text) and fxb.FX_BEND_ONE == ONE == BM.ONE
    assert fxb.bend_ratio_q24(0) == ONE and fxb.bend_ratio_q24(12) == 2 * ONE and fxb.bend_ratio_q24(-12) == ONE // 2
    assert "section \"pitch wheel\"" in text and "Q16 cannot tell adjacent positions" in text
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "**Pitch wheel on the fixed-point bank**" in readme
    float_header = open(os.path.join(ROOT, "include", "skred_amd.h")).read()
    assert "fixed-point twin, the drop-in mode, deferred items and pattern steps are follow-ups" not in float_header


# ---------------------------------------------------------------------------------------------- the model against plain integers

def brute_apply(bend, inc, v, r):
    """THE RULE on one voice, on Python integers.  Returns 1 stored or restored, 2 withheld, 0 neither."""
    key, inc_v = int(bend[v, KEY]), int(inc[v])
    if r == ONE:
        if key:
            inc[v] = key
        bend[v] = 0
        return 1 if key else 0
    k = key or inc_v
    p = (k * r) >> 24
    if k == 0 or p == 0 or p > TOP:
        return 2
    inc[v], bend[v] = p, (k, r)
    return 1


def random_state(rng, n):
    """increments as test_fx_glide_cpu.random_state draws them, plus 0 and 1 << 24 from the list of the edges; a third of the voices bent"""
    inc = np.where(rng.integers(0, 3, n) == 0, rng.choice(INCS, n), rng.integers(1, 1 << 32, n)).astype(np.uint32)
    bend = BM.new(n)
    bent = rng.integers(0, 3, n) == 0
    bend[:, KEY] = np.where(bent, np.where(rng.integers(0, 2, n) == 0, rng.choice(INCS[1:], n), rng.integers(1, 1 << 32, n)), 0)
    bend[:, RATIO] = np.where(bent, rng.choice(RATIOS[:2] + RATIOS[3:], n), 0)
    return inc, bend


def random_ratios(rng, n):
    return np.where(rng.integers(0, 2, n) == 0, rng.choice(RATIOS, n), rng.integers(1, 1 << 32, n)).astype(np.uint32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_plain_integers(seed):
    rng = np.random.default_rng(9300 + seed)
    n = 600
    seen = [0, 0, 0]
    for trial in range(12):
        inc, bend = random_state(rng, n)
        a, b = (inc.copy(), bend.copy()), (inc.copy(), bend.copy())
        for msg in range(6):
            vs = rng.permutation(n)[:int(rng.integers(1, n + 1))]
            one = msg % 2 == 0
            r = np.full(len(vs), int(rng.choice(RATIOS)) if msg < 4 else int(rng.integers(1, 1 << 32)), np.uint32) if one else random_ratios(rng, len(vs))
            got = BM.apply(a[1], a[0], vs, r[0] if one else r)
            did = [brute_apply(b[1], b[0], int(v), int(x)) for v, x in zip(vs, r)]
            want = [did.count(1), did.count(2)]
            assert got == want and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (trial, msg)
            seen = [seen[0] + got[0], seen[1] + got[1], seen[2] + did.count(0)]
        first = int(rng.integers(0, 100))
        count = int(rng.integers(1, n - first + 1))
        snap = trial % 2 == 0
        on = b[1][first:first + count, KEY] != 0
        want = np.where(on & snap, b[1][first:first + count, KEY], b[0][first:first + count])
        BM.clear(a[1], a[0], first, count, snap)
        assert not a[1][first:first + count].any() and np.array_equal(a[0][first:first + count], want)
        outside = np.r_[0:first, first + count:n]
        assert np.array_equal(a[0][outside], b[0][outside]) and np.array_equal(a[1][outside], b[1][outside])
    assert all(s > 100 for s in seen), seen


def test_every_edge_increment_against_every_edge_ratio():
    for k in INCS:
        for r in RATIOS:
            inc, bend = np.array([k], np.uint32), BM.new(1)
            got = BM.apply(bend, inc, [0], r)
            p = (k * r) >> 24
            if r == ONE:
                assert got == [0, 0] and inc[0] == k and not bend.any()
            elif k == 0 or p == 0 or p > TOP:
                assert got == [0, 1] and inc[0] == k and not bend.any(), (k, r)
            else:
                assert got == [1, 0] and inc[0] == p and bend[0].tolist() == [k, r], (k, r)


# ---------------------------------------------------------------------------------------------- what the definition promises

A3 = 39370534                                                   # round(220 / 48000 * 2^32)


def wheel_sweep(n, seed):
    """n random positions of a 14-bit wheel over +-2 semitones, as Q24 ratios"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, 1 << 14, n)
    return [BM.ratio_of((int(p) - 8192) / 8192.0 * 2.0) for p in pos]


@pytest.mark.parametrize("key", [1, 3, 70000, A3, 0x7FFFFFFF, 0x80000001])
def test_any_sweep_then_the_centre_gives_the_keys_bits(key):
    for seed, n in ((1, 1), (2, 17), (3, 1000)):
        inc, bend = np.array([5, key, 5], np.uint32), BM.new(3)
        sweep = wheel_sweep(n, seed)
        if key >= 0x7FFFFFFF:
            sweep += [TOP, 1 << 31]                             # withheld above 32 bits: the words stand
        for r in sweep:
            BM.apply(bend, inc, [1], r)
            if bend[1, KEY]:
                assert bend[1, KEY] == key and inc[1] == (key * int(bend[1, RATIO])) >> 24
        bent = 1 if bend[1, KEY] else 0
        assert BM.apply(bend, inc, [1], ONE) == [bent, 0]
        assert inc.tolist() == [5, key, 5] and not bend.any()


def test_the_inc_scale_route_does_not_come_back():
    """A3 at 48 kHz (39370534) under the 1000-position sweep of seed 3, driven through the Q16 ratios of ratios the host would send,
    wheel back at the centre: the increment ends BELOW the key's, every message having truncated.  The same sweep through THE RULE
    ends on the key's bits (the test above)."""
    sweep = wheel_sweep(1000, 3)
    end = BM.q16_sweep(A3, sweep)
    print(f"INC_SCALE route after 1000 messages and the centre: {end} against the key's {A3}: {A3 - end} low, "
          f"{1200 * np.log2(A3 / end):.3f} cent flat")
    assert end < A3 and A3 - end > 100
    # ... and Q16 cannot separate adjacent wheel positions that Q24 does
    pairs = [(BM.ratio_of((p - 8192) / 8192.0 * 2.0), BM.ratio_of((p + 1 - 8192) / 8192.0 * 2.0)) for p in range(8000, 8400)]
    assert all(a != b for a, b in pairs) and sum(BM.q16_of(a) == BM.q16_of(b) for a, b in pairs) > 20
    # ... and stalls on small increments, where the bend moves the voice
    assert GM.q16_route(5000, 65542) == 5000 and (1 << 30) * (65542 << 8) >> 24 != 1 << 30


def test_the_same_message_twice_gives_the_same_bits():
    rng = np.random.default_rng(11)
    inc, bend = random_state(rng, 400)
    r = random_ratios(rng, 400)
    v = np.arange(400)
    restored = int(((r == ONE) & (bend[:, KEY] != 0)).sum())
    first = BM.apply(bend, inc, v, r)
    a, b = inc.copy(), bend.copy()
    second = BM.apply(bend, inc, v, r)
    assert np.array_equal(a, inc) and np.array_equal(b, bend)
    assert first[1] == second[1] > 0, "a withheld bend is withheld again"
    assert restored > 0 and second[0] == first[0] - restored, "the centre restores once; the second centre finds an unbent voice"


def test_every_withheld_bend_leaves_all_words_as_they_were():
    cases = [(0, (0, 0), 5 * ONE),                              # a voice without pitch: key 0
             (1, (0, 0), ONE - 1),                              # the product would be 0
             (255, (0, 0), 1 << 16),                            # (255 << 16) >> 24 == 0
             ((1 << 24) + 1, (0, 0), TOP),                      # one above the last product that fits
             (0x80000000, (0, 0), 1 << 25),                     # exactly 2^32
             (77, (0x80000000, 3 * ONE // 2), 1 << 25),         # a bent voice: the KEY's product counts, not the increment's
             (77, (1, ONE + 5), ONE - 1)]
    for inc0, words, r in cases:
        inc, bend = np.array([9, inc0, 9], np.uint32), BM.new(3)
        bend[1] = words
        assert BM.apply(bend, inc, [1], r) == [0, 1], (inc0, words, r)
        assert inc.tolist() == [9, inc0, 9] and bend[1].tolist() == list(words) and not bend[[0, 2]].any()
    # the edges that still store: exactly 0xFFFFFFFF, exactly 1
    inc, bend = np.array([0xFFFFFFFF], np.uint32), BM.new(1)
    assert BM.apply(bend, inc, [0], ONE + 0) == [0, 0]
    inc, bend = np.array([1 << 24], np.uint32), BM.new(1)
    assert BM.apply(bend, inc, [0], TOP) == [1, 0] and inc[0] == TOP and bend[0].tolist() == [1 << 24, TOP]
    inc, bend = np.array([1 << 24], np.uint32), BM.new(1)
    assert BM.apply(bend, inc, [0], 1) == [1, 0] and inc[0] == 1 and bend[0].tolist() == [1 << 24, 1]
    assert BM.apply(bend, inc, [0], ONE) == [1, 0] and inc[0] == 1 << 24 and not bend.any()
    # the guard and the list rule: a wrong tag, a hole, an entry beyond the bank, a count below n
    owner, bend, inc = om.new(4), BM.new(4), np.array([1000] * 4, np.uint32)
    owner[2] = 7
    rs = [2 * ONE] * 4
    assert BM.bend_owned_each(owner, bend, inc, rs, [2, -1, 4, 2], [8, 7, 7, 7], count=3) == [0, 0, 1] and not bend.any()
    assert BM.bend_owned_each(owner, bend, inc, rs, [1, -1, 4, 2], [8, 7, 7, 7]) == [1, 0, 1] and inc[2] == 2000 and bend[2, KEY] == 1000
    # the channel wheel counts the voices of the range that did not match; the centre on unbent voices counts nothing
    owner[:] = [0x03000001, 0x04000001, 0x03000002, 0]
    assert BM.bend_match(owner, bend, inc, 0, 4, (0x03000000, 0xFF000000), ONE) == [1, 0, 2] and inc[2] == 1000 and not bend.any()
    assert BM.bend_match(owner, bend, inc, 1, 3, (0x03000000, 0xFF000000), 3 * ONE) == [1, 0, 2] and inc.tolist() == [1000, 1000, 3000, 1000]


# ---------------------------------------------------------------------------------------------- glides under a bend

def bent_voice(key, ratio, tag=7):
    owner, glide, bend = om.new(4), GM.new(4), BM.new(4)
    owner[2] = tag
    inc = np.array([1, 1, key, 1], np.uint32)
    assert BM.apply(bend, inc, [2], ratio) == [1, 0]
    return owner, glide, bend, inc


@pytest.mark.parametrize("lo, hi", [(3000017, 4000037), (44739243, 89478485), (1000, 1001)])
@pytest.mark.parametrize("ratio", [BM.ratio_of(1.7), BM.ratio_of(-2.0), ONE + 1])
def test_a_glide_under_a_bend_lands_on_target_times_ratio(lo, hi, ratio):
    up, down = GM.per_64(900.0)
    for a, b in ((lo, hi), (hi, lo)):                            # from below and from above
        owner, glide, bend, inc = bent_voice(a, ratio)
        assert BM.glide_start_owned(owner, glide, bend, inc, [G(GM.TO_INC, up, down, target_inc=b)], [2], [7]) == [1, 0, 0]
        assert bend[2].tolist() == [a, ratio] and inc[2] == (a * ratio) >> 24
        plain = (np.array([a], np.uint32), np.array([[b, up, down, 0]], np.uint32))
        for _ in range(100000):
            res = BM.glide_advance(glide, bend, inc, 0, 4, 64)
            GM.advance(plain[1], plain[0], 0, 1, 64)
            assert bend[2, KEY] == plain[0][0], "the key walks the unbent voice's way"
            assert inc[2] == (int(bend[2, KEY]) * ratio) >> 24
            if res == [0, 1]:
                break
        assert bend[2].tolist() == [b, ratio] and inc[2] == (b * ratio) >> 24 and not glide.any()
        assert BM.apply(bend, inc, [2], ONE) == [1, 0] and inc[2] == b and not bend.any(), "the centre gives the target's bits"
        assert inc[[0, 1, 3]].tolist() == [1, 1, 1]


def test_the_forms_and_the_snap_run_on_the_key():
    ratio = BM.ratio_of(2.0)
    key = A3
    owner, glide, bend, inc = bent_voice(key, ratio)
    s = GM.scale_q16(-5)
    assert BM.glide_start_owned(owner, glide, bend, inc, [G(GM.FROM_SCALE, 9, 9, s)], [2], [7]) == [1, 0, 0]
    k1 = (key * s) >> 16
    assert glide[2].tolist() == [key, 9, 9, 0] and bend[2].tolist() == [k1, ratio] and inc[2] == (k1 * ratio) >> 24
    assert BM.glide_start_owned(owner, glide, bend, inc, [G(GM.TO_SCALE, 9, 9, s)], [2], [7]) == [1, 0, 0]
    assert glide[2, GM.TARGET] == (key * s) >> 16 and bend[2, KEY] == k1, "TO_SCALE composes on the old target; the key stays"
    BM.glide_stop(glide, bend, inc, 0, 4, snap=False)
    assert not glide.any() and bend[2].tolist() == [k1, ratio] and inc[2] == (k1 * ratio) >> 24
    assert BM.glide_start_owned(owner, glide, bend, inc, [G(GM.TO_SCALE, 9, 9, 1 << 17)], [2], [7]) == [1, 0, 0]
    assert glide[2, GM.TARGET] == 2 * k1, "not gliding: TO_SCALE rests on the key, not on the bent increment"
    BM.glide_stop(glide, bend, inc, 0, 4, snap=True)
    assert not glide.any() and bend[2].tolist() == [2 * k1, ratio] and inc[2] == (2 * k1 * ratio) >> 24
    # a withheld start under a bend leaves every word alone: the KEY's product is the one that counts
    before = (inc.copy(), bend.copy())
    assert BM.glide_start_owned(owner, glide, bend, inc, [G(GM.FROM_SCALE, 9, 9, TOP)], [2], [7]) == [0, 1, 0]
    assert np.array_equal(inc, before[0]) and np.array_equal(bend, before[1]) and not glide.any()
    # voices without a key take the plain path byte for byte
    rng = np.random.default_rng(4)
    from test_fx_glide_cpu import random_state as glide_state
    inc, glide = glide_state(rng, 300)
    a, b = (inc.copy(), glide.copy()), (inc.copy(), glide.copy())
    assert BM.glide_advance(a[1], BM.new(300), a[0], 0, 300, 200) == GM.advance(b[1], b[0], 0, 300, 200)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_block_cutting_does_not_change_a_glide_under_a_bend():
    """512 frames as 8 x 64, as 1 x 512 and as 37 + 100 + 27 + 348 on a bank where half the voices are bent: the same increments,
    keys and glide words at every multiple of 64 frames the cuttings share (the end), and the bent voices sound key * ratio."""
    rng = np.random.default_rng(6)
    n = 600
    from test_fx_glide_cpu import random_state as glide_state
    inc, glide = glide_state(rng, n)
    inc[inc == 0] = 12345
    glide[:, GM.CARRY] = 0
    glide[::3, GM.UP], glide[::3, GM.DOWN] = 1 << 22, 1 << 22
    bend = BM.new(n)
    BM.apply(bend, inc, np.arange(0, n, 2), np.where(np.arange(0, n, 2) % 4 == 0, BM.ratio_of(1.0), BM.ratio_of(-1.0)).astype(np.uint32))
    assert int((bend[:, KEY] != 0).sum()) > 250
    ends = []
    for cut in CUTS:
        a, g, b = inc.copy(), glide.copy(), bend.copy()
        res = [BM.glide_advance(g, b, a, 0, n, f) for f in cut]
        ends.append((a, g, b, sum(r[1] for r in res), res[-1][0]))
    a, g, b = ends[0][:3]
    p = BM.product(b[:, KEY], b[:, RATIO])
    fits = (b[:, KEY] == 0) | ((p >= 1) & (p <= TOP))           # where the last re-derived store was not withheld
    for a2, g2, b2, arrived, still in ends[1:]:
        assert np.array_equal(g2, g) and np.array_equal(b2, b) and (arrived, still) == ends[0][3:]
        assert np.array_equal(a2[fits], a[fits])
    assert ends[0][3] > 50 and ends[0][4] > 50
    moved = (b[:, KEY] != 0) & (glide[:, GM.TARGET] != 0) & fits
    assert np.array_equal(a[moved], p[moved].astype(np.uint32)) and moved.sum() > 100
    # where the product of the last step does not fit, the increment is the last product that did: that one word alone depends on
    # where the host cut its blocks, as the header says of a withheld store; key and glide words never do
    assert 0 < (~fits).sum() < 100


def test_the_rederived_store_is_withheld_at_an_overflowing_product():
    """key 0x60000000 bent up by 2.5 (0xF0000000 sounds), gliding up towards 0x70000000: from the step at which key * 2.5 passes 32
    bits the sounding increment stays where it last fitted, uncounted, while key and glide words advance and land."""
    ratio = 5 * ONE // 2
    owner, glide, bend, inc = bent_voice(0x60000000, ratio)
    assert inc[2] == 0xF0000000
    assert BM.glide_start_owned(owner, glide, bend, inc, [G(GM.TO_INC, 1 << 26, 1 << 26, target_inc=0x70000000)], [2], [7]) == [1, 0, 0]
    last_fit, held = int(inc[2]), 0
    for _ in range(200):
        key0, carry0 = int(bend[2, KEY]), int(glide[2, GM.CARRY])
        res = BM.glide_advance(glide, bend, inc, 0, 4, 64)
        p = (int(bend[2, KEY]) * ratio) >> 24
        if p <= TOP:
            last_fit = p
        else:
            held += 1
            assert bend[2, KEY] > key0 or res == [0, 1], "the key advanced all the same"
        assert inc[2] == last_fit
        if res == [0, 1]:
            break
    assert held > 3 and bend[2].tolist() == [0x70000000, ratio] and not glide.any() and inc[2] == last_fit < TOP
    assert BM.apply(bend, inc, [2], ONE) == [1, 0] and inc[2] == 0x70000000


def test_check_through_ctypes():
    assert fxb.fx_bend_check(RATIOS) == 0 == BM.check(RATIOS)
    assert fxb.fx_bend_check([]) == 0 == BM.check([])
    assert fxb.fx_bend_check(None) == BAD == BM.check(None)
    assert fxb.fx_bend_check(RATIOS, n=-1) == BAD == BM.check(RATIOS, -1)
    assert fxb.fx_bend_check(RATIOS + [0]) == BAD == BM.check(RATIOS + [0]) and b"ratio" in device.load().skred_amd_last_error()
    assert fxb.fx_bend_check(RATIOS + [0], n=len(RATIOS)) == 0 == BM.check(RATIOS + [0], len(RATIOS))


# ---------------------------------------------------------------------------------------------- the host program

@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fxbend") / "c_fx_bend_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_fx_bend_host.c"), os.path.join(CSRC, "skred_fx_bend.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"),
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
    assert host_lines[-1] == "OK" and len(host_lines) > 60
    groups = {l.split("/")[0] for l in host_lines[:-1]}
    assert groups == {"const", "check", "pack", "match", "owned", "tags", "clear", "download", "untouched"}, groups


# ---------------------------------------------------------------------------------------------- the clear rule

N_SCENE = 600


def scene_stage(bend_clear_rule=True):
    bank, pool, c0 = fxb.bank_fx(N_SCENE)
    return BM.FxBendStage(bank, pool, c0, bend_clear_rule=bend_clear_rule)


@pytest.mark.parametrize("name", BM.SCENES)
def test_scene_on_the_oracle(name):
    st = scene_stage()
    BM.run_scene(name, st)
    assert not st.bend.any()


@pytest.mark.parametrize("name", BM.SCENES)
def test_the_scenes_bite_without_the_clear_rule(name):
    st = scene_stage(bend_clear_rule=False)
    with pytest.raises(AssertionError):
        BM.run_scene(name, st)


def test_tag_clear_clears_only_what_it_tags():
    bend = BM.new(16)
    bend[:] = 3
    BM.tag_clear(bend, [3, -1, 16, 5, 7], 5, count=4)
    assert [int(b.any()) for b in bend] == [1, 1, 1, 0, 1, 0] + [1] * 10


# ---------------------------------------------------------------------------------------------- a mono line on the oracle

def test_a_mono_line_under_a_held_wheel_on_the_oracle():
    """One voice of the bank_fx recipe plays three keys, each struck again in the same voice, while the channel's wheel is held a
    semitone and a half up and then let go.  The bent twin gets every key by the header's order -- the strike, then bend_tags_each with
    the channel's ratio -- and the centre at the end; the other twin is struck at the bent increments outright and at the last key's
    own at the end.  A bend stores increments and nothing else: mixes and stems are bit-equal block for block, the words end at 0."""
    bank, pool, c0 = fxb.bank_fx(N_SCENE)
    v, F, tag = 301, 64, [0x03000030]
    st = BM.FxBendStage(bank, pool, c0)
    struck, cnt = bank.copy(), c0
    base = int(bank["phase_inc"][v])
    keys = [base, (base * GM.scale_q16(5)) >> 16, (base * GM.scale_q16(2)) >> 16]
    ratio = BM.ratio_of(1.5)
    import fx_live_model as live
    for k, key in enumerate(keys):
        st.strike([v], tag, [key])
        assert not st.bend[v].any(), "a key struck again starts unbent"
        assert st.bend_tags([ratio], tag) == [1, 0, 0]
        struck["phase_inc"][v] = (key * ratio) >> 24
        live.stamp(struck, np.array([v], np.int32), fxb.STAMP_TRIGGER, cnt)
        for blk in range(4):
            a, sa, cnt = cpuref.fx_render(struck, pool, cnt, F, 1, want_stems=True)
            b, sb = st.block(F)
            assert cnt == st.now() and st.inc[v] == struck["phase_inc"][v] != key
            assert sa.tobytes() == sb.tobytes() and a.tobytes() == b.tobytes(), f"key {k}, block {blk}: the twins differ"
    assert st.wheel(BM.CHAN, ONE) == [1, 0, N_SCENE - 1]
    struck["phase_inc"][v] = keys[-1]
    a, sa, cnt = cpuref.fx_render(struck, pool, cnt, F, 1, want_stems=True)
    b, sb = st.block(F)
    assert st.inc[v] == keys[-1] and not st.bend.any() and sa.tobytes() == sb.tobytes() and a.tobytes() == b.tobytes()
