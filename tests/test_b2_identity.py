"""The premise of the b2-reusing frames of sk_render_fast2_kernel (skred_render_fast2.hip: fast2_post_lr<.., B2R>).

Four of the five RBJ forms of banks.biquad_coeffs (== the reference's mmf_set_params) have b2 = +b0 or b2 = -b0 bit for bit
in float32: both go through the same division by a0.  For those lanes b2 * s(n-2) is sigma * fl(b0 * s(n-2)), the product the
filter formed two frames earlier, and multiplying a float by -1 only flips its sign bit.  Mode 5 (all-pass) is the form without
the property: a wave that holds such a voice keeps the plain frames.
"""
import numpy as np

from skred_amd import banks

SR = 48000
SIGN = np.uint32(0x80000000)


def recipe_draws(n=4096, seed=11):
    """K log-uniform 100..8000, Q uniform 0.5..4 as banks.bank_c2 draws them, plus the four corners of the range."""
    u = banks.lcg_uniform(2 * n, seed).reshape(2, n)
    k = (np.float32(100.0) * np.power(np.float32(80.0), u[0])).astype(np.float32)
    q = (np.float32(0.5) + np.float32(3.5) * u[1]).astype(np.float32)
    k = np.concatenate([k, np.float32([100.0, 100.0, 8000.0, 8000.0])])
    q = np.concatenate([q, np.float32([0.5, 4.0, 0.5, 4.0])])
    return k, q


def qualifies(co):
    """The kernel's vote, per voice: the bits of b2 are the bits of b0, or those with the sign flipped."""
    b0, b2 = co["b0"].view(np.uint32), co["b2"].view(np.uint32)
    return ((b0 ^ b2) & ~SIGN) == 0


def test_modes_1_to_4_have_b2_equal_to_plus_or_minus_b0():
    k, q = recipe_draws()
    for mode, sign in ((1, 0), (2, 0), (3, 1), (4, 0)):
        co = banks.biquad_coeffs(np.full(len(k), mode), k, q, SR)
        assert np.isfinite(co["b0"]).all() and (co["b0"] != 0).all(), mode
        assert qualifies(co).all(), mode
        flipped = (co["b0"].view(np.uint32) ^ co["b2"].view(np.uint32)) >> np.uint32(31)
        assert (flipped == sign).all(), mode                     # low-pass, high-pass, notch: +b0; band-pass: -b0


def test_mode_5_does_not():
    k, q = recipe_draws()
    co = banks.biquad_coeffs(np.full(len(k), 5), k, q, SR)
    assert not qualifies(co).any()


def test_the_recipe_bank_qualifies_in_every_voice():
    bank, _, _ = banks.bank_c2(2048 + 384)
    flt = bank["voice_filter"]
    assert qualifies({"b0": np.asarray(flt["b0"], np.float32), "b2": np.asarray(flt["b2"], np.float32)}).all()
    assert sorted(set(np.asarray(bank["voice_filter_mode"]).tolist())) == [1, 2, 3, 4]


def test_negation_commutes_with_the_float32_product():
    """fl((-b0) * x) == -fl(b0 * x) bit for bit, subnormal and underflowing products included: rounding to nearest even is
    symmetric in the sign."""
    rng = np.random.default_rng(3)
    n = 200000
    b0 = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 4, n))).astype(np.float32)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 4, n))).astype(np.float32)
    # products around and below the smallest normal number (2^-126), down to the underflow to zero
    bs = (rng.standard_normal(n) * np.exp2(rng.integers(-90, -50, n))).astype(np.float32)
    xs = (rng.standard_normal(n) * np.exp2(rng.integers(-90, -50, n))).astype(np.float32)
    b0, x = np.concatenate([b0, bs, np.float32([0.0, -0.0, 1.0])]), np.concatenate([x, xs, np.float32([1.0, 1.0, 0.0])])
    p = (b0 * x).astype(np.float32)
    tiny = np.abs(p) < np.float32(2.0 ** -126)
    assert (tiny & (p != 0)).sum() > 1000 and (p == 0).sum() > 1000     # the subnormal and the flushed-by-rounding cases occur
    lhs = ((-b0).astype(np.float32) * x).astype(np.float32)
    rhs = (-p).astype(np.float32)
    assert (lhs.view(np.uint32) == rhs.view(np.uint32)).all()
    # ... and sigma * P with sigma = -1.0f is that negation, exactly
    assert ((np.float32(-1.0) * p).astype(np.float32).view(np.uint32) == rhs.view(np.uint32)).all()
