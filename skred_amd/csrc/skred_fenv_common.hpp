// skred_fenv_common.hpp -- the filter envelope's stage rule and its advance pass on one voice (include/skred_amd.h, "filter envelope",
// has the definition; tests/fenv_model.py restates it in numpy).  Shared by skred_fenv_kernels.hip (the records enter the attack) and
// skred_cutoff_kernels.hip (the envelope instantiation of sk_cutoff_advance_kernel steps the contour).  The envelope has no
// arithmetic of its own: a step is the cutoff advance's one __fmul_rn, a level is compared on the bit patterns as integers (every w
// and every level is positive and finite), and every coefficient store is sk_cutoff_store(sk_cutoff_coeffs(mode, w, q)).
#ifndef SKRED_FENV_COMMON_HPP
#define SKRED_FENV_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"
#include "skred_cutoff_common.hpp"

__device__ __forceinline__ uint4 *sk_fenv_a(sk_fenv_t *fenv, int v) { return reinterpret_cast<uint4 *>(&fenv[v].w[0]); }
__device__ __forceinline__ uint4 *sk_fenv_b(sk_fenv_t *fenv, int v) { return reinterpret_cast<uint4 *>(&fenv[v].w[SK_FENV_RATE_ATTACK]); }
__device__ __forceinline__ void sk_fenv_zero(sk_fenv_t *fenv, int v) {
  *sk_fenv_a(fenv, v) = make_uint4(0u, 0u, 0u, 0u);
  *sk_fenv_b(fenv, v) = make_uint4(0u, 0u, 0u, 0u);
}

// one level of the rule below: from w, a stage with level T and rate r lands at once (w = T's bits, `landed` set; returns false) when
// w is level with T or the rate points away from it; otherwise target = T, rate = r (returns true: the voice is in that stage)
__device__ __forceinline__ bool sk_fenv_aim(uint32_t T, uint32_t r, uint32_t &w, uint32_t &target, uint32_t &rate, bool &landed) {
  const bool up = __uint_as_float(r) > 1.0f;                             // (a rate is never 1: skred_fenv_check)
  if (w != T && (up ? w < T : w > T)) {
    target = T;
    rate = r;
    return true;
  }
  w = T;
  landed = true;
  return false;
}

// ENTERING A STAGE.  fa = stage, w_peak, w_sustain, w_end; fb = rate_attack, rate_decay, rate_release, 0.  Stage `stage` is entered
// from w; a stage that lands at once enters the next: attack, decay, sustain -- which rests (target = rate = 0) -- and release, behind
// which there is no stage (0, target = rate = 0: the caller clears the fenv words).  Returns the stage the voice is in.  Straight-line
// code on values (no indexed level: nothing here lives in memory).
__device__ __forceinline__ uint32_t sk_fenv_enter(uint32_t stage, const uint4 fa, const uint4 fb, uint32_t &w, uint32_t &target, uint32_t &rate,
                                                  bool &landed) {
  if (stage == SK_FENV_ATTACK) {
    if (sk_fenv_aim(fa.y, fb.x, w, target, rate, landed)) return SK_FENV_ATTACK;
    stage = SK_FENV_DECAY;
  }
  if (stage == SK_FENV_DECAY) {
    if (sk_fenv_aim(fa.z, fb.y, w, target, rate, landed)) return SK_FENV_DECAY;
    stage = SK_FENV_SUSTAIN;
  } else if (stage == SK_FENV_RELEASE) {
    if (sk_fenv_aim(fa.w, fb.z, w, target, rate, landed)) return SK_FENV_RELEASE;
    stage = SK_FENV_OFF;
  }
  target = 0u;
  rate = 0u;
  return stage;
}

// THE ADVANCE PASS on a voice that has a contour (fa.x != 0).  a = the voice's w, target, rate_up, rate_down as loaded.  `released`:
// its sample_release is not 0.  Stores what changed of the cutoff and fenv words and the coefficients; still / arrived as the plain
// pass counts them
__device__ __forceinline__ void sk_fenv_advance(sk_cut_t *cut, sk_fenv_t *fenv, const sk_cut_planes_t &p, int v, const uint4 &a, const uint4 &fa,
                                                bool released, uint32_t frames, bool &still, bool &arrived) {
  const uint4 fb = *sk_fenv_b(fenv, v);                                  // rate_attack, rate_decay, rate_release, 0
  const uint4 b = *reinterpret_cast<const uint4 *>(&cut[v].w[SK_CUT_CARRY]);   // carry, q, mode, 0
  uint32_t stage = fa.x, w = a.x, target = a.y, rate = a.z;              // (an enveloped voice's two rates are one)
  const bool enter = released && stage != SK_FENV_RELEASE;
  if (enter) stage = sk_fenv_enter(SK_FENV_RELEASE, fa, fb, w, target, rate, arrived);
  const bool coeffs = a.y != 0u || enter;                                // moving when the pass began, or released in it
  const uint32_t c = b.x + frames;
  for (uint32_t m = c >> 6; m && target != 0u; --m) {
    const bool up = w < target;
    w = __float_as_uint(__fmul_rn(__uint_as_float(w), __uint_as_float(rate)));
    if (up ? w >= target : w <= target) {
      w = target;
      arrived = true;
      stage = sk_fenv_enter(stage == SK_FENV_RELEASE ? (uint32_t)SK_FENV_OFF : stage + 1u, fa, fb, w, target, rate, arrived);
    }
  }
  still = target != 0u;
  if (w != a.x || target != a.y || rate != a.z) *reinterpret_cast<uint4 *>(&cut[v].w[0]) = make_uint4(w, target, rate, rate);
  const uint32_t carry = stage ? c & 63u : 0u;                           // the note's grid runs on through sustain; it ends with the contour
  if (carry != b.x) cut[v].w[SK_CUT_CARRY] = carry;
  if (stage == SK_FENV_OFF) sk_fenv_zero(fenv, v);
  else if (stage != fa.x) fenv[v].w[SK_FENV_STAGE] = stage;
  if (coeffs) sk_cutoff_store(p, v, sk_cutoff_coeffs(b.z, __uint_as_float(w), __uint_as_float(b.y)));
}

#endif
