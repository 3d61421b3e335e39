// skred_fx_fenv_common.hpp -- the fixed-point filter envelope's stage rule and its advance pass on one voice (include/skred_amd_fxpt.h,
// "filter envelope", has the definition; tests/fx_fenv_model.py restates it in numpy integers).  Shared by skred_fx_fenv_kernels.hip
// (the records enter the attack) and skred_fx_cutoff_kernels.hip (the ENV instantiation of sk_fx_cutoff_advance_kernel steps the
// contour).  The envelope has no arithmetic of its own: a step is skx_step_64 (skred_fx_step_common.hpp) with both rates the stage's,
// a level is compared as the uint32 it is, and every coefficient store is skx_cutoff_store(skx_cutoff_coeffs(mode, w, q)).  Exact
// integers: the same bits on every machine.
#ifndef SKRED_FX_FENV_COMMON_HPP
#define SKRED_FX_FENV_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_layout.h"
#include "skred_fx_cutoff_common.hpp"
#include "skred_fx_step_common.hpp"

// the planes the cutoff and envelope kernels touch: phase_inc read, the coefficient words stored
struct skx_cut_planes_t {
  const skx_plane_t *osc;
  skx_plane_t *filt, *filt2;
};

__device__ __forceinline__ uint4 *skx_cut_a(skx_cut_t *cut, int v) { return reinterpret_cast<uint4 *>(&cut[v].w[0]); }
__device__ __forceinline__ uint4 *skx_cut_b(skx_cut_t *cut, int v) { return reinterpret_cast<uint4 *>(&cut[v].w[SKX_CUT_CARRY]); }
__device__ __forceinline__ uint4 *skx_fenv_a(skx_fenv_t *fenv, int v) { return reinterpret_cast<uint4 *>(&fenv[v].w[0]); }
__device__ __forceinline__ uint4 *skx_fenv_b(skx_fenv_t *fenv, int v) { return reinterpret_cast<uint4 *>(&fenv[v].w[SKX_FENV_RATE_ATTACK]); }
__device__ __forceinline__ void skx_fenv_zero(skx_fenv_t *fenv, int v) {
  *skx_fenv_a(fenv, v) = make_uint4(0u, 0u, 0u, 0u);
  *skx_fenv_b(fenv, v) = make_uint4(0u, 0u, 0u, 0u);
}

// one level of the rule below: from w, a stage with level T and rate r lands at once (`landed` set; returns false) iff w == T -- an
// integer rate has no direction, the direction is w < T or w > T; otherwise target = T, rate = r (returns true: the voice is in that
// stage)
__device__ __forceinline__ bool skx_fenv_aim(uint32_t T, uint32_t r, uint32_t w, uint32_t &target, uint32_t &rate, bool &landed) {
  if (w != T) {
    target = T;
    rate = r;
    return true;
  }
  landed = true;
  return false;
}

// ENTERING A STAGE.  fa = stage, w_peak, w_sustain, w_end; fb = rate_attack, rate_decay, rate_release, 0.  Stage `stage` is entered
// from w; a stage that lands at once enters the next: attack, decay, sustain -- which rests (target = rate = 0) -- and release, behind
// which there is no stage (0, target = rate = 0: the caller clears the fenv words).  Returns the stage the voice is in.  Straight-line
// code on values (no indexed level: nothing here lives in memory).
__device__ __forceinline__ uint32_t skx_fenv_enter(uint32_t stage, const uint4 fa, const uint4 fb, uint32_t w, uint32_t &target, uint32_t &rate,
                                                   bool &landed) {
  if (stage == SKX_FENV_ATTACK) {
    if (skx_fenv_aim(fa.y, fb.x, w, target, rate, landed)) return SKX_FENV_ATTACK;
    stage = SKX_FENV_DECAY;
  }
  if (stage == SKX_FENV_DECAY) {
    if (skx_fenv_aim(fa.z, fb.y, w, target, rate, landed)) return SKX_FENV_DECAY;
    stage = SKX_FENV_SUSTAIN;
  } else if (stage == SKX_FENV_RELEASE) {
    if (skx_fenv_aim(fa.w, fb.z, w, target, rate, landed)) return SKX_FENV_RELEASE;
    stage = SKX_FENV_OFF;
  }
  target = 0u;
  rate = 0u;
  return stage;
}

// THE ADVANCE PASS on a voice that has a contour (fa.x != 0).  a = the voice's w, target, up, down as loaded.  `released`: its
// sample_release is not 0.  Stores what changed of the cutoff and fenv words and the coefficients; still / arrived as the plain pass
// counts them
__device__ __forceinline__ void skx_fenv_advance(skx_cut_t *cut, skx_fenv_t *fenv, const skx_cut_planes_t &p, int v, const uint4 &a,
                                                 const uint4 &fa, bool released, uint32_t frames, bool &still, bool &arrived) {
  const uint4 fb = *skx_fenv_b(fenv, v);                                 // rate_attack, rate_decay, rate_release, 0
  const uint4 b = *skx_cut_b(cut, v);                                    // carry, q, mode, 0
  uint32_t stage = fa.x, w = a.x, target = a.y, rate = a.z;              // (an enveloped voice's two rates are one)
  const bool enter = released && stage != SKX_FENV_RELEASE;
  if (enter) stage = skx_fenv_enter(SKX_FENV_RELEASE, fa, fb, w, target, rate, arrived);
  const bool coeffs = a.y != 0u || enter;                                // moving when the pass began, or released in it
  const uint32_t c = b.x + frames;                                       // (carry <= 63, frames <= 65536)
  for (uint32_t m = c >> 6; m && target != 0u; --m) {
    if (skx_step_64(w, target, rate, rate)) {                            // (w != target: a stage with a target was entered off its level)
      w = target;
      arrived = true;
      stage = skx_fenv_enter(stage == SKX_FENV_RELEASE ? (uint32_t)SKX_FENV_OFF : stage + 1u, fa, fb, w, target, rate, arrived);
    }
  }
  still = target != 0u;
  if (w != a.x || target != a.y || rate != a.z) *skx_cut_a(cut, v) = make_uint4(w, target, rate, rate);
  const uint32_t carry = stage ? c & 63u : 0u;                           // the note's grid runs on through sustain; it ends with the contour
  if (carry != b.x) cut[v].w[SKX_CUT_CARRY] = carry;
  if (stage == SKX_FENV_OFF) skx_fenv_zero(fenv, v);
  else if (stage != fa.x) fenv[v].w[SKX_FENV_STAGE] = stage;
  if (coeffs) skx_cutoff_store(p.filt, p.filt2, v, skx_cutoff_coeffs(b.z, w, b.y));
}

#endif
