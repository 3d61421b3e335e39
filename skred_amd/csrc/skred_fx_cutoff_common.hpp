// skred_fx_cutoff_common.hpp -- the defined coefficient arithmetic of the fixed-point bank on the device: the twin of
// skred_fx_filter_coeffs_w (skred_fx_cutoff.c; include/skred_amd_fxpt.h, "filter cutoff", has the definition step by step with the
// bound of every intermediate, and tests/fx_cutoff_model.py restates it in Python integers).  Integers only: 64-bit products with a
// stated shift, signed ones rounded by (x + half) >> s on an arithmetic shift (to nearest, ties towards plus infinity), the quotients
// on magnitudes (to nearest, ties away from zero).  Nothing leaves 64 bits inside the box (w_q29 in [2^19, 3 * 2^29], q_q16 in
// [2^10, 2^26]), no divisor is zero, and the device, the host function and the model give the same five words.  The 64-bit divides
// are software on this hardware: nine per voice at most.
#ifndef SKRED_FX_CUTOFF_COMMON_HPP
#define SKRED_FX_CUTOFF_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_layout.h"

struct skx_cut5_t {
  int32_t b0, b1, b2, a1, a2;
};

// (p * z + 2^31) >> 32: |p| < 2^31, z < 2^32, the product below 2^63
__device__ __forceinline__ int64_t skx_cut_mul(int64_t p, uint32_t z) { return (p * (int64_t)z + (1ll << 31)) >> 32; }

// round(|num| * 2^(s + 2) / a0), ties away from zero, the sign put back, clamped to int32: |num| <= a0 or 2^32, |num| << s < 2^64
__device__ __noinline__ int32_t skx_cut_quot(int64_t num, uint64_t a0, int s) {
  const uint64_t n = (uint64_t)(num < 0 ? -num : num) << s;
  const uint64_t qa = n / a0, ra = n - qa * a0;
  const uint64_t mag = (qa << 2) + ((ra << 2) + (a0 >> 1)) / a0;        // (ra < a0 < 2^36.1)
  if (num < 0) return mag > 0x80000000ull ? INT32_MIN : (int32_t)-(int64_t)mag;
  return mag > 0x7fffffffull ? INT32_MAX : (int32_t)mag;
}

__device__ __forceinline__ skx_cut5_t skx_cutoff_coeffs(uint32_t mode, uint32_t w, uint32_t q) {
  const bool upper = w > SKX_CUTOFF_HALF_PI_Q29;
  const uint32_t r = upper ? SKX_CUTOFF_PI_Q29 - w : w;                  // Q29, < 2^30
  const uint32_t z = (uint32_t)(((uint64_t)r * r + (1ull << 27)) >> 28);  // (r / 2)^2 in Q32, < 2^32
  int64_t p = SKX_CUTOFF_S5;
  p = skx_cut_mul(p, z) + SKX_CUTOFF_S4;
  p = skx_cut_mul(p, z) + SKX_CUTOFF_S3;
  p = skx_cut_mul(p, z) + SKX_CUTOFF_S2;
  p = skx_cut_mul(p, z) + SKX_CUTOFF_S1;
  const uint64_t sinc = (uint64_t)((1ll << 31) + skx_cut_mul(p, z));    // sin(r) / r in Q31, <= 2^31
  const uint64_t rs = (uint64_t)r * sinc;                               // sin(w) in Q60, < 2^61
  int64_t c = SKX_CUTOFF_C6;
  c = skx_cut_mul(c, z) + SKX_CUTOFF_C5;
  c = skx_cut_mul(c, z) + SKX_CUTOFF_C4;
  c = skx_cut_mul(c, z) + SKX_CUTOFF_C3;
  c = skx_cut_mul(c, z) + SKX_CUTOFF_C2;
  const int64_t t = skx_cut_mul(c, z);
  const int64_t cosr = (1ll << 31) - (int64_t)z + skx_cut_mul(t, z);    // cos(r) in Q31
  const int64_t cs = upper ? -cosr : cosr;
  const uint64_t den = (uint64_t)q << 15;                               // rs is Q60, q << 15 is 2 q in Q30; <= 2^41
  const uint64_t alpha = (rs + (den >> 1)) / den;                       // sn / (2 q) in Q30, <= 2^35
  const uint64_t a0 = (1ull << 30) + alpha;
  const int64_t one = 1ll << 30, one31 = 1ll << 31, ia = (int64_t)alpha;
  int64_t n0, n1;
  int s0 = 28, s1 = 28;
  switch (mode) {
    case 2:  n0 = one31 + cs; s0 = 26; n1 = -n0; s1 = 27; break;
    case 3:  n0 = ia; n1 = 0; break;
    case 4:  n0 = one; n1 = -cs; break;
    case 5:  n0 = one - ia; n1 = -cs; break;
    default: n0 = one31 - cs; s0 = 26; n1 = n0; s1 = 27; break;
  }
  skx_cut5_t o;
  o.a1 = skx_cut_quot(-cs, a0, 28);
  o.b0 = skx_cut_quot(n0, a0, s0);
  o.b1 = mode >= 4 ? o.a1 : mode == 3 ? 0 : skx_cut_quot(n1, a0, s1);  // (modes 4, 5: the same numerator, the same quotient)
  o.b2 = mode == 3 ? -o.b0 : mode == 5 ? (int32_t)(1 << 30) : o.b0;     // (-alpha / a0: the rule is symmetric; a0 / a0 is exact)
  o.a2 = skx_cut_quot(one - ia, a0, 28);
  return o;
}

// the five words of voice v: SKX_FILT is b0 b1 b2 a1 and nothing else, a2 is word 0 of SKX_FILT2 -- no neighbour is written
__device__ __forceinline__ void skx_cutoff_store(skx_plane_t *filt, skx_plane_t *filt2, int v, const skx_cut5_t &c) {
  *reinterpret_cast<uint4 *>(&filt[v]) = make_uint4((uint32_t)c.b0, (uint32_t)c.b1, (uint32_t)c.b2, (uint32_t)c.a1);
  filt2[v].w[0] = (uint32_t)c.a2;
}

#endif
