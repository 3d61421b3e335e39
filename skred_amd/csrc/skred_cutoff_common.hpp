// skred_cutoff_common.hpp -- the defined coefficient arithmetic on the device: the twin of skred_filter_coeffs_w (skred_bank_cutoff.c;
// include/skred_amd.h, "filter cutoff on the device", has the definition operation by operation, and tests/cutoff_model.py restates
// it in numpy).  Every multiply, add, subtract and divide below is ONE correctly rounded fp32 operation -- __fmul_rn, __fadd_rn,
// __fsub_rn, __fdiv_rn and nothing else; a negation flips the sign bit -- so the device, the host function and the model give the same
// bits for the same (mode, w, q).  Inside the box (w in [2^-10, 3], q in [2^-6, 2^10]) no intermediate is denormal, no divisor is
// zero and every result is finite.
#ifndef SKRED_CUTOFF_COMMON_HPP
#define SKRED_CUTOFF_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"

struct sk_cut5_t {
  float b0, b1, b2, a1, a2;
};

// sn = sin(w), cs = cos(w) for w in [0, 3]: r = w, or past pi / 2 r = (PI_HI - w) + PI_LO (the first difference is exact) with the
// cosine's sign flipped; z = r * r; both polynomials by Horner in z
__device__ __forceinline__ void sk_cutoff_sincos(float w, float &sn, float &cs) {
  const bool upper = w > SK_CUTOFF_HALF_PI;
  const float r = upper ? __fadd_rn(__fsub_rn(SK_CUTOFF_PI_HI, w), SK_CUTOFF_PI_LO) : w;
  const float z = __fmul_rn(r, r);
  float p = SK_CUTOFF_S4;
  p = __fadd_rn(__fmul_rn(p, z), SK_CUTOFF_S3);
  p = __fadd_rn(__fmul_rn(p, z), SK_CUTOFF_S2);
  p = __fadd_rn(__fmul_rn(p, z), SK_CUTOFF_S1);
  sn = __fadd_rn(r, __fmul_rn(__fmul_rn(r, z), p));
  float c = SK_CUTOFF_C5;
  c = __fadd_rn(__fmul_rn(c, z), SK_CUTOFF_C4);
  c = __fadd_rn(__fmul_rn(c, z), SK_CUTOFF_C3);
  c = __fadd_rn(__fmul_rn(c, z), SK_CUTOFF_C2);
  c = __fadd_rn(__fmul_rn(c, z), SK_CUTOFF_C1);
  c = __fadd_rn(1.0f, __fmul_rn(z, c));
  cs = upper ? -c : c;
}

// skred_filter_coeffs' sequence behind sn and cs, unchanged: alpha, a0, the mode's numerator, the five quotients
__device__ __forceinline__ sk_cut5_t sk_cutoff_coeffs(uint32_t mode, float w, float q) {
  float sn, cs;
  sk_cutoff_sincos(w, sn, cs);
  const float alpha = __fdiv_rn(sn, __fmul_rn(2.0f, q));
  const float a0 = __fadd_rn(1.0f, alpha);
  float b0, b1, b2;
  switch (mode) {
    case 2: { const float s = __fadd_rn(1.0f, cs); b0 = __fdiv_rn(s, 2.0f); b1 = -s; b2 = b0; break; }
    case 3: b0 = alpha; b1 = 0.0f; b2 = -alpha; break;
    case 4: b0 = 1.0f; b1 = __fmul_rn(-2.0f, cs); b2 = 1.0f; break;
    case 5: b0 = __fsub_rn(1.0f, alpha); b1 = __fmul_rn(-2.0f, cs); b2 = __fadd_rn(1.0f, alpha); break;
    default: { const float d = __fsub_rn(1.0f, cs); b0 = __fdiv_rn(d, 2.0f); b1 = d; b2 = b0; break; }
  }
  sk_cut5_t c;
  c.b0 = __fdiv_rn(b0, a0);
  c.b1 = __fdiv_rn(b1, a0);
  c.b2 = __fdiv_rn(b2, a0);
  c.a1 = __fdiv_rn(__fmul_rn(-2.0f, cs), a0);
  c.a2 = __fdiv_rn(__fsub_rn(1.0f, alpha), a0);
  return c;
}

// the five words of voice v, as word stores: velocity and smoothing (SKP_GAIN words 0, 1) and cz_distortion (SKP_FILT word 3) keep
// their bits, the filter memory is another plane
__device__ __forceinline__ void sk_cutoff_store(const sk_cut_planes_t &p, int v, const sk_cut5_t &c) {
  *reinterpret_cast<uint2 *>(&p.gain[v].w[2]) = make_uint2(__float_as_uint(c.b0), __float_as_uint(c.b1));
  *reinterpret_cast<uint2 *>(&p.filt[v].w[0]) = make_uint2(__float_as_uint(c.b2), __float_as_uint(c.a1));
  p.filt[v].w[2] = __float_as_uint(c.a2);
}

#endif
