// skred_fenv_kernels.hip -- the filter envelope: per-note cutoff contours that follow the gate (gfx950 / CDNA4, wave64).
//
// skred_bank_fenv_match / _fenv_owned_each / _fenv_tags_each (include/skred_amd.h, "filter envelope", has the definition).
// fenv[n_voices] lies beside the cutoff array: eight words per voice, two uint4 -- stage, w_peak, w_sustain, w_end (fp32 bit patterns
// inside the cutoff box) and rate_attack, rate_decay, rate_release, 0.  stage 0: no contour, and all eight words are 0.  The contour
// is a small program kept beside the voice: a record enters the attack here, skred_bank_cutoff_advance steps it (the envelope
// instantiation of sk_cutoff_advance_kernel, skred_cutoff_kernels.hip, through sk_fenv_advance) and enters the release from the
// voice's own release clock.  The envelope moves the voice's cutoff words and through them the five coefficients.
//
//   sk_fenv_clear_kernel   sk_cutoff_clear_kernel on this array: one thread per voice of a listed slot, both halves zeroed.  Launched
//                          behind every tag launch of a bank that has an fenv array.
//   sk_fenv_match_kernel   sk_cutoff_match_kernel's geometry, guard and counting: THE RECORD (sk_fenv_apply) as a kernel argument.
//   sk_fenv_each_kernel    sk_cutoff_each_kernel's geometry and guard, the workgroup's records staged in LDS (two 16-byte loads per
//                          entry, not per voice).
//
// Counts are sk_owner_count's.  Plain vector stores and ordinary atomics only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"
#include "skred_fenv_common.hpp"
#include "skred_update_common.hpp"   // sk_entry_decode, sk_entry_owned, sk_range_lane, sk_owner_count, sk_batch_done, the launch helpers

// a level of the record: the value's bits (ABS), or w_now * value, ONE multiply, clamped into the box (REL)
__device__ __forceinline__ uint32_t sk_fenv_level(bool rel, uint32_t w_now, uint32_t value, bool &clamped) {
  if (!rel) return value;
  const float f = __fmul_rn(__uint_as_float(w_now), __uint_as_float(value));
  if (!(f >= SK_CUTOFF_W_MIN && f <= SK_CUTOFF_W_MAX)) clamped = true;
  return __float_as_uint(f < SK_CUTOFF_W_MIN ? SK_CUTOFF_W_MIN : f > SK_CUTOFF_W_MAX ? SK_CUTOFF_W_MAX : f);
}

// THE RECORD on voice v: ra = set, start, peak, sustain; rb = end, rate_attack, rate_decay, rate_release.  Returns 1: started, 2:
// withheld (no cutoff word); clamped: a product lay outside the box
__device__ __forceinline__ int sk_fenv_apply(sk_fenv_t *fenv, sk_cut_t *cut, const sk_cut_planes_t &p, int v, const uint4 &ra, const uint4 &rb,
                                             bool &clamped) {
  const uint4 a = *reinterpret_cast<const uint4 *>(&cut[v].w[0]);        // w, target, rate_up, rate_down
  if (a.x == 0u) return 2;
  const uint2 qm = *reinterpret_cast<const uint2 *>(&cut[v].w[SK_CUT_Q]);   // q, mode
  const bool rel = (ra.x & SK_FENV_REL) != 0u;
  uint32_t w = (ra.x & SK_FENV_START) ? sk_fenv_level(rel, a.x, ra.y, clamped) : a.x;
  const uint4 fa = make_uint4(SK_FENV_ATTACK, sk_fenv_level(rel, a.x, ra.z, clamped), sk_fenv_level(rel, a.x, ra.w, clamped),
                              sk_fenv_level(rel, a.x, rb.x, clamped));
  const uint4 fb = make_uint4(rb.y, rb.z, rb.w, 0u);
  uint32_t target, rate;
  bool landed = false;
  const uint32_t stage = sk_fenv_enter(SK_FENV_ATTACK, fa, fb, w, target, rate, landed);   // (sustain at the latest: never 0)
  *reinterpret_cast<uint4 *>(&cut[v].w[0]) = make_uint4(w, target, rate, rate);
  cut[v].w[SK_CUT_CARRY] = 0u;
  *sk_fenv_a(fenv, v) = make_uint4(stage, fa.y, fa.z, fa.w);
  *sk_fenv_b(fenv, v) = fb;
  if (w != a.x) sk_cutoff_store(p, v, sk_cutoff_coeffs(qm.y, __uint_as_float(w), __uint_as_float(qm.x)));
  return 1;
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fenv_clear_kernel(sk_fenv_t *fenv, const int32_t *d_slots, int n, const uint32_t *d_count,
                                                                      int k_shift, int n_voices) {
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);
  if (t.valid) sk_fenv_zero(fenv, t.e + t.l);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fenv_match_kernel(sk_fenv_t *fenv, sk_cut_t *cut, sk_fenv_each_t rec, int K,
                                                                      uint64_t filter_mask, int first, int count,
                                                                      const uint32_t *__restrict__ owner, uint32_t value, uint32_t omask,
                                                                      sk_cut_planes_t p, uint32_t *d_result) {
  __shared__ uint32_t sums[4];
  const sk_lane_t t = sk_range_lane(first, count, K);
  const bool hit = t.in_range && sk_owner_matches(owner[t.v - t.l], value, omask);
  int did = 0;
  bool clamped = false;
  if (hit && ((filter_mask >> t.l) & 1))
    did = sk_fenv_apply(fenv, cut, p, t.v, make_uint4(rec.w[0], rec.w[1], rec.w[2], rec.w[3]), make_uint4(rec.w[4], rec.w[5], rec.w[6], rec.w[7]),
                        clamped);
  const bool flag[4] = { did == 1, did == 2, t.head && !hit, did == 1 && clamped };
  sk_owner_count<4>(sums, d_result, flag);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fenv_each_kernel(sk_fenv_t *fenv, sk_cut_t *cut, const sk_fenv_each_t *__restrict__ each,
                                                                     int k_shift, uint64_t filter_mask, const int32_t *d_slots,
                                                                     const uint32_t *__restrict__ tags, const uint32_t *__restrict__ owner, int n,
                                                                     const uint32_t *d_count, int n_voices, sk_cut_planes_t p, uint32_t *d_result,
                                                                     uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint4 ent_a[SK_CONTROL_SPAN];                               // set, start, peak, sustain of this workgroup's entries
  __shared__ uint4 ent_b[SK_CONTROL_SPAN];                               // end, rate_attack, rate_decay, rate_release
  __shared__ uint32_t sums[4];
  const int per_wg = SK_CONTROL_SPAN >> k_shift;
  const int64_t base = (int64_t)blockIdx.x * per_wg;
  if ((int)threadIdx.x < per_wg && base + (int)threadIdx.x < n) {
    ent_a[threadIdx.x] = *reinterpret_cast<const uint4 *>(&each[base + (int)threadIdx.x].w[0]);
    ent_b[threadIdx.x] = *reinterpret_cast<const uint4 *>(&each[base + (int)threadIdx.x].w[SK_FENV_E_END]);
  }
  __syncthreads();
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);   // (t.i == base + the entry's place)
  const bool owned = sk_entry_owned(owner, tags, t);
  int did = 0;
  bool clamped = false;
  if (owned && ((filter_mask >> t.l) & 1)) {
    const int at = (int)threadIdx.x >> k_shift;
    did = sk_fenv_apply(fenv, cut, p, t.e + t.l, ent_a[at], ent_b[at], clamped);
  }
  const bool flag[4] = { did == 1, did == 2, t.valid && !owned && t.l == 0, did == 1 && clamped };
  sk_owner_count<4>(sums, d_result, flag);
  sk_batch_done(cnt, done, seq);
}

extern "C" int sk_launch_fenv_clear(sk_fenv_t *fenv, const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices, int n_voices,
                                    hipStream_t stream) {
  if (n <= 0) return 0;
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_fenv_clear_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, fenv, d_slots, n, d_count, sh, n_voices);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_fenv_match(sk_fenv_t *fenv, sk_cut_t *cut, const sk_fenv_each_t *rec, int slot_voices, uint64_t filter_mask, int first,
                                    int count, const uint32_t *owner, uint32_t value, uint32_t mask, const sk_cut_planes_t *planes,
                                    uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 4, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_fenv_match_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, fenv, cut, *rec, slot_voices, filter_mask,
                     first, count, owner, value, mask, *planes, d_result);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_fenv_each(sk_fenv_t *fenv, sk_cut_t *cut, const sk_fenv_each_t *d_each, int slot_voices, uint64_t filter_mask,
                                   const int32_t *d_slots, const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count,
                                   int n_voices, const sk_cut_planes_t *planes, uint32_t *d_result, uint32_t *cnt, uint32_t *done,
                                   uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 4, stream);
  if (e != hipSuccess) return (int)e;
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_fenv_each_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, fenv, cut, d_each, sh, filter_mask,
                     d_slots, d_tags, owner, n, d_count, n_voices, *planes, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}
