// skred_ctl_common.hpp -- what the controller kernels share (skred_ctl_kernels.hip: a range, a list, a list under the note-owner
// guard; skred_expr_kernels.hip: a range under a masked owner match, a list with per-entry values): the records' way into LDS, the
// field stores with their two guards, and the counts.  One place for the stores, so that a guarded or per-entry controller
// cannot drift from skred_bank_ctl_range.
#ifndef SKRED_CTL_COMMON_HPP
#define SKRED_CTL_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"
#include "skred_update_common.hpp"   // sk_plane_ptrs_t, sk_list_voice

// the K records -> LDS (the unmasked ones arrive zeroed by the host: set == 0)
__device__ __forceinline__ void sk_ctl_stage(uint32_t *lds, const sk_ctl_t *__restrict__ recs, int K) {
  const uint32_t *src = reinterpret_cast<const uint32_t *>(recs);
  for (int i = threadIdx.x; i < K * SK_CTL_WORDS; i += SK_CONTROL_SPAN) lds[i] = src[i];
  __syncthreads();
}

__device__ __forceinline__ bool sk_ctl_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// The stores of record `r` (in LDS) on voice v.  Returns the stores withheld by the two guards (0, 1 or 2).
__device__ __forceinline__ uint32_t sk_ctl_store(const sk_plane_ptrs_t &p, uint64_t *mask, int v, const uint32_t *r) {
  const uint32_t set = r[SK_CTL_SET];
  uint32_t withheld = 0;
  if (set & SK_CTL_LISTS) sk_list_voice(mask, v);
  if (set & (SK_CTL_PHASE_INC | SK_CTL_INC_SCALE | SK_CTL_AMP)) {
    uint4 o = *reinterpret_cast<const uint4 *>(&p.ro[SKP_OSC][v]);
    if (set & SK_CTL_PHASE_INC) o.x = r[SK_CTL_W_PHASE_INC];
    if (set & SK_CTL_INC_SCALE) {
      const uint32_t prod = __float_as_uint(__fmul_rn(__uint_as_float(o.x), __uint_as_float(r[SK_CTL_W_INC_SCALE])));
      if (sk_ctl_finite(prod)) o.x = prod; else ++withheld;
    }
    if (set & SK_CTL_AMP) {
      if (__uint_as_float(o.w) != 0.0f) o.w = r[SK_CTL_W_AMP]; else ++withheld;
    }
    *reinterpret_cast<uint4 *>(&p.ro[SKP_OSC][v]) = o;
  }
  if (set & SK_CTL_PAN) {
    uint4 m = *reinterpret_cast<const uint4 *>(&p.rw[SKS_MISC][v]);
    m.z = r[SK_CTL_W_PAN_LEFT]; m.w = r[SK_CTL_W_PAN_RIGHT];
    *reinterpret_cast<uint4 *>(&p.rw[SKS_MISC][v]) = m;
  }
  if (set & (SK_CTL_FILTER | SK_CTL_VELOCITY | SK_CTL_SMOOTHING)) {
    uint4 g = *reinterpret_cast<const uint4 *>(&p.ro[SKP_GAIN][v]);
    if (set & SK_CTL_VELOCITY) g.x = r[SK_CTL_W_VELOCITY];
    if (set & SK_CTL_SMOOTHING) g.y = r[SK_CTL_W_SMOOTHING];
    if (set & SK_CTL_FILTER) { g.z = r[SK_CTL_W_B0]; g.w = r[SK_CTL_W_B1]; }
    *reinterpret_cast<uint4 *>(&p.ro[SKP_GAIN][v]) = g;
  }
  if (set & (SK_CTL_FILTER | SK_CTL_CZ_DIST)) {
    uint4 f = *reinterpret_cast<const uint4 *>(&p.ro[SKP_FILT][v]);
    if (set & SK_CTL_FILTER) { f.x = r[SK_CTL_W_B2]; f.y = r[SK_CTL_W_A1]; f.z = r[SK_CTL_W_A2]; }
    if (set & SK_CTL_CZ_DIST) f.w = r[SK_CTL_W_CZ_DIST];
    *reinterpret_cast<uint4 *>(&p.ro[SKP_FILT][v]) = f;
  }
  if (set & SK_CTL_ENV_TIMES)                            // (all four words of the plane are named: nothing to read)
    *reinterpret_cast<uint4 *>(&p.ro[SKP_ENV_T][v]) = make_uint4(r[SK_CTL_W_ATTACK], r[SK_CTL_W_DECAY], r[SK_CTL_W_SUSTAIN], r[SK_CTL_W_RELEASE]);
  if (set & (SK_CTL_FM_DEPTH | SK_CTL_FREQ_SCALE | SK_CTL_AM_DEPTH | SK_CTL_PAN_DEPTH)) {
    uint4 d = *reinterpret_cast<const uint4 *>(&p.ro[SKP_MODF][v]);
    if (set & SK_CTL_FM_DEPTH) d.x = r[SK_CTL_W_FM_DEPTH];
    if (set & SK_CTL_FREQ_SCALE) d.y = r[SK_CTL_W_FREQ_SCALE];
    if (set & SK_CTL_AM_DEPTH) d.z = r[SK_CTL_W_AM_DEPTH];
    if (set & SK_CTL_PAN_DEPTH) d.w = r[SK_CTL_W_PAN_DEPTH];
    *reinterpret_cast<uint4 *>(&p.ro[SKP_MODF][v]) = d;
  }
  if (set & SK_CTL_CZ_DEPTH) {
    uint4 x = *reinterpret_cast<const uint4 *>(&p.ro[SKP_MODX][v]);
    x.x = r[SK_CTL_W_CZ_DEPTH];
    *reinterpret_cast<uint4 *>(&p.ro[SKP_MODX][v]) = x;
  }
  return withheld;
}

// d_result[0] += voices written, d_result[1] += stores withheld and -- N == 3, the guarded controllers -- d_result[2] += slots missed,
// over the workgroup (sums[N] in LDS; every thread arrives: __syncthreads inside).  A miss is the ordinary case under a guard (fifteen
// slots of sixteen on a 16-channel range), so it goes through LDS like the other two: at most N global atomics per workgroup
template <int N>
__device__ __forceinline__ void sk_ctl_count(uint32_t *sums, uint32_t *d_result, bool wrote, uint32_t withheld, bool missed = false) {
  static_assert(N == 2 || N == 3, "two counts, or three under a guard");
  const int tid = threadIdx.x;
  if (tid < N) sums[tid] = 0;
  __syncthreads();
  const uint32_t w = (uint32_t)__popcll(__ballot(wrote));
  const uint32_t h = (uint32_t)__popcll(__ballot(withheld >= 1)) + (uint32_t)__popcll(__ballot(withheld >= 2));
  const uint32_t m = N == 3 ? (uint32_t)__popcll(__ballot(missed)) : 0u;
  if ((tid & 63) == 0) {
    if (w) atomicAdd(&sums[0], w);
    if (h) atomicAdd(&sums[1], h);
    if (N == 3 && m) atomicAdd(&sums[2], m);
  }
  __syncthreads();
  if (d_result && tid < N && sums[tid]) atomicAdd(d_result + tid, sums[tid]);
}

#endif
