// skred_fx_ctl_common.hpp -- what the fixed-point bank's control kernels share (skred_fx_live_kernels.hip: sk_fx_stamp_list_kernel;
// skred_fx_owner_kernels.hip: the guarded stamp; skred_fx_ctl_kernels.hip: the controllers; skred_fx_expr_kernels.hip: the masked
// matches and the per-entry controller; skred_fx_pedal_kernels.hip: the pedals): the stamp's stores, the controller's stores, the list
// bound, the counting, the launch grid.
#ifndef SKRED_FX_CTL_COMMON_HPP
#define SKRED_FX_CTL_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_layout.h"

// the public stamp bits (include/skred_amd.h: SKRED_STAMP_TRIGGER / _RELEASE; checked against the header in skred_fx_live.c)
enum { SKXS_STAMP_TRIGGER = 1u << 8, SKXS_STAMP_RELEASE = 1u << 9 };

// The stamps on voice v, as sk_fx_stamp_kernel applies them: the trigger first, then the release if the envelope is (now) active.
__device__ __forceinline__ void skx_stamp_store(skx_plane_t *time_plane, skx_plane_t *rw0, int v, uint32_t stamps, uint64_t now) {
  uint4 t = *reinterpret_cast<const uint4 *>(&time_plane[v]);
  uint32_t *flags = &rw0[v].w[3];
  uint32_t f = *flags;
  if (stamps & SKXS_STAMP_TRIGGER) { t.x = (uint32_t)now; t.y = (uint32_t)(now >> 32); t.z = 0; t.w = 0; f |= SKXR_ACTIVE; }
  if ((stamps & SKXS_STAMP_RELEASE) && (f & SKXR_ACTIVE)) { t.z = (uint32_t)now; t.w = (uint32_t)(now >> 32); }
  *reinterpret_cast<uint4 *>(&time_plane[v]) = t;
  *flags = f;
}

// entry i of a list in device memory: looked at when it lies below min(n, *d_count)
__device__ __forceinline__ bool skx_list_looked(int64_t i, int n, const uint32_t *d_count) {
  return i < n && !(d_count && (uint64_t)i >= (uint64_t)d_count[0]);
}

// d_result[k] += the workgroup's sum of val[k] (each 0, 1 or 2 per thread), k < N: wave ballots, LDS, one atomic add per workgroup
// and count -- integer sums, the same whatever the order of arrival.  Every thread of the workgroup arrives (__syncthreads inside).
template <int N>
__device__ __forceinline__ void skx_count(uint32_t *sums, uint32_t *d_result, const uint32_t (&val)[N]) {
  const int tid = threadIdx.x;
  if (tid < N) sums[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const uint32_t c = (uint32_t)__popcll(__ballot(val[k] >= 1u)) + (uint32_t)__popcll(__ballot(val[k] >= 2u));
    if ((tid & 63) == 0 && c) atomicAdd(&sums[k], c);
  }
  __syncthreads();
  if (d_result && tid < N && sums[tid]) atomicAdd(d_result + tid, sums[tid]);
}

// the public bit values (include/skred_amd.h: SKRED_CTL_*; checked against the header in skred_fx_ctl.c); one store for
// skred_fx_ctl_kernels.hip and skred_fx_expr_kernels.hip
enum { SKX_C_PHASE_INC = 1u << 0, SKX_C_INC_SCALE = 1u << 1, SKX_C_AMP = 1u << 2, SKX_C_PAN = 1u << 3, SKX_C_FILTER = 1u << 4,
       SKX_C_ENV_TIMES = 1u << 5, SKX_C_VELOCITY = 1u << 6, SKX_C_SMOOTHING = 1u << 7 };

struct skx_ctl_planes_t {
  skx_plane_t *osc, *gain, *env, *recip, *filt, *filt2;
};

// (host) workgroups of SKX_CTL_SPAN threads, one thread per voice or entry (the expression kernels' SKX_EXPR_SPAN is the same number:
// skred_fx_expr_kernels.hip asserts it)
static inline unsigned skx_grid(long long lanes) { return (unsigned)((lanes + SKX_CTL_SPAN - 1) / SKX_CTL_SPAN); }

// (host) the planes a controller can store to, out of the bank's array
static inline void skx_ctl_planes(skx_ctl_planes_t &p, skx_plane_t *const ro[SKX_COUNT]) {
  p.osc = ro[SKX_OSC]; p.gain = ro[SKX_GAIN]; p.env = ro[SKX_ENV]; p.recip = ro[SKX_RECIP]; p.filt = ro[SKX_FILT]; p.filt2 = ro[SKX_FILT2];
}

// The stores of record r on voice v.  Returns the stores withheld by the two guards (0, 1 or 2).
__device__ __forceinline__ uint32_t skx_ctl_store(const skx_ctl_planes_t &p, int v, const uint32_t *__restrict__ r) {
  const uint32_t which = r[SKX_CTL_WHICH];
  uint32_t withheld = 0;
  if (which & (SKX_C_PHASE_INC | SKX_C_INC_SCALE | SKX_C_AMP)) {
    uint4 o = *reinterpret_cast<const uint4 *>(&p.osc[v]);          // w[1] the table offset, w[2] log2_size and the flags: kept
    if (which & SKX_C_PHASE_INC) o.x = r[SKX_CTL_PHASE_INC];
    if (which & SKX_C_INC_SCALE) {
      const uint64_t prod = ((uint64_t)o.x * (uint64_t)r[SKX_CTL_INC_SCALE]) >> 16;
      if (prod <= 0xFFFFFFFFull) o.x = (uint32_t)prod; else ++withheld;
    }
    if (which & SKX_C_AMP) {
      if (o.w != 0u) o.w = r[SKX_CTL_AMP]; else ++withheld;
    }
    *reinterpret_cast<uint4 *>(&p.osc[v]) = o;
  }
  if (which & (SKX_C_PAN | SKX_C_VELOCITY | SKX_C_SMOOTHING)) {
    uint4 g = *reinterpret_cast<const uint4 *>(&p.gain[v]);
    if (which & SKX_C_PAN) { g.x = r[SKX_CTL_PAN_LEFT]; g.y = r[SKX_CTL_PAN_RIGHT]; }
    if (which & SKX_C_SMOOTHING) g.z = r[SKX_CTL_SMOOTHING];
    if (which & SKX_C_VELOCITY) g.w = r[SKX_CTL_VELOCITY];
    *reinterpret_cast<uint4 *>(&p.gain[v]) = g;
  }
  if (which & SKX_C_FILTER) {                                          // (all four words of SKX_FILT are named: nothing to read)
    *reinterpret_cast<uint4 *>(&p.filt[v]) = make_uint4(r[SKX_CTL_B0], r[SKX_CTL_B1], r[SKX_CTL_B2], r[SKX_CTL_A1]);
    p.filt2[v].w[0] = r[SKX_CTL_A2];
  }
  if (which & SKX_C_ENV_TIMES) {
    *reinterpret_cast<uint4 *>(&p.env[v]) = make_uint4(r[SKX_CTL_ATTACK], r[SKX_CTL_DECAY], r[SKX_CTL_RELEASE], r[SKX_CTL_SUSTAIN]);
    *reinterpret_cast<uint2 *>(&p.recip[v].w[0]) = make_uint2(r[SKX_CTL_RECIP_A], r[SKX_CTL_RECIP_D]);
    p.recip[v].w[2] = r[SKX_CTL_RECIP_R];
  }
  return withheld;
}

#endif
