// skred_fx_ctl_common.hpp -- what the fixed-point bank's list kernels share (skred_fx_live_kernels.hip: sk_fx_stamp_list_kernel;
// skred_fx_owner_kernels.hip: the guarded stamp; skred_fx_ctl_kernels.hip: the controllers).
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

#endif
