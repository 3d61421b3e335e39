// skred_fx_owner_kernels.hip -- note owners of the fixed-point bank: the stamp that only lands where the owner word is the expected
// one (gfx950 / CDNA4, wave64).
//
// skred_fxbank_stamp_owned / _release_tags (include/skred_amd_fxpt.h).  owner[n_voices] holds one tag per voice, 0 for nobody.  The
// tag and the find pass know nothing of a bank's planes: the fixed-point bank enters the float bank's sk_owner_tag_kernel and
// sk_owner_find_kernel through their launchers (skred_owner_kernels.hip, slot_voices = 1, no batch-done word: this bank's staging
// ring guards a slot with an event).  Only the guarded stamp reads the planes, so only it is new:
//
//   sk_fx_stamp_owned_kernel  sk_fx_stamp_list_kernel (one lane per entry of a list in device memory, skx_stamp_store's stores) with
//                             the guard owner[voice] == tag.  Stamped / stolen / no-voice entries are counted: wave ballots, LDS,
//                             one atomic add per workgroup and count -- integer sums.
//
// Plain vector stores and ordinary atomics only.  The owner words a launch reads are never written by that launch; no render kernel
// knows the array exists.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_ctl_common.hpp"   // skx_stamp_store, skx_list_looked, skx_count
#include "skred_fx_layout.h"

__global__ __launch_bounds__(SKX_CTL_SPAN) void sk_fx_stamp_owned_kernel(const uint32_t *__restrict__ owner, const int32_t *d_voices,
                                                                         const uint32_t *__restrict__ tags, int n, const uint32_t *d_count,
                                                                         int n_voices, uint32_t stamps, skx_plane_t *time_plane,
                                                                         skx_plane_t *rw0, uint64_t now, uint32_t *d_result) {
  __shared__ uint32_t sums[3];
  const int64_t i = (int64_t)blockIdx.x * SKX_CTL_SPAN + threadIdx.x;
  const bool looked = skx_list_looked(i, n, d_count);
  bool valid = false, mine = false;
  if (looked) {
    const int v = d_voices[i];
    valid = v >= 0 && v < n_voices;
    if (valid) mine = owner[v] == tags[i];                              // (tags are non-zero: an untagged voice never matches)
    if (mine) skx_stamp_store(time_plane, rw0, v, stamps, now);
  }
  const uint32_t val[3] = { mine ? 1u : 0u, (valid && !mine) ? 1u : 0u, (looked && !valid) ? 1u : 0u };
  skx_count<3>(sums, d_result, val);
}

extern "C" int skx_launch_stamp_owned(const uint32_t *owner, const int32_t *d_voices, const uint32_t *d_tags, int n, const uint32_t *d_count,
                                      int n_voices, uint32_t stamps, skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now,
                                      uint32_t *d_result, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = hipMemsetAsync(d_result, 0, 3 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return (int)e;
  const unsigned n_wg = (unsigned)(((long long)n + SKX_CTL_SPAN - 1) / SKX_CTL_SPAN);
  hipLaunchKernelGGL(sk_fx_stamp_owned_kernel, dim3(n_wg), dim3(SKX_CTL_SPAN), 0, stream, owner, d_voices, d_tags, n, d_count, n_voices,
                     stamps, time_plane, rw0, now, d_result);
  return (int)hipGetLastError();
}
