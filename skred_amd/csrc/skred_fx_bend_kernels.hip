// skred_fx_bend_kernels.hip -- the pitch wheel of the fixed-point bank: bends that return to the key's bits and compose with glides,
// in integers (gfx950 / CDNA4, wave64).
//
// skred_fxbank_bend_match / _bend_owned_each / _bend_tags_each / _bend_clear (include/skred_amd_fxpt.h has the definition).
// bend[n_voices] lies beside the glide array of skred_fx_glide.c: two words per voice -- key (the unbent phase_inc; 0: not bent) and
// ratio_q24.  Only these kernels, the BEND instantiations of skred_fx_glide_kernels.hip and the float bank's sk_bend_clear_kernel
// (entered through its launcher at slot_voices = 1 behind every tag launch of a bank that has the array) read or write it; no render
// kernel knows it exists.  The one bank word they store is phase_inc (SKX_OSC word 0), as a word store: the neighbours in the plane
// keep their bits.
//
//   sk_fx_bend_match_kernel        sk_fx_ctl_match_kernel's geometry and guard (one thread per voice of the range, the voice's owner
//                                  word against the masked match: one coalesced 4-byte load per lane): THE RULE (skx_bend_apply) to one
//                                  ratio, a kernel argument.
//   sk_fx_bend_each_kernel         sk_fx_glide_start_kernel's geometry and guard (one thread per entry of a list in device memory, the
//                                  owner word against the entry's tag); lane k reads ratio k: consecutive lanes, consecutive words.
//   sk_fx_bend_range_clear_kernel  one thread per voice of the range: the words cleared, with snap the key stored first.
//
// THE RULE is one 32 x 32 -> 64-bit product and a shift by 24: exact integer arithmetic, the same bits on every machine.  Counts are
// sk_owner_count's: wave ballots, LDS, at most one atomic add per workgroup and count -- integer sums, the same whatever the order of
// arrival.  Plain vector stores and ordinary atomics only; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_layout.h"
#include "skred_launch.h"
#include "skred_update_common.hpp"   // sk_entry_decode, sk_entry_owned, sk_range_lane, sk_owner_count, sk_grid, sk_list_grid, sk_result_clear

static_assert(sizeof(skx_bend_t) == 8, "one 8-byte load per voice");

// THE RULE on voice v.  Returns 1: stored or restored, 2: withheld, 0: neither (the centre on a voice that was not bent)
__device__ __forceinline__ int skx_bend_apply(skx_bend_t *bend, skx_plane_t *osc, int v, uint32_t ratio) {
  const uint2 b = *reinterpret_cast<const uint2 *>(&bend[v]);            // key, ratio_q24
  uint32_t *inc = &osc[v].w[0];
  if (ratio == SKX_BEND_ONE) {
    if (b.x) *inc = b.x;
    if (b.x | b.y) *reinterpret_cast<uint2 *>(&bend[v]) = make_uint2(0u, 0u);
    return b.x ? 1 : 0;
  }
  const uint32_t k = b.x ? b.x : *inc;
  const uint64_t p = ((uint64_t)k * (uint64_t)ratio) >> 24;             // (k == 0 gives p == 0)
  if (p < 1ull || p > 0xFFFFFFFFull) return 2;
  *inc = (uint32_t)p;
  *reinterpret_cast<uint2 *>(&bend[v]) = make_uint2(k, ratio);
  return 1;
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_bend_match_kernel(skx_bend_t *bend, uint32_t ratio, int first, int count,
                                                                         const uint32_t *__restrict__ owner, uint32_t value, uint32_t omask,
                                                                         skx_plane_t *osc, uint32_t *d_result) {
  __shared__ uint32_t sums[3];
  const sk_lane_t t = sk_range_lane(first, count, 1);                    // (inside the bank: checked on the host)
  const bool hit = t.in_range && sk_owner_matches(owner[t.v], value, omask);
  int did = 0;
  if (hit) did = skx_bend_apply(bend, osc, t.v, ratio);
  const bool flag[3] = { did == 1, did == 2, t.in_range && !hit };
  sk_owner_count<3>(sums, d_result, flag);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_bend_each_kernel(skx_bend_t *bend, const uint32_t *__restrict__ ratios,
                                                                        const int32_t *d_voices, const uint32_t *__restrict__ tags,
                                                                        const uint32_t *__restrict__ owner, int n, const uint32_t *d_count,
                                                                        int n_voices, skx_plane_t *osc, uint32_t *d_result) {
  __shared__ uint32_t sums[3];
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, 0, d_voices, n, d_count, n_voices);   // (valid: 0 <= t.e < n_voices)
  const bool owned = sk_entry_owned(owner, tags, t);
  int did = 0;
  if (owned) did = skx_bend_apply(bend, osc, t.e, ratios[t.i]);
  const bool flag[3] = { did == 1, did == 2, t.valid && !owned };
  sk_owner_count<3>(sums, d_result, flag);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_bend_range_clear_kernel(skx_bend_t *bend, skx_plane_t *osc, int first, int count,
                                                                               int snap) {
  const int64_t off = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  if (off >= count) return;
  const int v = first + (int)off;                                        // (inside the bank: checked on the host)
  const uint2 b = *reinterpret_cast<const uint2 *>(&bend[v]);
  if (!(b.x | b.y)) return;
  if (snap && b.x) osc[v].w[0] = b.x;
  *reinterpret_cast<uint2 *>(&bend[v]) = make_uint2(0u, 0u);
}

// d_result[3] (or NULL; zeroed on `stream` ahead of the kernel): voices stored or restored, bends withheld, voices of the range that
// did not match
extern "C" int skx_launch_bend_match(skx_bend_t *bend, uint32_t ratio_q24, int first, int count, const uint32_t *owner, uint32_t value,
                                     uint32_t mask, skx_plane_t *osc, uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 3, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_fx_bend_match_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, bend, ratio_q24, first, count, owner,
                     value, mask, osc, d_result);
  return (int)hipGetLastError();
}

// d_result[3] as above, [2]: voices whose owner differs
extern "C" int skx_launch_bend_each(skx_bend_t *bend, const uint32_t *d_ratios, const int32_t *d_voices, const uint32_t *d_tags,
                                    const uint32_t *owner, int n, const uint32_t *d_count, int n_voices, skx_plane_t *osc,
                                    uint32_t *d_result, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 3, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_fx_bend_each_kernel, dim3(sk_list_grid(n, 0)), dim3(SK_CONTROL_SPAN), 0, stream, bend, d_ratios, d_voices, d_tags,
                     owner, n, d_count, n_voices, osc, d_result);
  return (int)hipGetLastError();
}

extern "C" int skx_launch_bend_range_clear(skx_bend_t *bend, skx_plane_t *osc, int first, int count, int snap, hipStream_t stream) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL(sk_fx_bend_range_clear_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, bend, osc, first, count, snap);
  return (int)hipGetLastError();
}
