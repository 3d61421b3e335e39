// skred_bend_kernels.hip -- the pitch wheel: bends that return to the key's bits and compose with glides (gfx950 / CDNA4, wave64).
//
// skred_bank_bend_match / _bend_owned_each / _bend_tags_each / _bend_clear (include/skred_amd.h has the definition).  bend[n_voices]
// lies beside the glide array: two words per voice -- key (the unbent increment's bits; 0: not bent) and ratio.  Only these kernels
// and the BEND instantiations of skred_glide_kernels.hip read or write it; no render kernel knows it exists.  The one plane word they
// store is voice_phase_inc (SKP_OSC word 0), as a word store: the neighbours keep what they hold.
//
//   sk_bend_clear_kernel        sk_glide_clear_kernel on this array: one thread per voice of a listed slot, bend[slot + l] = 0.
//                               Launched behind every tag launch of a bank that has a bend array.
//   sk_bend_match_kernel        sk_ctl_match_kernel's geometry, guard and counting (one thread per voice of the range, the slot's
//                               owner word against the masked match): THE RULE (sk_bend_apply) to one ratio, a kernel argument.
//   sk_bend_each_kernel         sk_glide_start_kernel's geometry and guard (one thread per entry and voice of the slot, the owner word
//                               against the entry's tag), the workgroup's ratios staged in LDS (one load per entry, not one per voice).
//   sk_bend_range_clear_kernel  one thread per voice of the range: the words cleared, with snap the key stored first.
//
// Counts are sk_owner_count's: integer sums, the same whatever the order of arrival.  Plain vector stores and ordinary atomics only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"
#include "skred_update_common.hpp"   // sk_entry_decode, sk_entry_owned, sk_range_lane, sk_owner_count, sk_batch_done, the launch helpers

#define SK_BEND_ONE 0x3f800000u        // the bits of 1.0f: the wheel at centre

// finite and not zero: a key a bend can multiply, a product it can store
__device__ __forceinline__ bool sk_bend_usable(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u && (bits & 0x7fffffffu) != 0u; }

// THE RULE on voice v.  Returns 1: stored or restored, 2: withheld, 0: neither (the centre on a voice that was not bent)
__device__ __forceinline__ int sk_bend_apply(sk_bend_t *bend, sk_plane_t *osc, int v, uint32_t ratio) {
  const uint2 b = *reinterpret_cast<const uint2 *>(&bend[v]);            // key, ratio
  uint32_t *inc = &osc[v].w[0];
  if (ratio == SK_BEND_ONE) {
    if (b.x) *inc = b.x;
    if (b.x | b.y) *reinterpret_cast<uint2 *>(&bend[v]) = make_uint2(0u, 0u);
    return b.x ? 1 : 0;
  }
  const uint32_t k = b.x ? b.x : *inc;
  const uint32_t p = __float_as_uint(__fmul_rn(__uint_as_float(k), __uint_as_float(ratio)));
  if (!sk_bend_usable(k) || !sk_bend_usable(p)) return 2;
  *inc = p;
  *reinterpret_cast<uint2 *>(&bend[v]) = make_uint2(k, ratio);
  return 1;
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_bend_clear_kernel(sk_bend_t *bend, const int32_t *d_slots, int n, const uint32_t *d_count,
                                                                      int k_shift, int n_voices) {
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);
  if (t.valid) *reinterpret_cast<uint2 *>(&bend[t.e + t.l]) = make_uint2(0u, 0u);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_bend_match_kernel(sk_bend_t *bend, uint32_t ratio, int K, uint64_t voice_mask, int first,
                                                                      int count, const uint32_t *__restrict__ owner, uint32_t value,
                                                                      uint32_t omask, sk_plane_t *osc, uint32_t *d_result) {
  __shared__ uint32_t sums[3];
  const sk_lane_t t = sk_range_lane(first, count, K);
  const bool hit = t.in_range && sk_owner_matches(owner[t.v - t.l], value, omask);
  int did = 0;
  if (hit && ((voice_mask >> t.l) & 1)) did = sk_bend_apply(bend, osc, t.v, ratio);
  const bool flag[3] = { did == 1, did == 2, t.head && !hit };
  sk_owner_count<3>(sums, d_result, flag);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_bend_each_kernel(sk_bend_t *bend, const uint32_t *__restrict__ ratios, int k_shift,
                                                                     uint64_t voice_mask, const int32_t *d_slots,
                                                                     const uint32_t *__restrict__ tags, const uint32_t *__restrict__ owner,
                                                                     int n, const uint32_t *d_count, int n_voices, sk_plane_t *osc,
                                                                     uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t ent[SK_CONTROL_SPAN];                              // the ratios of this workgroup's entries
  __shared__ uint32_t sums[3];
  const int per_wg = SK_CONTROL_SPAN >> k_shift;
  const int64_t base = (int64_t)blockIdx.x * per_wg;
  if ((int)threadIdx.x < per_wg && base + (int)threadIdx.x < n) ent[threadIdx.x] = ratios[base + (int)threadIdx.x];
  __syncthreads();
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);   // (t.i == base + the entry's place)
  const bool owned = sk_entry_owned(owner, tags, t);
  int did = 0;
  if (owned && ((voice_mask >> t.l) & 1)) did = sk_bend_apply(bend, osc, t.e + t.l, ent[(int)threadIdx.x >> k_shift]);
  const bool flag[3] = { did == 1, did == 2, t.valid && !owned && t.l == 0 };
  sk_owner_count<3>(sums, d_result, flag);
  sk_batch_done(cnt, done, seq);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_bend_range_clear_kernel(sk_bend_t *bend, sk_plane_t *osc, int first, int count, int snap) {
  const int64_t off = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  if (off >= count) return;
  const int v = first + (int)off;
  const uint2 b = *reinterpret_cast<const uint2 *>(&bend[v]);
  if (!(b.x | b.y)) return;
  if (snap && b.x) osc[v].w[0] = b.x;
  *reinterpret_cast<uint2 *>(&bend[v]) = make_uint2(0u, 0u);
}

extern "C" int sk_launch_bend_clear(sk_bend_t *bend, const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices, int n_voices,
                                    hipStream_t stream) {
  if (n <= 0) return 0;
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_bend_clear_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, bend, d_slots, n, d_count, sh,
                     n_voices);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_bend_match(sk_bend_t *bend, uint32_t ratio, int slot_voices, uint64_t voice_mask, int first, int count,
                                    const uint32_t *owner, uint32_t value, uint32_t mask, sk_plane_t *osc, uint32_t *d_result,
                                    hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 3, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_bend_match_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, bend, ratio, slot_voices, voice_mask, first,
                     count, owner, value, mask, osc, d_result);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_bend_each(sk_bend_t *bend, const uint32_t *d_ratios, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                                   const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count, int n_voices,
                                   sk_plane_t *osc, uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 3, stream);
  if (e != hipSuccess) return (int)e;
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_bend_each_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, bend, d_ratios, sh, voice_mask, d_slots,
                     d_tags, owner, n, d_count, n_voices, osc, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_bend_range_clear(sk_bend_t *bend, sk_plane_t *osc, int first, int count, int snap, hipStream_t stream) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL(sk_bend_range_clear_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, bend, osc, first, count, snap);
  return (int)hipGetLastError();
}
