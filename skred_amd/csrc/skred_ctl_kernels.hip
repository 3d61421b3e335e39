// skred_ctl_kernels.hip -- patch controllers: a few parameter words of every copy of a tiled patch, changed on the device
// (gfx950 / CDNA4, wave64).
//
// skred_bank_ctl_range / skred_bank_ctl_slots (include/skred_amd.h).  A controller is K = slot_voices records, record l for voice l
// of a slot; a voice with bit l of voice_mask set receives the words its record names (sk_ctl_t: the `set` word) and nothing else.
//
//   sk_ctl_range_kernel   one lane per voice of [first, first + count), 256-thread workgroups, the grid sized from the range.  A
//                         wavefront's 64 lanes are 64 consecutive voices: every plane access is one coalesced 16-byte load or store
//                         per lane.  Bandwidth-bound: at most 7 planes * (16 read + 16 written) bytes per voice.
//   sk_ctl_slots_kernel   one lane per (entry, voice of the slot): the first min(n, *d_count) entries of a list in device memory,
//                         entries that are no slot of the bank skipped (sk_slot_valid: the rule of sk_slot_stamps_kernel).
//   sk_ctl_owned_kernel   sk_ctl_slots_kernel under the note-owner guard (skred_bank_ctl_owned): an entry whose owner word is not
//                         its tag is left alone and counted.
//
// All stage the K records in LDS once per workgroup (K * 96 bytes, 6 KiB at most) and share sk_ctl_store, the field stores
// (skred_ctl_common.hpp, shared with skred_expr_kernels.hip).  A
// plane that holds a named word is read, patched and written back whole (as sk_update_kernel patches the state planes); a plane
// without one is not touched.  Plain vector stores only.  No workgroup waits for another; the counts are integer sums (wave
// ballots, LDS, one atomic add per workgroup and count), so they do not depend on the order of arrival.
//
// The one piece of arithmetic is SK_CTL_INC_SCALE: ONE fp32 multiply (__fmul_rn: never contracted), whose product is stored only
// when it is finite -- the planner's class of a voice depends on that (skred_bank_update.c: SKC_EXOTIC).  SK_CTL_AMP is stored only
// where the voice's amp is not 0.0f: a voice that cannot sound stays one (SKC_LIVE, the packed lanes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"
#include "skred_ctl_common.hpp"      // sk_ctl_stage, sk_ctl_store, sk_ctl_count
#include "skred_update_common.hpp"   // sk_entry_decode, sk_entry_owned, sk_range_lane, sk_batch_done, the launch helpers

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_ctl_range_kernel(const sk_ctl_t *__restrict__ recs, int K, uint64_t voice_mask,
                                                                   int first, int count, sk_plane_ptrs_t p, uint64_t *mask,
                                                                   uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t lds[64 * SK_CTL_WORDS];
  __shared__ uint32_t sums[2];
  sk_ctl_stage(lds, recs, K);
  const sk_lane_t t = sk_range_lane(first, count, K);
  const bool mine = t.in_range && ((voice_mask >> t.l) & 1);
  uint32_t withheld = 0;
  if (mine) withheld = sk_ctl_store(p, mask, t.v, lds + t.l * SK_CTL_WORDS);
  sk_ctl_count<2>(sums, d_result, mine, withheld);
  sk_batch_done(cnt, done, seq);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_ctl_slots_kernel(const sk_ctl_t *__restrict__ recs, int k_shift, uint64_t voice_mask,
                                                                   const int32_t *d_slots, int n, const uint32_t *d_count, int n_voices,
                                                                   sk_plane_ptrs_t p, uint64_t *mask, uint32_t *d_result,
                                                                   uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t lds[64 * SK_CTL_WORDS];
  __shared__ uint32_t sums[2];
  sk_ctl_stage(lds, recs, 1 << k_shift);
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);
  const bool mine = t.valid && ((voice_mask >> t.l) & 1);
  uint32_t withheld = 0;
  if (mine) withheld = sk_ctl_store(p, mask, t.e + t.l, lds + t.l * SK_CTL_WORDS);
  sk_ctl_count<2>(sums, d_result, mine, withheld);
  sk_batch_done(cnt, done, seq);
}

// sk_ctl_slots_kernel under the note-owner guard (skred_bank_ctl_owned; skred_owner_kernels.hip has the array's rules): an entry
// receives the controller only when owner[entry] equals its (non-zero) tag.  d_result[2] += the entries whose owner differs, counted
// by the threads of voice 0 (sk_ctl_count's third sum).
__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_ctl_owned_kernel(const sk_ctl_t *__restrict__ recs, int k_shift, uint64_t voice_mask,
                                                                   const int32_t *d_slots, const uint32_t *__restrict__ tags,
                                                                   const uint32_t *__restrict__ owner, int n, const uint32_t *d_count,
                                                                   int n_voices, sk_plane_ptrs_t p, uint64_t *mask, uint32_t *d_result,
                                                                   uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t lds[64 * SK_CTL_WORDS];
  __shared__ uint32_t sums[3];
  sk_ctl_stage(lds, recs, 1 << k_shift);
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);
  const bool owned = sk_entry_owned(owner, tags, t);
  const bool mine = owned && ((voice_mask >> t.l) & 1);
  uint32_t withheld = 0;
  if (mine) withheld = sk_ctl_store(p, mask, t.e + t.l, lds + t.l * SK_CTL_WORDS);
  sk_ctl_count<3>(sums, d_result, mine, withheld, t.valid && !owned && t.l == 0);
  sk_batch_done(cnt, done, seq);
}

extern "C" int sk_launch_ctl_range(const sk_ctl_t *d_recs, int slot_voices, uint64_t voice_mask, int first, int count,
                                   sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t *mask,
                                   uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 2, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  hipLaunchKernelGGL(sk_ctl_range_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, d_recs, slot_voices, voice_mask, first, count, p,
                     mask, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_ctl_slots(const sk_ctl_t *d_recs, int slot_voices, uint64_t voice_mask, const int32_t *d_slots, int n,
                                   const uint32_t *d_count, int n_voices, sk_plane_t *const ro[SKP_COUNT],
                                   sk_plane_t *const rw[SKS_COUNT], uint64_t *mask, uint32_t *d_result, uint32_t *cnt, uint32_t *done,
                                   uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 2, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_ctl_slots_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, d_recs, sh, voice_mask, d_slots, n, d_count, n_voices,
                     p, mask, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_ctl_owned(const sk_ctl_t *d_recs, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                                   const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count, int n_voices,
                                   sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t *mask, uint32_t *d_result,
                                   uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 3, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_ctl_owned_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, d_recs, sh, voice_mask, d_slots, d_tags, owner, n,
                     d_count, n_voices, p, mask, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}
