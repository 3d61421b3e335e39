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
// without one is not touched.  Plain vector stores only.  No workgroup waits for another; the two counts are integer sums (wave
// ballots, LDS, one atomic add per workgroup and count), so they do not depend on the order of arrival.
//
// The one piece of arithmetic is SK_CTL_INC_SCALE: ONE fp32 multiply (__fmul_rn: never contracted), whose product is stored only
// when it is finite -- the planner's class of a voice depends on that (skred_bank_update.c: SKC_EXOTIC).  SK_CTL_AMP is stored only
// where the voice's amp is not 0.0f: a voice that cannot sound stays one (SKC_LIVE, the packed lanes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"
#include "skred_ctl_common.hpp"      // SK_CTL_SPAN, sk_ctl_stage, sk_ctl_store, sk_ctl_count
#include "skred_update_common.hpp"   // sk_plane_ptrs_t, sk_slot_valid, sk_batch_done

__global__ __launch_bounds__(SK_CTL_SPAN) void sk_ctl_range_kernel(const sk_ctl_t *__restrict__ recs, int K, uint64_t voice_mask,
                                                                   int first, int count, sk_plane_ptrs_t p, uint64_t *mask,
                                                                   uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t lds[64 * SK_CTL_WORDS];
  __shared__ uint32_t sums[2];
  sk_ctl_stage(lds, recs, K);
  const int64_t off = (int64_t)blockIdx.x * SK_CTL_SPAN + threadIdx.x;
  const int v = first + (int)(off < count ? off : 0), l = v & (K - 1);     // (first is a multiple of K)
  const bool mine = off < count && ((voice_mask >> l) & 1);
  uint32_t withheld = 0;
  if (mine) withheld = sk_ctl_store(p, mask, v, lds + l * SK_CTL_WORDS);
  sk_ctl_count(sums, d_result, mine, withheld);
  sk_batch_done(cnt, done, seq);
}

__global__ __launch_bounds__(SK_CTL_SPAN) void sk_ctl_slots_kernel(const sk_ctl_t *__restrict__ recs, int k_shift, uint64_t voice_mask,
                                                                   const int32_t *d_slots, int n, const uint32_t *d_count, int n_voices,
                                                                   sk_plane_ptrs_t p, uint64_t *mask, uint32_t *d_result,
                                                                   uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t lds[64 * SK_CTL_WORDS];
  __shared__ uint32_t sums[2];
  const int K = 1 << k_shift;
  sk_ctl_stage(lds, recs, K);
  const int64_t i = (int64_t)blockIdx.x * (SK_CTL_SPAN >> k_shift) + ((int)threadIdx.x >> k_shift);
  const int l = (int)threadIdx.x & (K - 1);
  bool mine = i < n && ((voice_mask >> l) & 1);
  if (mine && d_count && (uint64_t)i >= (uint64_t)d_count[0]) mine = false;
  int e = 0;
  if (mine) {
    e = d_slots[i];
    mine = sk_slot_valid(e, K, n_voices);
  }
  uint32_t withheld = 0;
  if (mine) withheld = sk_ctl_store(p, mask, e + l, lds + l * SK_CTL_WORDS);
  sk_ctl_count(sums, d_result, mine, withheld);
  sk_batch_done(cnt, done, seq);
}

// sk_ctl_slots_kernel under the note-owner guard (skred_bank_ctl_owned; skred_owner_kernels.hip has the array's rules): an entry
// receives the controller only when owner[entry] equals its (non-zero) tag.  d_result[2] += the entries whose owner differs, counted
// by the threads of voice 0: one atomic add per wave that saw any.
__global__ __launch_bounds__(SK_CTL_SPAN) void sk_ctl_owned_kernel(const sk_ctl_t *__restrict__ recs, int k_shift, uint64_t voice_mask,
                                                                   const int32_t *d_slots, const uint32_t *__restrict__ tags,
                                                                   const uint32_t *__restrict__ owner, int n, const uint32_t *d_count,
                                                                   int n_voices, sk_plane_ptrs_t p, uint64_t *mask, uint32_t *d_result,
                                                                   uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t lds[64 * SK_CTL_WORDS];
  __shared__ uint32_t sums[2];
  const int K = 1 << k_shift;
  sk_ctl_stage(lds, recs, K);
  const int64_t i = (int64_t)blockIdx.x * (SK_CTL_SPAN >> k_shift) + ((int)threadIdx.x >> k_shift);
  const int l = (int)threadIdx.x & (K - 1);
  bool looked = i < n;
  if (looked && d_count && (uint64_t)i >= (uint64_t)d_count[0]) looked = false;
  int e = 0;
  bool valid = false, owned = false;
  if (looked) {
    e = d_slots[i];
    valid = sk_slot_valid(e, K, n_voices);
    if (valid) owned = owner[e] == tags[i];
  }
  const bool mine = owned && ((voice_mask >> l) & 1);
  uint32_t withheld = 0;
  if (mine) withheld = sk_ctl_store(p, mask, e + l, lds + l * SK_CTL_WORDS);
  sk_ctl_count(sums, d_result, mine, withheld);
  const uint32_t missed = (uint32_t)__popcll(__ballot(valid && !owned && l == 0));
  if (d_result && ((int)threadIdx.x & 63) == 0 && missed) atomicAdd(d_result + 2, missed);
  sk_batch_done(cnt, done, seq);
}

static void sk_ctl_planes(sk_plane_ptrs_t &p, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT]) {
  for (int k = 0; k < SKP_COUNT; ++k) p.ro[k] = ro[k];
  for (int k = 0; k < SKS_COUNT; ++k) p.rw[k] = rw[k];
}

static hipError_t sk_ctl_clear(uint32_t *d_result, hipStream_t stream) {
  return d_result ? hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), stream) : hipSuccess;
}

extern "C" int sk_launch_ctl_range(const sk_ctl_t *d_recs, int slot_voices, uint64_t voice_mask, int first, int count,
                                   sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t *mask,
                                   uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_ctl_clear(d_result, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_ctl_planes(p, ro, rw);
  const unsigned n_wg = (unsigned)(((long long)count + SK_CTL_SPAN - 1) / SK_CTL_SPAN);
  hipLaunchKernelGGL(sk_ctl_range_kernel, dim3(n_wg), dim3(SK_CTL_SPAN), 0, stream, d_recs, slot_voices, voice_mask, first, count, p,
                     mask, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_ctl_slots(const sk_ctl_t *d_recs, int slot_voices, uint64_t voice_mask, const int32_t *d_slots, int n,
                                   const uint32_t *d_count, int n_voices, sk_plane_t *const ro[SKP_COUNT],
                                   sk_plane_t *const rw[SKS_COUNT], uint64_t *mask, uint32_t *d_result, uint32_t *cnt, uint32_t *done,
                                   uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_ctl_clear(d_result, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_ctl_planes(p, ro, rw);
  int sh = 0;
  while ((1 << sh) < slot_voices) ++sh;
  const int per_wg = SK_CTL_SPAN >> sh;
  const unsigned n_wg = (unsigned)(((long long)n + per_wg - 1) / per_wg);
  hipLaunchKernelGGL(sk_ctl_slots_kernel, dim3(n_wg), dim3(SK_CTL_SPAN), 0, stream, d_recs, sh, voice_mask, d_slots, n, d_count, n_voices,
                     p, mask, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_ctl_owned(const sk_ctl_t *d_recs, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                                   const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count, int n_voices,
                                   sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t *mask, uint32_t *d_result,
                                   uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  if (d_result) {
    const hipError_t e = hipMemsetAsync(d_result, 0, 3 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
  }
  sk_plane_ptrs_t p;
  sk_ctl_planes(p, ro, rw);
  int sh = 0;
  while ((1 << sh) < slot_voices) ++sh;
  const int per_wg = SK_CTL_SPAN >> sh;
  const unsigned n_wg = (unsigned)(((long long)n + per_wg - 1) / per_wg);
  hipLaunchKernelGGL(sk_ctl_owned_kernel, dim3(n_wg), dim3(SK_CTL_SPAN), 0, stream, d_recs, sh, voice_mask, d_slots, d_tags, owner, n,
                     d_count, n_voices, p, mask, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}
