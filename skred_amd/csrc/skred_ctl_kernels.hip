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
// All stage the K records in LDS once per workgroup (K * 96 bytes, 6 KiB at most) and share sk_ctl_store, the field stores.  A
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
#include "skred_update_common.hpp"   // sk_plane_ptrs_t, sk_list_voice, sk_slot_valid, sk_batch_done

#define SK_CTL_SPAN 256

// the K records -> LDS (the unmasked ones arrive zeroed by the host: set == 0)
__device__ __forceinline__ void sk_ctl_stage(uint32_t *lds, const sk_ctl_t *__restrict__ recs, int K) {
  const uint32_t *src = reinterpret_cast<const uint32_t *>(recs);
  for (int i = threadIdx.x; i < K * SK_CTL_WORDS; i += SK_CTL_SPAN) lds[i] = src[i];
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

// d_result[0] += voices written, d_result[1] += stores withheld, over the workgroup (every thread arrives: __syncthreads inside)
__device__ __forceinline__ void sk_ctl_count(uint32_t *sums, uint32_t *d_result, bool wrote, uint32_t withheld) {
  const int tid = threadIdx.x;
  if (tid < 2) sums[tid] = 0;
  __syncthreads();
  const uint32_t w = (uint32_t)__popcll(__ballot(wrote));
  const uint32_t h = (uint32_t)__popcll(__ballot(withheld >= 1)) + (uint32_t)__popcll(__ballot(withheld >= 2));
  if ((tid & 63) == 0) {
    if (w) atomicAdd(&sums[0], w);
    if (h) atomicAdd(&sums[1], h);
  }
  __syncthreads();
  if (d_result && tid < 2 && sums[tid]) atomicAdd(d_result + tid, sums[tid]);
}

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
