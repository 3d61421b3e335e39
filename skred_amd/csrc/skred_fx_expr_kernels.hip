// skred_fx_expr_kernels.hip -- channels and per-note expression on the fixed-point bank: masked owner matches over a range, and a
// guarded controller whose entries bring values of their own (gfx950 / CDNA4, wave64).
//
// skred_fxbank_stamp_match / _ctl_match / _ctl_owned_each / _ctl_tags_each and the two _each_filter calls (include/skred_amd_fxpt.h).  owner[n_voices] is the
// note-owner array of skred_fx_owner.c: one tag per voice, 0 for nobody.  A voice MATCHES (value, mask) when
// owner != 0 && (owner & mask) == value.  These kernels read the array and never write it.  The ordered list of the matching voices
// (skred_fxbank_find_match) needs no kernel of this bank's: it reads the owner array and the scan scratch alone, so the bank enters
// the float bank's sk_match_count_kernel and sk_match_scatter_kernel through sk_launch_match_find at slot_voices = 1.
//
//   sk_fx_match_stamps_kernel     one lane per voice of [first, first + count): skx_stamp_store on the matching voices, in one pass,
//                                 no list in between.  A wavefront's 64 lanes are 64 consecutive voices: the owner word is one
//                                 coalesced 4-byte load per lane, every plane access one coalesced 16-byte access per lane.
//   sk_fx_ctl_match_kernel        sk_fx_ctl_range_kernel under the match guard: skx_ctl_store's stores, the record read from device
//                                 memory at addresses uniform over the launch.
//   sk_fx_ctl_owned_each_kernel   sk_fx_ctl_list_kernel's guarded form, one lane per list entry, with entry k's 32-byte record laid
//                                 over the base record in registers before skx_ctl_store runs: INC_SCALE, VELOCITY and PAN add the
//                                 field to `which` and supply its value; AMP_SCALE replaces the record's amp by
//                                 ((uint64)amp_q15 * amp_scale_q16) >> 16, and a product of 0 or above 65535 takes SKX_C_AMP out of
//                                 `which` for that voice and counts as withheld -- the amp guard cannot count the voice again.
//                                 template <bool FILT>: the second instantiation (skred_fxbank_ctl_owned_each_filter /
//                                 _ctl_tags_each_filter) also takes filt[n] and lays entry k's five Q2.30 coefficients over the
//                                 record with SKX_C_FILTER: one 16-byte and one 4-byte load more per lane, skx_ctl_store's stores as
//                                 they are.  FILT = false is the kernel as it was (profiles/timbre_usage.txt).
//
// The stores are skx_stamp_store's and skx_ctl_store's (skred_fx_ctl_common.hpp): nothing here can drift from the unguarded calls.
// Misses are the ordinary case under a match guard (fifteen voices of sixteen on a 16-channel range), so every count goes through
// the workgroup's LDS sums (skx_count): at most one global atomic per workgroup and count.  Plain vector stores and ordinary atomics
// only; no workgroup waits for another; every arithmetic step is exact integer arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_ctl_common.hpp"   // skx_stamp_store, skx_ctl_store, skx_ctl_planes, skx_list_looked, skx_count, skx_grid
#include "skred_fx_layout.h"
#include "skred_launch.h"            // sk_owner_matches

static_assert(SKX_EXPR_SPAN == SKX_CTL_SPAN, "skx_count and the launch geometry are written for this span");

// this lane's voice of the range (in v; inside the bank: checked on the host) matches
__device__ __forceinline__ bool skx_match_hit(const uint32_t *__restrict__ owner, uint32_t value, uint32_t mask, int first, int count,
                                              int &v, bool &in_range) {
  const int64_t off = (int64_t)blockIdx.x * SKX_EXPR_SPAN + threadIdx.x;
  in_range = off < count;
  v = first + (int)(in_range ? off : 0);
  return in_range && sk_owner_matches(owner[v], value, mask);
}

__global__ __launch_bounds__(SKX_EXPR_SPAN) void sk_fx_match_stamps_kernel(const uint32_t *__restrict__ owner, uint32_t value, uint32_t omask,
                                                                           int first, int count, uint32_t stamps, skx_plane_t *time_plane,
                                                                           skx_plane_t *rw0, uint64_t now, uint32_t *d_result) {
  __shared__ uint32_t sums[2];
  int v;
  bool in_range;
  const bool hit = skx_match_hit(owner, value, omask, first, count, v, in_range);
  if (hit) skx_stamp_store(time_plane, rw0, v, stamps, now);
  const uint32_t val[2] = { hit ? 1u : 0u, (in_range && !hit) ? 1u : 0u };
  skx_count<2>(sums, d_result, val);
}

__global__ __launch_bounds__(SKX_EXPR_SPAN) void sk_fx_ctl_match_kernel(const skx_ctl_t *__restrict__ rec, int first, int count,
                                                                        const uint32_t *__restrict__ owner, uint32_t value, uint32_t omask,
                                                                        skx_ctl_planes_t p, uint32_t *d_result) {
  __shared__ uint32_t sums[3];
  int v;
  bool in_range;
  const bool hit = skx_match_hit(owner, value, omask, first, count, v, in_range);
  uint32_t withheld = 0;
  if (hit) withheld = skx_ctl_store(p, v, rec->w);
  const uint32_t val[3] = { hit ? 1u : 0u, withheld, (in_range && !hit) ? 1u : 0u };
  skx_count<3>(sums, d_result, val);
}

// what the FILT instantiation takes beside the rest: entry k's coefficients (FILT false: an empty struct the kernel never reads)
template <bool FILT> struct skx_each_filt_t {};
template <> struct skx_each_filt_t<true> {
  const skx_filt_each_t *filt;
};

template <bool FILT>
__global__ __launch_bounds__(SKX_EXPR_SPAN) void sk_fx_ctl_owned_each_kernel(const skx_ctl_t *__restrict__ rec, const skx_each_t *__restrict__ each,
                                                                             const int32_t *d_voices, const uint32_t *__restrict__ tags,
                                                                             const uint32_t *__restrict__ owner, int n, const uint32_t *d_count,
                                                                             int n_voices, skx_ctl_planes_t p, uint32_t *d_result,
                                                                             skx_each_filt_t<FILT> fa) {
  __shared__ uint32_t sums[3];
  const int64_t i = (int64_t)blockIdx.x * SKX_EXPR_SPAN + threadIdx.x;
  bool valid = false, mine = false;
  uint32_t withheld = 0;
  if (skx_list_looked(i, n, d_count)) {
    const int v = d_voices[i];
    valid = v >= 0 && v < n_voices;
    mine = valid && owner[v] == tags[i];                                // (tags are non-zero: an untagged voice never matches)
    if (mine) {
      uint32_t r[SKX_CTL_WORDS];                                        // the record with entry i laid over it (registers: constant indices)
#pragma unroll
      for (int k = 0; k < SKX_CTL_WORDS; ++k) r[k] = rec->w[k];
      uint4 ea = make_uint4(0u, 0u, 0u, 0u);                            // set, inc_scale_q16, amp_scale_q16, velocity_q15
      uint2 eb = make_uint2(0u, 0u);
      if (!FILT || each) {                                              // (FILT: no entries is "the coefficients only")
        ea = *reinterpret_cast<const uint4 *>(&each[i].w[0]);
        eb = *reinterpret_cast<const uint2 *>(&each[i].w[SKX_EACH_W_PAN_LEFT]);
      }
      const uint32_t es = ea.x;
      if (es & SKX_EACH_INC_SCALE) { r[SKX_CTL_WHICH] |= SKX_C_INC_SCALE; r[SKX_CTL_INC_SCALE] = ea.y; }   // (the record names no increment: checked on the host)
      if (es & SKX_EACH_AMP_SCALE) {                                    // (the record names SKX_C_AMP: checked on the host)
        const uint64_t prod = ((uint64_t)r[SKX_CTL_AMP] * (uint64_t)ea.z) >> 16;
        if (prod >= 1ull && prod <= 65535ull) r[SKX_CTL_AMP] = (uint32_t)prod;
        else { r[SKX_CTL_WHICH] &= ~(uint32_t)SKX_C_AMP; ++withheld; }
      }
      if (es & SKX_EACH_VELOCITY) { r[SKX_CTL_WHICH] |= SKX_C_VELOCITY; r[SKX_CTL_VELOCITY] = ea.w; }
      if (es & SKX_EACH_PAN) { r[SKX_CTL_WHICH] |= SKX_C_PAN; r[SKX_CTL_PAN_LEFT] = eb.x; r[SKX_CTL_PAN_RIGHT] = eb.y; }
      if constexpr (FILT) {                                             // (the record names no SKX_C_FILTER: checked on the host)
        const uint4 fc = *reinterpret_cast<const uint4 *>(&fa.filt[i].w[SKX_FILT_W_B0]);   // b0, b1, b2, a1 (Q2.30)
        r[SKX_CTL_WHICH] |= SKX_C_FILTER;
        r[SKX_CTL_B0] = fc.x; r[SKX_CTL_B1] = fc.y; r[SKX_CTL_B2] = fc.z; r[SKX_CTL_A1] = fc.w;
        r[SKX_CTL_A2] = fa.filt[i].w[SKX_FILT_W_A2];
      }
      withheld += skx_ctl_store(p, v, r);                               // (at most 2: one for the increment, one for the amp)
    }
  }
  const uint32_t val[3] = { mine ? 1u : 0u, withheld, (valid && !mine) ? 1u : 0u };
  skx_count<3>(sums, d_result, val);
}

// d_result[2] (required) is zeroed on `stream` ahead of the kernel: voices stamped, voices of the range that did not match
extern "C" int skx_launch_match_stamps(const uint32_t *owner, uint32_t value, uint32_t mask, int first, int count, uint32_t stamps,
                                       skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now, uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_fx_match_stamps_kernel, dim3(skx_grid(count)), dim3(SKX_EXPR_SPAN), 0, stream, owner, value, mask, first, count,
                     stamps, time_plane, rw0, now, d_result);
  return (int)hipGetLastError();
}

// d_result[3] (or NULL): voices written, stores withheld, voices of the range that did not match
extern "C" int skx_launch_ctl_match(const skx_ctl_t *d_rec, int first, int count, const uint32_t *owner, uint32_t value, uint32_t mask,
                                    skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  if (d_result) {
    const hipError_t e = hipMemsetAsync(d_result, 0, 3 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
  }
  skx_ctl_planes_t p;
  skx_ctl_planes(p, ro);
  hipLaunchKernelGGL(sk_fx_ctl_match_kernel, dim3(skx_grid(count)), dim3(SKX_EXPR_SPAN), 0, stream, d_rec, first, count, owner, value, mask,
                     p, d_result);
  return (int)hipGetLastError();
}

// d_rec: the base record (which == 0 when the caller gave none); d_each: 16-byte aligned; d_result[3] (or NULL): voices written,
// stores withheld (the two guards and the amp products), voices whose owner differs
// d_filt == NULL: the FILT = false instantiation, the per-entry controller without coefficients.  Else FILT = true: entry k's five
// coefficients d_filt[k] (16-byte aligned) laid over the record with SKX_C_FILTER; d_each may then be NULL (the coefficients alone)
extern "C" int skx_launch_ctl_owned_each_filter(const skx_ctl_t *d_rec, const skx_each_t *d_each, const skx_filt_each_t *d_filt,
                                                const int32_t *d_voices, const uint32_t *d_tags, const uint32_t *owner, int n,
                                                const uint32_t *d_count, int n_voices, skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result,
                                                hipStream_t stream) {
  if (n <= 0) return 0;
  if (d_result) {
    const hipError_t e = hipMemsetAsync(d_result, 0, 3 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
  }
  skx_ctl_planes_t p;
  skx_ctl_planes(p, ro);
  if (d_filt) {
    skx_each_filt_t<true> fa;
    fa.filt = d_filt;
    hipLaunchKernelGGL(sk_fx_ctl_owned_each_kernel<true>, dim3(skx_grid(n)), dim3(SKX_EXPR_SPAN), 0, stream, d_rec, d_each, d_voices,
                       d_tags, owner, n, d_count, n_voices, p, d_result, fa);
  } else {
    hipLaunchKernelGGL(sk_fx_ctl_owned_each_kernel<false>, dim3(skx_grid(n)), dim3(SKX_EXPR_SPAN), 0, stream, d_rec, d_each, d_voices,
                       d_tags, owner, n, d_count, n_voices, p, d_result, skx_each_filt_t<false>());
  }
  return (int)hipGetLastError();
}
