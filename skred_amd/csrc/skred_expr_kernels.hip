// skred_expr_kernels.hip -- channels and per-note expression: masked owner matches over a range, and a guarded controller whose
// entries bring values of their own (gfx950 / CDNA4, wave64).
//
// skred_bank_find_match / _stamp_match / _ctl_match / _ctl_owned_each / _ctl_tags_each and the two _each_filter calls (include/skred_amd.h).  owner[n_voices] is
// the note-owner array (skred_owner_kernels.hip has its rules): a slot's tag at its first voice, 0 for nobody.  A slot MATCHES
// (value, mask) when owner != 0 && (owner & mask) == value.  These kernels read the array and never write it.
//
//   sk_match_count_kernel    one lane per SLOT of the range (a load of stride K words); a listed lane is a matching slot.  The counts,
//   sk_match_scatter_kernel  the last arriver's exclusive offsets and the scatter are skred_idle_scan.hpp's, with `from` = the range's
//                            first voice (rank 0: no rotation): ascending by index, no workgroup waits for another.  The scatter
//                            launch also stores the total where the caller wants it, and runs with max_out == 0 for that alone.
//   sk_match_stamps_kernel   one thread per voice of the range: sk_stamp_store on the masked voices of the matching slots, in one
//                            pass, no list in between.  Stamped / unmatched SLOTS are counted by the threads of voice 0.
//   sk_ctl_match_kernel      sk_ctl_range_kernel under the match guard: the records staged in LDS, sk_ctl_store's stores.
//   sk_ctl_owned_each_kernel sk_ctl_owned_kernel with entry k's 32-byte record laid over record l in registers before sk_ctl_store
//                            runs: INC_SCALE, VELOCITY and PAN add the field to the record's `set` and supply its value; AMP_SCALE
//                            replaces the record's amp by ONE fp32 product (__fmul_rn: never contracted), and a product that is
//                            zero or not finite takes SK_CTL_AMP out of `set` for that voice and counts as withheld.
//                            template <bool FILT>: the second instantiation (skred_bank_ctl_owned_each_filter / _ctl_tags_each_filter)
//                            also takes filt[n] and a filter_mask, and on the lanes of that mask lays entry k's five coefficients
//                            over the record with SK_CTL_FILTER: one 16-byte and one 4-byte load more per such lane, sk_ctl_store's
//                            stores as they are.  FILT = false is the kernel as it was (profiles/timbre_usage.txt).
//
// The stores are sk_stamp_store's and sk_ctl_store's (skred_update_common.hpp, skred_ctl_common.hpp): nothing here can drift from
// the unguarded calls.  Plain vector stores and ordinary atomics only; every count is an integer sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_ctl_common.hpp"      // sk_ctl_stage, sk_ctl_store, sk_ctl_count, sk_ctl_finite
#include "skred_idle_scan.hpp"       // sk_idle_count_tail, sk_idle_scatter_tail
#include "skred_launch.h"
#include "skred_update_common.hpp"   // sk_entry_decode, sk_entry_owned, sk_range_lane, sk_stamp_store, sk_owner_count, sk_batch_done

static_assert(SK_CONTROL_SPAN == SK_IDLE_SPAN, "the match list's count and scatter tails are the idle query's");

// this lane's slot (its first voice in v) matches
__device__ __forceinline__ bool sk_match_listed(const sk_match_args_t &m, int &v) {
  const int64_t s = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  const bool in_range = s < m.n_slots;
  v = m.first + (int)((in_range ? s : 0) << m.k_shift);                 // (inside the bank: checked on the host)
  return in_range && sk_owner_matches(m.owner[v], m.value, m.mask);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_match_count_kernel(sk_match_args_t m) {
  __shared__ int lds[SK_IDLE_COUNT_LDS];
  int v;
  const bool listed = sk_match_listed(m, v);
  sk_idle_count_tail(m.idle, v, listed, lds);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_match_scatter_kernel(sk_match_args_t m) {
  __shared__ int lds[SK_IDLE_WAVES];
  if (blockIdx.x == 0 && threadIdx.x == 0) m.d_total[0] = m.idle.words[SK_IDLE_W_TOTAL];   // (the count launch is behind us on the stream)
  int v;
  const bool listed = sk_match_listed(m, v);
  sk_idle_scatter_tail(m.idle, v, listed, lds);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_match_stamps_kernel(const uint32_t *__restrict__ owner, uint32_t value, uint32_t omask,
                                                                       int first, int count, int K, uint64_t voice_mask, uint32_t dirty,
                                                                       sk_plane_ptrs_t p, uint64_t now, uint64_t *mask, uint32_t *d_result) {
  __shared__ uint32_t sums[2];
  const sk_lane_t t = sk_range_lane(first, count, K);
  const bool hit = t.in_range && sk_owner_matches(owner[t.v - t.l], value, omask);
  if (hit && ((voice_mask >> t.l) & 1)) sk_stamp_store(p, now, mask, t.v, dirty);
  const bool flag[2] = { t.head && hit, t.head && !hit };
  sk_owner_count<2>(sums, d_result, flag);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_ctl_match_kernel(const sk_ctl_t *__restrict__ recs, int K, uint64_t voice_mask, int first,
                                                                    int count, const uint32_t *__restrict__ owner, uint32_t value,
                                                                    uint32_t omask, sk_plane_ptrs_t p, uint64_t *mask, uint32_t *d_result,
                                                                    uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t lds[64 * SK_CTL_WORDS];
  __shared__ uint32_t sums[3];
  sk_ctl_stage(lds, recs, K);
  const sk_lane_t t = sk_range_lane(first, count, K);
  const bool hit = t.in_range && sk_owner_matches(owner[t.v - t.l], value, omask);
  const bool mine = hit && ((voice_mask >> t.l) & 1);
  uint32_t withheld = 0;
  if (mine) withheld = sk_ctl_store(p, mask, t.v, lds + t.l * SK_CTL_WORDS);
  sk_ctl_count<3>(sums, d_result, mine, withheld, t.head && !hit);
  sk_batch_done(cnt, done, seq);
}

// what the FILT instantiation takes beside the rest: entry k's coefficients and the voices of a slot that receive them (FILT false:
// an empty struct the kernel never reads)
template <bool FILT> struct sk_each_filt_t {};
template <> struct sk_each_filt_t<true> {
  const sk_filt_each_t *filt;
  uint64_t filter_mask;
};

template <bool FILT>
__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_ctl_owned_each_kernel(const sk_ctl_t *__restrict__ recs, const sk_each_t *__restrict__ each,
                                                                         int k_shift, uint64_t voice_mask, const int32_t *d_slots,
                                                                         const uint32_t *__restrict__ tags, const uint32_t *__restrict__ owner,
                                                                         int n, const uint32_t *d_count, int n_voices, sk_plane_ptrs_t p,
                                                                         uint64_t *mask, uint32_t *d_result, uint32_t *cnt, uint32_t *done,
                                                                         uint32_t seq, sk_each_filt_t<FILT> fa) {
  __shared__ uint32_t lds[64 * SK_CTL_WORDS];
  __shared__ uint32_t sums[3];
  sk_ctl_stage(lds, recs, 1 << k_shift);
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);
  const int64_t i = t.i;
  const int l = t.l;
  const bool owned = sk_entry_owned(owner, tags, t);
  const bool mine = owned && ((voice_mask >> l) & 1);
  uint32_t withheld = 0;
  if (mine) {
    uint32_t r[SK_CTL_WORDS];                                           // record l with entry i laid over it (registers: constant indices)
#pragma unroll
    for (int k = 0; k < SK_CTL_WORDS; ++k) r[k] = lds[l * SK_CTL_WORDS + k];
    uint4 ea = make_uint4(0u, 0u, 0u, 0u);                              // set, inc_scale, amp_scale, velocity
    uint2 eb = make_uint2(0u, 0u);
    if (!FILT || each) {                                                // (FILT: no entries is "the coefficients only")
      ea = *reinterpret_cast<const uint4 *>(&each[i].w[0]);
      eb = *reinterpret_cast<const uint2 *>(&each[i].w[SK_EACH_W_PAN_LEFT]);
    }
    const uint32_t es = ea.x;
    if (es & SK_EACH_INC_SCALE) { r[SK_CTL_SET] |= SK_CTL_INC_SCALE; r[SK_CTL_W_INC_SCALE] = ea.y; }   // (the record names no increment: checked on the host)
    if (es & SK_EACH_AMP_SCALE) {                                       // (the record names SK_CTL_AMP: checked on the host)
      const uint32_t prod = __float_as_uint(__fmul_rn(__uint_as_float(r[SK_CTL_W_AMP]), __uint_as_float(ea.z)));
      if (sk_ctl_finite(prod) && (prod & 0x7fffffffu) != 0u) r[SK_CTL_W_AMP] = prod;
      else { r[SK_CTL_SET] &= ~SK_CTL_AMP; ++withheld; }
    }
    if (es & SK_EACH_VELOCITY) { r[SK_CTL_SET] |= SK_CTL_VELOCITY; r[SK_CTL_W_VELOCITY] = ea.w; }
    if (es & SK_EACH_PAN) { r[SK_CTL_SET] |= SK_CTL_PAN; r[SK_CTL_W_PAN_LEFT] = eb.x; r[SK_CTL_W_PAN_RIGHT] = eb.y; }
    if constexpr (FILT) {
      if ((fa.filter_mask >> l) & 1) {                                  // (record l names no SK_CTL_FILTER: checked on the host)
        const uint4 fc = *reinterpret_cast<const uint4 *>(&fa.filt[i].w[SK_FILT_W_B0]);   // b0, b1, b2, a1
        r[SK_CTL_SET] |= SK_CTL_FILTER;
        r[SK_CTL_W_B0] = fc.x; r[SK_CTL_W_B1] = fc.y; r[SK_CTL_W_B2] = fc.z; r[SK_CTL_W_A1] = fc.w;
        r[SK_CTL_W_A2] = fa.filt[i].w[SK_FILT_W_A2];
      }
    }
    withheld += sk_ctl_store(p, mask, t.e + l, r);                       // (at most 2: one for the increment, one for the amp)
  }
  sk_ctl_count<3>(sums, d_result, mine, withheld, t.valid && !owned && l == 0);
  sk_batch_done(cnt, done, seq);
}

extern "C" int sk_launch_match_find(const sk_match_args_t *args, int first, int count, int slot_voices, hipStream_t stream) {
  if (count <= 0) return 0;
  sk_match_args_t m = *args;
  m.k_shift = sk_slot_shift(slot_voices);
  m.first = first;
  m.n_slots = count >> m.k_shift;
  m.idle.first = first; m.idle.end = first + count; m.idle.from = first;   // the list starts at the range's first slot: rank 0
  m.idle.base = first; m.idle.from_wg = 0;
  const unsigned n_wg = sk_grid(m.n_slots);
  hipLaunchKernelGGL(sk_match_count_kernel, dim3(n_wg), dim3(SK_CONTROL_SPAN), 0, stream, m);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_match_scatter_kernel, dim3(n_wg), dim3(SK_CONTROL_SPAN), 0, stream, m);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_match_stamps(const uint32_t *owner, uint32_t value, uint32_t mask, int first, int count, int slot_voices,
                                      uint64_t voice_mask, uint32_t dirty, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT],
                                      uint64_t now, uint64_t *mask_list, uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 2, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  hipLaunchKernelGGL(sk_match_stamps_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, owner, value, mask, first, count,
                     slot_voices, voice_mask, dirty, p, now, mask_list, d_result);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_ctl_match(const sk_ctl_t *d_recs, int slot_voices, uint64_t voice_mask, int first, int count, const uint32_t *owner,
                                   uint32_t value, uint32_t mask, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT],
                                   uint64_t *mask_list, uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 3, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  hipLaunchKernelGGL(sk_ctl_match_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, d_recs, slot_voices, voice_mask, first,
                     count, owner, value, mask, p, mask_list, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}

// d_filt == NULL: the FILT = false instantiation, the per-entry controller without coefficients; else FILT = true
extern "C" int sk_launch_ctl_owned_each_filter(const sk_ctl_t *d_recs, const sk_each_t *d_each, const sk_filt_each_t *d_filt, int slot_voices,
                                               uint64_t voice_mask, uint64_t filter_mask, const int32_t *d_slots, const uint32_t *d_tags,
                                               const uint32_t *owner, int n, const uint32_t *d_count, int n_voices,
                                               sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t *mask_list,
                                               uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 3, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  const int sh = sk_slot_shift(slot_voices);
  const unsigned n_wg = sk_list_grid(n, sh);
  if (d_filt) {
    sk_each_filt_t<true> fa;
    fa.filt = d_filt;
    fa.filter_mask = filter_mask;
    hipLaunchKernelGGL(sk_ctl_owned_each_kernel<true>, dim3(n_wg), dim3(SK_CONTROL_SPAN), 0, stream, d_recs, d_each, sh, voice_mask, d_slots,
                       d_tags, owner, n, d_count, n_voices, p, mask_list, d_result, cnt, done, seq, fa);
  } else {
    hipLaunchKernelGGL(sk_ctl_owned_each_kernel<false>, dim3(n_wg), dim3(SK_CONTROL_SPAN), 0, stream, d_recs, d_each, sh, voice_mask, d_slots,
                       d_tags, owner, n, d_count, n_voices, p, mask_list, d_result, cnt, done, seq, sk_each_filt_t<false>());
  }
  return (int)hipGetLastError();
}
