// skred_idle_scan.hpp -- the ordered compaction behind the free-voice list and the free-slot list: what a workgroup does with its
// lanes' "listed" bits once the predicate has run (skred_idle_kernels.hip: a listed lane is an idle voice; skred_slot_kernels.hip:
// a listed lane is the first voice of an idle slot).  One place for the counts, the last arriver's exclusive offsets, the rank of
// `from` and the rotated scatter, so the two lists cannot drift apart.
#ifndef SKRED_IDLE_SCAN_HPP
#define SKRED_IDLE_SCAN_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_kernel_common.hpp"   // sk_arrive_last, sk_gu32
#include "skred_launch.h"

#define SK_IDLE_WAVES (SK_IDLE_SPAN / 64)
#define SK_IDLE_COUNT_LDS (SK_IDLE_SPAN + 2 * SK_IDLE_WAVES + 1)   /* ints of LDS sk_idle_count_tail needs */

// the voice of this lane: every workgroup takes SK_IDLE_SPAN consecutive voices from `base` (`first` rounded down to 64)
__device__ __forceinline__ int sk_idle_voice(const sk_idle_args_t &a, bool &in_range) {
  const int v = a.base + (int)blockIdx.x * SK_IDLE_SPAN + (int)threadIdx.x;
  in_range = v >= a.first && v < a.end;
  return v;
}

// The count kernel behind the predicate.  `listed`: this lane's entry (voice index v) belongs on the list.  Publishes the
// workgroup's count; the workgroup that arrives last turns the counts into exclusive offsets, in index order, and writes d_count,
// the total and the rank of `from`.  lds: SK_IDLE_COUNT_LDS ints.
__device__ __forceinline__ void sk_idle_count_tail(const sk_idle_args_t &a, int v, bool listed, int *lds) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const unsigned long long ballot = __ballot(listed);
  // the rank of `from`: the listed entries below it.  Its workgroup counts the ones inside its own span.
  const unsigned long long below = __ballot(listed && v < a.from);
  if ((tid & 63) == 0) { lds[wave] = __popcll(ballot); lds[SK_IDLE_WAVES + wave] = __popcll(below); }
  __syncthreads();
  if (tid == 0) {
    int c = 0, p = 0;
#pragma unroll
    for (int w = 0; w < SK_IDLE_WAVES; ++w) { c += lds[w]; p += lds[SK_IDLE_WAVES + w]; }
    __hip_atomic_store((sk_gu32 *)(a.counts + blockIdx.x), (uint32_t)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((int)blockIdx.x == a.from_wg)
      __hip_atomic_store((sk_gu32 *)(a.words + SK_IDLE_W_PART), (uint32_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!sk_arrive_last(a.words + SK_IDLE_W_TICKET, gridDim.x, tid, &lds[2 * SK_IDLE_WAVES])) return;
  // ---- the last arriver: exclusive offsets of all workgroups, in index order.  Thread t owns a contiguous run of counts.
  const int n = (int)gridDim.x;
  const int per = (n + SK_IDLE_SPAN - 1) / SK_IDLE_SPAN;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += (int)a.counts[i];
  int *scan = &lds[2 * SK_IDLE_WAVES + 1];
  scan[tid] = sum;
  __syncthreads();
  for (int d = 1; d < SK_IDLE_SPAN; d <<= 1) {          // inclusive scan of the per-thread sums
    const int add = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  int run = scan[tid] - sum;
  for (int i = lo; i < hi; ++i) {
    a.offsets[i] = (uint32_t)run;
    if (i == a.from_wg) a.words[SK_IDLE_W_RANK] = (uint32_t)run + a.words[SK_IDLE_W_PART];
    run += (int)a.counts[i];
  }
  if (tid == SK_IDLE_SPAN - 1) {
    const uint32_t total = (uint32_t)scan[tid];
    a.words[SK_IDLE_W_TOTAL] = total;
    a.d_count[0] = total < (uint32_t)a.max_out ? total : (uint32_t)a.max_out;
    a.d_count[1] = total;
  }
}

// The scatter kernel behind the predicate: rank = workgroup offset + wave prefix + mbcnt of the ballot, rotated by the rank of
// `from` modulo the total, stored when it is below max_out.  lds: SK_IDLE_WAVES ints.
__device__ __forceinline__ void sk_idle_scatter_tail(const sk_idle_args_t &a, int v, bool listed, int *lds) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const unsigned long long ballot = __ballot(listed);
  if ((tid & 63) == 0) lds[wave] = __popcll(ballot);
  __syncthreads();
  if (!listed) return;
  int rank = (int)a.offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) rank += lds[w];
  rank += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
  const int total = (int)a.words[SK_IDLE_W_TOTAL];
  int at = rank - (int)a.words[SK_IDLE_W_RANK];       // the list starts at the first listed entry >= from and wraps
  if (at < 0) at += total;
  if (at >= 0 && at < a.max_out) a.d_voices[at] = v;
}

#endif
