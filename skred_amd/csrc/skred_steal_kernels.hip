// skred_steal_kernels.hip -- which sounding voices matter least: an ordered list of victims, built on the device (gfx950 / CDNA4).
//
// skred_bank_find_steal (include/skred_amd.h): every candidate of the range gets a 64-bit key (class << 62 | primary); the list
// is the k = min(max_out, candidates) <= SK_STEAL_MAX smallest keys, ties by voice index.  A most-significant-digit radix select,
// SK_STEAL_DIGITS + 3 launches on the caller's stream whatever the data:
//
//   sk_steal_keys_kernel     every workgroup takes SK_IDLE_SPAN consecutive voices (spans aligned to 64 voices, as the idle query's),
//                            evaluates the candidate predicate and the key from the planes the query's bits need -- flags and
//                            rwflags always; SKP_ENV_S for OLDEST, min_age > 0 or a RELEASED_* flag; SKS_OSC for QUIETEST or an
//                            ENV_DONE exclusion; SKP_OSC for an AMP_ZERO exclusion -- and stores ONE key per voice into `keys`
//                            (SK_STEAL_NOKEY: no candidate): the later launches read 8 bytes per voice, not the planes.  It also
//                            counts the first digit.
//   sk_steal_digit_kernel    digits 1 .. SK_STEAL_DIGITS - 1: the keys that match the digits fixed so far, counted by their next digit.
//     Both build the histogram of their span in LDS and add its non-empty bins to the global one with integer atomics; the
//     workgroup that ARRIVES LAST (skred_kernel_common.hpp: sk_arrive_last) finds the bin in which the k-th smallest key lies,
//     stores the longer prefix and how many keys are still to take from that bin, and zeroes the histogram for the next launch.
//     After the last digit the prefix IS the threshold key T, and `remain` of the keys equal to T belong to the list.
//   sk_steal_count_kernel    per workgroup: keys below T, keys equal to T; its last arriver turns both into exclusive offsets in
//                            index order (the idle query's count).
//   sk_steal_scatter_kernel  keys below T go to winners[offset + rank]; keys equal to T with an index-ordered rank below `remain` go
//                            behind them: ties at the threshold are resolved by voice index, however many workgroups they span.
//   sk_steal_sort_kernel     ONE workgroup: a bitonic sort of the at most SK_STEAL_MAX (key, voice) pairs in LDS (12 KiB), then
//                            d_voices and d_count.
//
// No workgroup waits for another: nothing here can spin or hang.  Integer sums and index-ordered ranks: the same state gives the
// same bytes.  Every kernel only READS the bank.  Branches on query bits depend on kernel arguments only: they are wave-uniform.
//
//   sk_launch_steal_select launches everything behind the key pass.  None of it reads a plane, so the fixed-point bank's query
//   (skred_fx_steal_kernels.hip: sk_fx_steal_keys_kernel) runs its own key pass into the same scratch layout and enters there.
//
//   sk_list_append_kernel    skred_bank_note_on_steal: the victims copied behind the idle list's entries, at the offset the idle
//                            query's count word holds on the device.
//   sk_chan_join_kernel      skred_bank_note_on_channel (and the fixed-point bank's): one workgroup -- how many notes of a burst take
//                            idle slots (the cap minus the channel's sounding count), how many steal, the victims copied behind the
//                            idle slots that are used.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_idle_common.hpp"
#include "skred_kernel_common.hpp"
#include "skred_launch.h"
#include "skred_steal_common.hpp"   // sk_key_t, the per-voice terms (shared with the slot key pass), sk_steal_histogram / _scan / _pick

#define SK_STEAL_WAVES (SK_IDLE_SPAN / 64)
#define SK_STEAL_SORT_THREADS 512

// the key of one voice, SK_STEAL_NOKEY when it is no candidate (skred_steal_common.hpp: the terms it is made of)
__device__ __forceinline__ sk_key_t sk_steal_key(const sk_steal_args_t &a, int v, bool in_range) {
  if (!in_range) return SK_STEAL_NOKEY;
  uint32_t flags;
  bool cand = sk_steal_live(a, v, flags);
  uint64_t t_release = 0, t_start = 0;
  if (sk_steal_reads_clocks(a)) sk_steal_clocks(a, v, t_start, t_release);
  const bool released = t_release != 0;
  if (a.min_age > 0) cand = cand && sk_steal_age(a, t_start) >= a.min_age;
  if (a.flags & SK_STEAL_RELEASED_ONLY) cand = cand && released;
  if (a.flags & SK_STEAL_UNNAMED) cand = cand && !((a.idle.named[v >> 6] >> (v & 63)) & 1);
  if (a.idle.which) cand = cand && !sk_idle_pred(a.idle, v, true);
  if (!cand) return SK_STEAL_NOKEY;
  const sk_key_t cls = ((a.flags & SK_STEAL_RELEASED_FIRST) && released) ? 0ull : 1ull;
  sk_key_t primary;
  if (a.policy == SK_STEAL_OLDEST) primary = cls == 0 ? t_release : t_start;
  else primary = sk_steal_loudness(a, v, flags);
  return sk_steal_pack(cls, primary);
}

__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_steal_keys_kernel(sk_steal_args_t a) {
  __shared__ uint32_t hist[SK_STEAL_BINS];
  __shared__ uint32_t scan[SK_IDLE_SPAN];
  __shared__ int flag;
  const int tid = threadIdx.x;
  bool in_range;
  const int v = sk_steal_voice(a, in_range);
  const sk_key_t key = sk_steal_key(a, v, in_range);
  a.keys[(size_t)blockIdx.x * SK_IDLE_SPAN + tid] = key;       // (read by later launches only)
  sk_steal_histogram(a, key != SK_STEAL_NOKEY, (uint32_t)(key >> sk_steal_shift(0)) & (SK_STEAL_BINS - 1), hist, tid);
  if (!sk_arrive_last(a.words + SK_STEAL_W_TICKET, gridDim.x, tid, &flag)) return;
  sk_steal_pick(a, 0, 0ull, 0u, scan, tid);
}

__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_steal_digit_kernel(sk_steal_args_t a) {
  __shared__ uint32_t hist[SK_STEAL_BINS];
  __shared__ uint32_t scan[SK_IDLE_SPAN];
  __shared__ int flag;
  const int tid = threadIdx.x;
  const sk_key_t prefix = ((sk_key_t)a.words[SK_STEAL_W_PREFIX_HI] << 32) | a.words[SK_STEAL_W_PREFIX_LO];   // (the launch before wrote them)
  const uint32_t remain = a.words[SK_STEAL_W_REMAIN];
  const sk_key_t key = a.keys[(size_t)blockIdx.x * SK_IDLE_SPAN + tid];
  const int shift = sk_steal_shift(a.digit);
  const bool counted = key != SK_STEAL_NOKEY && remain != 0 && (key >> (shift + SK_STEAL_BITS)) == prefix;
  sk_steal_histogram(a, counted, (uint32_t)(key >> shift) & (SK_STEAL_BINS - 1), hist, tid);
  if (!sk_arrive_last(a.words + SK_STEAL_W_TICKET, gridDim.x, tid, &flag)) return;
  sk_steal_pick(a, a.digit, prefix, remain, scan, tid);
}

// below / equal ballots of a thread's key against the threshold (an empty list has no winners: k == 0)
__device__ __forceinline__ void sk_steal_compare(const sk_steal_args_t &a, sk_key_t &key, bool &lt, bool &eq) {
  const sk_key_t T = ((sk_key_t)a.words[SK_STEAL_W_PREFIX_HI] << 32) | a.words[SK_STEAL_W_PREFIX_LO];
  const bool any = a.words[SK_STEAL_W_K] != 0;
  key = a.keys[(size_t)blockIdx.x * SK_IDLE_SPAN + threadIdx.x];
  lt = any && key < T;                                         // (SK_STEAL_NOKEY is above every threshold)
  eq = any && key == T;
}

__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_steal_count_kernel(sk_steal_args_t a) {
  __shared__ uint32_t wave_lt[SK_STEAL_WAVES], wave_eq[SK_STEAL_WAVES];
  __shared__ uint32_t scan[SK_IDLE_SPAN];
  __shared__ int flag;
  const int tid = threadIdx.x, wave = tid >> 6;
  sk_key_t key;
  bool lt, eq;
  sk_steal_compare(a, key, lt, eq);
  const unsigned long long b_lt = __ballot(lt), b_eq = __ballot(eq);
  if ((tid & 63) == 0) { wave_lt[wave] = (uint32_t)__popcll(b_lt); wave_eq[wave] = (uint32_t)__popcll(b_eq); }
  __syncthreads();
  if (tid == 0) {
    uint32_t l = 0, e = 0;
#pragma unroll
    for (int w = 0; w < SK_STEAL_WAVES; ++w) { l += wave_lt[w]; e += wave_eq[w]; }
    __hip_atomic_store((sk_gu32 *)(a.cnt_lt + blockIdx.x), l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((sk_gu32 *)(a.cnt_eq + blockIdx.x), e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!sk_arrive_last(a.words + SK_STEAL_W_TICKET, gridDim.x, tid, &flag)) return;
  // ---- the last arriver: exclusive offsets of all workgroups, in index order.  Thread t owns a contiguous run of counts.
  const int n = (int)gridDim.x;
  const int per = (n + SK_IDLE_SPAN - 1) / SK_IDLE_SPAN;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  uint32_t sum_lt = 0, sum_eq = 0;
  for (int i = lo; i < hi; ++i) {
    sum_lt += __hip_atomic_load((sk_gu32 *)(a.cnt_lt + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sum_eq += __hip_atomic_load((sk_gu32 *)(a.cnt_eq + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  uint32_t run_lt = sk_steal_scan(scan, sum_lt, tid) - sum_lt;
  uint32_t run_eq = sk_steal_scan(scan, sum_eq, tid) - sum_eq;
  for (int i = lo; i < hi; ++i) {
    a.off_lt[i] = run_lt;
    a.off_eq[i] = run_eq;
    run_lt += __hip_atomic_load((sk_gu32 *)(a.cnt_lt + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    run_eq += __hip_atomic_load((sk_gu32 *)(a.cnt_eq + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_steal_scatter_kernel(sk_steal_args_t a) {
  __shared__ uint32_t wave_lt[SK_STEAL_WAVES], wave_eq[SK_STEAL_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6;
  bool in_range;
  const int v = sk_steal_voice(a, in_range);
  sk_key_t key;
  bool lt, eq;
  sk_steal_compare(a, key, lt, eq);
  const unsigned long long b_lt = __ballot(lt), b_eq = __ballot(eq);
  if ((tid & 63) == 0) { wave_lt[wave] = (uint32_t)__popcll(b_lt); wave_eq[wave] = (uint32_t)__popcll(b_eq); }
  __syncthreads();
  if (!lt && !eq) return;
  const uint32_t k = a.words[SK_STEAL_W_K], remain = a.words[SK_STEAL_W_REMAIN];
  const unsigned long long b = lt ? b_lt : b_eq;
  uint32_t rank = lt ? a.off_lt[blockIdx.x] : a.off_eq[blockIdx.x];
  for (int w = 0; w < wave; ++w) rank += lt ? wave_lt[w] : wave_eq[w];
  rank += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
  uint32_t at = rank;                                          // keys below the threshold: all k - remain of them, in index order
  if (eq) {
    if (rank >= remain) return;                                // ties at the threshold: the first `remain` by voice index
    at = k - remain + rank;
  }
  if (at < (uint32_t)SK_STEAL_MAX) { a.win_keys[at] = key; a.win_voices[at] = v; }
}

__device__ __forceinline__ bool sk_steal_above(sk_key_t ka, int va, sk_key_t kb, int vb) { return ka > kb || (ka == kb && va > vb); }

__global__ __launch_bounds__(SK_STEAL_SORT_THREADS) void sk_steal_sort_kernel(sk_steal_args_t a) {
  __shared__ sk_key_t keys[SK_STEAL_MAX];
  __shared__ int voices[SK_STEAL_MAX];
  const int tid = threadIdx.x;
  const uint32_t total = a.words[SK_STEAL_W_TOTAL];
  int k = (int)a.words[SK_STEAL_W_K];
  if (k > SK_STEAL_MAX) k = SK_STEAL_MAX;                       // (the host refuses a larger max_out)
  if (k > a.max_out) k = a.max_out;
  int m = 2;
  while (m < k) m <<= 1;
  for (int i = tid; i < m; i += SK_STEAL_SORT_THREADS) {
    keys[i] = i < k ? a.win_keys[i] : SK_STEAL_NOKEY;           // the padding sorts behind every winner
    voices[i] = i < k ? a.win_voices[i] : 0x7fffffff;
  }
  for (int size = 2; size <= m; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (m >> 1); t += SK_STEAL_SORT_THREADS) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool up = (i & size) == 0;
        const sk_key_t ki = keys[i], kj = keys[j];
        const int vi = voices[i], vj = voices[j];
        if (sk_steal_above(ki, vi, kj, vj) == up) { keys[i] = kj; keys[j] = ki; voices[i] = vj; voices[j] = vi; }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < k; i += SK_STEAL_SORT_THREADS) a.d_voices[i] = voices[i];
  if (tid == 0) { a.d_count[0] = (uint32_t)k; a.d_count[1] = total; }
}

__global__ __launch_bounds__(SK_STEAL_MAX) void sk_list_append_kernel(int32_t *dst, const uint32_t *dst_count, const int32_t *src,
                                                                      const uint32_t *src_count, int room, uint32_t *out_count,
                                                                      uint32_t *stolen) {
  const uint32_t held = dst_count[0];
  const uint32_t at = held < (uint32_t)room ? held : (uint32_t)room;
  uint32_t n = src_count[0] < (uint32_t)SK_STEAL_MAX ? src_count[0] : (uint32_t)SK_STEAL_MAX;
  if (n > (uint32_t)room - at) n = (uint32_t)room - at;
  const uint32_t t = threadIdx.x;
  if (t < n) dst[at + t] = src[t];
  if (t == 0) { out_count[0] = at + n; stolen[0] = n; }
}

__global__ __launch_bounds__(SK_STEAL_MAX) void sk_chan_join_kernel(int32_t *list, const uint32_t *idle_count, const int32_t *victims,
                                                                    const uint32_t *victim_count, int n, uint32_t cap,
                                                                    uint32_t *out_count, uint32_t *d_result) {
  const uint32_t un = (uint32_t)n;
  const uint32_t idle = idle_count[0] < un ? idle_count[0] : un;
  const uint32_t snd = victim_count[2];
  const uint32_t room = cap > snd ? cap - snd : 0u;
  uint32_t a = idle < room ? idle : room;                      // (<= n: `idle` is)
  uint32_t b = victim_count[0] < (uint32_t)SK_STEAL_MAX ? victim_count[0] : (uint32_t)SK_STEAL_MAX;
  if (b > un - a) b = un - a;
  const uint32_t t = threadIdx.x;
  if (t < b) list[a + t] = victims[t];                         // (a + t < a + b <= n: inside the list)
  if (t == 0) { out_count[0] = a + b; d_result[2] = b; d_result[3] = snd; }
}

// everything behind a key pass: it reads a.keys and the words the key pass's last arriver left, never a plane
extern "C" int sk_launch_steal_select(const sk_steal_args_t *args, hipStream_t stream) {
  sk_steal_args_t a = *args;
  a.base = a.first & ~63;
  if (a.max_out <= 0) return (int)hipSuccess;
  const dim3 grid((unsigned)sk_idle_workgroups(a.first, a.end - a.first)), block(SK_IDLE_SPAN);
  hipError_t e;
  for (int d = 1; d < SK_STEAL_DIGITS; ++d) {
    a.digit = d;
    hipLaunchKernelGGL(sk_steal_digit_kernel, grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(sk_steal_count_kernel, grid, block, 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_steal_scatter_kernel, grid, block, 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_steal_sort_kernel, dim3(1), dim3(SK_STEAL_SORT_THREADS), 0, stream, a);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_steal(const sk_steal_args_t *args, hipStream_t stream) {
  sk_steal_args_t a = *args;
  a.base = a.first & ~63;
  a.idle.first = a.first;
  a.idle.end = a.end;
  const dim3 grid((unsigned)sk_idle_workgroups(a.first, a.end - a.first)), block(SK_IDLE_SPAN);
  a.digit = 0;
  hipLaunchKernelGGL(sk_steal_keys_kernel, grid, block, 0, stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return sk_launch_steal_select(&a, stream);
}

extern "C" int sk_launch_list_append(int32_t *dst, const uint32_t *dst_count, const int32_t *src, const uint32_t *src_count, int room,
                                     uint32_t *out_count, uint32_t *stolen, hipStream_t stream) {
  hipLaunchKernelGGL(sk_list_append_kernel, dim3(1), dim3(SK_STEAL_MAX), 0, stream, dst, dst_count, src, src_count, room, out_count, stolen);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_chan_join(int32_t *list, const uint32_t *idle_count, const int32_t *victims, const uint32_t *victim_count,
                                   int n, uint32_t cap, uint32_t *out_count, uint32_t *d_result, hipStream_t stream) {
  hipLaunchKernelGGL(sk_chan_join_kernel, dim3(1), dim3(SK_STEAL_MAX), 0, stream, list, idle_count, victims, victim_count, n, cap,
                     out_count, d_result);
  return (int)hipGetLastError();
}
