// skred_steal_common.hpp -- the parts of the radix select that the key passes share (skred_steal_kernels.hip: the float bank's
// sk_steal_keys_kernel and every launch behind it; skred_fx_steal_kernels.hip: the fixed-point bank's sk_fx_steal_keys_kernel).
// A key pass evaluates its bank's candidate predicate, stores one key per voice, counts the first digit with sk_steal_histogram
// and lets its last arriver pick the first bin with sk_steal_pick; nothing behind it reads a plane.
// The float bank has two key passes -- one key per voice (sk_steal_keys_kernel) and one per slot of a tiled patch
// (skred_slot_steal_kernels.hip: sk_slot_steal_keys_kernel); the per-voice terms both are made of are stated once, below.
// The slot key pass and the fixed-point one have a MATCHED instantiation each (one channel's victims: an owner guard in front, and a
// count of the match's sounding slots beside the keys); the count is stated once, at the end.
#ifndef SKRED_STEAL_COMMON_HPP
#define SKRED_STEAL_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_kernel_common.hpp"
#include "skred_launch.h"

#define SK_STEAL_PER (SK_STEAL_BINS / SK_IDLE_SPAN)   // histogram bins per thread of the last arriver

typedef unsigned long long sk_key_t;

__device__ __forceinline__ int sk_steal_shift(int digit) { return SK_STEAL_BITS * (SK_STEAL_DIGITS - 1 - digit); }

// ---- the terms of one voice of the float bank (include/skred_amd.h states the definition field by field), read from the planes the
// query's bits ask for: flags and rwflags always; SKP_ENV_S for OLDEST, min_age > 0 or a RELEASED_* flag; SKS_OSC for QUIETEST
__device__ __forceinline__ int sk_steal_voice(const sk_steal_args_t &a, bool &in_range) {
  const int v = a.base + (int)blockIdx.x * SK_IDLE_SPAN + (int)threadIdx.x;   // base: `first` rounded down to 64
  in_range = v >= a.first && v < a.end;
  return v;
}

// voice_use_amp_envelope != 0 && is_active != 0 (`flags`: the voice's flag word, for sk_steal_loudness)
__device__ __forceinline__ bool sk_steal_live(const sk_steal_args_t &a, int v, uint32_t &flags) {
  flags = a.idle.tab[v].w[2];
  const uint32_t rwf = a.idle.filt[v].w[3];
  return (flags & SKF_USE_ENV) && (rwf & SKR_ENV_ACTIVE);
}

// the query reads sample_start / sample_release (kernel arguments only: wave-uniform)
__device__ __forceinline__ bool sk_steal_reads_clocks(const sk_steal_args_t &a) {
  return a.policy == SK_STEAL_OLDEST || a.min_age > 0 || (a.flags & (SK_STEAL_RELEASED_FIRST | SK_STEAL_RELEASED_ONLY));
}

__device__ __forceinline__ void sk_steal_clocks(const sk_steal_args_t &a, int v, uint64_t &t_start, uint64_t &t_release) {
  const uint4 es = *reinterpret_cast<const uint4 *>(&a.env_s[v]);
  t_start = ((uint64_t)es.y << 32) | es.x;
  t_release = ((uint64_t)es.w << 32) | es.z;
}

__device__ __forceinline__ uint64_t sk_steal_age(const sk_steal_args_t &a, uint64_t t_start) { return t_start > a.now ? 0 : a.now - t_start; }

// QUIETEST's primary: the bits of fabsf(voice_smoother_gain), 0x7fffffff without a smoother
__device__ __forceinline__ sk_key_t sk_steal_loudness(const sk_steal_args_t &a, int v, uint32_t flags) {
  const uint32_t gain = a.idle.osc_rw[v].w[1] & 0x7fffffffu;
  return (flags & SKF_SMOOTH) ? gain : 0x7fffffffu;
}

__device__ __forceinline__ sk_key_t sk_steal_pack(sk_key_t cls, sk_key_t primary) {
  const sk_key_t cap = (1ull << 62) - 1;
  return (cls << 62) | (primary < cap ? primary : cap);
}

// One workgroup's share of a digit histogram: `hist` (LDS, SK_STEAL_BINS words) is zeroed, filled and its non-empty bins added
// to the global histogram.  A wave whose counted keys all hold the same digit -- a bank uploaded in one go has one sample_start --
// adds once instead of 64 times to one LDS word.
__device__ __forceinline__ void sk_steal_histogram(const sk_steal_args_t &a, bool counted, uint32_t digit, uint32_t *hist, int tid) {
  for (int b = tid; b < SK_STEAL_BINS; b += SK_IDLE_SPAN) hist[b] = 0;
  __syncthreads();
  const unsigned long long m = __ballot(counted);
  if (m) {                                                     // wave-uniform
    const int lead = __ffsll((long long)m) - 1;
    const uint32_t d0 = (uint32_t)__shfl((int)digit, lead);
    const unsigned long long same = __ballot(counted && digit == d0);
    if (same == m) {
      if ((tid & 63) == lead) atomicAdd(&hist[d0], (uint32_t)__popcll(m));
    } else if (counted) {
      atomicAdd(&hist[digit], 1u);
    }
  }
  __syncthreads();
  for (int b = tid; b < SK_STEAL_BINS; b += SK_IDLE_SPAN) {
    const uint32_t c = hist[b];
    if (c) __hip_atomic_fetch_add((sk_gu32 *)(a.hist + b), c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// inclusive scan of one word per thread of a SK_IDLE_SPAN-thread workgroup (as sk_idle_count_kernel's)
__device__ __forceinline__ uint32_t sk_steal_scan(uint32_t *scan, uint32_t mine, int tid) {
  __syncthreads();
  scan[tid] = mine;
  __syncthreads();
  for (int d = 1; d < SK_IDLE_SPAN; d <<= 1) {
    const uint32_t add = tid >= d ? scan[tid - d] : 0u;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  return scan[tid];
}

// The last arriver of a digit launch: the bin of this digit in which the remain-th smallest of the counted keys lies.  Thread t owns
// SK_STEAL_PER consecutive bins.  `prefix` / `remain`: what the launch started from (digit 0: nothing fixed, remain = k, made here).
__device__ __forceinline__ void sk_steal_pick(const sk_steal_args_t &a, int digit, sk_key_t prefix, uint32_t remain, uint32_t *scan, int tid) {
  uint32_t c[SK_STEAL_PER], sum = 0;
#pragma unroll
  for (int i = 0; i < SK_STEAL_PER; ++i) {
    sk_gu32 *bin = (sk_gu32 *)(a.hist + tid * SK_STEAL_PER + i);
    c[i] = __hip_atomic_load(bin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(bin, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next launch (stream-ordered)
    sum += c[i];
  }
  const uint32_t incl = sk_steal_scan(scan, sum, tid), excl = incl - sum;
  if (digit == 0) {
    const uint32_t total = scan[SK_IDLE_SPAN - 1];
    remain = total < (uint32_t)a.max_out ? total : (uint32_t)a.max_out;
    if (tid == 0) {
      a.words[SK_STEAL_W_TOTAL] = total;
      a.words[SK_STEAL_W_K] = remain;
      if (a.max_out <= 0) { a.d_count[0] = 0u; a.d_count[1] = total; }   // count only: this launch is the query
    }
  }
  if (remain == 0) {                                           // an empty list: no key is below or equal to a threshold of 0 ...
    if (tid == 0) {                                            // ... that counts (`remain` of the equal ones are taken: none)
      a.words[SK_STEAL_W_REMAIN] = 0u;
      a.words[SK_STEAL_W_PREFIX_LO] = 0u;
      a.words[SK_STEAL_W_PREFIX_HI] = 0u;
    }
    return;
  }
  if (excl < remain && remain <= incl) {                       // exactly one thread: the counts are a partition of >= remain keys
    uint32_t run = excl;
    int d = 0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < SK_STEAL_PER; ++i) {
      if (!found) {
        if (run + c[i] >= remain) { found = true; d = i; }
        else run += c[i];
      }
    }
    const sk_key_t longer = (prefix << SK_STEAL_BITS) | (sk_key_t)(tid * SK_STEAL_PER + d);
    a.words[SK_STEAL_W_REMAIN] = remain - run;
    a.words[SK_STEAL_W_PREFIX_LO] = (uint32_t)longer;
    a.words[SK_STEAL_W_PREFIX_HI] = (uint32_t)(longer >> 32);
  }
}

// ---- the sounding count of a matched key pass: how many slots (voices) of the match sound in the range, candidates or not.  Each
// wave counts with one ballot, the SK_STEAL_WAVES counts meet in LDS, and ONE lane per workgroup adds the sum to word
// SK_CHAN_W_SOUNDING of the steal scratch (workgroups without a sounding slot add nothing).  The last arriver -- sk_arrive_last,
// after the adds of every workgroup have left their CUs -- stores the sum to d_count[2] and re-arms the word.
#define SK_STEAL_WAVES (SK_IDLE_SPAN / 64)

// sk_steal_histogram with one workgroup's share of the count around it: `snd` is the wave's ballot of its sounding lanes (taken with
// the whole wavefront active), `row` SK_STEAL_WAVES words of LDS.  The histogram's barriers stand between the waves' stores to the
// row and the sum, which is why the two travel together
__device__ __forceinline__ void sk_steal_histogram_sounding(const sk_steal_args_t &a, bool counted, uint32_t digit, uint32_t *hist,
                                                            uint32_t *row, unsigned long long snd, int tid) {
  if ((tid & 63) == 0) row[tid >> 6] = (uint32_t)__popcll(snd);
  sk_steal_histogram(a, counted, digit, hist, tid);
  if (tid == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < SK_STEAL_WAVES; ++w) sum += row[w];
    if (sum) __hip_atomic_fetch_add((sk_gu32 *)(a.words + SK_CHAN_W_SOUNDING), sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the last arriver's publish-and-re-arm (every thread of the workgroup that sk_arrive_last let through calls it)
__device__ __forceinline__ void sk_steal_sounding_publish(const sk_steal_args_t &a, int tid) {
  if (tid == 0) {
    sk_gu32 *w = (sk_gu32 *)(a.words + SK_CHAN_W_SOUNDING);
    a.d_count[2] = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next query (stream-ordered)
  }
}

#endif
