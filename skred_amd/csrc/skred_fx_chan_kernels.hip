// skred_fx_chan_kernels.hip -- channel polyphony on the fixed-point bank: the victim query of ONE channel (gfx950 / CDNA4, wave64).
// include/skred_amd_fxpt.h, section "channel polyphony", has the definition.
//
//   sk_fx_chan_steal_keys_kernel  sk_fx_steal_keys_kernel (skred_fx_steal_kernels.hip) plus two things.
//                                 THE OWNER GUARD: every lane of the range loads owner[v] first.  A voice whose owner is 0 or
//                                 fails (owner & mask) == value issues no plane load at all -- not the flags, not the clocks, not
//                                 the exclusion's words --, is no candidate and is not counted.
//                                 THE SOUNDING COUNT: a voice of the match whose envelope runs and which the exclusion does not
//                                 call idle.  Each wave counts its voices with one ballot, the four counts meet in LDS, and ONE
//                                 lane per workgroup adds the sum to a word of the steal scratch (workgroups without a sounding
//                                 voice add nothing).  The last arriver -- sk_arrive_last, after the adds of every workgroup have
//                                 left their CUs -- stores the sum to d_count[2] and re-arms the word.
//                                 The key of a matching voice is skx_steal_key (skred_fx_steal_common.hpp), the histogram and the
//                                 pick are the float key pass's (skred_steal_common.hpp).
//
// sk_launch_steal_select then runs unchanged, and the join of a capped burst is the float bank's sk_launch_chan_join
// (skred_chan_kernels.hip), which knows no bank.  No workgroup waits for another; integer atomics only; every store to global
// memory is a plain vector store or an atomic; branches on query bits depend on kernel arguments only and are wave-uniform.  The
// kernel only READS the bank and the owner array: the same state gives the same bytes.  With mask == 0 and every sounding voice
// tagged the keys, and so the list and the first two count words, are sk_fx_steal_keys_kernel's bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_chan.h"
#include "skred_fx_steal_common.hpp"
#include "skred_kernel_common.hpp"

#define SKX_CHAN_WAVES (SK_IDLE_SPAN / 64)

__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_fx_chan_steal_keys_kernel(skx_steal_args_t a, const uint32_t *__restrict__ owner,
                                                                             uint32_t value, uint32_t mask) {
  __shared__ uint32_t hist[SK_STEAL_BINS];
  __shared__ uint32_t scan[SK_IDLE_SPAN];
  __shared__ uint32_t sounding[SKX_CHAN_WAVES];
  __shared__ int flag;
  const int tid = threadIdx.x;
  const int v = a.s.base + (int)blockIdx.x * SK_IDLE_SPAN + tid;   // base: `first` rounded down to 64
  const bool in_range = v >= a.s.first && v < a.s.end;
  // ---- the owner guard (in range: 0 <= first <= v < end <= n_voices, the owner array's length)
  uint32_t own = 0;
  if (in_range) own = owner[v];
  const bool member = in_range && own != 0 && (own & mask) == value;
  // ---- this lane's voice: no plane is read unless `member`
  const bool sounds = skx_steal_sounding(a, v, member);
  const sk_key_t key = skx_steal_key(a, v, member);
  a.s.keys[(size_t)blockIdx.x * SK_IDLE_SPAN + tid] = key;         // (read by later launches only)
  // ---- the sounding count: a ballot per wave (the whole wavefront active), the workgroup's sum in LDS, one atomic per workgroup
  const unsigned long long snd = __ballot(sounds);
  if ((tid & 63) == 0) sounding[tid >> 6] = (uint32_t)__popcll(snd);
  sk_steal_histogram(a.s, key != SK_STEAL_NOKEY, (uint32_t)(key >> sk_steal_shift(0)) & (SK_STEAL_BINS - 1), hist, tid);   // (barriers inside)
  if (tid == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < SKX_CHAN_WAVES; ++w) sum += sounding[w];
    if (sum) __hip_atomic_fetch_add((sk_gu32 *)(a.s.words + SK_CHAN_W_SOUNDING), sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!sk_arrive_last(a.s.words + SK_STEAL_W_TICKET, gridDim.x, tid, &flag)) return;
  if (tid == 0) {
    sk_gu32 *w = (sk_gu32 *)(a.s.words + SK_CHAN_W_SOUNDING);
    a.s.d_count[2] = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next query (stream-ordered)
  }
  sk_steal_pick(a.s, 0, 0ull, 0u, scan, tid);
}

extern "C" int skx_launch_chan_steal(const skx_steal_args_t *args, const uint32_t *owner, uint32_t value, uint32_t mask,
                                     hipStream_t stream) {
  skx_steal_args_t a = *args;
  a.s.base = a.s.first & ~63;
  a.s.digit = 0;
  a.idle.first = a.s.first;
  a.idle.end = a.s.end;
  const dim3 grid((unsigned)sk_idle_workgroups(a.s.first, a.s.end - a.s.first)), block(SK_IDLE_SPAN);
  hipLaunchKernelGGL(sk_fx_chan_steal_keys_kernel, grid, block, 0, stream, a, owner, value, mask);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return sk_launch_steal_select(&a.s, stream);
}
