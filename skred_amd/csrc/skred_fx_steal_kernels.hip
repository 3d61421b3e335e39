// skred_fx_steal_kernels.hip -- voice stealing on the fixed-point bank: the key pass (gfx950 / CDNA4, wave64).
//
// skred_fxbank_find_steal and, the MATCHED instantiation, skred_fxbank_find_steal_match (include/skred_amd_fxpt.h states the
// definitions field by field; its section "channel polyphony" has the match).  The only pass of the select that depends on the
// bank is the first one:
//
//   sk_fx_steal_keys_kernel  every workgroup takes SK_IDLE_SPAN consecutive voices (spans aligned to 64 voices, as the idle
//                            query's), evaluates the candidate predicate and the key from the planes the query's bits need --
//                            SKX_OSC word 2 (flags) and word 3 of read-write plane 0 always; SKX_TIME for OLDEST, min_age > 0 or a
//                            RELEASED_* flag; word 1 of read-write plane 0 (the smoother's gain) for QUIETEST or an ENV_DONE
//                            exclusion; SKX_OSC word 3 (amp_q15) for an AMP_ZERO exclusion -- and stores ONE key per voice
//                            (SK_STEAL_NOKEY: no candidate).  It counts the first digit, and its last arriver picks the first bin.
//     <MATCH = true>         the same lines plus two things.
//                            THE OWNER GUARD: every lane of the range loads owner[v] first.  A voice whose owner is 0 or fails
//                            (owner & mask) == value issues no plane load at all -- not the flags, not the clocks, not the
//                            exclusion's words --, is no candidate and is not counted.
//                            THE SOUNDING COUNT (skred_steal_common.hpp): a voice of the match whose envelope runs and which the
//                            exclusion does not call idle, whether or not it is a candidate; the sum goes to d_count[2].
//
// The per-voice terms are skred_fx_steal_common.hpp's, the exclusion is the idle query's own predicate (skred_fx_idle_common.hpp),
// the histogram, scan and pick are the float key pass's (skred_steal_common.hpp), and everything behind this launch is
// sk_launch_steal_select (skred_steal_kernels.hip): digit passes, count, scatter, sort.  Those read 8 bytes per voice from `keys`,
// never a plane, so they do not care which bank made them; the join of a capped burst is sk_launch_chan_join, which knows no bank.
//
// The kernel only READS the bank (matched: and the owner array): the same state gives the same bytes.  No workgroup waits for
// another; integer atomics only; every store to global memory is a plain vector store or an atomic; branches on query bits depend
// on kernel arguments only and are wave-uniform; every ballot runs with the whole wavefront active.  Matched, with mask == 0 and
// every sounding voice tagged, the keys, and so the list and the first two count words, are the plain instantiation's bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_steal_common.hpp"   // skx_steal_key, skx_steal_sounding
#include "skred_fx_steal.h"
#include "skred_kernel_common.hpp"

// owner, value, mask: the match (MATCH only; the plain instantiation never looks at them)
template <bool MATCH>
__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_fx_steal_keys_kernel(skx_steal_args_t a, const uint32_t *__restrict__ owner,
                                                                        uint32_t value, uint32_t mask) {
  __shared__ uint32_t hist[SK_STEAL_BINS];
  __shared__ uint32_t scan[SK_IDLE_SPAN];
  __shared__ uint32_t sounding[SK_STEAL_WAVES];                    // (MATCH only)
  __shared__ int flag;
  const int tid = threadIdx.x;
  const int v = a.s.base + (int)blockIdx.x * SK_IDLE_SPAN + tid;   // base: `first` rounded down to 64
  const bool in_range = v >= a.s.first && v < a.s.end;
  bool member = in_range, sounds = false;                          // no plane is read unless `member`
  if constexpr (MATCH) {                                           // the owner guard (in range: 0 <= first <= v < end <= n_voices, the owner array's length)
    uint32_t own = 0;
    if (in_range) own = owner[v];
    member = in_range && own != 0 && (own & mask) == value;
    sounds = skx_steal_sounding(a, v, member);
  }
  const sk_key_t key = skx_steal_key(a, v, member);
  a.s.keys[(size_t)blockIdx.x * SK_IDLE_SPAN + tid] = key;         // (read by later launches only)
  const uint32_t digit = (uint32_t)(key >> sk_steal_shift(0)) & (SK_STEAL_BINS - 1);
  if constexpr (MATCH) sk_steal_histogram_sounding(a.s, key != SK_STEAL_NOKEY, digit, hist, sounding, __ballot(sounds), tid);
  else sk_steal_histogram(a.s, key != SK_STEAL_NOKEY, digit, hist, tid);
  if (!sk_arrive_last(a.s.words + SK_STEAL_W_TICKET, gridDim.x, tid, &flag)) return;
  if constexpr (MATCH) sk_steal_sounding_publish(a.s, tid);
  sk_steal_pick(a.s, 0, 0ull, 0u, scan, tid);
}

extern "C" int skx_launch_steal(const skx_steal_args_t *args, const uint32_t *owner, uint32_t value, uint32_t mask, hipStream_t stream) {
  skx_steal_args_t a = *args;
  a.s.base = a.s.first & ~63;
  a.s.digit = 0;
  a.idle.first = a.s.first;
  a.idle.end = a.s.end;
  const dim3 grid((unsigned)sk_idle_workgroups(a.s.first, a.s.end - a.s.first)), block(SK_IDLE_SPAN);
  hipLaunchKernelGGL(owner ? sk_fx_steal_keys_kernel<true> : sk_fx_steal_keys_kernel<false>, grid, block, 0, stream, a, owner, value, mask);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return sk_launch_steal_select(&a.s, stream);
}
