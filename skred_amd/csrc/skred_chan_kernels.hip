// skred_chan_kernels.hip -- channel polyphony: the victim query of ONE channel of a tiled patch, and the join of a capped burst
// (gfx950 / CDNA4, wave64).  include/skred_amd.h, section "channel polyphony", has the definition.
//
//   sk_chan_steal_keys_kernel  sk_slot_steal_keys_kernel (skred_slot_steal_kernels.hip) plus two things.
//                              THE OWNER GUARD: the lane of a slot's first voice reads the slot's owner word -- one load per slot --
//                              and __shfl broadcasts it to the slot's K lanes (the slot is aligned to K inside the wavefront).  A
//                              slot whose owner is 0 or fails (owner & mask) == value has no members: its lanes issue no plane
//                              load at all, it is no candidate and it is not counted.
//                              THE SOUNDING COUNT: a slot of the match with a live member that the exclusion does not call idle.
//                              Each wave counts its slots with one ballot, the four counts meet in LDS, and ONE lane per workgroup
//                              adds the sum to a word of the steal scratch (workgroups without a sounding slot add nothing).  The
//                              last arriver -- sk_arrive_last, after the adds of every workgroup have left their CUs -- stores the
//                              sum to d_count[2] and re-arms the word.
//                              Every other line is the slot key pass's: the per-voice terms of skred_steal_common.hpp, the ballots,
//                              the max butterfly, one key per slot at its first voice, first-digit histogram, last-arriver pick.
//   sk_chan_join_kernel        one workgroup: how many notes of a burst take idle slots (the cap minus the channel's sounding
//                              count), how many steal, the victims copied behind the idle slots that are used.
//
// sk_launch_steal_select then runs unchanged.  No workgroup waits for another; integer atomics only; every store to global memory
// is a plain vector store or an atomic; branches on query bits and on K depend on kernel arguments only and are wave-uniform.  The
// key pass only READS the bank and the owner array.  With mask == 0 and every sounding slot tagged the keys, and so the list and
// the first two count words, are sk_slot_steal_keys_kernel's bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_chan.h"
#include "skred_idle_common.hpp"   // sk_idle_pred: the exclusion
#include "skred_kernel_common.hpp"
#include "skred_launch.h"
#include "skred_steal_common.hpp"

#define SK_CHAN_WAVES (SK_IDLE_SPAN / 64)

__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_chan_steal_keys_kernel(sk_steal_args_t a, uint64_t member_mask, int slot_voices,
                                                                          const uint32_t *__restrict__ owner, uint32_t value,
                                                                          uint32_t mask) {
  __shared__ uint32_t hist[SK_STEAL_BINS];
  __shared__ uint32_t scan[SK_IDLE_SPAN];
  __shared__ uint32_t sounding[SK_CHAN_WAVES];
  __shared__ int flag;
  const int tid = threadIdx.x;
  bool in_range;
  const int v = sk_steal_voice(a, in_range);                   // (first and end are multiples of K: a slot is in range or out of it)
  const int lane = tid & 63, l = lane & (slot_voices - 1);
  // ---- the owner guard: one word per slot, read by the lane of its first voice (in range: v < end <= n_voices)
  uint32_t own = 0;
  if (l == 0 && in_range) own = owner[v];
  own = (uint32_t)__shfl((int)own, lane - l);
  const bool match = own != 0 && (own & mask) == value;
  const bool member = in_range && match && ((member_mask >> l) & 1);
  // ---- this lane's voice
  uint32_t flags = 0;
  const bool live = member && sk_steal_live(a, v, flags);
  uint64_t t_start = 0, t_release = 0;
  if (sk_steal_reads_clocks(a) && live) sk_steal_clocks(a, v, t_start, t_release);
  const bool released = t_release != 0;
  const bool young = a.min_age > 0 && sk_steal_age(a, t_start) < a.min_age;
  bool idle = false;
  if (a.idle.which) idle = sk_idle_pred(a.idle, v, member);
  const unsigned long long at_rest = __ballot(idle);           // (every ballot with the whole wavefront active: none under a lane's condition)
  // ---- its slot: the members' lanes of the wavefront's ballots
  const unsigned long long slot = (unsigned long long)member_mask << (lane - l);
  const unsigned long long some_live = __ballot(live) & slot, too_young = __ballot(live && young) & slot,
                           held = __ballot(live && !released) & slot;
  bool sounds = l == 0 && some_live != 0;                      // (a live member is a member: in range, and the owner matches)
  if (a.idle.which) sounds = sounds && (at_rest & slot) != slot;
  bool cand = sounds && too_young == 0;
  if (a.flags & SK_STEAL_RELEASED_ONLY) cand = cand && held == 0;
  const sk_key_t cls = ((a.flags & SK_STEAL_RELEASED_FIRST) && held == 0) ? 0ull : 1ull;
  sk_key_t primary = 0;                                        // (a candidate has a live member: 0 never wins for it)
  if (live) primary = a.policy == SK_STEAL_OLDEST ? (cls == 0 ? t_release : t_start) : sk_steal_loudness(a, v, flags);
  for (int m = 1; m < slot_voices; m <<= 1) {                  // lanes l ^ m stay inside the slot: it is aligned to K
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)primary, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(primary >> 32), m);
    const sk_key_t other = ((sk_key_t)hi << 32) | lo;
    primary = other > primary ? other : primary;
  }
  const sk_key_t key = cand ? sk_steal_pack(cls, primary) : SK_STEAL_NOKEY;
  a.keys[(size_t)blockIdx.x * SK_IDLE_SPAN + tid] = key;       // (read by later launches only)
  // ---- the sounding count: a ballot per wave, the workgroup's sum in LDS, one atomic per workgroup
  const unsigned long long snd = __ballot(sounds);
  if (lane == 0) sounding[tid >> 6] = (uint32_t)__popcll(snd);
  sk_steal_histogram(a, key != SK_STEAL_NOKEY, (uint32_t)(key >> sk_steal_shift(0)) & (SK_STEAL_BINS - 1), hist, tid);   // (barriers inside)
  if (tid == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < SK_CHAN_WAVES; ++w) sum += sounding[w];
    if (sum) __hip_atomic_fetch_add((sk_gu32 *)(a.words + SK_CHAN_W_SOUNDING), sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!sk_arrive_last(a.words + SK_STEAL_W_TICKET, gridDim.x, tid, &flag)) return;
  if (tid == 0) {
    sk_gu32 *w = (sk_gu32 *)(a.words + SK_CHAN_W_SOUNDING);
    a.d_count[2] = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next query (stream-ordered)
  }
  sk_steal_pick(a, 0, 0ull, 0u, scan, tid);
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

extern "C" int sk_launch_chan_steal(const sk_steal_args_t *args, uint64_t member_mask, int slot_voices, const uint32_t *owner,
                                    uint32_t value, uint32_t mask, hipStream_t stream) {
  sk_steal_args_t a = *args;
  a.base = a.first & ~63;
  a.idle.first = a.first;
  a.idle.end = a.end;
  const dim3 grid((unsigned)sk_idle_workgroups(a.first, a.end - a.first)), block(SK_IDLE_SPAN);
  a.digit = 0;
  hipLaunchKernelGGL(sk_chan_steal_keys_kernel, grid, block, 0, stream, a, member_mask, slot_voices, owner, value, mask);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return sk_launch_steal_select(&a, stream);
}

extern "C" int sk_launch_chan_join(int32_t *list, const uint32_t *idle_count, const int32_t *victims, const uint32_t *victim_count,
                                   int n, uint32_t cap, uint32_t *out_count, uint32_t *d_result, hipStream_t stream) {
  hipLaunchKernelGGL(sk_chan_join_kernel, dim3(1), dim3(SK_STEAL_MAX), 0, stream, list, idle_count, victims, victim_count, n, cap,
                     out_count, d_result);
  return (int)hipGetLastError();
}
