// skred_slot_steal_kernels.hip -- which sounding copies of a tiled patch matter least: the key pass of skred_bank_find_steal_slots
// and, its MATCHED instantiation, of skred_bank_find_steal_slots_match (gfx950 / CDNA4, wave64).  include/skred_amd.h, section
// "channel polyphony", has the definition of the match.
//
// A slot is an aligned run of K voices, K a power of two <= 64, named by its first voice (skred_slot_kernels.hip).  The victim query
// on slots is the radix select of skred_steal_kernels.hip behind another key pass:
//
//   sk_slot_steal_keys_kernel  the geometry of sk_steal_keys_kernel -- SK_IDLE_SPAN voices per workgroup, spans aligned to 64 voices --
//                              so a wavefront holds 64 / K whole slots.  Every lane evaluates the terms of ITS voice
//                              (skred_steal_common.hpp: the ones sk_steal_keys_kernel is made of, from the planes the query's bits
//                              ask for); a lane without a bit in member_mask issues no load, a member that is not live reads
//                              neither its clocks nor its gain.  The slot's conditions are ballots masked with
//                              member_mask << (the slot's first lane): some member live, a live member too young, a live member
//                              still held, every member idle.  The class follows from the "held" ballot, so every lane knows which
//                              clock its slot ranks by; the 64-bit primary is reduced with a max butterfly over the slot's K lanes,
//                              log2(K) __shfl_xor steps on both halves of the word (K = 64: the last step crosses the wavefront's
//                              32-lane halves).  The lane of the slot's first voice stores the key or SK_STEAL_NOKEY, every other
//                              lane SK_STEAL_NOKEY: one key per SLOT at its first voice.  First-digit histogram and last-arriver
//                              pick as in the voice key pass.
//     <MATCH = true>           the same lines plus two things.
//                              THE OWNER GUARD: the lane of a slot's first voice reads the slot's owner word -- one load per slot --
//                              and __shfl broadcasts it to the slot's K lanes (the slot is aligned to K inside the wavefront).  A
//                              slot whose owner is 0 or fails (owner & mask) == value has no members: its lanes issue no plane
//                              load at all, it is no candidate and it is not counted.
//                              THE SOUNDING COUNT (skred_steal_common.hpp): a slot of the match with a live member that the
//                              exclusion does not call idle, whether or not it is a candidate; the sum goes to d_count[2].
//
// sk_launch_steal_select then runs unchanged: it never reads a plane, and its index-ordered tie-break works on first voices, which
// is the slot order.  No workgroup waits for another; integer atomics only; every store to global memory is a plain vector store
// or an atomic; branches on query bits and on K depend on kernel arguments only and are wave-uniform; every ballot runs with the
// whole wavefront active.  The kernel only READS the bank (matched: and the owner array).  With K = 1, mask 1 every line reduces to
// sk_steal_key's: the keys, and so the list, are the same bytes.  Matched, with mask == 0 and every sounding slot tagged, the keys,
// and so the list and the first two count words, are the plain instantiation's bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_idle_common.hpp"   // sk_idle_pred: the exclusion
#include "skred_kernel_common.hpp"
#include "skred_launch.h"
#include "skred_steal_common.hpp"

// owner, value, mask: the match (MATCH only; the plain instantiation never looks at them)
template <bool MATCH>
__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_slot_steal_keys_kernel(sk_steal_args_t a, uint64_t member_mask, int slot_voices,
                                                                          const uint32_t *__restrict__ owner, uint32_t value,
                                                                          uint32_t mask) {
  __shared__ uint32_t hist[SK_STEAL_BINS];
  __shared__ uint32_t scan[SK_IDLE_SPAN];
  __shared__ uint32_t sounding[SK_STEAL_WAVES];                // (MATCH only)
  __shared__ int flag;
  const int tid = threadIdx.x;
  bool in_range;
  const int v = sk_steal_voice(a, in_range);                   // (first and end are multiples of K: a slot is in range or out of it)
  const int lane = tid & 63, l = lane & (slot_voices - 1);
  bool match = true;
  if constexpr (MATCH) {                                       // the owner guard: one word per slot, read by the lane of its first voice ...
    uint32_t own = 0;
    if (l == 0 && in_range) own = owner[v];                    // (... in range: v < end <= n_voices)
    own = (uint32_t)__shfl((int)own, lane - l);
    match = own != 0 && (own & mask) == value;
  }
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
  bool sounds = false, cand;                                   // (sounds: MATCH only -- a candidate before its age and release terms)
  if constexpr (MATCH) {
    sounds = l == 0 && some_live != 0;                         // (a live member is a member: in range, and the owner matches)
    if (a.idle.which) sounds = sounds && (at_rest & slot) != slot;
    cand = sounds && too_young == 0;
    if (a.flags & SK_STEAL_RELEASED_ONLY) cand = cand && held == 0;
  } else {                                                     // (the same terms in the order the compiler has always seen them here)
    cand = l == 0 && in_range && some_live != 0 && too_young == 0;
    if (a.flags & SK_STEAL_RELEASED_ONLY) cand = cand && held == 0;
    if (a.idle.which) cand = cand && (at_rest & slot) != slot;
  }
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
  const uint32_t digit = (uint32_t)(key >> sk_steal_shift(0)) & (SK_STEAL_BINS - 1);
  if constexpr (MATCH) sk_steal_histogram_sounding(a, key != SK_STEAL_NOKEY, digit, hist, sounding, __ballot(sounds), tid);
  else sk_steal_histogram(a, key != SK_STEAL_NOKEY, digit, hist, tid);
  if (!sk_arrive_last(a.words + SK_STEAL_W_TICKET, gridDim.x, tid, &flag)) return;
  if constexpr (MATCH) sk_steal_sounding_publish(a, tid);
  sk_steal_pick(a, 0, 0ull, 0u, scan, tid);
}

extern "C" int sk_launch_slot_steal(const sk_steal_args_t *args, uint64_t member_mask, int slot_voices, const uint32_t *owner,
                                    uint32_t value, uint32_t mask, hipStream_t stream) {
  sk_steal_args_t a = *args;
  a.base = a.first & ~63;
  a.idle.first = a.first;
  a.idle.end = a.end;
  const dim3 grid((unsigned)sk_idle_workgroups(a.first, a.end - a.first)), block(SK_IDLE_SPAN);
  a.digit = 0;
  hipLaunchKernelGGL(owner ? sk_slot_steal_keys_kernel<true> : sk_slot_steal_keys_kernel<false>, grid, block, 0, stream, a, member_mask,
                     slot_voices, owner, value, mask);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return sk_launch_steal_select(&a, stream);
}
