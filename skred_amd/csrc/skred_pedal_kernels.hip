// skred_pedal_kernels.hip -- pedals: note-offs the sustain and sostenuto pedals hold back, remembered per slot on the device
// (gfx950 / CDNA4, wave64).
//
// skred_bank_stamp_owned_pedal / _release_tags_pedal / _pedal_latch / _pedal_up (include/skred_amd.h).  pedal[n_voices] lies beside
// the note-owner array (skred_owner_kernels.hip has its rules): a slot's word at its first voice, SK_PEDAL_PENDING = a note-off arrived
// and was held back, SK_PEDAL_LATCHED = sostenuto caught this note.  Only these kernels read or write it; no render kernel knows it
// exists.
//
//   sk_pedal_clear_kernel   sk_owner_tag_kernel's list rule (the first min(n, *d_count) entries that are slots of the bank) with
//                           pedal[entry] = 0: launched behind every tag launch of a bank that has a pedal array, so a new note starts
//                           with no bit of the note it replaces.  One plain dword store.
//   sk_pedal_stamps_kernel  sk_owner_stamps_kernel (one thread per entry and voice of the slot) with the stamp fixed to a release and
//                           one more decision where the owner is the expected one: hold_all != 0 or a LATCHED slot sets PENDING and
//                           stores nothing else.  The K threads of an entry lie in one wavefront and all read the word; the thread of
//                           voice 0 writes it.  The decision reads LATCHED alone, which this launch never changes, and the word
//                           stored is (word read) | PENDING: an entry named twice stores the same word twice.
//   sk_pedal_match_kernel   sk_match_stamps_kernel's geometry (one thread per voice of the range, a slot's K threads aligned to K
//                           inside a wavefront), two instantiations:
//     <UP = false>          sostenuto down.  A voice is HELD when it is live and not released -- sk_steal_live and sk_steal_clocks
//                           (skred_steal_common.hpp), the terms the slot key pass tells held members by.  A matching slot whose
//                           PENDING bit is clear and whose ballot of held voice_mask voices is not empty gets LATCHED.  Only matching
//                           slots read a plane.
//     <UP = true>           a pedal goes up.  LIFT_SOSTENUTO clears LATCHED; a slot that is then PENDING, not LATCHED and not kept by
//                           SUSTAIN_DOWN gets sk_stamp_store's release on its voice_mask voices and loses PENDING.
//                           In both, the thread of voice 0 stores the word, and only when it changed.
//
// Counts are sk_owner_count's: wave ballots, LDS, at most one atomic add per workgroup and count -- integer sums, the same whatever
// the order of arrival.  Plain vector stores and ordinary atomics only.  The stores to the planes are sk_stamp_store's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"
#include "skred_steal_common.hpp"    // sk_steal_live, sk_steal_clocks
#include "skred_update_common.hpp"   // the list rule, sk_entry_decode, sk_entry_owned, sk_range_lane, sk_stamp_store, sk_owner_count, sk_batch_done

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_pedal_clear_kernel(uint32_t *pedal, const int32_t *d_slots, int n,
                                                                       const uint32_t *d_count, int K, int n_voices) {
  const int64_t i = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  if (sk_list_looked(i, n, d_count)) {
    const int e = d_slots[i];
    if (sk_slot_valid(e, K, n_voices)) pedal[e] = 0u;
  }
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_pedal_stamps_kernel(const uint32_t *__restrict__ owner, uint32_t *pedal,
                                                                        const int32_t *d_slots, const uint32_t *__restrict__ tags, int n,
                                                                        const uint32_t *d_count, int k_shift, uint64_t voice_mask,
                                                                        int n_voices, int hold_all, sk_plane_ptrs_t p, uint64_t now,
                                                                        uint64_t *mask, uint32_t *d_result, uint32_t *cnt, uint32_t *done,
                                                                        uint32_t seq) {
  __shared__ uint32_t sums[4];
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);
  const bool mine = sk_entry_owned(owner, tags, t);
  const uint32_t word = mine ? pedal[t.e] : 0u;
  const bool hold = mine && (hold_all != 0 || (word & SK_PEDAL_LATCHED));
  if (mine && !hold && ((voice_mask >> t.l) & 1)) sk_stamp_store(p, now, mask, t.e + t.l, SKU_STAMP_RELEASE);
  if (hold && t.l == 0 && !(word & SK_PEDAL_PENDING)) pedal[t.e] = word | SK_PEDAL_PENDING;
  const bool head = t.looked && t.l == 0;                               // one thread per entry counts it
  const bool flag[4] = { head && mine && !hold, head && t.valid && !mine, head && !t.valid, head && hold };
  sk_owner_count<4>(sums, d_result, flag);
  sk_batch_done(cnt, done, seq);
}

// the view of the planes sk_steal_live and sk_steal_clocks read through (nothing else of a query is looked at)
__device__ __forceinline__ void sk_pedal_view(sk_steal_args_t &a, const sk_plane_ptrs_t &p) {
  a.idle.tab = p.ro[SKP_TAB];
  a.idle.filt = p.rw[SKS_FILT];
  a.env_s = p.ro[SKP_ENV_S];
}

template <bool UP>
__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_pedal_match_kernel(const uint32_t *__restrict__ owner, uint32_t *pedal, uint32_t value,
                                                                       uint32_t omask, int first, int count, int K, uint64_t voice_mask,
                                                                       uint32_t flags, sk_plane_ptrs_t p, uint64_t now, uint64_t *mask,
                                                                       uint32_t *d_result) {
  __shared__ uint32_t sums[UP ? 3 : 2];
  const sk_lane_t t = sk_range_lane(first, count, K);                  // (head: counts the slot and stores its word)
  const int v = t.v, l = t.l;
  const bool head = t.head;
  const int lane = (int)threadIdx.x & 63;                               // (lane - l: the lane of the slot's first voice)
  const bool hit = t.in_range && sk_owner_matches(owner[v - l], value, omask);
  const uint32_t word = hit ? pedal[v - l] : 0u;
  const bool masked = (voice_mask >> l) & 1;
  if constexpr (UP) {
    uint32_t next = word;
    if (flags & SK_PEDAL_LIFT_SOSTENUTO) next &= ~SK_PEDAL_LATCHED;
    const bool release = hit && (next & SK_PEDAL_PENDING) && !(next & SK_PEDAL_LATCHED) && !(flags & SK_PEDAL_SUSTAIN_DOWN);
    if (release) next &= ~SK_PEDAL_PENDING;
    if (release && masked) sk_stamp_store(p, now, mask, v, SKU_STAMP_RELEASE);
    if (head && hit && next != word) pedal[v] = next;
    const bool flag[3] = { head && release, head && hit && (next & SK_PEDAL_PENDING), head && !hit };
    sk_owner_count<3>(sums, d_result, flag);
  } else {
    sk_steal_args_t a = {};
    sk_pedal_view(a, p);
    bool held = false;
    if (hit && masked) {
      uint32_t vflags;
      if (sk_steal_live(a, v, vflags)) {
        uint64_t t_start, t_release;
        sk_steal_clocks(a, v, t_start, t_release);
        held = t_release == 0;
      }
    }
    const unsigned long long slot = (unsigned long long)voice_mask << (lane - l);   // (the ballot with the whole wavefront active)
    const bool some_held = (__ballot(held) & slot) != 0;
    const bool latch = hit && !(word & SK_PEDAL_PENDING) && some_held;
    if (head && latch && !(word & SK_PEDAL_LATCHED)) pedal[v] = word | SK_PEDAL_LATCHED;
    const bool flag[2] = { head && latch, head && !hit };
    sk_owner_count<2>(sums, d_result, flag);
  }
}

extern "C" int sk_launch_pedal_clear(uint32_t *pedal, const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices, int n_voices,
                                     hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(sk_pedal_clear_kernel, dim3(sk_grid(n)), dim3(SK_CONTROL_SPAN), 0, stream, pedal, d_slots, n, d_count, slot_voices,
                     n_voices);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_pedal_stamps(const uint32_t *owner, uint32_t *pedal, const int32_t *d_slots, const uint32_t *d_tags, int n,
                                      const uint32_t *d_count, int slot_voices, uint64_t voice_mask, int n_voices, int hold_all,
                                      sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t now, uint64_t *mask,
                                      uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 4, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_pedal_stamps_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, owner, pedal, d_slots, d_tags, n, d_count, sh,
                     voice_mask, n_voices, hold_all, p, now, mask, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_pedal_latch(const uint32_t *owner, uint32_t *pedal, uint32_t value, uint32_t mask, int first, int count,
                                     int slot_voices, uint64_t voice_mask, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT],
                                     uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 2, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  hipLaunchKernelGGL(sk_pedal_match_kernel<false>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, owner, pedal, value, mask,
                     first, count, slot_voices, voice_mask, 0u, p, (uint64_t)0, (uint64_t *)nullptr, d_result);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_pedal_up(const uint32_t *owner, uint32_t *pedal, uint32_t value, uint32_t mask, int first, int count,
                                  int slot_voices, uint64_t voice_mask, uint32_t flags, sk_plane_t *const ro[SKP_COUNT],
                                  sk_plane_t *const rw[SKS_COUNT], uint64_t now, uint64_t *mask_list, uint32_t *d_result,
                                  hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 3, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  hipLaunchKernelGGL(sk_pedal_match_kernel<true>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, owner, pedal, value, mask,
                     first, count, slot_voices, voice_mask, flags, p, now, mask_list, d_result);
  return (int)hipGetLastError();
}
