// skred_fx_pedal_kernels.hip -- pedals on the fixed-point bank: note-offs the sustain and sostenuto pedals hold back, remembered per
// voice on the device (gfx950 / CDNA4, wave64).
//
// skred_fxbank_stamp_owned_pedal / _release_tags_pedal / _pedal_latch / _pedal_up (include/skred_amd_fxpt.h).  pedal[n_voices] lies
// beside the note-owner array of skred_fx_owner.c: one word per voice, SK_PEDAL_PENDING = a note-off arrived and was held back,
// SK_PEDAL_LATCHED = sostenuto caught this note.  Only these kernels and the float bank's sk_pedal_clear_kernel (entered through its
// launcher at slot_voices = 1 behind every tag launch of a bank that has the array) read or write it; no render kernel knows it exists.
//
//   sk_fx_pedal_stamps_kernel  sk_fx_stamp_owned_kernel (one lane per entry of a list in device memory) with the stamp fixed to a
//                              release and one more decision where the owner is the expected one: hold_all != 0 or a LATCHED voice
//                              sets PENDING and stores nothing else.  The decision reads LATCHED alone, which this launch never
//                              changes, and the word stored is (word read) | PENDING: an entry named twice stores the same word twice.
//   sk_fx_pedal_match_kernel   sk_fx_match_stamps_kernel's geometry (one lane per voice of the range, 64 consecutive voices per
//                              wavefront); the owner word is loaded first, the pedal word and the planes on a hit only.
//     <UP = false>             sostenuto down.  A matching voice whose PENDING bit is clear and that is HELD (skx_steal_held: an
//                              envelope that runs, no release clock) gets LATCHED.
//     <UP = true>              a pedal goes up.  LIFT_SOSTENUTO clears LATCHED; a voice that is then PENDING, not LATCHED and not kept
//                              by SUSTAIN_DOWN gets skx_stamp_store's release and loses PENDING.
//                              In both, every lane owns its voice's word and stores it only when it changed.
//
// Counts are skx_count's: wave ballots, LDS, at most one atomic add per workgroup and count -- integer sums, the same whatever the
// order of arrival.  Plain vector stores and ordinary atomics only; no workgroup waits for another.  The stores to the planes are
// skx_stamp_store's: a voice whose envelope is not active gets no release clock and is counted as stamped or released all the same,
// as sk_fx_stamp_owned_kernel counts it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"              // SK_PEDAL_*, sk_owner_matches
#include "skred_fx_ctl_common.hpp"     // skx_stamp_store, skx_list_looked, skx_count, skx_grid
#include "skred_fx_steal_common.hpp"   // skx_steal_held
#include "skred_fx_layout.h"

static_assert(SKX_CTL_SPAN == 256 && SKX_CTL_SPAN % 64 == 0, "skx_count and the launch geometry are written for this span");

__global__ __launch_bounds__(SKX_CTL_SPAN) void sk_fx_pedal_stamps_kernel(const uint32_t *__restrict__ owner, uint32_t *pedal,
                                                                          const int32_t *d_voices, const uint32_t *__restrict__ tags, int n,
                                                                          const uint32_t *d_count, int n_voices, int hold_all,
                                                                          skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now,
                                                                          uint32_t *d_result) {
  __shared__ uint32_t sums[4];
  const int64_t i = (int64_t)blockIdx.x * SKX_CTL_SPAN + threadIdx.x;
  const bool looked = skx_list_looked(i, n, d_count);
  bool valid = false, mine = false, hold = false;
  if (looked) {
    const int v = d_voices[i];
    valid = v >= 0 && v < n_voices;
    if (valid) mine = owner[v] == tags[i];                              // (tags are non-zero: an untagged voice never matches)
    if (mine) {
      const uint32_t word = pedal[v];
      hold = hold_all != 0 || (word & SK_PEDAL_LATCHED);
      if (!hold) skx_stamp_store(time_plane, rw0, v, SKXS_STAMP_RELEASE, now);
      else if (!(word & SK_PEDAL_PENDING)) pedal[v] = word | SK_PEDAL_PENDING;
    }
  }
  const uint32_t val[4] = { (mine && !hold) ? 1u : 0u, (valid && !mine) ? 1u : 0u, (looked && !valid) ? 1u : 0u, hold ? 1u : 0u };
  skx_count<4>(sums, d_result, val);
}

template <bool UP>
__global__ __launch_bounds__(SKX_CTL_SPAN) void sk_fx_pedal_match_kernel(const uint32_t *__restrict__ owner, uint32_t *pedal, uint32_t value,
                                                                         uint32_t omask, int first, int count, uint32_t flags,
                                                                         const skx_plane_t *osc, skx_plane_t *time_plane, skx_plane_t *rw0,
                                                                         uint64_t now, uint32_t *d_result) {
  __shared__ uint32_t sums[UP ? 3 : 2];
  const int64_t off = (int64_t)blockIdx.x * SKX_CTL_SPAN + threadIdx.x;
  const bool in_range = off < count;
  const int v = first + (int)(in_range ? off : 0);                      // (inside the bank: checked on the host)
  const bool hit = in_range && sk_owner_matches(owner[v], value, omask);
  const uint32_t word = hit ? pedal[v] : 0u;
  if constexpr (UP) {
    uint32_t next = word;
    if (flags & SK_PEDAL_LIFT_SOSTENUTO) next &= ~SK_PEDAL_LATCHED;
    const bool release = hit && (next & SK_PEDAL_PENDING) && !(next & SK_PEDAL_LATCHED) && !(flags & SK_PEDAL_SUSTAIN_DOWN);
    if (release) {
      next &= ~SK_PEDAL_PENDING;
      skx_stamp_store(time_plane, rw0, v, SKXS_STAMP_RELEASE, now);
    }
    if (hit && next != word) pedal[v] = next;
    const uint32_t val[3] = { release ? 1u : 0u, (hit && (next & SK_PEDAL_PENDING)) ? 1u : 0u, (in_range && !hit) ? 1u : 0u };
    skx_count<3>(sums, d_result, val);
  } else {
    const bool latch = hit && !(word & SK_PEDAL_PENDING) && skx_steal_held(osc, rw0, time_plane, v);
    if (latch && !(word & SK_PEDAL_LATCHED)) pedal[v] = word | SK_PEDAL_LATCHED;
    const uint32_t val[2] = { latch ? 1u : 0u, (in_range && !hit) ? 1u : 0u };
    skx_count<2>(sums, d_result, val);
  }
}

extern "C" int skx_launch_pedal_stamps(const uint32_t *owner, uint32_t *pedal, const int32_t *d_voices, const uint32_t *d_tags, int n,
                                       const uint32_t *d_count, int n_voices, int hold_all, skx_plane_t *time_plane, skx_plane_t *rw0,
                                       uint64_t now, uint32_t *d_result, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = hipMemsetAsync(d_result, 0, 4 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_fx_pedal_stamps_kernel, dim3(skx_grid(n)), dim3(SKX_CTL_SPAN), 0, stream, owner, pedal, d_voices, d_tags, n,
                     d_count, n_voices, hold_all, time_plane, rw0, now, d_result);
  return (int)hipGetLastError();
}

extern "C" int skx_launch_pedal_latch(const uint32_t *owner, uint32_t *pedal, uint32_t value, uint32_t mask, int first, int count,
                                      const skx_plane_t *osc, skx_plane_t *time_plane, skx_plane_t *rw0, uint32_t *d_result,
                                      hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_fx_pedal_match_kernel<false>, dim3(skx_grid(count)), dim3(SKX_CTL_SPAN), 0, stream, owner, pedal, value, mask,
                     first, count, 0u, osc, time_plane, rw0, (uint64_t)0, d_result);
  return (int)hipGetLastError();
}

extern "C" int skx_launch_pedal_up(const uint32_t *owner, uint32_t *pedal, uint32_t value, uint32_t mask, int first, int count,
                                   uint32_t flags, skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now, uint32_t *d_result,
                                   hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = hipMemsetAsync(d_result, 0, 3 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_fx_pedal_match_kernel<true>, dim3(skx_grid(count)), dim3(SKX_CTL_SPAN), 0, stream, owner, pedal, value, mask,
                     first, count, flags, (const skx_plane_t *)nullptr, time_plane, rw0, now, d_result);
  return (int)hipGetLastError();
}
