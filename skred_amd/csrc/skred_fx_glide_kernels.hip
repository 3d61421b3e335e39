// skred_fx_glide_kernels.hip -- portamento on the fixed-point bank: pitch glides that advance and land on the device, in integers
// (gfx950 / CDNA4, wave64).
//
// skred_fxbank_glide_owned / _glide_tags / _glide_advance / _glide_stop (include/skred_amd_fxpt.h has the definition).  glide[n_voices]
// lies beside the note-owner array of skred_fx_owner.c: four words per voice -- target, up_q32, down_q32, carry (frames not yet spent,
// 0 .. 63) -- and target == 0 means "not gliding".  Only these kernels and the float bank's sk_glide_clear_kernel (entered through its
// launcher at slot_voices = 1 behind every tag launch of a bank that has the array) read or write it; no render kernel knows it exists.
// The one bank word they store is phase_inc (SKX_OSC word 0), as a word store: the neighbours in the plane keep their bits.
//
//   sk_fx_glide_start_kernel    sk_fx_ctl_owned_each_kernel's geometry and guard (one thread per entry of a list in device memory, the
//                               owner word against the entry's tag; the list rule and the guard are sk_entry_decode / sk_entry_owned at
//                               one voice per slot).  An owned entry loads its 16 bytes set, up_q32, down_q32, scale_q16 -- lane k reads
//                               entry k: consecutive lanes, consecutive 32-byte records -- and, for TO_INC alone, one word more.
//                               FROM_SCALE: target = inc, inc = (inc * scale) >> 16.  TO_SCALE: target = ((gliding ? the old target :
//                               inc) * scale) >> 16.  TO_INC: target = target_inc.  64-bit products; where inc, the new inc or the
//                               target is 0 or above 0xFFFFFFFF nothing is stored and the start counts as withheld.
//   sk_fx_glide_advance_kernel  one thread per voice of the range.  A voice that does not glide costs its 16-byte load and nothing else.
//                               A gliding one loads its increment, takes up to (carry + F) >> 6 steps -- skx_step_64: one 32 x 32 ->
//                               high-word multiply, a max and an add or subtract per 64 frames -- and stores the last increment (only if it
//                               differs) and the carry, or on arrival the target's bits and four zero words.
//   sk_fx_glide_stop_kernel     one thread per voice of the range: the words cleared, with snap the target stored first.
//
// BEND.  The start, advance and stop kernels are templates: the BEND = true instantiations serve a bank that has a pitch-wheel array
// (skred_fx_bend_kernels.hip; include/skred_amd_fxpt.h, "glides under a bend").  On a voice whose key word is not 0 the glide runs on
// the KEY -- every read and store of the increment below is one of bend[v].key -- and the sounding increment is stored again as
// (key * ratio_q24) >> 24 (skx_glide_sound: one 64-bit product, that store withheld where it is 0 or above 0xFFFFFFFF).  On a voice
// with key == 0 they take the BEND = false path; the BEND = false instantiations are the kernels as they were
// (profiles/fxglide_usage.txt, profiles/fxbend_usage.txt).
//
// Every step is exact integer arithmetic: the same bits on every machine.  Counts are sk_owner_count's: wave ballots, LDS, at most one
// atomic add per workgroup and count -- integer sums, the same whatever the order of arrival.  Plain vector stores and ordinary atomics
// only; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_layout.h"
#include "skred_launch.h"
#include "skred_fx_step_common.hpp"     // skx_step_64: the 64-frame step, stated once for the glide and the filter cutoff
#include "skred_update_common.hpp"   // sk_entry_decode, sk_entry_owned, sk_owner_count, sk_grid, sk_list_grid, sk_result_clear

static_assert(sizeof(skx_glide_t) == 16 && sizeof(skx_glide_each_t) == 32, "one 16-byte load per voice, one per entry");

__device__ __forceinline__ uint32_t *skx_glide_inc(skx_plane_t *osc, int v) { return &osc[v].w[0]; }

// what the BEND instantiations take beside the rest (BEND false: an empty struct the kernel never reads)
template <bool BEND> struct skx_glide_bend_t {};
template <> struct skx_glide_bend_t<true> {
  skx_bend_t *bend;
};
// where voice v's glide reads and stores its increment: the key word of a bent voice, else phase_inc.  ratio: the bent voice's
// (0: not bent -- a stored ratio is never 0 -- and skx_glide_sound has nothing to do)
template <bool BEND>
__device__ __forceinline__ uint32_t *skx_glide_word(const skx_glide_bend_t<BEND> &ba, skx_plane_t *osc, int v, uint32_t &ratio) {
  ratio = 0u;
  if constexpr (BEND) {
    const uint2 b = *reinterpret_cast<const uint2 *>(&ba.bend[v]);      // key, ratio_q24
    if (b.x) {
      ratio = b.y;
      return &ba.bend[v].w[SKX_BEND_KEY];
    }
  }
  return skx_glide_inc(osc, v);
}
// a bent voice's sounding increment after its key moved or was confirmed: (key * ratio_q24) >> 24, withheld if 0 or above 32 bits
__device__ __forceinline__ void skx_glide_sound(skx_plane_t *osc, int v, uint32_t key, uint32_t ratio) {
  const uint64_t p = ((uint64_t)key * (uint64_t)ratio) >> 24;
  if (p >= 1ull && p <= 0xFFFFFFFFull) *skx_glide_inc(osc, v) = (uint32_t)p;
}

template <bool BEND>
__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_glide_start_kernel(skx_glide_t *glide, const skx_glide_each_t *__restrict__ each,
                                                                          const int32_t *d_voices, const uint32_t *__restrict__ tags,
                                                                          const uint32_t *__restrict__ owner, int n, const uint32_t *d_count,
                                                                          int n_voices, skx_plane_t *osc, uint32_t *d_result,
                                                                          skx_glide_bend_t<BEND> ba) {
  __shared__ uint32_t sums[3];
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, 0, d_voices, n, d_count, n_voices);   // (valid: 0 <= t.e < n_voices)
  const bool owned = sk_entry_owned(owner, tags, t);
  bool started = false, withheld = false;
  if (owned) {
    const int v = t.e;
    const uint4 g = *reinterpret_cast<const uint4 *>(&each[t.i].w[0]);   // set, up_q32, down_q32, scale_q16
    uint32_t ratio;
    uint32_t *const word = skx_glide_word<BEND>(ba, osc, v, ratio);
    const uint32_t inc = *word;
    uint64_t target, next = inc;
    if (g.x & SKX_GLIDE_FROM_SCALE) {
      target = inc;
      next = ((uint64_t)inc * (uint64_t)g.w) >> 16;
    } else if (g.x & SKX_GLIDE_TO_SCALE) {
      const uint32_t old = glide[v].w[SKX_GLIDE_TARGET];
      target = ((uint64_t)(old ? old : inc) * (uint64_t)g.w) >> 16;
    } else {
      target = each[t.i].w[SKX_GLIDE_E_TARGET_INC];
    }
    if (inc != 0u && next >= 1ull && next <= 0xFFFFFFFFull && target >= 1ull && target <= 0xFFFFFFFFull) {
      if ((uint32_t)next != inc) *word = (uint32_t)next;
      *reinterpret_cast<uint4 *>(&glide[v]) = make_uint4((uint32_t)target, g.y, g.z, 0u);
      if (BEND && ratio) skx_glide_sound(osc, v, (uint32_t)next, ratio);
      started = true;
    } else {
      withheld = true;
    }
  }
  const bool flag[3] = { started, withheld, t.valid && !owned };
  sk_owner_count<3>(sums, d_result, flag);
}

template <bool BEND>
__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_glide_advance_kernel(skx_glide_t *glide, skx_plane_t *osc, int first, int count,
                                                                            uint32_t frames, uint32_t *d_result, skx_glide_bend_t<BEND> ba) {
  __shared__ uint32_t sums[2];
  const int64_t off = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  bool still = false, arrived = false;
  if (off < count) {
    const int v = first + (int)off;                                     // (inside the bank: checked on the host)
    const uint4 g = *reinterpret_cast<const uint4 *>(&glide[v]);       // target, up_q32, down_q32, carry
    if (g.x != 0u) {
      uint32_t ratio;
      uint32_t *const word = skx_glide_word<BEND>(ba, osc, v, ratio);
      const uint32_t inc0 = *word, target = g.x;
      uint32_t inc = inc0;
      bool there = inc == 0u || inc == target;
      const uint32_t c = g.w + frames;                                  // (carry <= 63, frames <= 65536)
      for (uint32_t m = c >> 6; m && !there; --m) there = skx_step_64(inc, target, g.y, g.z);   // (the step the filter cutoff shares)
      if (there) {
        *word = target;
        *reinterpret_cast<uint4 *>(&glide[v]) = make_uint4(0u, 0u, 0u, 0u);
        arrived = true;
        inc = target;
      } else {
        if (inc != inc0) *word = inc;
        glide[v].w[SKX_GLIDE_CARRY] = c & 63u;
        still = true;
      }
      if (BEND && ratio) skx_glide_sound(osc, v, inc, ratio);
    }
  }
  const bool flag[2] = { still, arrived };
  sk_owner_count<2>(sums, d_result, flag);
}

template <bool BEND>
__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_glide_stop_kernel(skx_glide_t *glide, skx_plane_t *osc, int first, int count, int snap,
                                                                         skx_glide_bend_t<BEND> ba) {
  const int64_t off = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  if (off >= count) return;
  const int v = first + (int)off;
  const uint4 g = *reinterpret_cast<const uint4 *>(&glide[v]);
  if (!(g.x | g.y | g.z | g.w)) return;
  if (snap && g.x) {
    uint32_t ratio;
    *skx_glide_word<BEND>(ba, osc, v, ratio) = g.x;
    if (BEND && ratio) skx_glide_sound(osc, v, g.x, ratio);
  }
  *reinterpret_cast<uint4 *>(&glide[v]) = make_uint4(0u, 0u, 0u, 0u);
}

// bend == NULL: the BEND = false instantiations, the kernels of a bank without a pitch-wheel array; else BEND = true.
// d_each: 16-byte aligned; d_result[3] (or NULL; zeroed on `stream` ahead of the kernel): voices set gliding, starts withheld, voices
// whose owner differs
extern "C" int skx_launch_glide_start(skx_glide_t *glide, skx_bend_t *bend, const skx_glide_each_t *d_each, const int32_t *d_voices, const uint32_t *d_tags,
                                      const uint32_t *owner, int n, const uint32_t *d_count, int n_voices, skx_plane_t *osc,
                                      uint32_t *d_result, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 3, stream);
  if (e != hipSuccess) return (int)e;
  if (bend) {
    skx_glide_bend_t<true> ba;
    ba.bend = bend;
    hipLaunchKernelGGL(sk_fx_glide_start_kernel<true>, dim3(sk_list_grid(n, 0)), dim3(SK_CONTROL_SPAN), 0, stream, glide, d_each, d_voices,
                       d_tags, owner, n, d_count, n_voices, osc, d_result, ba);
  } else {
    hipLaunchKernelGGL(sk_fx_glide_start_kernel<false>, dim3(sk_list_grid(n, 0)), dim3(SK_CONTROL_SPAN), 0, stream, glide, d_each, d_voices,
                       d_tags, owner, n, d_count, n_voices, osc, d_result, skx_glide_bend_t<false>());
  }
  return (int)hipGetLastError();
}

// d_result[2] (or NULL; zeroed on `stream` ahead of the kernel): voices still gliding, voices that arrived
extern "C" int skx_launch_glide_advance(skx_glide_t *glide, skx_bend_t *bend, skx_plane_t *osc, int first, int count, int num_frames, uint32_t *d_result,
                                        hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 2, stream);
  if (e != hipSuccess) return (int)e;
  if (bend) {
    skx_glide_bend_t<true> ba;
    ba.bend = bend;
    hipLaunchKernelGGL(sk_fx_glide_advance_kernel<true>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, glide, osc, first, count,
                       (uint32_t)num_frames, d_result, ba);
  } else {
    hipLaunchKernelGGL(sk_fx_glide_advance_kernel<false>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, glide, osc, first, count,
                       (uint32_t)num_frames, d_result, skx_glide_bend_t<false>());
  }
  return (int)hipGetLastError();
}

extern "C" int skx_launch_glide_stop(skx_glide_t *glide, skx_bend_t *bend, skx_plane_t *osc, int first, int count, int snap,
                                     hipStream_t stream) {
  if (count <= 0) return 0;
  if (bend) {
    skx_glide_bend_t<true> ba;
    ba.bend = bend;
    hipLaunchKernelGGL(sk_fx_glide_stop_kernel<true>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, glide, osc, first, count, snap, ba);
  } else {
    hipLaunchKernelGGL(sk_fx_glide_stop_kernel<false>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, glide, osc, first, count, snap,
                       skx_glide_bend_t<false>());
  }
  return (int)hipGetLastError();
}
