// skred_glide_kernels.hip -- portamento: pitch glides that advance and land on the device (gfx950 / CDNA4, wave64).
//
// skred_bank_glide_owned / _glide_tags / _glide_advance / _glide_stop (include/skred_amd.h has the definition).  glide[n_voices] lies
// beside the note-owner array: four words per voice -- target, rate_up, rate_down (fp32 bit patterns), carry (frames not yet spent,
// 0 .. 63) -- and target == 0 means "not gliding".  Only these kernels read or write it; no render kernel knows it exists.  The one
// plane word they store is voice_phase_inc (SKP_OSC word 0), as a word store: the neighbours keep what they hold.
//
//   sk_glide_clear_kernel    sk_owner_tag_kernel's list rule (the first min(n, *d_count) entries that are slots of the bank), one
//                            thread per voice of a listed slot: glide[slot + l] = 0.  Launched behind every tag launch of a bank that
//                            has a glide array, so a new note starts with no glide of the note it replaces.
//   sk_glide_start_kernel    sk_ctl_owned_each_kernel's geometry and guard (one thread per entry and voice of the slot, the owner
//                            word against the entry's tag), the workgroup's entries staged in LDS (one 16-byte load per entry, not
//                            one per voice).  FROM_SCALE: target = inc, inc = inc * scale.  TO_SCALE: target = (gliding ? the old
//                            target : inc) * scale.  ONE __fmul_rn either way; where the product or inc is zero or not finite nothing
//                            is stored and the start counts as withheld.
//   sk_glide_advance_kernel  one thread per voice of the range.  A voice that does not glide costs its 16-byte load and nothing else.
//                            A gliding one loads its increment, makes up to (carry + F) >> 6 products -- __fmul_rn, one per 64
//                            frames -- and stores the last one, or on arrival the target's bits and four zero words.
//   sk_glide_stop_kernel     one thread per voice of the range: the words cleared, with snap the target stored first.
//
// |x| < |y| on finite fp32 values is decided on the bit patterns without their sign bits, as integers: the same order, and no
// question of how a comparison treats a denormal.
//
// BEND.  The start, advance and stop kernels are templates: the BEND = true instantiations serve a bank that has a pitch-wheel array
// (skred_bend_kernels.hip; include/skred_amd.h, "glides under a bend").  On a voice whose key word is not 0 the glide runs on the KEY
// -- every read and store of the increment below is one of bend[v].key -- and the sounding increment is stored again as key * ratio
// (sk_glide_sound: one multiply, that store withheld where the product is zero or not finite).  On a voice with key == 0 they take
// the BEND = false path; the BEND = false instantiations are the kernels as they were (profiles/glide_usage.txt).  Counts are sk_owner_count's: wave ballots, LDS, at most one atomic add per
// workgroup and count -- integer sums, the same whatever the order of arrival.  Plain vector stores and ordinary atomics only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"
#include "skred_update_common.hpp"   // sk_entry_decode, sk_entry_owned, sk_owner_count, sk_batch_done, the launch helpers

#define SK_GLIDE_ABS 0x7fffffffu

__device__ __forceinline__ bool sk_glide_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }
// a value a glide can start from or aim at: finite and not zero
__device__ __forceinline__ bool sk_glide_usable(uint32_t bits) { return sk_glide_finite(bits) && (bits & SK_GLIDE_ABS) != 0u; }
__device__ __forceinline__ uint32_t sk_glide_mul(uint32_t a, uint32_t b) {
  return __float_as_uint(__fmul_rn(__uint_as_float(a), __uint_as_float(b)));
}
__device__ __forceinline__ uint32_t *sk_glide_inc(sk_plane_t *osc, int v) { return &osc[v].w[0]; }

// what the BEND instantiations take beside the rest (BEND false: an empty struct the kernel never reads)
template <bool BEND> struct sk_glide_bend_t {};
template <> struct sk_glide_bend_t<true> {
  sk_bend_t *bend;
};
// where voice v's glide reads and stores its increment: the key word of a bent voice, else voice_phase_inc.  ratio: the bent voice's
// (0: not bent, and sk_glide_sound has nothing to do)
template <bool BEND>
__device__ __forceinline__ uint32_t *sk_glide_word(const sk_glide_bend_t<BEND> &ba, sk_plane_t *osc, int v, uint32_t &ratio) {
  ratio = 0u;
  if constexpr (BEND) {
    const uint2 b = *reinterpret_cast<const uint2 *>(&ba.bend[v]);      // key, ratio
    if (b.x) {
      ratio = b.y;
      return &ba.bend[v].w[SK_BEND_KEY];
    }
  }
  return sk_glide_inc(osc, v);
}
// a bent voice's sounding increment after its key moved or was confirmed: key * ratio, ONE multiply, withheld if zero or not finite
__device__ __forceinline__ void sk_glide_sound(sk_plane_t *osc, int v, uint32_t key, uint32_t ratio) {
  const uint32_t p = sk_glide_mul(key, ratio);
  if (sk_glide_usable(p)) *sk_glide_inc(osc, v) = p;
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_glide_clear_kernel(sk_glide_t *glide, const int32_t *d_slots, int n,
                                                                       const uint32_t *d_count, int k_shift, int n_voices) {
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);
  if (t.valid) *reinterpret_cast<uint4 *>(&glide[t.e + t.l]) = make_uint4(0u, 0u, 0u, 0u);
}

template <bool BEND>
__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_glide_start_kernel(sk_glide_t *glide, const sk_glide_each_t *__restrict__ each,
                                                                       int k_shift, uint64_t voice_mask, const int32_t *d_slots,
                                                                       const uint32_t *__restrict__ tags,
                                                                       const uint32_t *__restrict__ owner, int n, const uint32_t *d_count,
                                                                       int n_voices, sk_plane_t *osc, uint32_t *d_result, uint32_t *cnt,
                                                                       uint32_t *done, uint32_t seq, sk_glide_bend_t<BEND> ba) {
  __shared__ uint4 ent[SK_CONTROL_SPAN];                                  // set, rate_up, rate_down, scale of this workgroup's entries
  __shared__ uint32_t sums[3];
  const int per_wg = SK_CONTROL_SPAN >> k_shift;
  const int64_t base = (int64_t)blockIdx.x * per_wg;
  if ((int)threadIdx.x < per_wg && base + (int)threadIdx.x < n)
    ent[threadIdx.x] = *reinterpret_cast<const uint4 *>(&each[base + (int)threadIdx.x].w[0]);
  __syncthreads();
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);   // (t.i == base + the entry's place)
  const bool owned = sk_entry_owned(owner, tags, t);
  bool started = false, withheld = false;
  if (owned && ((voice_mask >> t.l) & 1)) {
    const int v = t.e + t.l;
    const uint4 g = ent[(int)threadIdx.x >> k_shift];
    uint32_t ratio;
    uint32_t *const word = sk_glide_word<BEND>(ba, osc, v, ratio);
    const uint32_t inc = *word;
    uint32_t target, next = inc;
    if (g.x & SK_GLIDE_FROM_SCALE) {
      target = inc;
      next = sk_glide_mul(inc, g.w);
    } else {
      const uint32_t old = glide[v].w[SK_GLIDE_TARGET];
      target = sk_glide_mul(old ? old : inc, g.w);
    }
    if (sk_glide_usable(inc) && sk_glide_usable(target) && sk_glide_usable(next)) {
      if (next != inc) *word = next;
      *reinterpret_cast<uint4 *>(&glide[v]) = make_uint4(target, g.y, g.z, 0u);
      if (BEND && ratio) sk_glide_sound(osc, v, next, ratio);
      started = true;
    } else {
      withheld = true;
    }
  }
  const bool flag[3] = { started, withheld, t.valid && !owned && t.l == 0 };
  sk_owner_count<3>(sums, d_result, flag);
  sk_batch_done(cnt, done, seq);
}

template <bool BEND>
__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_glide_advance_kernel(sk_glide_t *glide, sk_plane_t *osc, int first, int count,
                                                                         uint32_t frames, uint32_t *d_result, sk_glide_bend_t<BEND> ba) {
  __shared__ uint32_t sums[2];
  const int64_t off = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  bool still = false, arrived = false;
  if (off < count) {
    const int v = first + (int)off;
    const uint4 g = *reinterpret_cast<const uint4 *>(&glide[v]);       // target, rate_up, rate_down, carry
    if (g.x != 0u) {
      uint32_t ratio;
      uint32_t *const word = sk_glide_word<BEND>(ba, osc, v, ratio);
      const uint32_t inc0 = *word, t = g.x & SK_GLIDE_ABS;
      uint32_t inc = inc0;
      bool there = !sk_glide_usable(inc) || ((inc ^ g.x) >> 31);        // a glide cannot cross zero
      const uint32_t c = g.w + frames;
      for (uint32_t m = c >> 6; m && !there; --m) {
        const uint32_t a = inc & SK_GLIDE_ABS;
        if (a < t) {
          inc = sk_glide_mul(inc, g.y);
          there = !sk_glide_finite(inc) || (inc & SK_GLIDE_ABS) >= t;
        } else if (a > t) {
          inc = sk_glide_mul(inc, g.z);
          there = !sk_glide_finite(inc) || (inc & SK_GLIDE_ABS) <= t;
        } else {
          there = true;
        }
      }
      if (there) {
        *word = g.x;
        *reinterpret_cast<uint4 *>(&glide[v]) = make_uint4(0u, 0u, 0u, 0u);
        arrived = true;
        inc = g.x;
      } else {
        if (inc != inc0) *word = inc;                                   // (not arrived: every product was finite)
        glide[v].w[SK_GLIDE_CARRY] = c & 63u;
        still = true;
      }
      if (BEND && ratio) sk_glide_sound(osc, v, inc, ratio);
    }
  }
  const bool flag[2] = { still, arrived };
  sk_owner_count<2>(sums, d_result, flag);
}

template <bool BEND>
__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_glide_stop_kernel(sk_glide_t *glide, sk_plane_t *osc, int first, int count, int snap,
                                                                      sk_glide_bend_t<BEND> ba) {
  const int64_t off = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  if (off >= count) return;
  const int v = first + (int)off;
  const uint4 g = *reinterpret_cast<const uint4 *>(&glide[v]);
  if (!(g.x | g.y | g.z | g.w)) return;
  if (snap && g.x) {
    uint32_t ratio;
    *sk_glide_word<BEND>(ba, osc, v, ratio) = g.x;
    if (BEND && ratio) sk_glide_sound(osc, v, g.x, ratio);
  }
  *reinterpret_cast<uint4 *>(&glide[v]) = make_uint4(0u, 0u, 0u, 0u);
}

extern "C" int sk_launch_glide_clear(sk_glide_t *glide, const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices,
                                     int n_voices, hipStream_t stream) {
  if (n <= 0) return 0;
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_glide_clear_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, glide, d_slots, n, d_count, sh,
                     n_voices);
  return (int)hipGetLastError();
}

// bend == NULL: the BEND = false instantiations, the kernels of a bank without a pitch-wheel array; else BEND = true
extern "C" int sk_launch_glide_start(sk_glide_t *glide, sk_bend_t *bend, const sk_glide_each_t *d_each, int slot_voices, uint64_t voice_mask,
                                     const int32_t *d_slots, const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count,
                                     int n_voices, sk_plane_t *osc, uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq,
                                     hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 3, stream);
  if (e != hipSuccess) return (int)e;
  const int sh = sk_slot_shift(slot_voices);
  if (bend) {
    sk_glide_bend_t<true> ba;
    ba.bend = bend;
    hipLaunchKernelGGL(sk_glide_start_kernel<true>, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, glide, d_each, sh, voice_mask,
                       d_slots, d_tags, owner, n, d_count, n_voices, osc, d_result, cnt, done, seq, ba);
  } else {
    hipLaunchKernelGGL(sk_glide_start_kernel<false>, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, glide, d_each, sh, voice_mask,
                       d_slots, d_tags, owner, n, d_count, n_voices, osc, d_result, cnt, done, seq, sk_glide_bend_t<false>());
  }
  return (int)hipGetLastError();
}

extern "C" int sk_launch_glide_advance(sk_glide_t *glide, sk_bend_t *bend, sk_plane_t *osc, int first, int count, int num_frames,
                                       uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 2, stream);
  if (e != hipSuccess) return (int)e;
  if (bend) {
    sk_glide_bend_t<true> ba;
    ba.bend = bend;
    hipLaunchKernelGGL(sk_glide_advance_kernel<true>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, glide, osc, first, count,
                       (uint32_t)num_frames, d_result, ba);
  } else {
    hipLaunchKernelGGL(sk_glide_advance_kernel<false>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, glide, osc, first, count,
                       (uint32_t)num_frames, d_result, sk_glide_bend_t<false>());
  }
  return (int)hipGetLastError();
}

extern "C" int sk_launch_glide_stop(sk_glide_t *glide, sk_bend_t *bend, sk_plane_t *osc, int first, int count, int snap, hipStream_t stream) {
  if (count <= 0) return 0;
  if (bend) {
    sk_glide_bend_t<true> ba;
    ba.bend = bend;
    hipLaunchKernelGGL(sk_glide_stop_kernel<true>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, glide, osc, first, count, snap, ba);
  } else {
    hipLaunchKernelGGL(sk_glide_stop_kernel<false>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, glide, osc, first, count, snap,
                       sk_glide_bend_t<false>());
  }
  return (int)hipGetLastError();
}
