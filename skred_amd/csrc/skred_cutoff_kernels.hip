// skred_cutoff_kernels.hip -- filter cutoff on the device: key-tracked cutoffs that glide and land (gfx950 / CDNA4, wave64).
//
// skred_bank_cutoff_match / _cutoff_owned_each / _cutoff_tags_each / _cutoff_advance / _cutoff_stop (include/skred_amd.h has the
// definition).  cut[n_voices] lies beside the bend array: eight words per voice, two uint4 -- w, target, rate_up, rate_down (fp32 bit
// patterns; w == 0: no device cutoff, target == 0: not moving) and carry (0 .. 63), q, mode, 0.  Only these kernels read or write it;
// no render kernel knows it exists.  The plane words they store are the five coefficients (skred_cutoff_common.hpp: sk_cutoff_store),
// as word stores; they read voice_phase_inc (SKP_OSC word 0) and, on a bank with a pitch-wheel array, a bent voice's key.
//
//   sk_cutoff_clear_kernel    sk_glide_clear_kernel on this array: one thread per voice of a listed slot, both halves zeroed.
//                             Launched behind every tag launch of a bank that has a cutoff array.
//   sk_cutoff_match_kernel    sk_ctl_match_kernel's geometry, guard and counting: THE RULE (sk_cutoff_apply) to one record, a kernel
//                             argument.
//   sk_cutoff_each_kernel     sk_glide_start_kernel's geometry and guard, the workgroup's records staged in LDS (one 16-byte and one
//                             8-byte load per entry, not one per voice).
//   sk_cutoff_advance_kernel  one thread per voice of the range.  A voice that does not move costs its 16-byte load and nothing else.
//                             A moving one loads its second half, makes up to (carry + F) >> 6 products -- __fmul_rn, one per 64
//                             frames -- stores the last one, or on arrival the target's bits, and computes the coefficients ONCE.
//   sk_cutoff_stop_kernel     one thread per voice of the range: target, rates and carry cleared; with snap w = target first.
//
// THE FILTER ENVELOPE (skred_bank_fenv.c, skred_fenv_kernels.hip).  On a bank that has an fenv array the match, each and stop kernels
// receive it (NULL otherwise: a wave-uniform branch, and the bytes stored are the ones stored without it) and zero the eight fenv
// words of every voice they set, start or stop: a new cutoff ends the contour.  The advance kernel is a template: ENV = false is the
// kernel as it was (profiles/cutoff_usage.txt), ENV = true loads the voice's stage word beside its first half and hands a voice that
// has a contour to sk_fenv_advance (skred_fenv_common.hpp), which also reads its release clock.
//
// Every w is positive and finite, so w < target is decided on the bit patterns as integers (sk_glide_advance_kernel's rule without a
// sign to mask).  Counts are sk_owner_count's.  Plain vector stores and ordinary atomics only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"
#include "skred_cutoff_common.hpp"
#include "skred_fenv_common.hpp"
#include "skred_update_common.hpp"   // sk_entry_decode, sk_entry_owned, sk_range_lane, sk_owner_count, sk_batch_done, the launch helpers

__device__ __forceinline__ uint4 *sk_cut_a(sk_cut_t *cut, int v) { return reinterpret_cast<uint4 *>(&cut[v].w[0]); }
__device__ __forceinline__ uint4 *sk_cut_b(sk_cut_t *cut, int v) { return reinterpret_cast<uint4 *>(&cut[v].w[SK_CUT_CARRY]); }

// THE RULE on voice v: ra = set, value, q, mode; rb = rate_up, rate_down.  Returns 1: set or started, 2: withheld; clamped: the
// tracked product lay outside the box.  fenv (or NULL): a voice set or started loses its contour
__device__ __forceinline__ int sk_cutoff_apply(sk_cut_t *cut, const sk_bend_t *bend, sk_fenv_t *fenv, const sk_cut_planes_t &p, int v,
                                               const uint4 &ra, const uint2 &rb, bool &clamped) {
  const uint4 a = *sk_cut_a(cut, v);                                     // w, target, rate_up, rate_down
  const uint4 b = *sk_cut_b(cut, v);                                     // carry, q, mode, 0
  const uint32_t set = ra.x;
  const bool has = a.x != 0u;
  if (!has && (set & (SK_CUTOFF_Q | SK_CUTOFF_MODE)) != (SK_CUTOFF_Q | SK_CUTOFF_MODE)) return 2;   // a first cutoff names both
  const uint32_t q = (set & SK_CUTOFF_Q) ? ra.z : b.y, mode = (set & SK_CUTOFF_MODE) ? ra.w : b.z;
  uint32_t wn = ra.y;
  if (set & SK_CUTOFF_TRACK) {
    uint32_t k = p.osc[v].w[0];
    if (bend) {
      const uint32_t key = bend[v].w[SK_BEND_KEY];
      if (key) k = key;
    }
    k &= 0x7fffffffu;
    if (k == 0u || k >= 0x7f800000u) return 2;                          // zero or not finite
    const float f = __fmul_rn(__uint_as_float(k), __uint_as_float(ra.y));
    clamped = !(f >= SK_CUTOFF_W_MIN && f <= SK_CUTOFF_W_MAX);
    wn = __float_as_uint(f < SK_CUTOFF_W_MIN ? SK_CUTOFF_W_MIN : f > SK_CUTOFF_W_MAX ? SK_CUTOFF_W_MAX : f);
  }
  if (fenv) sk_fenv_zero(fenv, v);
  if ((set & SK_CUTOFF_GLIDE) && has) {                                  // a pure start: w and the coefficients stand
    *sk_cut_a(cut, v) = make_uint4(a.x, wn, rb.x, rb.y);
    *sk_cut_b(cut, v) = make_uint4(0u, q, mode, 0u);
    return 1;
  }
  *sk_cut_a(cut, v) = make_uint4(wn, 0u, 0u, 0u);
  *sk_cut_b(cut, v) = make_uint4(0u, q, mode, 0u);
  sk_cutoff_store(p, v, sk_cutoff_coeffs(mode, __uint_as_float(wn), __uint_as_float(q)));
  return 1;
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_cutoff_clear_kernel(sk_cut_t *cut, const int32_t *d_slots, int n, const uint32_t *d_count,
                                                                        int k_shift, int n_voices) {
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);
  if (t.valid) {
    *sk_cut_a(cut, t.e + t.l) = make_uint4(0u, 0u, 0u, 0u);
    *sk_cut_b(cut, t.e + t.l) = make_uint4(0u, 0u, 0u, 0u);
  }
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_cutoff_match_kernel(sk_cut_t *cut, const sk_bend_t *bend, sk_fenv_t *fenv, sk_cut_each_t rec, int K,
                                                                        uint64_t filter_mask, int first, int count,
                                                                        const uint32_t *__restrict__ owner, uint32_t value, uint32_t omask,
                                                                        sk_cut_planes_t p, uint32_t *d_result) {
  __shared__ uint32_t sums[4];
  const sk_lane_t t = sk_range_lane(first, count, K);
  const bool hit = t.in_range && sk_owner_matches(owner[t.v - t.l], value, omask);
  int did = 0;
  bool clamped = false;
  if (hit && ((filter_mask >> t.l) & 1))
    did = sk_cutoff_apply(cut, bend, fenv, p, t.v, make_uint4(rec.w[0], rec.w[1], rec.w[2], rec.w[3]), make_uint2(rec.w[4], rec.w[5]), clamped);
  const bool flag[4] = { did == 1, did == 2, t.head && !hit, did == 1 && clamped };
  sk_owner_count<4>(sums, d_result, flag);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_cutoff_each_kernel(sk_cut_t *cut, const sk_bend_t *bend, sk_fenv_t *fenv,
                                                                       const sk_cut_each_t *__restrict__ each, int k_shift, uint64_t filter_mask, const int32_t *d_slots,
                                                                       const uint32_t *__restrict__ tags, const uint32_t *__restrict__ owner,
                                                                       int n, const uint32_t *d_count, int n_voices, sk_cut_planes_t p,
                                                                       uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint4 ent_a[SK_CONTROL_SPAN];                               // set, value, q, mode of this workgroup's entries
  __shared__ uint2 ent_b[SK_CONTROL_SPAN];                               // rate_up, rate_down
  __shared__ uint32_t sums[4];
  const int per_wg = SK_CONTROL_SPAN >> k_shift;
  const int64_t base = (int64_t)blockIdx.x * per_wg;
  if ((int)threadIdx.x < per_wg && base + (int)threadIdx.x < n) {
    ent_a[threadIdx.x] = *reinterpret_cast<const uint4 *>(&each[base + (int)threadIdx.x].w[0]);
    ent_b[threadIdx.x] = *reinterpret_cast<const uint2 *>(&each[base + (int)threadIdx.x].w[SK_CUT_E_RATE_UP]);
  }
  __syncthreads();
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);   // (t.i == base + the entry's place)
  const bool owned = sk_entry_owned(owner, tags, t);
  int did = 0;
  bool clamped = false;
  if (owned && ((filter_mask >> t.l) & 1)) {
    const int at = (int)threadIdx.x >> k_shift;
    did = sk_cutoff_apply(cut, bend, fenv, p, t.e + t.l, ent_a[at], ent_b[at], clamped);
  }
  const bool flag[4] = { did == 1, did == 2, t.valid && !owned && t.l == 0, did == 1 && clamped };
  sk_owner_count<4>(sums, d_result, flag);
  sk_batch_done(cnt, done, seq);
}

// what the ENV instantiation takes beside the rest (ENV false: an empty struct the kernel never reads)
template <bool ENV> struct sk_cutoff_env_t {};
template <> struct sk_cutoff_env_t<true> {
  sk_fenv_t *fenv;
  const sk_plane_t *env_s;                                               // SKP_ENV_S: words 2, 3 are sample_release
};

template <bool ENV>
__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_cutoff_advance_kernel(sk_cut_t *cut, sk_cut_planes_t p, int first, int count,
                                                                          uint32_t frames, uint32_t *d_result, sk_cutoff_env_t<ENV> ea) {
  __shared__ uint32_t sums[2];
  const int64_t off = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  bool still = false, arrived = false;
  if (off < count) {
    const int v = first + (int)off;
    const uint4 a = *sk_cut_a(cut, v);                                   // w, target, rate_up, rate_down
    bool contour = false;
    if constexpr (ENV) {
      if (ea.fenv[v].w[SK_FENV_STAGE] != 0u) {                           // (a voice without a contour: this 4-byte load and no more)
        contour = true;
        const uint4 fa = *sk_fenv_a(ea.fenv, v);                         // stage, w_peak, w_sustain, w_end
        const uint2 rel = *reinterpret_cast<const uint2 *>(&ea.env_s[v].w[2]);
        sk_fenv_advance(cut, ea.fenv, p, v, a, fa, (rel.x | rel.y) != 0u, frames, still, arrived);
      }
    }
    if (!contour && a.y != 0u) {
      const uint4 b = *sk_cut_b(cut, v);                                 // carry, q, mode, 0
      uint32_t w = a.x;
      bool there = false;
      const uint32_t c = b.x + frames;
      for (uint32_t m = c >> 6; m && !there; --m) {
        if (w < a.y) {
          w = __float_as_uint(__fmul_rn(__uint_as_float(w), __uint_as_float(a.z)));
          there = w >= a.y;
        } else if (w > a.y) {
          w = __float_as_uint(__fmul_rn(__uint_as_float(w), __uint_as_float(a.w)));
          there = w <= a.y;
        } else {
          there = true;
        }
      }
      if (there) {
        w = a.y;
        *sk_cut_a(cut, v) = make_uint4(w, 0u, 0u, 0u);
        cut[v].w[SK_CUT_CARRY] = 0u;
        arrived = true;
      } else {
        if (w != a.x) cut[v].w[SK_CUT_W] = w;
        cut[v].w[SK_CUT_CARRY] = c & 63u;
        still = true;
      }
      sk_cutoff_store(p, v, sk_cutoff_coeffs(b.z, __uint_as_float(w), __uint_as_float(b.y)));
    }
  }
  const bool flag[2] = { still, arrived };
  sk_owner_count<2>(sums, d_result, flag);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_cutoff_stop_kernel(sk_cut_t *cut, sk_fenv_t *fenv, sk_cut_planes_t p, int first, int count,
                                                                       int snap) {
  const int64_t off = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  if (off >= count) return;
  const int v = first + (int)off;
  if (fenv && fenv[v].w[SK_FENV_STAGE] != 0u) sk_fenv_zero(fenv, v);     // (a resting contour has no target: ahead of the early return)
  const uint4 a = *sk_cut_a(cut, v);
  if (a.y == 0u) return;                                                 // (not moving: rates and carry are 0 already)
  uint32_t w = a.x;
  if (snap) {
    const uint4 b = *sk_cut_b(cut, v);
    w = a.y;
    sk_cutoff_store(p, v, sk_cutoff_coeffs(b.z, __uint_as_float(w), __uint_as_float(b.y)));
  }
  *sk_cut_a(cut, v) = make_uint4(w, 0u, 0u, 0u);
  cut[v].w[SK_CUT_CARRY] = 0u;
}

extern "C" int sk_launch_cutoff_clear(sk_cut_t *cut, const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices, int n_voices,
                                      hipStream_t stream) {
  if (n <= 0) return 0;
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_cutoff_clear_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, cut, d_slots, n, d_count, sh,
                     n_voices);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_cutoff_match(sk_cut_t *cut, const sk_bend_t *bend, sk_fenv_t *fenv, const sk_cut_each_t *rec, int slot_voices,
                                      uint64_t filter_mask, int first, int count, const uint32_t *owner, uint32_t value, uint32_t mask,
                                      const sk_cut_planes_t *planes, uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 4, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_cutoff_match_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, cut, bend, fenv, *rec, slot_voices,
                     filter_mask, first, count, owner, value, mask, *planes, d_result);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_cutoff_each(sk_cut_t *cut, const sk_bend_t *bend, sk_fenv_t *fenv, const sk_cut_each_t *d_each, int slot_voices,
                                     uint64_t filter_mask, const int32_t *d_slots, const uint32_t *d_tags, const uint32_t *owner, int n,
                                     const uint32_t *d_count, int n_voices, const sk_cut_planes_t *planes, uint32_t *d_result, uint32_t *cnt,
                                     uint32_t *done, uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 4, stream);
  if (e != hipSuccess) return (int)e;
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_cutoff_each_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, cut, bend, fenv, d_each, sh,
                     filter_mask, d_slots, d_tags, owner, n, d_count, n_voices, *planes, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}

// fenv == NULL: the ENV = false instantiation, the kernel of a bank without a filter-envelope array; else ENV = true
extern "C" int sk_launch_cutoff_advance(sk_cut_t *cut, sk_fenv_t *fenv, const sk_plane_t *env_s, const sk_cut_planes_t *planes, int first,
                                        int count, int num_frames, uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 2, stream);
  if (e != hipSuccess) return (int)e;
  if (fenv) {
    sk_cutoff_env_t<true> ea;
    ea.fenv = fenv;
    ea.env_s = env_s;
    hipLaunchKernelGGL(sk_cutoff_advance_kernel<true>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, cut, *planes, first, count,
                       (uint32_t)num_frames, d_result, ea);
  } else {
    hipLaunchKernelGGL(sk_cutoff_advance_kernel<false>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, cut, *planes, first, count,
                       (uint32_t)num_frames, d_result, sk_cutoff_env_t<false>());
  }
  return (int)hipGetLastError();
}

extern "C" int sk_launch_cutoff_stop(sk_cut_t *cut, sk_fenv_t *fenv, const sk_cut_planes_t *planes, int first, int count, int snap,
                                     hipStream_t stream) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL(sk_cutoff_stop_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, cut, fenv, *planes, first, count, snap);
  return (int)hipGetLastError();
}
