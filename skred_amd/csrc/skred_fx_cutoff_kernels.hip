// skred_fx_cutoff_kernels.hip -- filter cutoff on the fixed-point bank: key-tracked cutoffs that glide and land, in integers
// (gfx950 / CDNA4, wave64).
//
// skred_fxbank_cutoff_match / _cutoff_owned_each / _cutoff_tags_each / _cutoff_advance / _cutoff_stop (include/skred_amd_fxpt.h has the
// definition).  cut[n_voices] lies beside the bend array of skred_fx_bend.c: eight words per voice, two uint4 -- w_q29, target_q29,
// up_q32, down_q32 (w == 0: no device cutoff, target == 0: not moving) and carry (0 .. 63), q_q16, mode, 0.  Only these kernels and the
// float bank's sk_cutoff_clear_kernel (entered through its launcher at slot_voices = 1 behind every tag launch of a bank that has the
// array) read or write it; no render kernel knows it exists.  The bank words they store are the five coefficients
// (skred_fx_cutoff_common.hpp: skx_cutoff_store -- the whole SKX_FILT plane word and word 0 of SKX_FILT2); they read phase_inc
// (SKX_OSC word 0) and, on a bank with a pitch-wheel array, a bent voice's key.
//
//   sk_fx_cutoff_match_kernel    sk_fx_bend_match_kernel's geometry, guard and counting: THE RULE (skx_cutoff_apply) to one record, a
//                                kernel argument.
//   sk_fx_cutoff_each_kernel     sk_fx_bend_each_kernel's geometry and guard; lane k reads record k: one 16-byte and one 8-byte load,
//                                consecutive lanes, consecutive 32-byte records.
//   sk_fx_cutoff_advance_kernel  one thread per voice of the range.  A voice that does not move costs its 16-byte load and nothing else.
//                                A moving one loads its second half, takes up to (carry + F) >> 6 steps (skx_step_64: the portamento's),
//                                stores the last w, or on arrival the target's bits, and computes the coefficients ONCE.
//   sk_fx_cutoff_stop_kernel     one thread per voice of the range: target, rates and carry cleared; with snap w = target first.
//
// THE FILTER ENVELOPE (skred_fx_fenv.c, skred_fx_fenv_kernels.hip).  On a bank that has an fenv array the match, each and stop kernels
// receive it (NULL otherwise: a wave-uniform branch, and the bytes stored are the ones stored without it) and zero the eight fenv
// words of every voice they set, start or stop: a new cutoff ends the contour.  The advance kernel is a template: ENV = false is the
// kernel as it was (profiles/fxcutoff_usage.txt), ENV = true loads the voice's stage word beside its first half and hands a voice that
// has a contour to skx_fenv_advance (skred_fx_fenv_common.hpp), which also reads its release clock (SKX_TIME words 2, 3).
//
// Every step is exact integer arithmetic: the same bits on every machine.  Counts are sk_owner_count's.  Plain vector stores and
// ordinary atomics only; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_layout.h"
#include "skred_launch.h"
#include "skred_fx_cutoff_common.hpp"
#include "skred_fx_step_common.hpp"
#include "skred_fx_fenv_common.hpp"   // skx_cut_planes_t, skx_cut_a / _b, skx_fenv_zero, skx_fenv_advance
#include "skred_update_common.hpp"   // sk_entry_decode, sk_entry_owned, sk_range_lane, sk_owner_count, sk_grid, sk_list_grid, sk_result_clear

static_assert(sizeof(skx_cut_t) == 32 && sizeof(skx_cut_each_t) == 32, "two 16-byte loads per voice; a record is 32 bytes");

// THE RULE on voice v: ra = set, value, q_q16, mode; rb = up_q32, down_q32.  Returns 1: set or started, 2: withheld; clamped: the
// tracked product lay outside the box.  fenv (or NULL): a voice set or started loses its contour
__device__ __forceinline__ int skx_cutoff_apply(skx_cut_t *cut, const skx_bend_t *bend, skx_fenv_t *fenv, const skx_cut_planes_t &p, int v,
                                                const uint4 &ra, const uint2 &rb, bool &clamped) {
  const uint4 a = *skx_cut_a(cut, v);                                    // w, target, up, down
  const uint4 b = *skx_cut_b(cut, v);                                    // carry, q, mode, 0
  const uint32_t set = ra.x;
  const bool has = a.x != 0u;
  if (!has && (set & (SKX_CUTOFF_Q | SKX_CUTOFF_MODE)) != (SKX_CUTOFF_Q | SKX_CUTOFF_MODE)) return 2;   // a first cutoff names both
  const uint32_t q = (set & SKX_CUTOFF_Q) ? ra.z : b.y, mode = (set & SKX_CUTOFF_MODE) ? ra.w : b.z;
  uint32_t wn = ra.y;
  if (set & SKX_CUTOFF_TRACK) {
    uint32_t k = p.osc[v].w[0];
    if (bend) {
      const uint32_t key = bend[v].w[SKX_BEND_KEY];
      if (key) k = key;
    }
    if (k == 0u) return 2;                                               // a voice without pitch
    const uint64_t f = ((uint64_t)k * (uint64_t)ra.y) >> 27;             // (below 2^64 for every k and value)
    clamped = f < SKX_CUTOFF_W_MIN || f > SKX_CUTOFF_W_MAX;
    wn = f < SKX_CUTOFF_W_MIN ? SKX_CUTOFF_W_MIN : f > SKX_CUTOFF_W_MAX ? SKX_CUTOFF_W_MAX : (uint32_t)f;
  }
  if (fenv) skx_fenv_zero(fenv, v);
  if ((set & SKX_CUTOFF_GLIDE) && has) {                                 // a pure start: w and the coefficients stand
    *skx_cut_a(cut, v) = make_uint4(a.x, wn, rb.x, rb.y);
    *skx_cut_b(cut, v) = make_uint4(0u, q, mode, 0u);
    return 1;
  }
  *skx_cut_a(cut, v) = make_uint4(wn, 0u, 0u, 0u);
  *skx_cut_b(cut, v) = make_uint4(0u, q, mode, 0u);
  skx_cutoff_store(p.filt, p.filt2, v, skx_cutoff_coeffs(mode, wn, q));
  return 1;
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_cutoff_match_kernel(skx_cut_t *cut, const skx_bend_t *bend, skx_fenv_t *fenv, skx_cut_each_t rec,
                                                                           int first, int count, const uint32_t *__restrict__ owner, uint32_t value,
                                                                           uint32_t omask, skx_cut_planes_t p, uint32_t *d_result) {
  __shared__ uint32_t sums[4];
  const sk_lane_t t = sk_range_lane(first, count, 1);                    // (inside the bank: checked on the host)
  const bool hit = t.in_range && sk_owner_matches(owner[t.v], value, omask);
  int did = 0;
  bool clamped = false;
  if (hit) did = skx_cutoff_apply(cut, bend, fenv, p, t.v, make_uint4(rec.w[0], rec.w[1], rec.w[2], rec.w[3]), make_uint2(rec.w[4], rec.w[5]), clamped);
  const bool flag[4] = { did == 1, did == 2, t.in_range && !hit, did == 1 && clamped };
  sk_owner_count<4>(sums, d_result, flag);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_cutoff_each_kernel(skx_cut_t *cut, const skx_bend_t *bend, skx_fenv_t *fenv,
                                                                          const skx_cut_each_t *__restrict__ each, const int32_t *d_voices,
                                                                          const uint32_t *__restrict__ tags, const uint32_t *__restrict__ owner,
                                                                          int n, const uint32_t *d_count, int n_voices, skx_cut_planes_t p,
                                                                          uint32_t *d_result) {
  __shared__ uint32_t sums[4];
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, 0, d_voices, n, d_count, n_voices);   // (valid: 0 <= t.e < n_voices)
  const bool owned = sk_entry_owned(owner, tags, t);
  int did = 0;
  bool clamped = false;
  if (owned) {
    const uint4 ra = *reinterpret_cast<const uint4 *>(&each[t.i].w[0]);
    const uint2 rb = *reinterpret_cast<const uint2 *>(&each[t.i].w[SKX_CUT_E_UP]);
    did = skx_cutoff_apply(cut, bend, fenv, p, t.e, ra, rb, clamped);
  }
  const bool flag[4] = { did == 1, did == 2, t.valid && !owned, did == 1 && clamped };
  sk_owner_count<4>(sums, d_result, flag);
}

// what the ENV instantiation takes beside the rest (ENV false: an empty struct the kernel never reads)
template <bool ENV> struct skx_cutoff_env_t {};
template <> struct skx_cutoff_env_t<true> {
  skx_fenv_t *fenv;
  const skx_plane_t *time;                                               // SKX_TIME: words 2, 3 are sample_release
};

template <bool ENV>
__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_cutoff_advance_kernel(skx_cut_t *cut, skx_cut_planes_t p, int first, int count,
                                                                             uint32_t frames, uint32_t *d_result, skx_cutoff_env_t<ENV> ea) {
  __shared__ uint32_t sums[2];
  const int64_t off = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  bool still = false, arrived = false;
  if (off < count) {
    const int v = first + (int)off;                                      // (inside the bank: checked on the host)
    const uint4 a = *skx_cut_a(cut, v);                                  // w, target, up, down
    bool contour = false;
    if constexpr (ENV) {
      if (ea.fenv[v].w[SKX_FENV_STAGE] != 0u) {                          // (a voice without a contour: this 4-byte load and no more)
        contour = true;
        const uint4 fa = *skx_fenv_a(ea.fenv, v);                        // stage, w_peak, w_sustain, w_end
        const uint2 rel = *reinterpret_cast<const uint2 *>(&ea.time[v].w[2]);
        skx_fenv_advance(cut, ea.fenv, p, v, a, fa, (rel.x | rel.y) != 0u, frames, still, arrived);
      }
    }
    if (!contour && a.y != 0u) {
      const uint4 b = *skx_cut_b(cut, v);                                // carry, q, mode, 0
      uint32_t w = a.x;
      bool there = w == a.y;
      const uint32_t c = b.x + frames;                                   // (carry <= 63, frames <= 65536)
      for (uint32_t m = c >> 6; m && !there; --m) there = skx_step_64(w, a.y, a.z, a.w);
      if (there) {
        w = a.y;
        *skx_cut_a(cut, v) = make_uint4(w, 0u, 0u, 0u);
        cut[v].w[SKX_CUT_CARRY] = 0u;
        arrived = true;
      } else {
        if (w != a.x) cut[v].w[SKX_CUT_W] = w;
        cut[v].w[SKX_CUT_CARRY] = c & 63u;
        still = true;
      }
      skx_cutoff_store(p.filt, p.filt2, v, skx_cutoff_coeffs(b.z, w, b.y));
    }
  }
  const bool flag[2] = { still, arrived };
  sk_owner_count<2>(sums, d_result, flag);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_cutoff_stop_kernel(skx_cut_t *cut, skx_fenv_t *fenv, skx_cut_planes_t p, int first, int count,
                                                                          int snap) {
  const int64_t off = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  if (off >= count) return;
  const int v = first + (int)off;
  if (fenv && fenv[v].w[SKX_FENV_STAGE] != 0u) skx_fenv_zero(fenv, v);   // (a resting contour has no target: ahead of the early return)
  const uint4 a = *skx_cut_a(cut, v);
  if (a.y == 0u) return;                                                 // (not moving: rates and carry are 0 already)
  uint32_t w = a.x;
  if (snap) {
    const uint4 b = *skx_cut_b(cut, v);
    w = a.y;
    skx_cutoff_store(p.filt, p.filt2, v, skx_cutoff_coeffs(b.z, w, b.y));
  }
  *skx_cut_a(cut, v) = make_uint4(w, 0u, 0u, 0u);
  cut[v].w[SKX_CUT_CARRY] = 0u;
}

static skx_cut_planes_t skx_cut_planes(skx_plane_t *const ro[SKX_COUNT]) {
  skx_cut_planes_t p;
  p.osc = ro[SKX_OSC];
  p.filt = ro[SKX_FILT];
  p.filt2 = ro[SKX_FILT2];
  return p;
}

// d_result[4] (or NULL; zeroed on `stream` ahead of the kernel): voices set or started, records withheld, voices of the range that did
// not match, cutoffs clamped.  fenv: the bank's filter-envelope array or NULL (a voice set or started loses its contour)
extern "C" int skx_launch_cutoff_match(skx_cut_t *cut, const skx_bend_t *bend, skx_fenv_t *fenv, const skx_cut_each_t *rec, int first, int count,
                                       const uint32_t *owner, uint32_t value, uint32_t mask, skx_plane_t *const ro[SKX_COUNT],
                                       uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 4, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_fx_cutoff_match_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, cut, bend, fenv, *rec, first, count, owner,
                     value, mask, skx_cut_planes(ro), d_result);
  return (int)hipGetLastError();
}

// d_result[4] as above, [2]: voices whose owner differs.  d_each: 16-byte aligned
extern "C" int skx_launch_cutoff_each(skx_cut_t *cut, const skx_bend_t *bend, skx_fenv_t *fenv, const skx_cut_each_t *d_each, const int32_t *d_voices,
                                      const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count, int n_voices,
                                      skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 4, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_fx_cutoff_each_kernel, dim3(sk_list_grid(n, 0)), dim3(SK_CONTROL_SPAN), 0, stream, cut, bend, fenv, d_each, d_voices, d_tags,
                     owner, n, d_count, n_voices, skx_cut_planes(ro), d_result);
  return (int)hipGetLastError();
}

// d_result[2] (or NULL; zeroed on `stream` ahead of the kernel): voices still moving, voices that arrived.  fenv == NULL: the ENV = false
// instantiation, the kernel of a bank without a filter-envelope array; else ENV = true
extern "C" int skx_launch_cutoff_advance(skx_cut_t *cut, skx_fenv_t *fenv, skx_plane_t *const ro[SKX_COUNT], int first, int count, int num_frames,
                                         uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 2, stream);
  if (e != hipSuccess) return (int)e;
  if (fenv) {
    skx_cutoff_env_t<true> ea;
    ea.fenv = fenv;
    ea.time = ro[SKX_TIME];
    hipLaunchKernelGGL(sk_fx_cutoff_advance_kernel<true>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, cut, skx_cut_planes(ro), first,
                       count, (uint32_t)num_frames, d_result, ea);
  } else {
    hipLaunchKernelGGL(sk_fx_cutoff_advance_kernel<false>, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, cut, skx_cut_planes(ro), first,
                       count, (uint32_t)num_frames, d_result, skx_cutoff_env_t<false>());
  }
  return (int)hipGetLastError();
}

extern "C" int skx_launch_cutoff_stop(skx_cut_t *cut, skx_fenv_t *fenv, skx_plane_t *const ro[SKX_COUNT], int first, int count, int snap,
                                      hipStream_t stream) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL(sk_fx_cutoff_stop_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, cut, fenv, skx_cut_planes(ro), first, count, snap);
  return (int)hipGetLastError();
}
