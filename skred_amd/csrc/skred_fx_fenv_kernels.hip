// skred_fx_fenv_kernels.hip -- the filter envelope on the fixed-point bank: per-note cutoff contours that follow the gate, in integers
// (gfx950 / CDNA4, wave64).
//
// skred_fxbank_fenv_match / _fenv_owned_each / _fenv_tags_each (include/skred_amd_fxpt.h, "filter envelope", has the definition).
// fenv[n_voices] lies beside the cutoff array of skred_fx_cutoff.c: eight words per voice, two uint4 -- stage, w_peak, w_sustain, w_end
// (w_q29 values inside the cutoff box) and rate_attack_q32, rate_decay_q32, rate_release_q32, 0.  stage 0: no contour, and all eight
// words are 0.  The contour is a small program kept beside the voice: a record enters the attack here, skred_fxbank_cutoff_advance
// steps it (the ENV instantiation of sk_fx_cutoff_advance_kernel, skred_fx_cutoff_kernels.hip, through skx_fenv_advance) and enters the
// release from the voice's own release clock.  The envelope moves the voice's cutoff words and through them the five coefficients.
// The clear behind a tag launch is the float bank's sk_fenv_clear_kernel, entered through its launcher at slot_voices = 1.
//
//   sk_fx_fenv_match_kernel   sk_fx_cutoff_match_kernel's geometry, guard and counting: THE RECORD (skx_fenv_apply) as a kernel argument.
//   sk_fx_fenv_each_kernel    sk_fx_cutoff_each_kernel's geometry and guard; lane k reads record k: two 16-byte loads, consecutive
//                             lanes, consecutive 32-byte records.
//
// Every step is exact integer arithmetic: the same bits on every machine.  Counts are sk_owner_count's.  Plain vector stores and
// ordinary atomics only; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_layout.h"
#include "skred_launch.h"
#include "skred_fx_fenv_common.hpp"
#include "skred_update_common.hpp"   // sk_entry_decode, sk_entry_owned, sk_range_lane, sk_owner_count, sk_grid, sk_list_grid, sk_result_clear

static_assert(sizeof(skx_fenv_t) == 32 && sizeof(skx_fenv_each_t) == 32, "two 16-byte loads per voice; a record is 32 bytes");

// a level of the record: the value itself (ABS), or (w_now * value_q16) >> 16 clamped into the box (REL).  w_now <= 3 * 2^29 < 2^31
// and value < 2^32: the product is below 2^63
__device__ __forceinline__ uint32_t skx_fenv_level(bool rel, uint32_t w_now, uint32_t value, bool &clamped) {
  if (!rel) return value;
  const uint64_t f = ((uint64_t)w_now * (uint64_t)value) >> 16;
  if (f < SKX_CUTOFF_W_MIN || f > SKX_CUTOFF_W_MAX) clamped = true;
  return f < SKX_CUTOFF_W_MIN ? SKX_CUTOFF_W_MIN : f > SKX_CUTOFF_W_MAX ? SKX_CUTOFF_W_MAX : (uint32_t)f;
}

// THE RECORD on voice v: ra = set, start, peak, sustain; rb = end, rate_attack, rate_decay, rate_release.  Returns 1: started, 2:
// withheld (no cutoff word); clamped: a product lay outside the box
__device__ __forceinline__ int skx_fenv_apply(skx_fenv_t *fenv, skx_cut_t *cut, const skx_cut_planes_t &p, int v, const uint4 &ra,
                                              const uint4 &rb, bool &clamped) {
  const uint4 a = *skx_cut_a(cut, v);                                    // w, target, up, down
  if (a.x == 0u) return 2;
  const uint2 qm = *reinterpret_cast<const uint2 *>(&cut[v].w[SKX_CUT_Q]);   // q, mode
  const bool rel = (ra.x & SKX_FENV_REL) != 0u;
  const uint32_t w = (ra.x & SKX_FENV_START) ? skx_fenv_level(rel, a.x, ra.y, clamped) : a.x;
  const uint4 fa = make_uint4(SKX_FENV_ATTACK, skx_fenv_level(rel, a.x, ra.z, clamped), skx_fenv_level(rel, a.x, ra.w, clamped),
                              skx_fenv_level(rel, a.x, rb.x, clamped));
  const uint4 fb = make_uint4(rb.y, rb.z, rb.w, 0u);
  uint32_t target, rate;
  bool landed = false;
  const uint32_t stage = skx_fenv_enter(SKX_FENV_ATTACK, fa, fb, w, target, rate, landed);   // (sustain at the latest: never 0)
  *skx_cut_a(cut, v) = make_uint4(w, target, rate, rate);
  cut[v].w[SKX_CUT_CARRY] = 0u;
  *skx_fenv_a(fenv, v) = make_uint4(stage, fa.y, fa.z, fa.w);
  *skx_fenv_b(fenv, v) = fb;
  if (w != a.x) skx_cutoff_store(p.filt, p.filt2, v, skx_cutoff_coeffs(qm.y, w, qm.x));
  return 1;
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_fenv_match_kernel(skx_fenv_t *fenv, skx_cut_t *cut, skx_fenv_each_t rec, int first,
                                                                         int count, const uint32_t *__restrict__ owner, uint32_t value,
                                                                         uint32_t omask, skx_cut_planes_t p, uint32_t *d_result) {
  __shared__ uint32_t sums[4];
  const sk_lane_t t = sk_range_lane(first, count, 1);                    // (inside the bank: checked on the host)
  const bool hit = t.in_range && sk_owner_matches(owner[t.v], value, omask);
  int did = 0;
  bool clamped = false;
  if (hit)
    did = skx_fenv_apply(fenv, cut, p, t.v, make_uint4(rec.w[0], rec.w[1], rec.w[2], rec.w[3]), make_uint4(rec.w[4], rec.w[5], rec.w[6], rec.w[7]),
                         clamped);
  const bool flag[4] = { did == 1, did == 2, t.in_range && !hit, did == 1 && clamped };
  sk_owner_count<4>(sums, d_result, flag);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_fx_fenv_each_kernel(skx_fenv_t *fenv, skx_cut_t *cut, const skx_fenv_each_t *__restrict__ each,
                                                                        const int32_t *d_voices, const uint32_t *__restrict__ tags,
                                                                        const uint32_t *__restrict__ owner, int n, const uint32_t *d_count,
                                                                        int n_voices, skx_cut_planes_t p, uint32_t *d_result) {
  __shared__ uint32_t sums[4];
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, 0, d_voices, n, d_count, n_voices);   // (valid: 0 <= t.e < n_voices)
  const bool owned = sk_entry_owned(owner, tags, t);
  int did = 0;
  bool clamped = false;
  if (owned) {
    const uint4 ra = *reinterpret_cast<const uint4 *>(&each[t.i].w[0]);
    const uint4 rb = *reinterpret_cast<const uint4 *>(&each[t.i].w[SKX_FENV_E_END]);
    did = skx_fenv_apply(fenv, cut, p, t.e, ra, rb, clamped);
  }
  const bool flag[4] = { did == 1, did == 2, t.valid && !owned, did == 1 && clamped };
  sk_owner_count<4>(sums, d_result, flag);
}

static skx_cut_planes_t skx_fenv_planes(skx_plane_t *const ro[SKX_COUNT]) {
  skx_cut_planes_t p;
  p.osc = ro[SKX_OSC];
  p.filt = ro[SKX_FILT];
  p.filt2 = ro[SKX_FILT2];
  return p;
}

// d_result[4] (or NULL; zeroed on `stream` ahead of the kernel): voices started, records withheld, voices of the range that did not
// match, voices clamped
extern "C" int skx_launch_fenv_match(skx_fenv_t *fenv, skx_cut_t *cut, const skx_fenv_each_t *rec, int first, int count, const uint32_t *owner,
                                     uint32_t value, uint32_t mask, skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result, hipStream_t stream) {
  if (count <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 4, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_fx_fenv_match_kernel, dim3(sk_grid(count)), dim3(SK_CONTROL_SPAN), 0, stream, fenv, cut, *rec, first, count, owner, value,
                     mask, skx_fenv_planes(ro), d_result);
  return (int)hipGetLastError();
}

// d_result[4] as above, [2]: voices whose owner differs.  d_each: 16-byte aligned
extern "C" int skx_launch_fenv_each(skx_fenv_t *fenv, skx_cut_t *cut, const skx_fenv_each_t *d_each, const int32_t *d_voices,
                                    const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count, int n_voices,
                                    skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 4, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_fx_fenv_each_kernel, dim3(sk_list_grid(n, 0)), dim3(SK_CONTROL_SPAN), 0, stream, fenv, cut, d_each, d_voices, d_tags,
                     owner, n, d_count, n_voices, skx_fenv_planes(ro), d_result);
  return (int)hipGetLastError();
}
