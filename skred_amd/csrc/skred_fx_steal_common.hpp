// skred_fx_steal_common.hpp -- the fixed-point bank's per-voice steal terms, for the two instantiations of its key pass
// (skred_fx_steal_kernels.hip: sk_fx_steal_keys_kernel -- every voice of the range, or the voices of one owner match).
// include/skred_amd_fxpt.h states the definition field by field.
#ifndef SKRED_FX_STEAL_COMMON_HPP
#define SKRED_FX_STEAL_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_idle_common.hpp"
#include "skred_fx_steal.h"
#include "skred_steal_common.hpp"

static_assert(SKX_IDLE_SPAN == SK_IDLE_SPAN, "the two banks' queries share their span: the scratch is sized with sk_idle_workgroups");

// the key of one voice, SK_STEAL_NOKEY when it is no candidate
__device__ __forceinline__ sk_key_t skx_steal_key(const skx_steal_args_t &a, int v, bool in_range) {
  if (!in_range) return SK_STEAL_NOKEY;
  const sk_steal_args_t &s = a.s;
  const uint32_t flags = a.idle.osc[v].w[2] >> 8;
  const uint32_t rwf = a.idle.rw0[v].w[3];
  bool cand = (flags & SKXF_USE_ENV) && (rwf & SKXR_ACTIVE);
  uint64_t t_start = 0, t_release = 0;
  if (s.policy == SK_STEAL_OLDEST || s.min_age > 0 || (s.flags & (SK_STEAL_RELEASED_FIRST | SK_STEAL_RELEASED_ONLY))) {
    const uint4 t = *reinterpret_cast<const uint4 *>(&a.time[v]);
    t_start = ((uint64_t)t.y << 32) | t.x;
    t_release = ((uint64_t)t.w << 32) | t.z;
  }
  const bool released = t_release != 0;
  if (s.min_age > 0) {
    const uint64_t age = t_start > s.now ? 0 : s.now - t_start;   // a start ahead of the clock: age 0
    cand = cand && age >= s.min_age;
  }
  if (s.flags & SK_STEAL_RELEASED_ONLY) cand = cand && released;
  if (a.idle.which) cand = cand && !skx_idle_pred(a.idle, v, true);
  if (!cand) return SK_STEAL_NOKEY;
  const sk_key_t cls = ((s.flags & SK_STEAL_RELEASED_FIRST) && released) ? 0ull : 1ull;
  sk_key_t primary;
  if (s.policy == SK_STEAL_OLDEST) {
    primary = cls == 0 ? t_release : t_start;
  } else {
    const long long gain = (long long)(int32_t)a.idle.rw0[v].w[1];
    const long long mag = gain < 0 ? -gain : gain;                // (|-2^31| needs 64 bits)
    primary = (flags & SKXF_SMOOTH) ? (sk_key_t)(mag < 0x7fffffffll ? mag : 0x7fffffffll) : 0x7fffffffull;
  }
  const sk_key_t cap = (1ull << 62) - 1;
  return (cls << 62) | (primary < cap ? primary : cap);
}

// the candidate predicate without its age and release terms: an envelope that runs, on a voice the exclusion does not call idle
__device__ __forceinline__ bool skx_steal_sounding(const skx_steal_args_t &a, int v, bool in_range) {
  if (!in_range) return false;
  const uint32_t flags = a.idle.osc[v].w[2] >> 8;
  const uint32_t rwf = a.idle.rw0[v].w[3];
  bool snd = (flags & SKXF_USE_ENV) && (rwf & SKXR_ACTIVE);
  if (a.idle.which) snd = snd && !skx_idle_pred(a.idle, v, true);
  return snd;
}

// HELD, for the sostenuto latch (skred_fx_pedal_kernels.hip): the candidate's first two terms -- an envelope that runs -- on a voice
// that is not released (no release clock).  The same words of the same planes skx_steal_key reads
__device__ __forceinline__ bool skx_steal_held(const skx_plane_t *osc, const skx_plane_t *rw0, const skx_plane_t *time, int v) {
  const uint32_t flags = osc[v].w[2] >> 8;
  const uint32_t rwf = rw0[v].w[3];
  if (!((flags & SKXF_USE_ENV) && (rwf & SKXR_ACTIVE))) return false;
  const uint2 r = *reinterpret_cast<const uint2 *>(&time[v].w[2]);     // sample_release lo, hi
  return (r.x | r.y) == 0u;
}

#endif
