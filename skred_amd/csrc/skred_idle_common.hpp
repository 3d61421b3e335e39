// skred_idle_common.hpp -- the idle predicate, shared by the kernels that ask "is this voice free" (skred_idle_kernels.hip: the
// free-voice list; skred_steal_kernels.hip: a voice the idle query would list is no candidate for stealing).
#ifndef SKRED_IDLE_COMMON_HPP
#define SKRED_IDLE_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"

// the predicate of one voice (v inside the padded bank; `in_range`: inside the query's range).  Reads a.which, a.settle_level and
// the planes a.which asks for: filt (FINISHED, ENV_DONE), tab and osc_rw (ENV_DONE), osc_ro (AMP_ZERO), named (UNNAMED).
__device__ __forceinline__ bool sk_idle_pred(const sk_idle_args_t &a, int v, bool in_range) {
  if (!in_range) return false;
  const uint32_t which = a.which;   // wave-uniform: the branches below are scalar
  bool idle = false;
  uint32_t rwf = 0;
  if (which & (SK_IDLE_FINISHED | SK_IDLE_ENV_DONE)) rwf = a.filt[v].w[3];
  if (which & SK_IDLE_FINISHED) idle = (rwf & SKR_FINISHED) != 0;
  if (which & SK_IDLE_ENV_DONE) {
    const uint32_t flags = a.tab[v].w[2];
    const float gain = __uint_as_float(a.osc_rw[v].w[1]);
    const bool settled = !(flags & SKF_SMOOTH) || fabsf(gain) <= a.settle_level;
    idle = idle || ((flags & SKF_USE_ENV) && !(rwf & SKR_ENV_ACTIVE) && settled);
  }
  if (which & SK_IDLE_AMP_ZERO) idle = idle || __uint_as_float(a.osc_ro[v].w[3]) == 0.0f;
  if (which & SK_IDLE_UNNAMED) idle = idle && !((a.named[v >> 6] >> (v & 63)) & 1);
  return idle;
}

#endif
