// skred_fx_idle_common.hpp -- the fixed-point bank's idle predicate, shared by the kernels that ask "is this voice free"
// (skred_fx_live_kernels.hip: the free-voice list; skred_fx_steal_kernels.hip: a voice the idle query would list is no candidate
// for stealing).
#ifndef SKRED_FX_IDLE_COMMON_HPP
#define SKRED_FX_IDLE_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_layout.h"

// the public bit values (include/skred_amd.h: SKRED_IDLE_*; checked against the header in skred_fx_live.c)
enum { SKXI_FINISHED = 1u << 0, SKXI_ENV_DONE = 1u << 1, SKXI_AMP_ZERO = 1u << 2 };

// the predicate of one voice; every comparison is exact
__device__ __forceinline__ bool skx_idle_pred(const skx_idle_args_t &a, int v, bool in_range) {
  if (!in_range) return false;
  const uint32_t which = a.which;   // wave-uniform: the branches below are scalar
  bool idle = false;
  uint32_t rwf = 0;
  if (which & (SKXI_FINISHED | SKXI_ENV_DONE)) rwf = a.rw0[v].w[3];
  if (which & SKXI_FINISHED) idle = (rwf & SKXR_FINISHED) != 0;
  if (which & SKXI_ENV_DONE) {
    const uint32_t flags = a.osc[v].w[2] >> 8;
    const long long gain = (long long)(int32_t)a.rw0[v].w[1];
    const bool settled = !(flags & SKXF_SMOOTH) || (gain < 0 ? -gain : gain) <= (long long)a.settle_q15;
    idle = idle || ((flags & SKXF_USE_ENV) && !(rwf & SKXR_ACTIVE) && settled);
  }
  if (which & SKXI_AMP_ZERO) idle = idle || a.osc[v].w[3] == 0u;
  return idle;
}

#endif
