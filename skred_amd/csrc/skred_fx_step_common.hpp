// skred_fx_step_common.hpp -- the 64-frame step of the fixed-point bank's moving words, stated once: the portamento applies it to a
// voice's increment or key (skred_fx_glide_kernels.hip), the filter cutoff to w_q29 (skred_fx_cutoff_kernels.hip).
// include/skred_amd_fxpt.h, sections "portamento" and "filter cutoff", have the definition.  Exact integer arithmetic.
#ifndef SKRED_FX_STEP_COMMON_HPP
#define SKRED_FX_STEP_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

// one 64-frame step of a word x != target towards it: up by max(1, (x * up_q32) >> 32), down by max(1, (x * down_q32) >> 32).
// Returns true on arrival (the step reached or passed the target); x then holds the step's low 32 bits and the caller stores the target
__device__ __forceinline__ bool skx_step_64(uint32_t &x, uint32_t target, uint32_t up_q32, uint32_t down_q32) {
  if (x < target) {
    const uint32_t d = __umulhi(x, up_q32);
    const uint64_t next = (uint64_t)x + (uint64_t)(d ? d : 1u);
    x = (uint32_t)next;                                                 // (not there: next < target, 32 bits hold it)
    return next >= (uint64_t)target;
  }
  const uint32_t d = __umulhi(x, down_q32);                             // (d < x: the difference cannot wrap)
  x -= d ? d : 1u;
  return x <= target;
}

#endif
