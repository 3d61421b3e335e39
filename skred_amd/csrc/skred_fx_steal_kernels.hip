// skred_fx_steal_kernels.hip -- voice stealing on the fixed-point bank: the key pass (gfx950 / CDNA4).
//
// skred_fxbank_find_steal (include/skred_amd_fxpt.h states the definition field by field).  The only pass of the select that
// depends on the bank is the first one:
//
//   sk_fx_steal_keys_kernel  every workgroup takes SK_IDLE_SPAN consecutive voices (spans aligned to 64 voices, as the idle
//                            query's), evaluates the candidate predicate and the key from the planes the query's bits need --
//                            SKX_OSC word 2 (flags) and word 3 of read-write plane 0 always; SKX_TIME for OLDEST, min_age > 0 or a
//                            RELEASED_* flag; word 1 of read-write plane 0 (the smoother's gain) for QUIETEST or an ENV_DONE
//                            exclusion; SKX_OSC word 3 (amp_q15) for an AMP_ZERO exclusion -- and stores ONE key per voice
//                            (SK_STEAL_NOKEY: no candidate).  It counts the first digit, and its last arriver picks the first bin.
//
// The exclusion is the idle query's own predicate (skred_fx_idle_common.hpp), the histogram, scan and pick are the float key
// pass's (skred_steal_common.hpp), and everything behind this launch is sk_launch_steal_select (skred_steal_kernels.hip): digit
// passes, count, scatter, sort.  Those read 8 bytes per voice from `keys`, never a plane, so they do not care which bank made them.
//
// The kernel only READS the bank.  Branches on query bits depend on kernel arguments only: they are wave-uniform.  No workgroup
// waits for another; integer atomics and index-ordered ranks only: the same state gives the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_steal_common.hpp"   // skx_steal_key: shared with skred_fx_chan_kernels.hip
#include "skred_fx_steal.h"
#include "skred_kernel_common.hpp"

__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_fx_steal_keys_kernel(skx_steal_args_t a) {
  __shared__ uint32_t hist[SK_STEAL_BINS];
  __shared__ uint32_t scan[SK_IDLE_SPAN];
  __shared__ int flag;
  const int tid = threadIdx.x;
  const int v = a.s.base + (int)blockIdx.x * SK_IDLE_SPAN + tid;   // base: `first` rounded down to 64
  const bool in_range = v >= a.s.first && v < a.s.end;
  const sk_key_t key = skx_steal_key(a, v, in_range);
  a.s.keys[(size_t)blockIdx.x * SK_IDLE_SPAN + tid] = key;         // (read by later launches only)
  sk_steal_histogram(a.s, key != SK_STEAL_NOKEY, (uint32_t)(key >> sk_steal_shift(0)) & (SK_STEAL_BINS - 1), hist, tid);
  if (!sk_arrive_last(a.s.words + SK_STEAL_W_TICKET, gridDim.x, tid, &flag)) return;
  sk_steal_pick(a.s, 0, 0ull, 0u, scan, tid);
}

extern "C" int skx_launch_steal(const skx_steal_args_t *args, hipStream_t stream) {
  skx_steal_args_t a = *args;
  a.s.base = a.s.first & ~63;
  a.s.digit = 0;
  a.idle.first = a.s.first;
  a.idle.end = a.s.end;
  const dim3 grid((unsigned)sk_idle_workgroups(a.s.first, a.s.end - a.s.first)), block(SK_IDLE_SPAN);
  hipLaunchKernelGGL(sk_fx_steal_keys_kernel, grid, block, 0, stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return sk_launch_steal_select(&a.s, stream);
}
