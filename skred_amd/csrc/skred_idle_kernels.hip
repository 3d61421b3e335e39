// skred_idle_kernels.hip -- which voices of a range are idle: an ordered list, built on the device (gfx950 / CDNA4).
//
// skred_bank_find_idle (include/skred_amd.h): a sweep over the few state words the predicate needs, and an ordered
// compaction.  Two launches on the caller's stream, behind the renders and updates queued on it:
//
//   sk_idle_count_kernel    every workgroup takes SK_IDLE_SPAN consecutive voices (spans are aligned to 64 voices, so a
//                           wavefront reads 1 KiB of a plane and one word of the named set), evaluates the predicate,
//                           ballots per wave and publishes its count.  The workgroup that ARRIVES LAST
//                           (skred_kernel_common.hpp: sk_arrive_last -- write-through stores, one ticket, re-armed for the
//                           next launch) turns the counts into exclusive offsets and writes d_count and the rank of `from`.
//                           No workgroup waits for another: nothing here can spin or hang.
//   sk_idle_scatter_kernel  the same spans, evaluated again (the lines are in L2 for small banks, and the sweep is a few
//                           words per voice): rank = workgroup offset + wave prefix + mbcnt of the ballot, rotated by the
//                           rank of `from` modulo the total, stored when it is below max_out.
//
// The order is fixed by the voice index, never by arrival: two queries on the same state write the same bytes.  Both
// kernels only READ the bank.  Only the planes the query's bits need are requested: flags (SKP_TAB.z) and the smoother
// gain (SKS_OSC.y) for ENV_DONE, amp (SKP_OSC.w) for AMP_ZERO, rwflags (SKS_FILT.w) for FINISHED and ENV_DONE -- a word
// costs its 16-byte plane entry, 64 bytes per voice at most.
//
//   sk_named_kernel         the named set (bit v: some voice of the bank names v as FM / AM / pan / CZ modulator), rebuilt
//                           from the SKP_MODI plane when the routing changed and a query asks for SKRED_IDLE_UNNAMED.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_idle_common.hpp"   // sk_idle_pred: the predicate of one voice
#include "skred_idle_scan.hpp"     // the counts, the last arriver's offsets and the rotated scatter (shared with skred_slot_kernels.hip)
#include "skred_kernel_common.hpp"
#include "skred_launch.h"

__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_idle_count_kernel(sk_idle_args_t a) {
  __shared__ int lds[SK_IDLE_COUNT_LDS];
  bool in_range;
  const int v = sk_idle_voice(a, in_range);
  sk_idle_count_tail(a, v, sk_idle_pred(a, v, in_range), lds);
}

__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_idle_scatter_kernel(sk_idle_args_t a) {
  __shared__ int lds[SK_IDLE_WAVES];
  bool in_range;
  const int v = sk_idle_voice(a, in_range);
  sk_idle_scatter_tail(a, v, sk_idle_pred(a, v, in_range), lds);
}

// one thread per voice of the padded bank; `named` was cleared ahead of the launch
__global__ __launch_bounds__(256) void sk_named_kernel(const sk_plane_t *__restrict__ tab, const sk_plane_t *__restrict__ modi,
                                                       int n_padded, int n_voices, uint64_t *named) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n_padded) return;
  if (!(tab[v].w[2] & SKF_HAS_MOD)) return;           // (a slot nobody uploaded holds zeros in SKP_MODI, not -1)
  const uint4 m = *reinterpret_cast<const uint4 *>(&modi[v]);
  const int32_t w[4] = { (int32_t)m.x, (int32_t)m.y, (int32_t)m.z, (int32_t)m.w };
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // skred_bank_update.c, sk_pack_voice: a lane of the carrier's own 64-voice group, the tape code -2 - md of a voice in
    // another group, or -1 (unused; FM by the voice itself; a CZ source with CZ off; a modulator outside the bank)
    int md = -1;
    if (w[k] >= 0 && w[k] < 64) md = (v & ~63) | w[k];
    else if (w[k] <= -2) md = -2 - w[k];
    if (md >= 0 && md < n_voices)
      atomicOr(reinterpret_cast<unsigned long long *>(named) + (md >> 6), 1ull << (md & 63));
  }
}

extern "C" int sk_launch_named(const sk_plane_t *tab, const sk_plane_t *modi, int n_padded, int n_voices, uint64_t *named,
                               hipStream_t stream) {
  hipError_t e = hipMemsetAsync(named, 0, (size_t)(n_padded / 64) * sizeof(uint64_t), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_named_kernel, dim3((unsigned)((n_padded + 255) / 256)), dim3(256), 0, stream, tab, modi, n_padded, n_voices, named);
  return (int)hipGetLastError();
}

extern "C" int sk_idle_workgroups(int first, int count) {
  const int base = first & ~63;
  return (first + count - base + SK_IDLE_SPAN - 1) / SK_IDLE_SPAN;
}

extern "C" int sk_launch_idle(const sk_idle_args_t *args, hipStream_t stream) {
  sk_idle_args_t a = *args;
  a.base = a.first & ~63;
  const int n_wg = sk_idle_workgroups(a.first, a.end - a.first);
  a.from_wg = (a.from - a.base) / SK_IDLE_SPAN;
  hipLaunchKernelGGL(sk_idle_count_kernel, dim3((unsigned)n_wg), dim3(SK_IDLE_SPAN), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.max_out <= 0) return (int)e;
  hipLaunchKernelGGL(sk_idle_scatter_kernel, dim3((unsigned)n_wg), dim3(SK_IDLE_SPAN), 0, stream, a);
  return (int)hipGetLastError();
}
