// skred_fx_ctl_kernels.hip -- controllers of the fixed-point bank: a few parameter words of resident voices, changed on the device
// (gfx950 / CDNA4, wave64).
//
// skred_fxbank_ctl_range / _ctl_list / _ctl_owned (include/skred_amd_fxpt.h).  A controller is ONE record (skx_ctl_t: the image of
// skred_fx_ctl_t, the reciprocals of the frame counts in its last three words); a voice receives the words its `which` names and
// nothing else.
//
//   sk_fx_ctl_range_kernel  one lane per voice of [first, first + count), 256-thread workgroups.  A wavefront's 64 lanes are 64
//                           consecutive voices: every plane access is one coalesced 16-byte load or store per lane (the lone a2 word
//                           of SKX_FILT2 and the three words of SKX_RECIP are narrower stores).  Bandwidth-bound.
//   sk_fx_ctl_list_kernel   one lane per entry of a list in device memory: the first min(n, *d_count) entries, entries outside the
//                           bank skipped.  With `owner` non-NULL it is the guarded form (skred_fxbank_ctl_owned): an entry whose owner
//                           word is not its tag is left alone and counted.
//
// The record is read from DEVICE memory (the staging slot's twin) at addresses uniform over the launch -- never from the pinned
// host buffer, which every workgroup of a bank-wide range would fetch over the bus.  A plane that holds a named word beside unnamed
// ones is read, patched and written back whole; a plane without a named word is not touched.  Plain vector stores only.  No
// workgroup waits for another; the counts are integer sums (skx_count).
//
// The one piece of arithmetic is SKX_C_INC_SCALE: a 32 x 32 -> 64 bit product shifted right by 16, stored only when it fits 32 bits.
// SKX_C_AMP is stored only where the voice's amp_q15 is not 0: a voice that cannot sound stays one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_ctl_common.hpp"   // skx_ctl_store, skx_ctl_planes_t, skx_list_looked, skx_count
#include "skred_fx_layout.h"

__global__ __launch_bounds__(SKX_CTL_SPAN) void sk_fx_ctl_range_kernel(const skx_ctl_t *__restrict__ rec, int first, int count,
                                                                       skx_ctl_planes_t p, uint32_t *d_result) {
  __shared__ uint32_t sums[2];
  const int64_t off = (int64_t)blockIdx.x * SKX_CTL_SPAN + threadIdx.x;
  const bool mine = off < count;
  uint32_t withheld = 0;
  if (mine) withheld = skx_ctl_store(p, first + (int)off, rec->w);     // (inside the bank: checked on the host)
  const uint32_t val[2] = { mine ? 1u : 0u, withheld };
  skx_count<2>(sums, d_result, val);
}

__global__ __launch_bounds__(SKX_CTL_SPAN) void sk_fx_ctl_list_kernel(const skx_ctl_t *__restrict__ rec, const int32_t *d_voices,
                                                                      const uint32_t *__restrict__ tags,
                                                                      const uint32_t *__restrict__ owner, int n, const uint32_t *d_count,
                                                                      int n_voices, skx_ctl_planes_t p, uint32_t *d_result) {
  __shared__ uint32_t sums[3];
  const int64_t i = (int64_t)blockIdx.x * SKX_CTL_SPAN + threadIdx.x;
  bool valid = false, mine = false;
  uint32_t withheld = 0;
  if (skx_list_looked(i, n, d_count)) {
    const int v = d_voices[i];
    valid = v >= 0 && v < n_voices;
    mine = valid && (!owner || owner[v] == tags[i]);
    if (mine) withheld = skx_ctl_store(p, v, rec->w);
  }
  if (owner) {
    const uint32_t val[3] = { mine ? 1u : 0u, withheld, (valid && !mine) ? 1u : 0u };
    skx_count<3>(sums, d_result, val);
  } else {
    const uint32_t val[2] = { mine ? 1u : 0u, withheld };
    skx_count<2>(sums, d_result, val);
  }
}

extern "C" int skx_launch_ctl_range(const skx_ctl_t *d_rec, int first, int count, skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result,
                                    hipStream_t stream) {
  if (count <= 0) return 0;
  if (d_result) {
    const hipError_t e = hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
  }
  skx_ctl_planes_t p;
  skx_ctl_planes(p, ro);
  const unsigned n_wg = (unsigned)(((long long)count + SKX_CTL_SPAN - 1) / SKX_CTL_SPAN);
  hipLaunchKernelGGL(sk_fx_ctl_range_kernel, dim3(n_wg), dim3(SKX_CTL_SPAN), 0, stream, d_rec, first, count, p, d_result);
  return (int)hipGetLastError();
}

// d_tags and owner both NULL: skred_fxbank_ctl_list (d_result[2]); both set: skred_fxbank_ctl_owned (d_result[3])
extern "C" int skx_launch_ctl_list(const skx_ctl_t *d_rec, const int32_t *d_voices, const uint32_t *d_tags, const uint32_t *owner, int n,
                                   const uint32_t *d_count, int n_voices, skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result,
                                   hipStream_t stream) {
  if (n <= 0) return 0;
  if (d_result) {
    const hipError_t e = hipMemsetAsync(d_result, 0, (owner ? 3 : 2) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
  }
  skx_ctl_planes_t p;
  skx_ctl_planes(p, ro);
  const unsigned n_wg = (unsigned)(((long long)n + SKX_CTL_SPAN - 1) / SKX_CTL_SPAN);
  hipLaunchKernelGGL(sk_fx_ctl_list_kernel, dim3(n_wg), dim3(SKX_CTL_SPAN), 0, stream, d_rec, d_voices, owner ? d_tags : nullptr, owner, n,
                     d_count, n_voices, p, d_result);
  return (int)hipGetLastError();
}
