// skred_owner_kernels.hip -- note owners: one 32-bit tag per slot, and stamps that only land where the tag is the expected one
// (gfx950 / CDNA4, wave64).
//
// skred_bank_tag_slots / _find_owned / _stamp_owned / _release_tags (include/skred_amd.h).  owner[n_voices] holds a slot's tag at
// the slot's first voice, 0 for nobody; only these kernels and sk_ctl_owned_kernel (skred_ctl_kernels.hip) read or write it, no
// render kernel knows it exists.
//
//   sk_owner_tag_kernel     one lane per entry of a list in device memory: owner[entry] = tag for the first min(n, *d_count) entries
//                           that are slots of the bank (sk_slot_valid: the rule of sk_slot_stamps_kernel).  One plain dword store.
//   sk_owner_find_kernel    one lane per SLOT of [first, first + count): the lane reads its slot's owner word (a load of stride K
//                           words); a workgroup in which no lane holds a tag is done.  Otherwise the n sorted tags and where each
//                           stood in the caller's array are staged in LDS (8 bytes a tag, 8 KiB at most, padded with all-ones to a
//                           power of two), every lane with a non-zero word runs a lower-bound search over them -- log2 steps, each
//                           one LDS read and a select on an UNSIGNED compare, no divergence -- and on a hit takes an unsigned
//                           atomicMin of its first voice onto d_out[perm[j]], preset to all-ones (-1) on the stream.  A minimum
//                           does not depend on the order of arrival, and no workgroup waits for another.
//   sk_owner_stamps_kernel  sk_slot_stamps_kernel (one thread per entry and voice of the slot) with the guard owner[entry] == tag;
//                           the stores are sk_stamp_store's.  Stamped / stolen / no-slot ENTRIES are counted by the threads of
//                           voice 0: wave ballots, LDS, one atomic add per workgroup and count -- integer sums.
//
// Plain vector stores and ordinary atomics only.  The owner words a launch reads are never written by that launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"
#include "skred_update_common.hpp"   // the list rule, sk_entry_decode, sk_entry_owned, sk_stamp_store, sk_owner_count, sk_batch_done

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_owner_tag_kernel(uint32_t *owner, const int32_t *d_slots,
                                                                     const uint32_t *__restrict__ tags, int n, const uint32_t *d_count,
                                                                     int K, int n_voices, uint32_t *d_result, uint32_t *cnt,
                                                                     uint32_t *done, uint32_t seq) {
  __shared__ uint32_t sums[2];
  const int64_t i = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  const bool looked = sk_list_looked(i, n, d_count);
  bool valid = false;
  if (looked) {
    const int e = d_slots[i];
    valid = sk_slot_valid(e, K, n_voices);
    if (valid) owner[e] = tags[i];
  }
  const bool flag[2] = { valid, looked && !valid };
  sk_owner_count<2>(sums, d_result, flag);
  sk_batch_done(cnt, done, seq);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_owner_find_kernel(const uint32_t *__restrict__ owner, int first, int n_slots,
                                                                      int k_shift, const uint32_t *__restrict__ sorted,
                                                                      const uint32_t *__restrict__ perm, int n, int padded,
                                                                      uint32_t *d_out, uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t lds_tag[SK_OWNER_MAX_TAGS];
  __shared__ uint32_t lds_perm[SK_OWNER_MAX_TAGS];
  const int64_t s = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  const int v = first + (int)((s < n_slots ? s : 0) << k_shift);        // (inside the bank: checked on the host)
  const uint32_t w = s < n_slots ? owner[v] : 0u;
  if (__syncthreads_or(w != 0u)) {                                      // (uniform over the workgroup)
    for (int i = threadIdx.x; i < padded; i += SK_CONTROL_SPAN) {
      lds_tag[i] = i < n ? sorted[i] : 0xFFFFFFFFu;
      lds_perm[i] = i < n ? perm[i] : 0u;
    }
    __syncthreads();
    if (w != 0u) {
      // the first position whose tag is >= w (padded - 1 when every tag is below w): `padded` is a power of two
      int base = 0;
      for (int half = padded >> 1; half > 0; half >>= 1) base += lds_tag[base + half - 1] < w ? half : 0;
      if (base < n && lds_tag[base] == w) atomicMin(d_out + lds_perm[base], (uint32_t)v);
    }
  }
  sk_batch_done(cnt, done, seq);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_owner_stamps_kernel(const uint32_t *__restrict__ owner, const int32_t *d_slots,
                                                                        const uint32_t *__restrict__ tags, int n, const uint32_t *d_count,
                                                                        int k_shift, uint64_t voice_mask, int n_voices, uint32_t dirty,
                                                                        sk_plane_ptrs_t p, uint64_t now, uint64_t *mask,
                                                                        uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t sums[3];
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);
  const bool mine = sk_entry_owned(owner, tags, t);
  if (mine && ((voice_mask >> t.l) & 1)) sk_stamp_store(p, now, mask, t.e + t.l, dirty);
  const bool head = t.looked && t.l == 0;                               // one thread per entry counts it
  const bool flag[3] = { head && mine, head && t.valid && !mine, head && !t.valid };
  sk_owner_count<3>(sums, d_result, flag);
  sk_batch_done(cnt, done, seq);
}

extern "C" int sk_launch_owner_tag(uint32_t *owner, const int32_t *d_slots, const uint32_t *d_tags, int n, const uint32_t *d_count,
                                   int slot_voices, int n_voices, uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq,
                                   hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 2, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sk_owner_tag_kernel, dim3(sk_grid(n)), dim3(SK_CONTROL_SPAN), 0, stream, owner, d_slots, d_tags, n, d_count, slot_voices,
                     n_voices, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_owner_find(const uint32_t *owner, int first, int count, int slot_voices, const uint32_t *d_sorted,
                                    const uint32_t *d_perm, int n, int32_t *d_out, uint32_t *cnt, uint32_t *done, uint32_t seq,
                                    hipStream_t stream) {
  if (n <= 0 || n > SK_OWNER_MAX_TAGS || count <= 0) return 0;
  const hipError_t e = hipMemsetAsync(d_out, 0xFF, (size_t)n * sizeof(int32_t), stream);
  if (e != hipSuccess) return (int)e;
  const int sh = sk_slot_shift(slot_voices), n_slots = count >> sh;
  int padded = 1;
  while (padded < n) padded <<= 1;
  hipLaunchKernelGGL(sk_owner_find_kernel, dim3(sk_grid(n_slots)), dim3(SK_CONTROL_SPAN), 0, stream, owner, first, n_slots, sh, d_sorted, d_perm, n,
                     padded, reinterpret_cast<uint32_t *>(d_out), cnt, done, seq);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_owner_stamps(const uint32_t *owner, const int32_t *d_slots, const uint32_t *d_tags, int n, const uint32_t *d_count,
                                      int slot_voices, uint64_t voice_mask, int n_voices, uint32_t dirty, sk_plane_t *const ro[SKP_COUNT],
                                      sk_plane_t *const rw[SKS_COUNT], uint64_t now, uint64_t *mask, uint32_t *d_result, uint32_t *cnt,
                                      uint32_t *done, uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  const hipError_t e = sk_result_clear(d_result, 3, stream);
  if (e != hipSuccess) return (int)e;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_owner_stamps_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, owner, d_slots, d_tags, n, d_count, sh,
                     voice_mask, n_voices, dirty, p, now, mask, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}
