// skred_slot_kernels.hip -- patch notes: which slots of a range are idle, and notes and stamps on the voices of listed slots
// (gfx950 / CDNA4, wave64).
//
// skred_bank_find_idle_slots / _notes_on_slots / _stamp_slots (include/skred_amd.h).  A slot is an aligned run of K voices, K a
// power of two <= 64, named by its first voice: one copy of a patch tiled over the bank.  A wavefront's 64 voices hold 64 / K whole
// slots, so everything a slot needs to know about its voices is in one ballot.
//
//   sk_slot_count_kernel    sk_idle_count_kernel with another notion of "listed": one lane per voice, sk_idle_pred per lane, one
//   sk_slot_scatter_kernel  __ballot per wave; the lane of a slot's FIRST voice is listed when every member voice of its slot (a bit in
//                           member_mask) is idle: (ballot >> lane) & member_mask == member_mask.  Voices outside the mask never
//                           decide anything.  The counts, the last arriver's exclusive offsets, the rank of `from` and the rotated
//                           scatter are skred_idle_scan.hpp's, shared with the free-voice list: the order is fixed by the voice
//                           index, no workgroup waits for another, and with K = 1, mask 1 the two lists are the same bytes.
//   sk_slot_notes_kernel    one thread per (note, voice of the slot).  Note k takes entry first_entry + k of the list when that
//                           entry exists (below d_count[0], read here, at this point of the stream) and is a slot of the bank;
//                           otherwise it is dropped whole.  Each lane with a bit in voice_mask stores sk_note_store's words for
//                           ITS record -- the increments arrive finished, there is no arithmetic here -- and lanes without a
//                           bit neither read their record nor touch their voice.  Placed / dropped NOTES are counted per wave
//                           (ballot of the first lanes) and per workgroup (LDS); one workgroup stores the result words itself, a
//                           larger launch adds integer sums onto words the launcher zeroed on the stream.
//   sk_slot_stamps_kernel   one thread per (entry, voice of the slot): sk_stamp_store on the masked voices of the first
//                           min(n, *d_count) entries that are slots of the bank (the -1 of a dropped note is none).
//
// All stores into the planes are plain vector stores.  A list the query wrote names distinct slots, so two threads never store to
// one voice.  The notes and stamps kernels take ANY list, though -- an earlier d_assigned, one the caller made -- and with an entry
// named twice the threads of both race on that slot's words, as on the per-voice path: which note a voice ends with is then
// unspecified, nothing else is affected (include/skred_amd.h says so for both calls).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_idle_common.hpp"   // sk_idle_pred: the predicate of one voice
#include "skred_idle_scan.hpp"     // counts, offsets, rank of `from`, scatter
#include "skred_launch.h"
#include "skred_update_common.hpp" // sk_note_store, sk_stamp_store, sk_slot_valid, sk_entry_decode, sk_batch_done, the launch helpers

// this lane is the first voice of an idle slot (v: its voice; a slot never straddles a wavefront: spans start at a multiple of 64)
__device__ __forceinline__ bool sk_slot_listed(const sk_slot_args_t &s, int v, bool in_range) {
  const bool idle = sk_idle_pred(s.idle, v, in_range);
  const unsigned long long ballot = __ballot(idle);
  const int lane = (int)threadIdx.x & 63;
  const bool head = (lane & (s.slot_voices - 1)) == 0;          // (first and count are multiples of K: a head in range has its slot in range)
  return head && in_range && ((ballot >> lane) & s.member_mask) == s.member_mask;
}

__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_slot_count_kernel(sk_slot_args_t s) {
  __shared__ int lds[SK_IDLE_COUNT_LDS];
  bool in_range;
  const int v = sk_idle_voice(s.idle, in_range);
  sk_idle_count_tail(s.idle, v, sk_slot_listed(s, v, in_range), lds);
}

__global__ __launch_bounds__(SK_IDLE_SPAN) void sk_slot_scatter_kernel(sk_slot_args_t s) {
  __shared__ int lds[SK_IDLE_WAVES];
  bool in_range;
  const int v = sk_idle_voice(s.idle, in_range);
  sk_idle_scatter_tail(s.idle, v, sk_slot_listed(s, v, in_range), lds);
}

__global__ __launch_bounds__(SK_NOTE_SPAN) void sk_slot_notes_kernel(const sk_note_t *__restrict__ notes, int n, int k_shift,
                                                                     uint64_t voice_mask, const int32_t *d_slots,
                                                                     const uint32_t *d_count, int first_entry, int n_voices,
                                                                     sk_plane_ptrs_t p, uint64_t now, uint64_t *mask,
                                                                     int32_t *d_assigned, uint32_t *d_result,
                                                                     uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t placed_w[SK_NOTE_SPAN / 64];
  const int tid = threadIdx.x;
  const int K = 1 << k_shift, per_wg = SK_NOTE_SPAN >> k_shift;               // notes per workgroup
  const int k = (int)blockIdx.x * per_wg + (tid >> k_shift), l = tid & (K - 1);
  const uint32_t listed = d_count[0];
  int e = -1;
  if (k < n) {
    const uint64_t at = (uint64_t)(uint32_t)first_entry + (uint64_t)(uint32_t)k;   // (both non-negative: checked on the host)
    if (at < (uint64_t)listed) {
      const int c = d_slots[at];
      if (sk_slot_valid(c, K, n_voices)) e = c;
    }
  }
  if (e >= 0 && ((voice_mask >> l) & 1)) {
    const sk_note_t r = notes[((size_t)k << k_shift) + l];
    sk_note_store(p, now, mask, e + l, r);
  }
  if (d_assigned && k < n && l == 0) d_assigned[k] = e;
  const unsigned long long placed = __ballot(e >= 0 && l == 0);
  if ((tid & 63) == 0) placed_w[tid >> 6] = (uint32_t)__popcll(placed);
  __syncthreads();
  if (tid == 0) {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < SK_NOTE_SPAN / 64; ++w) c += placed_w[w];
    const int here = min(n - (int)blockIdx.x * per_wg, per_wg);                // notes of this workgroup
    if (gridDim.x == 1) { d_result[0] = c; d_result[1] = (uint32_t)here - c; }
    else { atomicAdd(d_result, c); atomicAdd(d_result + 1, (uint32_t)here - c); }
  }
  sk_batch_done(cnt, done, seq);
}

__global__ __launch_bounds__(SK_CONTROL_SPAN) void sk_slot_stamps_kernel(const int32_t *d_slots, int n, const uint32_t *d_count, int k_shift,
                                                                         uint64_t voice_mask, int n_voices, uint32_t dirty,
                                                                         sk_plane_ptrs_t p, uint64_t now, uint64_t *mask) {
  const sk_entry_t t = sk_entry_decode(SK_CONTROL_SPAN, k_shift, d_slots, n, d_count, n_voices);
  if (t.valid && ((voice_mask >> t.l) & 1)) sk_stamp_store(p, now, mask, t.e + t.l, dirty);
}

extern "C" int sk_launch_slots(const sk_slot_args_t *args, hipStream_t stream) {
  sk_slot_args_t s = *args;
  s.idle.base = s.idle.first & ~63;
  const int n_wg = sk_idle_workgroups(s.idle.first, s.idle.end - s.idle.first);
  s.idle.from_wg = (s.idle.from - s.idle.base) / SK_IDLE_SPAN;
  hipLaunchKernelGGL(sk_slot_count_kernel, dim3((unsigned)n_wg), dim3(SK_IDLE_SPAN), 0, stream, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || s.idle.max_out <= 0) return (int)e;
  hipLaunchKernelGGL(sk_slot_scatter_kernel, dim3((unsigned)n_wg), dim3(SK_IDLE_SPAN), 0, stream, s);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_slot_notes(const sk_note_t *d_notes, int n, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                                    const uint32_t *d_count, int first_entry, int n_voices, sk_plane_t *const ro[SKP_COUNT],
                                    sk_plane_t *const rw[SKS_COUNT], uint64_t now, uint64_t *mask, int32_t *d_assigned,
                                    uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  const int sh = sk_slot_shift(slot_voices), per_wg = SK_NOTE_SPAN >> sh;
  const unsigned n_wg = (unsigned)(((long long)n + per_wg - 1) / per_wg);
  if (n_wg > 1) {
    const hipError_t e = hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(sk_slot_notes_kernel, dim3(n_wg), dim3(SK_NOTE_SPAN), 0, stream, d_notes, n, sh, voice_mask, d_slots, d_count,
                     first_entry, n_voices, p, now, mask, d_assigned, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_slot_stamps(const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices, uint64_t voice_mask,
                                     int n_voices, uint32_t dirty, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT],
                                     uint64_t now, uint64_t *mask, hipStream_t stream) {
  if (n <= 0) return 0;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  const int sh = sk_slot_shift(slot_voices);
  hipLaunchKernelGGL(sk_slot_stamps_kernel, dim3(sk_list_grid(n, sh)), dim3(SK_CONTROL_SPAN), 0, stream, d_slots, n, d_count, sh, voice_mask, n_voices, dirty, p, now,
                     mask);
  return (int)hipGetLastError();
}
