// skred_note_kernels.hip -- control actions on voices only the device can name (gfx950 / CDNA4).
//
// skred_bank_notes_on_list / _note_on_idle / _stamp_list (include/skred_amd.h): the voices come from a list in device memory
// -- what skred_bank_find_idle left there, or an earlier call's d_assigned -- so the host never waits for it.
//
//   sk_notes_kernel       one thread per note.  Note k takes entry first_entry + k of the list when that entry exists
//                         (below d_count[0], read here, at this point of the stream) and names a voice of the bank; otherwise
//                         it is dropped.  On its voice it stores the reference's note-on and nothing else (synth.c:1153-1156):
//                         the increment, the velocity, with SET_PHASE osc_trigger's phase and voice_finished = 0 (synth.c:316-339),
//                         with SET_PAN the pan pair (synth.c:838-847), amp_envelope_trigger's stamp (synth.c:383-388), and the
//                         voice's bit on the motion list.  Word stores into the planes: the neighbours of a word (amp, the
//                         loop window, the smoother's k, the filter) keep what they hold.
//                         The result words: placed / dropped notes are counted per wave (ballot) and per workgroup (LDS);
//                         a launch of ONE workgroup -- up to SK_NOTE_SPAN notes, a block's worth -- stores them itself, a larger
//                         one adds its workgroups' counts onto words the launcher zeroed on the stream.  Integer sums: the
//                         same bytes whatever the arrival order.
//   sk_stamp_list_kernel  sk_stamp_kernel's stores (skred_update_kernels.hip) for the first min(n, *d_count) entries of a
//                         list, skipping entries that name no voice of the bank (the -1 of a dropped note).
//
// The list names distinct voices (find_idle's does), so two threads never store to one voice.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"
#include "skred_update_common.hpp"

__global__ __launch_bounds__(SK_NOTE_SPAN) void sk_notes_kernel(const sk_note_t *__restrict__ notes, int n, const int32_t *d_voices,
                                                                const uint32_t *d_count, int first_entry, int n_voices,
                                                                sk_plane_ptrs_t p, uint64_t now, uint64_t *mask,
                                                                int32_t *d_assigned, uint32_t *d_result,
                                                                uint32_t *cnt, uint32_t *done, uint32_t seq) {
  __shared__ uint32_t placed_w[SK_NOTE_SPAN / 64];
  const int tid = threadIdx.x;
  const int k = blockIdx.x * SK_NOTE_SPAN + tid;
  const uint32_t listed = d_count[0];
  int v = -1;
  if (k < n) {
    const uint64_t at = (uint64_t)(uint32_t)first_entry + (uint64_t)(uint32_t)k;   // (both non-negative: checked on the host)
    if (at < (uint64_t)listed) {
      const int e = d_voices[at];
      if (e >= 0 && e < n_voices) v = e;
    }
  }
  if (v >= 0) {
    const sk_note_t r = notes[k];
    sk_note_store(p, now, mask, v, r);
  }
  if (d_assigned && k < n) d_assigned[k] = v;
  const unsigned long long placed = __ballot(v >= 0);
  if ((tid & 63) == 0) placed_w[tid >> 6] = (uint32_t)__popcll(placed);
  __syncthreads();
  if (tid == 0) {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < SK_NOTE_SPAN / 64; ++w) c += placed_w[w];
    const int here = min(n - (int)blockIdx.x * SK_NOTE_SPAN, SK_NOTE_SPAN);       // notes of this workgroup
    if (gridDim.x == 1) { d_result[0] = c; d_result[1] = (uint32_t)here - c; }
    else { atomicAdd(d_result, c); atomicAdd(d_result + 1, (uint32_t)here - c); }
  }
  sk_batch_done(cnt, done, seq);
}

__global__ __launch_bounds__(256) void sk_stamp_list_kernel(const int32_t *d_voices, int n, const uint32_t *d_count, int n_voices,
                                                            uint32_t dirty, sk_plane_ptrs_t p, uint64_t now, uint64_t *mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (!sk_list_looked(i, n, d_count)) return;
  const int v = d_voices[i];
  if (v < 0 || v >= n_voices) return;
  sk_stamp_store(p, now, mask, v, dirty);
}

extern "C" int sk_launch_notes(const sk_note_t *d_notes, int n, const int32_t *d_voices, const uint32_t *d_count, int first_entry,
                               int n_voices, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t now,
                               uint64_t *mask, int32_t *d_assigned, uint32_t *d_result, uint32_t *cnt, uint32_t *done,
                               uint32_t seq, hipStream_t stream) {
  if (n <= 0) return 0;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  const unsigned n_wg = (unsigned)((n + SK_NOTE_SPAN - 1) / SK_NOTE_SPAN);
  if (n_wg > 1) {
    const hipError_t e = hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(sk_notes_kernel, dim3(n_wg), dim3(SK_NOTE_SPAN), 0, stream, d_notes, n, d_voices, d_count, first_entry,
                     n_voices, p, now, mask, d_assigned, d_result, cnt, done, seq);
  return (int)hipGetLastError();
}

extern "C" int sk_launch_stamp_list(const int32_t *d_voices, int n, const uint32_t *d_count, int n_voices, uint32_t dirty,
                                    sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t now, uint64_t *mask,
                                    hipStream_t stream) {
  if (n <= 0) return 0;
  sk_plane_ptrs_t p;
  sk_planes(p, ro, rw);
  hipLaunchKernelGGL(sk_stamp_list_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_voices, n, d_count, n_voices,
                     dirty, p, now, mask);
  return (int)hipGetLastError();
}
