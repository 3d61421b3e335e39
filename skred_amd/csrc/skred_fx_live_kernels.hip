// skred_fx_live_kernels.hip -- live control of the fixed-point bank (gfx950 / CDNA4): updates, the free-voice list, note-ons.
//
// The fixed-point twins of skred_update_kernels.hip, skred_idle_kernels.hip and skred_note_kernels.hip, on the planes of
// skred_fx_layout.h (include/skred_amd_fxpt.h: skred_fxbank_update / _find_idle / _notes_on_list / _stamp_list).  The render
// kernel (skred_fx_kernels.hip) is not involved: everything it reads lives in those planes.
//
//   sk_fx_update_kernel        one thread per record of a batch.  PARAMS overwrites the parameter planes whole -- except SKX_TIME,
//                              which is its own kind (a stamped note-off must survive), and the two pan words of SKX_GAIN, which
//                              are PAN's --; the read-write planes are patched word by word and the flags word bit by bit, so
//                              whatever the update does not name keeps the value the render kernel last stored.  Records of one
//                              launch name distinct voices (the host splits batches): no write conflicts.
//   sk_fx_idle_count_kernel    every workgroup takes SKX_IDLE_SPAN consecutive voices (spans aligned to 64 voices), evaluates the
//                              predicate, ballots per wave and publishes its count write-through.  The workgroup that ARRIVES LAST
//                              (sk_arrive_last: one ticket, re-armed for the next launch) turns the counts into exclusive offsets
//                              and writes d_count and the rank of `from`.  No workgroup waits for another.
//   sk_fx_idle_scatter_kernel  the same spans, evaluated again: rank = workgroup offset + wave prefix + mbcnt of the ballot,
//                              rotated by the rank of `from` modulo the total, stored when it is below max_out.
//   sk_fx_notes_kernel         one thread per note: note k takes entry first_entry + k of a list in device memory when that entry
//                              exists and names a voice of the bank, otherwise it is dropped.  Word stores only.
//   sk_fx_stamp_list_kernel    sk_fx_stamp_kernel's stores for the first min(n, *d_count) entries of a device list, skipping
//                              entries that name no voice of the bank.
//
// The order of a list is fixed by the voice index, never by arrival, and the result counts are integer sums: the same state
// gives the same bytes.  The query kernels only READ the bank, and only the words the query's bits need: the flags word of
// read-write plane 0 for FINISHED and ENV_DONE, the smoother gain and SKX_OSC's flags for ENV_DONE, amp_q15 for AMP_ZERO.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_fx_ctl_common.hpp"  // skx_stamp_store: shared with skred_fx_owner_kernels.hip
#include "skred_fx_idle_common.hpp" // skx_idle_pred, SKXI_*: shared with skred_fx_steal_kernels.hip
#include "skred_fx_layout.h"
#include "skred_kernel_common.hpp"   // sk_arrive_last, sk_gu32

// the public bit values (include/skred_amd.h: SKRED_DIRTY_* / SKRED_STAMP_* / SKRED_NOTE_*, and SKRED_IDLE_* in
// skred_fx_idle_common.hpp; checked against the header in skred_fx_live.c)
enum { SKXU_PARAMS = 1u << 0, SKXU_PHASE = 1u << 1, SKXU_ENV_STATE = 1u << 2, SKXU_PAN = 1u << 3, SKXU_FILTER_STATE = 1u << 4,
       SKXU_SMOOTHER = 1u << 5, SKXU_SAMPLE = 1u << 7, SKXU_STAMP_TRIGGER = 1u << 8, SKXU_STAMP_RELEASE = 1u << 9,
       SKXU_ENV_CLOCK = 1u << 10 };
enum { SKXN_SET_PHASE = 1u << 0, SKXN_SET_PAN = 1u << 1 };

struct skx_plane_ptrs_t {
  skx_plane_t *ro[SKX_COUNT];
  skx_plane_t *rw[SKX_RW_COUNT];
};

// ---------------------------------------------------------------------------------------------------------------- updates

__global__ __launch_bounds__(64) void sk_fx_update_kernel(const skx_update_t *__restrict__ u, int n, skx_plane_ptrs_t p, uint64_t now) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const skx_update_t r = u[i];
  const int v = r.voice;
  const uint32_t d = r.dirty;
  if (d & SKXU_PARAMS) {
    *reinterpret_cast<uint4 *>(&p.ro[SKX_OSC][v]) = *reinterpret_cast<const uint4 *>(&r.ro[SKX_OSC]);
    *reinterpret_cast<uint4 *>(&p.ro[SKX_ENV][v]) = *reinterpret_cast<const uint4 *>(&r.ro[SKX_ENV]);
    *reinterpret_cast<uint4 *>(&p.ro[SKX_RECIP][v]) = *reinterpret_cast<const uint4 *>(&r.ro[SKX_RECIP]);
    *reinterpret_cast<uint4 *>(&p.ro[SKX_FILT][v]) = *reinterpret_cast<const uint4 *>(&r.ro[SKX_FILT]);
    *reinterpret_cast<uint4 *>(&p.ro[SKX_FILT2][v]) = *reinterpret_cast<const uint4 *>(&r.ro[SKX_FILT2]);
    *reinterpret_cast<uint2 *>(&p.ro[SKX_GAIN][v].w[2]) = make_uint2(r.ro[SKX_GAIN].w[2], r.ro[SKX_GAIN].w[3]);   // smoother k, velocity
  }
  if (d & SKXU_PAN) *reinterpret_cast<uint2 *>(&p.ro[SKX_GAIN][v].w[0]) = make_uint2(r.ro[SKX_GAIN].w[0], r.ro[SKX_GAIN].w[1]);
  if (d & SKXU_ENV_CLOCK) *reinterpret_cast<uint4 *>(&p.ro[SKX_TIME][v]) = *reinterpret_cast<const uint4 *>(&r.ro[SKX_TIME]);
  if (d & SKXU_FILTER_STATE) *reinterpret_cast<uint4 *>(&p.rw[1][v]) = *reinterpret_cast<const uint4 *>(&r.rw[1]);
  if (d & (SKXU_PHASE | SKXU_ENV_STATE | SKXU_SMOOTHER | SKXU_SAMPLE | SKXU_STAMP_TRIGGER | SKXU_STAMP_RELEASE)) {
    uint4 s = *reinterpret_cast<const uint4 *>(&p.rw[0][v]);
    const uint32_t rf = r.rw[0].w[3];
    if (d & SKXU_PHASE) { s.x = r.rw[0].w[0]; s.w = (s.w & ~SKXR_FINISHED) | (rf & SKXR_FINISHED); }
    if (d & SKXU_ENV_STATE) s.w = (s.w & ~SKXR_ACTIVE) | (rf & SKXR_ACTIVE);
    if (d & SKXU_SMOOTHER) s.y = r.rw[0].w[1];
    if (d & SKXU_SAMPLE) s.z = r.rw[0].w[2];
    if (d & (SKXU_STAMP_TRIGGER | SKXU_STAMP_RELEASE)) {
      uint4 t = *reinterpret_cast<const uint4 *>(&p.ro[SKX_TIME][v]);   // after the ENV_CLOCK write above, if any
      if (d & SKXU_STAMP_TRIGGER) { t.x = (uint32_t)now; t.y = (uint32_t)(now >> 32); t.z = 0; t.w = 0; s.w |= SKXR_ACTIVE; }
      if ((d & SKXU_STAMP_RELEASE) && (s.w & SKXR_ACTIVE)) { t.z = (uint32_t)now; t.w = (uint32_t)(now >> 32); }
      *reinterpret_cast<uint4 *>(&p.ro[SKX_TIME][v]) = t;
    }
    *reinterpret_cast<uint4 *>(&p.rw[0][v]) = s;
  }
}

static void skx_plane_ptrs(skx_plane_ptrs_t &p, skx_plane_t *const ro[SKX_COUNT], skx_plane_t *const rw[SKX_RW_COUNT]) {
  for (int k = 0; k < SKX_COUNT; ++k) p.ro[k] = ro[k];
  for (int k = 0; k < SKX_RW_COUNT; ++k) p.rw[k] = rw[k];
}

extern "C" int skx_launch_update(const skx_update_t *d_updates, int n, skx_plane_t *const ro[SKX_COUNT],
                                 skx_plane_t *const rw[SKX_RW_COUNT], uint64_t now, hipStream_t stream) {
  if (n <= 0) return 0;
  skx_plane_ptrs_t p;
  skx_plane_ptrs(p, ro, rw);
  hipLaunchKernelGGL(sk_fx_update_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, d_updates, n, p, now);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- the idle list

#define SKX_IDLE_WAVES (SKX_IDLE_SPAN / 64)

__device__ __forceinline__ int skx_idle_voice(const skx_idle_args_t &a, bool &in_range) {
  const int v = a.base + (int)blockIdx.x * SKX_IDLE_SPAN + (int)threadIdx.x;   // base: `first` rounded down to 64
  in_range = v >= a.first && v < a.end;
  return v;
}

__global__ __launch_bounds__(SKX_IDLE_SPAN) void sk_fx_idle_count_kernel(skx_idle_args_t a) {
  __shared__ int lds[SKX_IDLE_SPAN + 2 * SKX_IDLE_WAVES + 1];
  const int tid = threadIdx.x, wave = tid >> 6;
  bool in_range;
  const int v = skx_idle_voice(a, in_range);
  const bool idle = skx_idle_pred(a, v, in_range);
  const unsigned long long ballot = __ballot(idle);
  // the rank of `from`: the idle voices below it.  Its workgroup counts the ones inside its own span.
  const unsigned long long below = __ballot(idle && v < a.from);
  if ((tid & 63) == 0) { lds[wave] = __popcll(ballot); lds[SKX_IDLE_WAVES + wave] = __popcll(below); }
  __syncthreads();
  if (tid == 0) {
    int c = 0, p = 0;
#pragma unroll
    for (int w = 0; w < SKX_IDLE_WAVES; ++w) { c += lds[w]; p += lds[SKX_IDLE_WAVES + w]; }
    __hip_atomic_store((sk_gu32 *)(a.counts + blockIdx.x), (uint32_t)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((int)blockIdx.x == a.from_wg)
      __hip_atomic_store((sk_gu32 *)(a.words + SKX_IDLE_W_PART), (uint32_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!sk_arrive_last(a.words + SKX_IDLE_W_TICKET, gridDim.x, tid, &lds[2 * SKX_IDLE_WAVES])) return;
  // ---- the last arriver: exclusive offsets of all workgroups, in index order.  Thread t owns a contiguous run of counts.
  const int n = (int)gridDim.x;
  const int per = (n + SKX_IDLE_SPAN - 1) / SKX_IDLE_SPAN;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += (int)a.counts[i];
  int *scan = &lds[2 * SKX_IDLE_WAVES + 1];
  scan[tid] = sum;
  __syncthreads();
  for (int d = 1; d < SKX_IDLE_SPAN; d <<= 1) {         // inclusive scan of the per-thread sums
    const int add = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  int run = scan[tid] - sum;
  for (int i = lo; i < hi; ++i) {
    a.offsets[i] = (uint32_t)run;
    if (i == a.from_wg) a.words[SKX_IDLE_W_RANK] = (uint32_t)run + a.words[SKX_IDLE_W_PART];
    run += (int)a.counts[i];
  }
  if (tid == SKX_IDLE_SPAN - 1) {
    const uint32_t total = (uint32_t)scan[tid];
    a.words[SKX_IDLE_W_TOTAL] = total;
    a.d_count[0] = total < (uint32_t)a.max_out ? total : (uint32_t)a.max_out;
    a.d_count[1] = total;
  }
}

__global__ __launch_bounds__(SKX_IDLE_SPAN) void sk_fx_idle_scatter_kernel(skx_idle_args_t a) {
  __shared__ int lds[SKX_IDLE_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6;
  bool in_range;
  const int v = skx_idle_voice(a, in_range);
  const bool idle = skx_idle_pred(a, v, in_range);
  const unsigned long long ballot = __ballot(idle);
  if ((tid & 63) == 0) lds[wave] = __popcll(ballot);
  __syncthreads();
  if (!idle) return;
  int rank = (int)a.offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) rank += lds[w];
  rank += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
  const int total = (int)a.words[SKX_IDLE_W_TOTAL];
  int at = rank - (int)a.words[SKX_IDLE_W_RANK];      // the list starts at the first idle voice >= from and wraps
  if (at < 0) at += total;
  if (at >= 0 && at < a.max_out) a.d_voices[at] = v;
}

extern "C" int skx_idle_workgroups(int first, int count) {
  const int base = first & ~63;
  return (first + count - base + SKX_IDLE_SPAN - 1) / SKX_IDLE_SPAN;
}

extern "C" int skx_launch_idle(const skx_idle_args_t *args, hipStream_t stream) {
  skx_idle_args_t a = *args;
  a.base = a.first & ~63;
  const int n_wg = skx_idle_workgroups(a.first, a.end - a.first);
  a.from_wg = (a.from - a.base) / SKX_IDLE_SPAN;
  hipLaunchKernelGGL(sk_fx_idle_count_kernel, dim3((unsigned)n_wg), dim3(SKX_IDLE_SPAN), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.max_out <= 0) return (int)e;
  hipLaunchKernelGGL(sk_fx_idle_scatter_kernel, dim3((unsigned)n_wg), dim3(SKX_IDLE_SPAN), 0, stream, a);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- note-ons

// The list names distinct voices (find_idle's does), so two threads never store to one voice.
__global__ __launch_bounds__(SKX_NOTE_SPAN) void sk_fx_notes_kernel(const skx_note_t *__restrict__ notes, int n, const int32_t *d_voices,
                                                                    const uint32_t *d_count, int first_entry, int n_voices,
                                                                    skx_plane_ptrs_t p, uint64_t now, int32_t *d_assigned,
                                                                    uint32_t *d_result) {
  __shared__ uint32_t placed_w[SKX_NOTE_SPAN / 64];
  const int tid = threadIdx.x;
  const int k = blockIdx.x * SKX_NOTE_SPAN + tid;
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
    const skx_note_t r = notes[k];
    p.ro[SKX_OSC][v].w[0] = r.w[SKX_NOTE_PHASE_INC];
    p.ro[SKX_GAIN][v].w[3] = r.w[SKX_NOTE_VELOCITY];
    const uint32_t flags = r.w[SKX_NOTE_FLAGS];
    uint32_t *rwflags = &p.rw[0][v].w[3];
    uint32_t f = *rwflags | SKXR_ACTIVE;
    if (flags & SKXN_SET_PHASE) {
      p.rw[0][v].w[0] = r.w[SKX_NOTE_PHASE];
      f &= ~SKXR_FINISHED;
    }
    *rwflags = f;
    if (flags & SKXN_SET_PAN)
      *reinterpret_cast<uint2 *>(&p.ro[SKX_GAIN][v].w[0]) = make_uint2(r.w[SKX_NOTE_PAN_LEFT], r.w[SKX_NOTE_PAN_RIGHT]);
    *reinterpret_cast<uint4 *>(&p.ro[SKX_TIME][v]) = make_uint4((uint32_t)now, (uint32_t)(now >> 32), 0u, 0u);
  }
  if (d_assigned && k < n) d_assigned[k] = v;
  const unsigned long long placed = __ballot(v >= 0);
  if ((tid & 63) == 0) placed_w[tid >> 6] = (uint32_t)__popcll(placed);
  __syncthreads();
  if (tid == 0) {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < SKX_NOTE_SPAN / 64; ++w) c += placed_w[w];
    const int here = min(n - (int)blockIdx.x * SKX_NOTE_SPAN, SKX_NOTE_SPAN);      // notes of this workgroup
    if (gridDim.x == 1) { d_result[0] = c; d_result[1] = (uint32_t)here - c; }
    else { atomicAdd(d_result, c); atomicAdd(d_result + 1, (uint32_t)here - c); }
  }
}

__global__ __launch_bounds__(256) void sk_fx_stamp_list_kernel(const int32_t *d_voices, int n, const uint32_t *d_count, int n_voices,
                                                               uint32_t stamps, skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (d_count && (uint32_t)i >= d_count[0]) return;
  const int v = d_voices[i];
  if (v < 0 || v >= n_voices) return;
  skx_stamp_store(time_plane, rw0, v, stamps, now);
}

// more than SKX_NOTE_SPAN notes: d_result is zeroed on `stream` ahead of the launch, the workgroups add their counts onto it
extern "C" int skx_launch_notes(const skx_note_t *d_notes, int n, const int32_t *d_voices, const uint32_t *d_count, int first_entry,
                                int n_voices, skx_plane_t *const ro[SKX_COUNT], skx_plane_t *const rw[SKX_RW_COUNT], uint64_t now,
                                int32_t *d_assigned, uint32_t *d_result, hipStream_t stream) {
  if (n <= 0) return 0;
  skx_plane_ptrs_t p;
  skx_plane_ptrs(p, ro, rw);
  const unsigned n_wg = (unsigned)((n + SKX_NOTE_SPAN - 1) / SKX_NOTE_SPAN);
  if (n_wg > 1) {
    const hipError_t e = hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(sk_fx_notes_kernel, dim3(n_wg), dim3(SKX_NOTE_SPAN), 0, stream, d_notes, n, d_voices, d_count, first_entry,
                     n_voices, p, now, d_assigned, d_result);
  return (int)hipGetLastError();
}

extern "C" int skx_launch_stamp_list(const int32_t *d_voices, int n, const uint32_t *d_count, int n_voices, uint32_t stamps,
                                     skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(sk_fx_stamp_list_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_voices, n, d_count, n_voices,
                     stamps, time_plane, rw0, now);
  return (int)hipGetLastError();
}
