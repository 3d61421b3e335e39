// skred_update_common.hpp -- what the kernels that apply control actions share, device side first, the launchers' helpers behind it.
//
//   sk_list_voice, sk_note_store, sk_stamp_store   the stores of a note-on and of a stamp: skred_update_kernels.hip (voices the host
//                                                  names), skred_note_kernels.hip (voices a list in device memory names),
//                                                  skred_slot_kernels.hip (the voices of listed slots), and sk_stamp_store again in
//                                                  skred_owner_kernels.hip, skred_expr_kernels.hip, skred_pedal_kernels.hip
//   sk_list_looked, sk_slot_valid                  THE LIST RULE, once: sk_owner_tag_kernel, sk_pedal_clear_kernel (one thread per
//                                                  entry), sk_stamp_list_kernel (entries are voices), and through sk_entry_decode
//   sk_entry_decode, sk_entry_owned                K threads per entry: sk_slot_stamps_kernel, sk_ctl_slots_kernel, sk_glide_clear_kernel;
//                                                  with the owner guard sk_owner_stamps_kernel, sk_pedal_stamps_kernel,
//                                                  sk_ctl_owned_kernel, sk_ctl_owned_each_kernel, sk_glide_start_kernel
//   sk_range_lane                                  one thread per voice of a range of whole slots: sk_ctl_range_kernel,
//                                                  sk_ctl_match_kernel, sk_match_stamps_kernel, sk_pedal_match_kernel
//   sk_owner_count                                 the owner, expression, pedal and glide kernels' counts
//   sk_batch_done                                  every kernel that reads a staged batch
//   sk_planes, sk_slot_shift, sk_grid,             (host) the launchers of all of these units
//   sk_list_grid, sk_result_clear
//
// sk_notes_kernel and sk_slot_notes_kernel keep a rule of their own: note k reads entry first_entry + k, bounded by d_count[0] alone
// (required, read by every thread), and n bounds the notes, not the list.  The masked match (sk_owner_matches) is skred_launch.h's:
// the fixed-point bank's units use it too.
#ifndef SKRED_UPDATE_COMMON_HPP
#define SKRED_UPDATE_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skred_launch.h"

struct sk_plane_ptrs_t {
  sk_plane_t *ro[SKP_COUNT];
  sk_plane_t *rw[SKS_COUNT];
};

// Every voice a control action touches goes on the motion list of the two-per-lane render family (a bit per voice, carried on
// the device: skred_device_layout.h, mask_cur): whatever the action did to its envelope, the envelope kernel renders it in the
// next block and keeps it until it is at rest again.  The render kernels therefore never have to be TOLD that a note started.
__device__ __forceinline__ void sk_list_voice(uint64_t *mask, int v) {
  atomicOr(reinterpret_cast<unsigned long long *>(mask) + (v >> 6), 1ull << (v & 63));
}

// A note-on's stores on voice v (skred_note_kernels.hip: one note per voice; skred_slot_kernels.hip: one record per voice of a slot):
// the reference's note-on and nothing else (synth.c:1153-1156) -- the increment, the velocity, with SET_PHASE osc_trigger's phase
// and voice_finished = 0 (synth.c:316-339), with SET_PAN the pan pair (synth.c:838-847), amp_envelope_trigger's stamp
// (synth.c:383-388), and the voice's bit on the motion list.  Word stores: the neighbours of a word keep what they hold.
__device__ __forceinline__ void sk_note_store(const sk_plane_ptrs_t &p, uint64_t now, uint64_t *mask, int v, const sk_note_t &r) {
  sk_list_voice(mask, v);
  reinterpret_cast<uint32_t *>(&p.ro[SKP_OSC][v])[0] = r.w[SK_NOTE_PHASE_INC];
  reinterpret_cast<uint32_t *>(&p.ro[SKP_GAIN][v])[0] = r.w[SK_NOTE_VELOCITY];
  const uint32_t flags = r.w[SK_NOTE_FLAGS];
  uint32_t *rwflags = reinterpret_cast<uint32_t *>(&p.rw[SKS_FILT][v]) + 3;
  uint32_t f = *rwflags | SKR_ENV_ACTIVE;
  if (flags & SK_NOTE_SET_PHASE) {
    reinterpret_cast<uint32_t *>(&p.rw[SKS_OSC][v])[0] = r.w[SK_NOTE_PHASE];
    f &= ~SKR_FINISHED;
  }
  *rwflags = f;
  if (flags & SK_NOTE_SET_PAN)
    *reinterpret_cast<uint2 *>(reinterpret_cast<uint32_t *>(&p.rw[SKS_MISC][v]) + 2) = make_uint2(r.w[SK_NOTE_PAN_LEFT], r.w[SK_NOTE_PAN_RIGHT]);
  *reinterpret_cast<uint4 *>(&p.ro[SKP_ENV_S][v]) = make_uint4((uint32_t)now, (uint32_t)(now >> 32), 0u, 0u);
}

// SKU_STAMP_TRIGGER and / or SKU_STAMP_RELEASE on voice v, as sk_stamp_kernel (skred_update_kernels.hip) applies them: a release
// only counts on an envelope that is active.
__device__ __forceinline__ void sk_stamp_store(const sk_plane_ptrs_t &p, uint64_t now, uint64_t *mask, int v, uint32_t dirty) {
  sk_list_voice(mask, v);
  uint32_t *rwflags = reinterpret_cast<uint32_t *>(&p.rw[SKS_FILT][v]) + 3;
  uint4 es = *reinterpret_cast<const uint4 *>(&p.ro[SKP_ENV_S][v]);
  uint32_t f = *rwflags;
  if (dirty & SKU_STAMP_TRIGGER) {
    es.x = (uint32_t)now; es.y = (uint32_t)(now >> 32); es.z = 0; es.w = 0;
    f |= SKR_ENV_ACTIVE;
  }
  if ((dirty & SKU_STAMP_RELEASE) && (f & SKR_ENV_ACTIVE)) {
    es.z = (uint32_t)now; es.w = (uint32_t)(now >> 32);
  }
  *reinterpret_cast<uint4 *>(&p.ro[SKP_ENV_S][v]) = es;
  *rwflags = f;
}

// THE LIST RULE.  Entry i of a list in device memory is looked at when it lies below min(n, *d_count) (d_count NULL: n) ...
__device__ __forceinline__ bool sk_list_looked(int64_t i, int n, const uint32_t *d_count) {
  return i < n && !(d_count && (uint64_t)i >= (uint64_t)d_count[0]);
}

// ... and its value e names a slot of the bank when it is the first voice of one (the -1 of a dropped note is none)
__device__ __forceinline__ bool sk_slot_valid(int e, int slot_voices, int n_voices) {
  return e >= 0 && (e & (slot_voices - 1)) == 0 && e <= n_voices - slot_voices;
}

// K = 1 << k_shift threads per entry, span >> k_shift entries per workgroup: this thread's entry i, and l, the voice of the slot it
// serves (voice e + l).  d_slots[i] is loaded when the entry is looked at, and nothing else is; e is 0 where it was not.
struct sk_entry_t {
  int64_t i;
  int l, e;
  bool looked, valid;
};
__device__ __forceinline__ sk_entry_t sk_entry_decode(int span, int k_shift, const int32_t *d_slots, int n, const uint32_t *d_count,
                                                      int n_voices) {
  sk_entry_t t;
  const int K = 1 << k_shift;
  t.i = (int64_t)blockIdx.x * (span >> k_shift) + ((int)threadIdx.x >> k_shift);
  t.l = (int)threadIdx.x & (K - 1);
  t.looked = sk_list_looked(t.i, n, d_count);
  t.e = 0;
  t.valid = false;
  if (t.looked) {
    t.e = d_slots[t.i];
    t.valid = sk_slot_valid(t.e, K, n_voices);
  }
  return t;
}

// the note-owner guard: the slot's owner word is the entry's tag.  Tags are non-zero, so an untagged slot never matches
__device__ __forceinline__ bool sk_entry_owned(const uint32_t *__restrict__ owner, const uint32_t *__restrict__ tags, const sk_entry_t &t) {
  return t.valid && owner[t.e] == tags[t.i];
}

// One thread per voice of [first, first + count), whole slots of K voices (first is a multiple of K), SK_CONTROL_SPAN voices per
// workgroup: this thread's voice v (`first` beyond the range, so that v - l can always be read), its place l in its slot, and head:
// the one thread per slot that counts it
struct sk_lane_t {
  int v, l;
  bool in_range, head;
};
__device__ __forceinline__ sk_lane_t sk_range_lane(int first, int count, int K) {
  sk_lane_t t;
  const int64_t off = (int64_t)blockIdx.x * SK_CONTROL_SPAN + threadIdx.x;
  t.in_range = off < count;
  t.v = first + (int)(t.in_range ? off : 0);
  t.l = t.v & (K - 1);
  t.head = t.in_range && t.l == 0;
  return t;
}

// d_result[k] += the workgroup's number of threads with flag k set, k < N (every thread arrives: __syncthreads inside).  Integer
// sums: the same whatever the order of arrival (skred_owner_kernels.hip, skred_expr_kernels.hip)
template <int N>
__device__ __forceinline__ void sk_owner_count(uint32_t *sums, uint32_t *d_result, const bool (&flag)[N]) {
  const int tid = threadIdx.x;
  if (tid < N) sums[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const uint32_t c = (uint32_t)__popcll(__ballot(flag[k]));
    if ((tid & 63) == 0 && c) atomicAdd(&sums[k], c);
  }
  __syncthreads();
  if (d_result && tid < N && sums[tid]) atomicAdd(d_result + tid, sums[tid]);
}

// The batch was read (straight from the host's pinned staging buffer, for small batches): the workgroup that finishes last tells
// the host, which then reuses the buffer -- a word in pinned memory the host polls, instead of an event behind every batch
// (an event record costs the stream ~5 us of gap in front of the next kernel: four per block under note traffic).
__device__ __forceinline__ void sk_batch_done(uint32_t *cnt, uint32_t *done, uint32_t seq) {
  if (!done) return;
  __syncthreads();                                   // every thread of this workgroup holds its record in registers
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(cnt, 1u) == gridDim.x - 1) {
      __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the slot's next batch ...
      __threadfence_system();                                                   // ... before the host can know the slot is free
      __hip_atomic_store(done, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ---- (host) what the launchers of these units share ----

static inline void sk_planes(sk_plane_ptrs_t &p, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT]) {
  for (int k = 0; k < SKP_COUNT; ++k) p.ro[k] = ro[k];
  for (int k = 0; k < SKS_COUNT; ++k) p.rw[k] = rw[k];
}

// log2 of slot_voices (a power of two: checked by the callers)
static inline int sk_slot_shift(int slot_voices) {
  int sh = 0;
  while ((1 << sh) < slot_voices) ++sh;
  return sh;
}

// workgroups of SK_CONTROL_SPAN threads: one thread per lane; one thread per entry and voice of its slot (sk_entry_decode's geometry)
static inline unsigned sk_grid(long long lanes) { return (unsigned)((lanes + SK_CONTROL_SPAN - 1) / SK_CONTROL_SPAN); }
static inline unsigned sk_list_grid(int n, int shift) {
  const int per_wg = SK_CONTROL_SPAN >> shift;
  return (unsigned)(((long long)n + per_wg - 1) / per_wg);
}

// the result words a kernel adds onto, zeroed on `stream` ahead of it (d_result NULL: the caller wants none)
static inline hipError_t sk_result_clear(uint32_t *d_result, int words, hipStream_t stream) {
  return d_result ? hipMemsetAsync(d_result, 0, (size_t)words * sizeof(uint32_t), stream) : hipSuccess;
}

#endif
