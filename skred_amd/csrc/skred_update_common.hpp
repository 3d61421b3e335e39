// skred_update_common.hpp -- what the kernels that apply control actions share (skred_update_kernels.hip: updates and stamps
// named by the host; skred_note_kernels.hip: note-ons and stamps on voices named by a list in device memory; skred_slot_kernels.hip:
// the same on the voices of slots named by a list in device memory; skred_ctl_kernels.hip: patch controllers).
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

// entry e of a slot list names a slot of the bank (skred_slot_kernels.hip: notes and stamps; skred_ctl_kernels.hip: controllers)
__device__ __forceinline__ bool sk_slot_valid(int e, int slot_voices, int n_voices) {
  return e >= 0 && (e & (slot_voices - 1)) == 0 && e <= n_voices - slot_voices;
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

#endif
