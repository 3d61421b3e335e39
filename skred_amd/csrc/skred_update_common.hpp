// skred_update_common.hpp -- what the kernels that apply control actions share (skred_update_kernels.hip: updates and stamps
// named by the host; skred_note_kernels.hip: note-ons and stamps on voices named by a list in device memory).
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
