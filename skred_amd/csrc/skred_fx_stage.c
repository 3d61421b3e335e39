/*
 * skred_fx_stage.c -- the one way a host-written batch reaches a kernel of the fixed-point bank: the staging ring and the batch path
 * on top of it (skx_batch_begin / _send / _end), which every control call that ships bytes goes through (skred_fx_live.c, _owner.c,
 * _ctl.c, _expr.c).  Shaped like the float bank's (skred_bank_stage.c); the ring's protocol is this bank's own
 * (skred_fxbank_priv.h: events, always the device twin behind a copy, no time limit).
 *
 *   begin   a slot of the ring with room for the batch, not in flight; the caller fills bt->h
 *   send    the copy into the slot's device twin, which is where every kernel of the batch reads the bytes
 *   end     the slot's event behind everything queued, whatever the launches said, then their verdict under `who`
 */
#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

/* the next slot, with room for `bytes`, not in flight */
static int skx_ring_take(skred_fxbank_t *fx, size_t bytes, skx_slot_t **out) {
  skx_slot_t *sl = &fx->ring[fx->ring_head++ % SKX_RING];
  if (!sl->ev) HIP_TRY(hipEventCreateWithFlags(&sl->ev, hipEventDisableTiming));
  if (sl->in_flight) {
    HIP_TRY(hipEventSynchronize(sl->ev));      /* this slot's batch alone: not the stream, not the device */
    sl->in_flight = 0;
  }
  if (bytes > sl->cap) {
    if (sl->d) { (void)hipFree(sl->d); sl->d = NULL; }
    if (sl->h) { (void)hipHostFree(sl->h); sl->h = NULL; }
    sl->cap = 0;
    size_t cap = 64 * 1024;
    while (cap < bytes) cap *= 2;
    HIP_TRY(hipMalloc(&sl->d, cap));
    HIP_TRY(hipHostMalloc(&sl->h, cap, hipHostMallocDefault));
    sl->cap = cap;
  }
  *out = sl;
  return SKRED_OK;
}

/* the slot's pinned bytes -> its device twin, on `s` */
static int skx_ring_send(skx_slot_t *sl, size_t bytes, hipStream_t s) {
  HIP_TRY(hipMemcpyAsync(sl->d, sl->h, bytes, hipMemcpyHostToDevice, s));
  return SKRED_OK;
}

/* behind the copy and the kernels that read the twin.  A failure to record leaves nothing to wait for later: wait now. */
static int skx_ring_guard(skx_slot_t *sl, hipStream_t s) {
  if (hipEventRecord(sl->ev, s) != hipSuccess) {
    (void)hipStreamSynchronize(s);
    return fail(SKRED_E_NO_DEVICE, "fx staging: hipEventRecord failed");
  }
  sl->in_flight = 1;
  return SKRED_OK;
}

int skx_batch_begin(skred_fxbank_t *fx, size_t bytes, skx_batch_t *bt) {
  const int rc = skx_ring_take(fx, bytes, &bt->sl);
  if (rc) return rc;
  bt->h = bt->sl->h;
  return SKRED_OK;
}

const void *skx_batch_send(skx_batch_t *bt, size_t bytes, hipStream_t s) {
  return skx_ring_send(bt->sl, bytes, s) ? NULL : bt->sl->d;
}

/* `e`: the first launch of the batch that failed, or hipSuccess.  The event is recorded either way: the copy, and the launches
 * queued before the failing one, still read the slot */
int skx_batch_end(skx_batch_t *bt, hipError_t e, const char *who, hipStream_t s) {
  const int rc = skx_ring_guard(bt->sl, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "%s launch -> %s", who, hipGetErrorString(e));
  return rc;
}
