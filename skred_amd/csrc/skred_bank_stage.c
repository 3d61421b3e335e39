/*
 * skred_bank_stage.c -- the one way a host-written batch reaches a kernel of the float bank: the staging ring (sk_staging_slot,
 * sk_stage) and the batch path on top of it (sk_batch_begin / _send / _end), which every control call that ships bytes goes through
 * (skred_bank_update.c, _notes.c, _slots.c, _ctl.c, _owner.c, _expr.c).
 *
 *   begin   a slot of the ring with room for the batch; the caller fills bt->h
 *   send    where the kernel reads the bytes from, and the batch's number: the launcher gets bt->cnt, bt->done, bt->seq
 *   end     takes the launch's verdict: the slot is the batch's until its kernel has run; after a failed launch the stream is
 *           waited for, because a copy into the slot's device twin, or an earlier launch of the batch, may still read the slot
 *
 * Also the read-back ending of the _host queries (sk_read_back), the room of the grow-on-demand answer buffers (sk_answer_room) and
 * the per-voice side arrays' allocation, clear and download (sk_side_alloc / _clear / _download).
 * The fixed-point bank guards its ring with events instead (skred_fxbank_priv.h says why); nothing here serves it but those five, which
 * take plain pointers.  Its own ring and batch path, shaped like this one: skred_fx_stage.c.
 */
#include <sched.h>
#include <string.h>
#include <time.h>

#include "skred_bank_priv.h"

/* One staging slot of the ring: pinned host buffer, device buffer, and the number of the batch after which both may be
 * reused -- the batch's last kernel stores it into pinned memory (sk_batch_done), the host looks there.  With a ring the
 * host only ever waits for a batch issued SK_UPD_RING batches ago (a host that queues blocks far ahead of the device is
 * held back here, as an event would hold it); a single slot would stall every update behind the render that precedes it in
 * the stream. */
int sk_staging_slot(skred_bank_t *b, size_t bytes, hipStream_t s, sk_upd_slot_t **out) {
  const int idx = (int)(b->upd_head++ % SK_UPD_RING);
  sk_upd_slot_t *sl = &b->upd[idx];
  if (!b->h_upd_done) {
    HIP_TRY(hipHostMalloc((void **)&b->h_upd_done, SK_UPD_RING * sizeof(uint32_t), hipHostMallocCoherent));   /* (the host polls words the device stores while kernels run) */
    for (int i = 0; i < SK_UPD_RING; i++) b->h_upd_done[i] = 0;
    HIP_TRY(hipMalloc((void **)&b->d_upd_cnt, SK_UPD_RING * sizeof(uint32_t)));
    HIP_TRY(hipMemset(b->d_upd_cnt, 0, SK_UPD_RING * sizeof(uint32_t)));
  }
  if (sl->seq) {
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (unsigned spins = 0; __atomic_load_n(&b->h_upd_done[idx], __ATOMIC_ACQUIRE) != sl->seq; spins++) {
      if ((spins & 63) == 63) {
        sched_yield();
        clock_gettime(CLOCK_MONOTONIC, &t1);
        /* Five seconds without the batch's kernel having run: its stream is blocked -- e.g. behind an event the caller means to record
         * only after this call returns.  Waiting for the device here would turn that into a deadlock, so the call fails instead; the
         * slot stays marked in flight (its buffers are still the batch's), and the ring moves on to the next slot. */
        if (t1.tv_sec - t0.tv_sec > 5)
          return fail(SKRED_E_NO_DEVICE, "update: staging slot %d is still in flight after 5 s (batch %u of a stream that has not run): "
                                         "the bank is %d update batches ahead of the device", idx, sl->seq, SK_UPD_RING);
      }
    }
    sl->seq = 0;
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
  (void)s;
  *out = sl;
  return SKRED_OK;
}

/* Where the scatter kernel reads a staged batch from.  A small batch -- the notes of one audio block -- is read straight out
 * of the pinned host buffer (it is mapped into the device's address space): a copy engine transfer in front of a 5 us kernel
 * cost the stream ~12 us each (the copy and the gap behind it), four times per block under note traffic.  A large batch goes
 * through the copy engine into the slot's device twin: bandwidth matters there, not latency. */
#define SK_UPD_ZERO_COPY_MAX (256 * 1024)
const void *sk_stage(sk_upd_slot_t *sl, size_t bytes, hipStream_t s) {
  if (bytes <= SK_UPD_ZERO_COPY_MAX) return sl->h;
  const hipError_t e = hipMemcpyAsync(sl->d, sl->h, bytes, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) { (void)fail(SKRED_E_NO_DEVICE, "update copy -> %s", hipGetErrorString(e)); return NULL; }
  return sl->d;
}

int sk_batch_begin(skred_bank_t *b, size_t bytes, hipStream_t s, sk_batch_t *bt) {
  const int rc = sk_staging_slot(b, bytes, s, &bt->sl);
  if (rc) return rc;
  bt->h = bt->sl->h;
  return SKRED_OK;
}

/* `wide`: the caller knows that many workgroups will each read every byte -- a few KB of records in front of a bank-wide range.
 * Over the bus that cost the stream 0.3 ms at 2^20 voices; such a launch reads the slot's device twin behind one small copy,
 * whatever sk_stage's own rule (made for few readers of many bytes) says.  Returns NULL when the copy failed (the error is set) */
const void *sk_batch_send(skred_bank_t *b, sk_batch_t *bt, size_t bytes, int wide, hipStream_t s) {
  const void *src = bt->sl->d;
  if (!wide) src = sk_stage(bt->sl, bytes, s);
  else {
    const hipError_t e = hipMemcpyAsync(bt->sl->d, bt->sl->h, bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { (void)fail(SKRED_E_NO_DEVICE, "staged copy -> %s", hipGetErrorString(e)); return NULL; }
  }
  const int idx = (int)(bt->sl - b->upd);
  if (++b->upd_seq == 0) b->upd_seq = 1;               /* (0 means "not in flight") */
  bt->cnt = b->d_upd_cnt + idx;
  bt->done = (uint32_t *)b->h_upd_done + idx;
  bt->seq = b->upd_seq;
  return src;
}

int sk_batch_end(sk_batch_t *bt, hipError_t e, const char *who, hipStream_t s) {
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);
    return fail(SKRED_E_NO_DEVICE, "%s launch -> %s", who, hipGetErrorString(e));
  }
  bt->sl->seq = bt->seq;
  return SKRED_OK;
}

/* Room for `need` entries behind `head` words in an answer buffer on the device and -- h_buf != NULL -- its pinned twin, all 32-bit
 * words: *cap entries, the next power of two >= need, from 1024.  The old buffers are freed first, and nothing reads them any more: a
 * _host query waited for its copy before it returned, and hipFree waits for the device (a list an earlier placement still reads).
 * *cap stays 0 when an allocation fails */
int sk_answer_room(void **d_buf, void **h_buf, size_t *cap, size_t head, size_t need) {
  if (*d_buf && need <= *cap) return SKRED_OK;
  if (*d_buf) { (void)hipFree(*d_buf); *d_buf = NULL; }
  if (h_buf && *h_buf) { (void)hipHostFree(*h_buf); *h_buf = NULL; }
  *cap = 0;
  size_t entries = 1024;
  while (entries < need) entries *= 2;
  HIP_TRY(hipMalloc(d_buf, (head + entries) * sizeof(uint32_t)));
  if (h_buf) HIP_TRY(hipHostMalloc(h_buf, (head + entries) * sizeof(uint32_t), hipHostMallocDefault));
  *cap = entries;
  return SKRED_OK;
}

/* The per-voice side arrays of both banks (note owners, pedals, glides: one element per voice, NULL until the first call that needs
 * them, freed with the bank), as plain pointers.  alloc: `bytes` on the current device, zeroed so that whatever stream the first
 * caller uses sees the zeros; fails under `what`.  clear: the checked window [first, +count) of `elem`-byte elements zeroed on `s` --
 * an array that was never allocated holds zeros already.  download: the same window to the host behind everything queued, zeros
 * where the array was never allocated.  `who` names the entry point in the window's error text */
int sk_side_alloc(void **d_arr, size_t bytes, const char *what) {
  void *p = NULL;
  HIP_TRY(hipMalloc((void **)&p, bytes));
  hipError_t e = hipMemset(p, 0, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { (void)hipFree(p); return fail(SKRED_E_NO_DEVICE, "%s -> %s", what, hipGetErrorString(e)); }
  *d_arr = p;
  return SKRED_OK;
}

int sk_side_clear(void *d_arr, size_t elem, int device, int n_voices, int first, int count, hipStream_t s, const char *who) {
  const int rc = sk_check_window(n_voices, first, count, who);
  if (rc) return rc;
  if (count == 0 || !d_arr) return SKRED_OK;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemsetAsync((char *)d_arr + (size_t)first * elem, 0, (size_t)count * elem, s));
  return SKRED_OK;
}

int sk_side_download(const void *d_arr, size_t elem, int device, int n_voices, void *host, int first, int count, const char *who) {
  const int rc = sk_check_window(n_voices, first, count, who);
  if (rc) return rc;
  if (count == 0) return SKRED_OK;
  if (!d_arr) { memset(host, 0, (size_t)count * elem); return SKRED_OK; }
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host, (const char *)d_arr + (size_t)first * elem, (size_t)count * elem, hipMemcpyDeviceToHost));
  return SKRED_OK;
}

/* What a _host query ends in: the device's `counts` report words (2; a matched victim query's 3) and max_out entries behind them ->
 * the pinned twin, the stream waited for, the entries handed to the caller.  `bound`: the most report word 0 can honestly say --
 * max_out where it counts the entries written, the slots of the range where it is a total (skred_bank_find_match_host).  Returns the
 * entries copied to `out`, or an error */
int sk_read_back(const int32_t *d_out, int32_t *h_out, int counts, int max_out, int bound, int32_t *out, hipStream_t s, const char *who) {
  HIP_TRY(hipMemcpyAsync(h_out, d_out, ((size_t)counts + (size_t)max_out) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h_out[0] < 0 || h_out[0] > bound) return fail(SKRED_E_NO_DEVICE, "%s: the device reported %d of at most %d", who, h_out[0], bound);
  const int written = h_out[0] < max_out ? h_out[0] : max_out;
  if (written > 0) memcpy(out, h_out + counts, (size_t)written * sizeof(int32_t));
  return written;
}
