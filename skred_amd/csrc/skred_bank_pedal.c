/*
 * skred_bank_pedal.c -- pedals: note-offs the sustain and sostenuto pedals hold back, remembered per slot on the device
 * (include/skred_amd.h: skred_pedal_check, skred_bank_stamp_owned_pedal / _release_tags_pedal / _pedal_latch / _pedal_up /
 * _pedal_clear / _download_pedals).
 *
 * The host side of skred_pedal_kernels.hip, on the pieces of skred_bank_checks.c and skred_bank_stage.c and on the owner array and
 * find pass of skred_bank_owner.c: the checks (made before anything touches the device), the tags' way through the batch path, the
 * launches.  Nothing here waits for the device except the download and the allocation of the array by the first call that needs
 * it.  The pedal array is no part of the bank the planner knows: no class, counter, lane word or report depends on it.  What the
 * stamping calls tell the bank is what their twins without a pedal tell it -- n * popcount(mask) more voices may be on the motion
 * list for the list calls, (count / K) * popcount(mask) for the pedal-up (upper bounds: a held note-off only takes voices away);
 * the latch stores no plane word and tells it nothing.  The hook that clears a re-tagged slot's word is in skred_bank_owner.c
 * (sk_owner_tag_launch).
 *
 * Out of scope: the fixed-point bank, the drop-in mode, deferred items and pattern steps.
 */
#include <stddef.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(SK_PEDAL_PENDING == SKRED_PEDAL_PENDING && SK_PEDAL_LATCHED == SKRED_PEDAL_LATCHED, "the pedal bits travel as they are");
_Static_assert(SK_PEDAL_LIFT_SUSTAIN == SKRED_PEDAL_LIFT_SUSTAIN && SK_PEDAL_LIFT_SOSTENUTO == SKRED_PEDAL_LIFT_SOSTENUTO &&
               SK_PEDAL_SUSTAIN_DOWN == SKRED_PEDAL_SUSTAIN_DOWN, "the pedal-up flags travel as they are");

#define SK_PEDAL_LIFTS (SKRED_PEDAL_LIFT_SUSTAIN | SKRED_PEDAL_LIFT_SOSTENUTO)
#define SK_PEDAL_FLAGS (SK_PEDAL_LIFTS | SKRED_PEDAL_SUSTAIN_DOWN)

static int pedal_check(int call, int n_voices, int first, int count, int K, uint64_t voice_mask, const skred_owner_match_t *m, uint32_t flags,
                       const uint32_t *tags, int n, const char *who) {
  int rc;
  switch (call) {
  case SKRED_PEDAL_CALL_STAMP_OWNED:                     /* skred_bank_stamp_owned's order */
    if ((rc = skred_owner_tags_check(tags, n, 0))) return rc;
    if ((rc = sk_check_list_n(n, who))) return rc;
    return sk_check_slot_shape(K, voice_mask, "voice_mask", who);
  case SKRED_PEDAL_CALL_RELEASE_TAGS:                    /* skred_bank_release_tags' */
    if ((rc = skred_owner_tags_check(tags, n, SKRED_OWNER_UNIQUE))) return rc;
    if ((rc = sk_check_slot_shape(K, 0, NULL, who))) return rc;
    if ((rc = sk_check_slot_range(n_voices, first, count, K, 0, who))) return rc;
    return sk_check_slot_shape(K, voice_mask, "voice_mask", who);
  case SKRED_PEDAL_CALL_LATCH:
  case SKRED_PEDAL_CALL_UP:                              /* skred_bank_stamp_match's, the flags where its stamp bits stand */
    if ((rc = skred_owner_match_check(m))) return rc;
    if (call == SKRED_PEDAL_CALL_UP) {
      if (flags & ~(uint32_t)SK_PEDAL_FLAGS) return fail(SKRED_E_BAD_ARG, "%s: unknown bits in flags = 0x%x", who, flags);
      if (!(flags & SK_PEDAL_LIFTS)) return fail(SKRED_E_BAD_ARG, "%s: flags = 0x%x lift no pedal", who, flags);
      if ((flags & SKRED_PEDAL_SUSTAIN_DOWN) && (flags & SKRED_PEDAL_LIFT_SUSTAIN))
        return fail(SKRED_E_BAD_ARG, "%s: flags = 0x%x lift the sustain pedal and say it stays down", who, flags);
    }
    if ((rc = sk_check_slot_shape(K, voice_mask, "voice_mask", who))) return rc;
    return sk_check_slot_range(n_voices, first, count, K, 0, who);
  default:
    return fail(SKRED_E_BAD_ARG, "%s: call = %d", who, call);
  }
}

int skred_pedal_check(int call, int n_voices, int first, int count, int slot_voices, uint64_t voice_mask, const skred_owner_match_t *m,
                      uint32_t flags, const uint32_t *tags, int n) {
  return pedal_check(call, n_voices, first, count, slot_voices, voice_mask, m, flags, tags, n, "pedal_check");
}

/* the array behind the owner array, allocated and zeroed by the first call that needs it (the owner array first, when no owner call
 * came before) */
static int pedal_ensure(skred_bank_t *b) {
  if (b->d_pedal) return SKRED_OK;
  const int rc = sk_owner_ensure(b);
  if (rc) return rc;
  return sk_side_alloc((void **)&b->d_pedal, (size_t)b->n_voices * sizeof(uint32_t), "pedal array");
}

void sk_pedal_free(skred_bank_t *b) {
  if (b->d_pedal) (void)hipFree(b->d_pedal);
  b->d_pedal = NULL;
}

/* the held-back or stamped note-offs of n checked tags on a list in device memory */
static int stamps_launch(skred_bank_t *b, const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count, int slot_voices,
                         uint64_t voice_mask, int hold_all, uint32_t *d_result, const char *who, hipStream_t s) {
  const size_t bytes = (size_t)n * sizeof(uint32_t);
  sk_batch_t bt;
  int rc = sk_batch_begin(b, bytes, s, &bt);
  if (rc) return rc;
  memcpy(bt.h, tags, bytes);
  const uint32_t *src = (const uint32_t *)sk_batch_send(b, &bt, bytes, 0, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)sk_launch_pedal_stamps(b->d_owner, b->d_pedal, d_slots, src, n, d_count, slot_voices, voice_mask, b->n_voices,
                                                          hold_all, b->d_ro, b->d_rw, b->g.synth_sample_count, b->d_mask[b->mask_p], d_result,
                                                          bt.cnt, bt.done, bt.seq, s);
  if ((rc = sk_batch_end(&bt, e, who, s))) return rc;
  sk_touched(b, (uint64_t)n * (uint64_t)__builtin_popcountll(voice_mask));
  return SKRED_OK;
}

int skred_bank_stamp_owned_pedal(skred_bank_t *b, const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                                 int slot_voices, uint64_t voice_mask, int hold_all, uint32_t *d_result, void *stream) {
  if (!b || !d_slots || !d_result) return fail(SKRED_E_BAD_ARG, "stamp_owned_pedal: no bank, list or result");
  int rc = pedal_check(SKRED_PEDAL_CALL_STAMP_OWNED, b->n_voices, 0, 0, slot_voices, voice_mask, NULL, 0, tags, n, "stamp_owned_pedal");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = pedal_ensure(b))) return rc;
  return stamps_launch(b, d_slots, tags, n, d_count_or_null, slot_voices, voice_mask, hold_all, d_result, "stamp_owned_pedal", (hipStream_t)stream);
}

int skred_bank_release_tags_pedal(skred_bank_t *b, int first, int count, int slot_voices, uint64_t voice_mask, const uint32_t *tags, int n,
                                  int hold_all, uint32_t *d_result, void *stream) {
  if (!b || !d_result) return fail(SKRED_E_BAD_ARG, "release_tags_pedal: no bank or no result");
  int rc = pedal_check(SKRED_PEDAL_CALL_RELEASE_TAGS, b->n_voices, first, count, slot_voices, voice_mask, NULL, 0, tags, n, "release_tags_pedal");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = pedal_ensure(b))) return rc;
  if ((rc = sk_owner_find_launch(b, first, count, slot_voices, tags, n, b->d_owner_slots, s))) return rc;
  /* entry k is the lowest slot that carries tags[k], or -1: the guard holds on every entry that is a slot */
  return stamps_launch(b, b->d_owner_slots, tags, n, NULL, slot_voices, voice_mask, hold_all, d_result, "release_tags_pedal", s);
}

int skred_bank_pedal_latch(skred_bank_t *b, int first, int count, int slot_voices, uint64_t voice_mask, const skred_owner_match_t *m,
                           uint32_t *d_result, void *stream) {
  if (!b || !d_result) return fail(SKRED_E_BAD_ARG, "pedal_latch: no bank or no result");
  int rc = pedal_check(SKRED_PEDAL_CALL_LATCH, b->n_voices, first, count, slot_voices, voice_mask, m, 0, NULL, 0, "pedal_latch");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = pedal_ensure(b))) return rc;
  const hipError_t e = (hipError_t)sk_launch_pedal_latch(b->d_owner, b->d_pedal, m->value, m->mask, first, count, slot_voices, voice_mask, b->d_ro,
                                                         b->d_rw, d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "pedal_latch launch -> %s", hipGetErrorString(e));
  return SKRED_OK;                                       /* (no plane word was stored: the planner's reports stand) */
}

int skred_bank_pedal_up(skred_bank_t *b, int first, int count, int slot_voices, uint64_t voice_mask, const skred_owner_match_t *m,
                        uint32_t flags, uint32_t *d_result, void *stream) {
  if (!b || !d_result) return fail(SKRED_E_BAD_ARG, "pedal_up: no bank or no result");
  int rc = pedal_check(SKRED_PEDAL_CALL_UP, b->n_voices, first, count, slot_voices, voice_mask, m, flags, NULL, 0, "pedal_up");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = pedal_ensure(b))) return rc;
  const hipError_t e = (hipError_t)sk_launch_pedal_up(b->d_owner, b->d_pedal, m->value, m->mask, first, count, slot_voices, voice_mask, flags,
                                                      b->d_ro, b->d_rw, b->g.synth_sample_count, b->d_mask[b->mask_p], d_result,
                                                      (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "pedal_up launch -> %s", hipGetErrorString(e));
  /* every slot of the range may be released: what skred_bank_stamp_match on the same range adds */
  sk_touched(b, (uint64_t)(count / slot_voices) * (uint64_t)__builtin_popcountll(voice_mask));
  return SKRED_OK;
}

int skred_bank_pedal_clear(skred_bank_t *b, int first, int count, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "pedal_clear: no bank");
  return sk_side_clear(b->d_pedal, sizeof(uint32_t), b->device, b->n_voices, first, count, (hipStream_t)stream, "pedal_clear");
}

int skred_bank_download_pedals(skred_bank_t *b, uint32_t *host_u32, int first, int count) {
  if (!b || !host_u32 || count < 0) return fail(SKRED_E_BAD_ARG, "download_pedals: bad arguments");
  return sk_side_download(b->d_pedal, sizeof(uint32_t), b->device, b->n_voices, host_u32, first, count, "download_pedals");
}
