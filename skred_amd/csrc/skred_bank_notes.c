/*
 * skred_bank_notes.c -- note-ons and stamps on voices that a list in device memory names (include/skred_amd.h:
 * skred_notes_check, skred_bank_notes_on_list / _note_on_idle / _note_on_steal / _stamp_list).
 *
 * The host side of skred_note_kernels.hip: the checks (made before anything touches the device), the notes' way through the
 * batch path (skred_bank_stage.c), the launches, and the list skred_bank_note_on_idle's query leaves for its placement.
 * Nothing here waits for the device, and nothing here learns which voice took which note: the host's shadow of the bank
 * (h_class, the counters, the lane words) does not depend on what a note stores -- see the header -- so it stays as it is;
 * what the calls do tell the bank is what every control action tells it: `n` more voices may be on the motion list
 * (touched_total, an upper bound whether or not every note is placed), and earlier launches' reports are out of date.
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(sizeof(skred_note_t) == sizeof(sk_note_t) && sizeof(skred_note_t) == 32 &&
               offsetof(skred_note_t, phase_inc) == 4 * SK_NOTE_PHASE_INC && offsetof(skred_note_t, velocity) == 4 * SK_NOTE_VELOCITY &&
               offsetof(skred_note_t, phase) == 4 * SK_NOTE_PHASE && offsetof(skred_note_t, pan_left) == 4 * SK_NOTE_PAN_LEFT &&
               offsetof(skred_note_t, pan_right) == 4 * SK_NOTE_PAN_RIGHT && offsetof(skred_note_t, flags) == 4 * SK_NOTE_FLAGS,
               "the device's note record must be skred_note_t word for word");
_Static_assert(SK_NOTE_SET_PHASE == SKRED_NOTE_SET_PHASE && SK_NOTE_SET_PAN == SKRED_NOTE_SET_PAN,
               "device note flags must equal the public SKRED_NOTE_* values");

void sk_notes_free(skred_bank_t *b) {
  if (b->d_note_list) hipFree(b->d_note_list);
  b->d_note_list = NULL;
  b->note_list_cap = 0;
}

/* one record (`k`: its number in the error text) */
int sk_note_check_one(const skred_note_t *t, int k) {
  if (t->flags & ~(uint32_t)(SKRED_NOTE_SET_PHASE | SKRED_NOTE_SET_PAN)) return fail(SKRED_E_BAD_ARG, "note %d: unknown bits in flags = 0x%x", k, t->flags);
  if (t->reserved[0] || t->reserved[1]) return fail(SKRED_E_BAD_ARG, "note %d: reserved words must be 0", k);
  /* a non-finite increment or phase would change the voice's class (sk_pack_voice: SKC_EXOTIC) behind the host's back */
  if (!isfinite(t->phase_inc)) return fail(SKRED_E_BAD_ARG, "note %d: phase_inc %g", k, (double)t->phase_inc);
  if (!isfinite(t->velocity)) return fail(SKRED_E_BAD_ARG, "note %d: velocity %g", k, (double)t->velocity);
  if ((t->flags & SKRED_NOTE_SET_PHASE) && !isfinite(t->phase)) return fail(SKRED_E_BAD_ARG, "note %d: phase %g", k, (double)t->phase);
  if ((t->flags & SKRED_NOTE_SET_PAN) && (!isfinite(t->pan_left) || !isfinite(t->pan_right)))
    return fail(SKRED_E_BAD_ARG, "note %d: pan (%g, %g)", k, (double)t->pan_left, (double)t->pan_right);
  return SKRED_OK;
}

int skred_notes_check(const skred_note_t *notes, int n) {
  if (!notes || n < 0) return fail(SKRED_E_BAD_ARG, "notes: no notes or n = %d", n);
  for (int k = 0; k < n; k++) {
    const int rc = sk_note_check_one(&notes[k], k);
    if (rc) return rc;
  }
  return SKRED_OK;
}

/* the checked notes -> a staging slot -> the placement kernel */
static int notes_launch(skred_bank_t *b, const skred_note_t *notes, int n, const int32_t *d_voices, const uint32_t *d_count,
                        int first_entry, int32_t *d_assigned, uint32_t *d_result, hipStream_t s) {
  HIP_TRY(hipSetDevice(b->device));
  const size_t bytes = (size_t)n * sizeof(skred_note_t);
  sk_batch_t bt;
  int rc = sk_batch_begin(b, bytes, s, &bt);
  if (rc) return rc;
  memcpy(bt.h, notes, bytes);
  const sk_note_t *src = (const sk_note_t *)sk_batch_send(b, &bt, bytes, 0, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)sk_launch_notes(src, n, d_voices, d_count, first_entry, b->n_voices, b->d_ro, b->d_rw,
                                                   b->g.synth_sample_count, b->d_mask[b->mask_p], d_assigned, d_result,
                                                   bt.cnt, bt.done, bt.seq, s);
  if ((rc = sk_batch_end(&bt, e, "notes", s))) return rc;
  sk_touched(b, (uint64_t)n);
  return SKRED_OK;
}

int skred_bank_notes_on_list(skred_bank_t *b, const skred_note_t *notes, int n, const int32_t *d_voices, const uint32_t *d_count,
                             int first_entry, int32_t *d_assigned, uint32_t *d_result, void *stream) {
  if (!b || !notes || !d_voices || !d_count || !d_result) return fail(SKRED_E_BAD_ARG, "notes_on_list: no bank, notes, list, count or result");
  if (n < 0 || first_entry < 0) return fail(SKRED_E_BAD_ARG, "notes_on_list: n = %d, first_entry = %d", n, first_entry);
  if (n == 0) return SKRED_OK;
  const int rc = skred_notes_check(notes, n);
  if (rc) return rc;
  return notes_launch(b, notes, n, d_voices, d_count, first_entry, d_assigned, d_result, (hipStream_t)stream);
}

/* room for n entries in the bank's own list (skred_bank_slots.c: the slot list of skred_bank_note_on_idle_slots) */
int sk_note_list_room(skred_bank_t *b, int n) {
  return sk_answer_room((void **)&b->d_note_list, NULL, &b->note_list_cap, SK_NOTE_LIST_WORDS, (size_t)n);
}

int skred_bank_note_on_idle(skred_bank_t *b, const skred_idle_query_t *q, const skred_note_t *notes, int n, int32_t *d_assigned,
                            uint32_t *d_result, void *stream) {
  if (!b || !q || !notes || !d_result) return fail(SKRED_E_BAD_ARG, "note_on_idle: no bank, query, notes or result");
  if (n < 0) return fail(SKRED_E_BAD_ARG, "note_on_idle: n = %d", n);
  if (q->which & SKRED_IDLE_AMP_ZERO)
    return fail(SKRED_E_BAD_ARG, "note_on_idle: SKRED_IDLE_AMP_ZERO -- a note-on leaves voice_amp alone: the voice would stay silent and be listed again");
  skred_idle_query_t qq = *q;
  qq.max_out = n;
  int rc = sk_idle_check(b, &qq, b, b, "note_on_idle");   /* (the list and the counts go into the bank's own scratch) */
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  if ((rc = skred_notes_check(notes, n))) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_note_list_room(b, n))) return rc;
  uint32_t *d_count = b->d_note_list;
  int32_t *d_list = (int32_t *)(b->d_note_list + SK_NOTE_LIST_WORDS);
  if ((rc = skred_bank_find_idle(b, &qq, d_list, d_count, stream))) return rc;
  return notes_launch(b, notes, n, d_list, d_count, 0, d_assigned, d_result, s);
}

int skred_bank_note_on_steal(skred_bank_t *b, const skred_idle_query_t *idle_q, const skred_steal_query_t *steal_q,
                             const skred_note_t *notes, int n, int32_t *d_assigned, uint32_t *d_result, void *stream) {
  if (!b || !idle_q || !steal_q || !notes || !d_result) return fail(SKRED_E_BAD_ARG, "note_on_steal: no bank, query, notes or result");
  if (n < 0) return fail(SKRED_E_BAD_ARG, "note_on_steal: n = %d", n);
  if (idle_q->which & SKRED_IDLE_AMP_ZERO)
    return fail(SKRED_E_BAD_ARG, "note_on_steal: SKRED_IDLE_AMP_ZERO -- a note-on leaves voice_amp alone: the voice would stay silent and be listed again");
  skred_idle_query_t iq = *idle_q;
  iq.max_out = n;
  skred_steal_query_t sq = *steal_q;
  sq.exclude_idle = idle_q->which;
  sq.settle_level = idle_q->settle_level;
  sq.max_out = n < SKRED_STEAL_MAX ? n : SKRED_STEAL_MAX;
  int rc = sk_idle_check(b, &iq, b, b, "note_on_steal");   /* (the lists and the counts go into the bank's own scratch) */
  if (rc) return rc;
  if ((rc = sk_steal_check_bank(b, &sq, b, b, "note_on_steal"))) return rc;
  if (n == 0) return SKRED_OK;
  if ((rc = skred_notes_check(notes, n))) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_note_list_room(b, n))) return rc;
  uint32_t *d_idle_count = b->d_note_list, *d_joined = b->d_note_list + 2;
  int32_t *d_list = (int32_t *)(b->d_note_list + SK_NOTE_LIST_WORDS);
  if ((rc = skred_bank_find_idle(b, &iq, d_list, d_idle_count, stream))) return rc;
  if ((rc = sk_steal_into_scratch(b, &sq, s))) return rc;
  /* the victims behind the idle entries, as far as the batch reaches; d_result[2]: the notes that will land on them (every entry
   * of the joined list names a voice, and the list is no longer than the batch) */
  const hipError_t e = (hipError_t)sk_launch_list_append(d_list, d_idle_count, b->d_steal_out + 2, (const uint32_t *)b->d_steal_out, n,
                                                         d_joined, d_result + 2, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "list append launch -> %s", hipGetErrorString(e));
  return notes_launch(b, notes, n, d_list, d_joined, 0, d_assigned, d_result, s);
}

int skred_bank_stamp_list(skred_bank_t *b, const int32_t *d_voices, int n, const uint32_t *d_count_or_null, uint32_t stamps,
                          void *stream) {
  if (!b || !d_voices || n < 0) return fail(SKRED_E_BAD_ARG, "stamp_list: no bank, no list or n = %d", n);
  const int rc = sk_check_stamps(stamps, "stamp_list");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  const hipError_t e = (hipError_t)sk_launch_stamp_list(d_voices, n, d_count_or_null, b->n_voices, stamps, b->d_ro, b->d_rw,
                                                        b->g.synth_sample_count, b->d_mask[b->mask_p], (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "stamp_list launch -> %s", hipGetErrorString(e));
  sk_touched(b, (uint64_t)n);
  return SKRED_OK;
}
