/*
 * skred_bank_slots.c -- patch notes: idle slots, and note-ons and stamps on the voices of listed slots (include/skred_amd.h:
 * skred_slot_query_check, skred_slot_notes_check, skred_bank_find_idle_slots / _find_idle_slots_host / _notes_on_slots /
 * _note_on_idle_slots / _stamp_slots), and slot stealing (skred_slot_steal_check, skred_bank_find_steal_slots / _find_steal_slots_host /
 * _note_on_steal_slots): the victim query of skred_bank_steal.c behind the key pass of skred_slot_steal_kernels.hip, and channel
 * polyphony (skred_chan_check, skred_bank_find_steal_slots_match / _find_steal_slots_match_host / _note_on_channel): the same query
 * restricted to one owner match, and the capped, tagged burst on top of it.  The fixed-point bank's twin is skred_fx_steal.c.
 *
 * The host side of skred_slot_kernels.hip, on the pieces of skred_bank_checks.c and skred_bank_stage.c: the checks (made before
 * anything touches the device), the bank's idle scratch, the notes' way through the batch path, the launches.  Nothing here waits for the device except the _host query, which waits for its stream.  What a call tells the bank is
 * what every control action tells it -- with n * popcount(voice_mask) voices, not n: that many more voices may be on the motion
 * list (touched_total, the bound behind the in-place rule), and earlier launches' reports are out of date.
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(sizeof(skred_slot_steal_query_t) == 56 && offsetof(skred_slot_steal_query_t, member_mask) == 16 &&
               offsetof(skred_slot_steal_query_t, flags) == 32 && offsetof(skred_slot_steal_query_t, reserved) == 48,
               "skred_slot_steal_query_t is 56 bytes (skred_amd/bank.py: SlotStealQueryC)");

#define SK_SLOT_CRITERIA (SKRED_IDLE_FINISHED | SKRED_IDLE_ENV_DONE | SKRED_IDLE_AMP_ZERO)

static int slot_query_check(const skred_slot_query_t *q, int n_voices, const char *who) {
  if (!q) return fail(SKRED_E_BAD_ARG, "%s: no query", who);
  if (q->max_out < 0) return fail(SKRED_E_BAD_ARG, "%s: max_out %d", who, q->max_out);
  if (q->which & SKRED_IDLE_UNNAMED) return fail(SKRED_E_BAD_ARG, "%s: SKRED_IDLE_UNNAMED -- the voices of a patch name one another by design", who);
  if (q->which & ~(uint32_t)SK_SLOT_CRITERIA) return fail(SKRED_E_BAD_ARG, "%s: unknown bits in which = 0x%x", who, q->which);
  if (!(q->which & SK_SLOT_CRITERIA)) return fail(SKRED_E_BAD_ARG, "%s: which = 0x%x selects no criterion", who, q->which);
  if (!(q->settle_level >= 0.0f) || isinf(q->settle_level)) return fail(SKRED_E_BAD_ARG, "%s: settle_level %g", who, (double)q->settle_level);
  int rc = sk_check_slot_shape(q->slot_voices, q->member_mask, "member_mask", who);
  if (rc) return rc;
  const int K = q->slot_voices;
  if ((rc = sk_check_slot_range(n_voices, q->first, q->count, K, 0, who))) return rc;
  if (q->from < q->first || q->from - q->first >= q->count)
    return fail(SKRED_E_RANGE, "%s: from = %d outside the range [%d,+%d)", who, q->from, q->first, q->count);
  if (q->from & (K - 1)) return fail(SKRED_E_RANGE, "%s: from = %d is not the first voice of a slot of %d voices", who, q->from, K);
  return SKRED_OK;
}

int skred_slot_query_check(const skred_slot_query_t *q, int n_voices) { return slot_query_check(q, n_voices, "slot_query_check"); }

static int slot_notes_check(const skred_note_t *notes, int n, int slot_voices, uint64_t voice_mask, const char *who) {
  if (!notes || n < 0) return fail(SKRED_E_BAD_ARG, "%s: no notes or n = %d", who, n);
  int rc = sk_check_slot_shape(slot_voices, voice_mask, "voice_mask", who);
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, who))) return rc;
  for (int k = 0; k < n; k++)
    for (int l = 0; l < slot_voices; l++) {
      if (!((voice_mask >> l) & 1)) continue;              /* a record no voice receives is not looked at */
      const int at = k * slot_voices + l, rc1 = sk_note_check_one(&notes[at], at);
      if (rc1) return rc1;
    }
  return SKRED_OK;
}

int skred_slot_notes_check(const skred_note_t *notes, int n, int slot_voices, uint64_t voice_mask) {
  return slot_notes_check(notes, n, slot_voices, voice_mask, "slot_notes_check");
}

static int slots_launch(skred_bank_t *b, const skred_slot_query_t *q, int32_t *d_slots, uint32_t *d_count, hipStream_t s) {
  HIP_TRY(hipSetDevice(b->device));
  const int rc = sk_idle_scratch(b, s);
  if (rc) return rc;
  sk_slot_args_t a;
  memset(&a, 0, sizeof(a));
  sk_idle_args(b, &a.idle, q->first, q->count, q->from, q->max_out, q->which, q->settle_level, d_slots, d_count);
  a.member_mask = q->member_mask;
  a.slot_voices = q->slot_voices;
  if (sk_idle_workgroups(q->first, q->count) > b->idle_wgs) return fail(SKRED_E_RANGE, "find_idle_slots: scratch too small");   /* (unreachable: sized for the bank) */
  const hipError_t e = (hipError_t)sk_launch_slots(&a, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "find_idle_slots launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

static int slots_check(const skred_bank_t *b, const skred_slot_query_t *q, const void *slots, const void *count, const char *who) {
  if (!b || !q) return fail(SKRED_E_BAD_ARG, "%s: no bank or no query", who);
  if (!count) return fail(SKRED_E_BAD_ARG, "%s: nowhere to put the counts", who);
  if (q->max_out > 0 && !slots) return fail(SKRED_E_BAD_ARG, "%s: max_out %d and no list to fill", who, q->max_out);
  return slot_query_check(q, b->n_voices, who);
}

int skred_bank_find_idle_slots(skred_bank_t *b, const skred_slot_query_t *q, int32_t *d_slots, uint32_t *d_count, void *stream) {
  const int rc = slots_check(b, q, d_slots, d_count, "find_idle_slots");
  if (rc) return rc;
  return slots_launch(b, q, d_slots, d_count, (hipStream_t)stream);
}

int skred_bank_find_idle_slots_host(skred_bank_t *b, const skred_slot_query_t *q, int32_t *slots, int *total_out, void *stream) {
  int dummy = 0;
  int rc = slots_check(b, q, slots, &dummy, "find_idle_slots_host");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_idle_out_room(b, (size_t)q->max_out))) return rc;
  rc = slots_launch(b, q, b->d_idle_out + 2, (uint32_t *)b->d_idle_out, s);
  if (rc) return rc;
  const int written = sk_read_back(b->d_idle_out, b->h_idle_out, 2, q->max_out, q->max_out, slots, s, "find_idle_slots_host");
  if (written >= 0 && total_out) *total_out = b->h_idle_out[1];
  return written;
}

/* what a call adds to touched_total: every voice it MAY put on the motion list -- an upper bound whether or not every note is placed
 * or every entry is a slot (the count word and the entries are on the device); the bound behind the in-place rule only has to hold */
static uint64_t slot_touched(int n, uint64_t voice_mask) { return (uint64_t)n * (uint64_t)__builtin_popcountll(voice_mask); }

/* the checked records -> a staging slot (sized for all n * K of them) -> the placement kernel */
static int slot_notes_launch(skred_bank_t *b, const skred_note_t *notes, int n, int slot_voices, uint64_t voice_mask,
                             const int32_t *d_slots, const uint32_t *d_count, int first_entry, int32_t *d_assigned,
                             uint32_t *d_result, hipStream_t s) {
  HIP_TRY(hipSetDevice(b->device));
  const size_t bytes = (size_t)n * (size_t)slot_voices * sizeof(skred_note_t);
  sk_batch_t bt;
  int rc = sk_batch_begin(b, bytes, s, &bt);
  if (rc) return rc;
  memcpy(bt.h, notes, bytes);
  const sk_note_t *src = (const sk_note_t *)sk_batch_send(b, &bt, bytes, 0, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)sk_launch_slot_notes(src, n, slot_voices, voice_mask, d_slots, d_count, first_entry, b->n_voices,
                                                        b->d_ro, b->d_rw, b->g.synth_sample_count, b->d_mask[b->mask_p], d_assigned,
                                                        d_result, bt.cnt, bt.done, bt.seq, s);
  if ((rc = sk_batch_end(&bt, e, "slot notes", s))) return rc;
  sk_touched(b, slot_touched(n, voice_mask));
  return SKRED_OK;
}

int skred_bank_notes_on_slots(skred_bank_t *b, const skred_note_t *notes, int n, int slot_voices, uint64_t voice_mask,
                              const int32_t *d_slots, const uint32_t *d_count, int first_entry, int32_t *d_assigned,
                              uint32_t *d_result, void *stream) {
  if (!b || !notes || !d_slots || !d_count || !d_result) return fail(SKRED_E_BAD_ARG, "notes_on_slots: no bank, notes, list, count or result");
  if (n < 0 || first_entry < 0) return fail(SKRED_E_BAD_ARG, "notes_on_slots: n = %d, first_entry = %d", n, first_entry);
  const int rc = slot_notes_check(notes, n, slot_voices, voice_mask, "notes_on_slots");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  return slot_notes_launch(b, notes, n, slot_voices, voice_mask, d_slots, d_count, first_entry, d_assigned, d_result, (hipStream_t)stream);
}

int skred_bank_note_on_idle_slots(skred_bank_t *b, const skred_slot_query_t *q, const skred_note_t *notes, int n, uint64_t voice_mask,
                                  int32_t *d_assigned, uint32_t *d_result, void *stream) {
  if (!b || !q || !notes || !d_result) return fail(SKRED_E_BAD_ARG, "note_on_idle_slots: no bank, query, notes or result");
  if (n < 0) return fail(SKRED_E_BAD_ARG, "note_on_idle_slots: n = %d", n);
  if (q->which & SKRED_IDLE_AMP_ZERO)
    return fail(SKRED_E_BAD_ARG, "note_on_idle_slots: SKRED_IDLE_AMP_ZERO -- a note-on leaves voice_amp alone: the slot would stay silent and be listed again");
  skred_slot_query_t qq = *q;
  qq.max_out = n;
  int rc = slots_check(b, &qq, b, b, "note_on_idle_slots");   /* (the list and the counts go into the bank's own scratch) */
  if (rc) return rc;
  if ((rc = slot_notes_check(notes, n, q->slot_voices, voice_mask, "note_on_idle_slots"))) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_note_list_room(b, n))) return rc;
  uint32_t *d_count = b->d_note_list;
  int32_t *d_list = (int32_t *)(b->d_note_list + SK_NOTE_LIST_WORDS);
  if ((rc = slots_launch(b, &qq, d_list, d_count, s))) return rc;
  return slot_notes_launch(b, notes, n, q->slot_voices, voice_mask, d_list, d_count, 0, d_assigned, d_result, s);
}

int skred_bank_stamp_slots(skred_bank_t *b, const int32_t *d_slots, int n, const uint32_t *d_count_or_null, int slot_voices,
                           uint64_t voice_mask, uint32_t stamps, void *stream) {
  if (!b || !d_slots || n < 0) return fail(SKRED_E_BAD_ARG, "stamp_slots: no bank, no list or n = %d", n);
  int rc = sk_check_stamps(stamps, "stamp_slots");
  if (rc) return rc;
  if ((rc = sk_check_slot_shape(slot_voices, voice_mask, "voice_mask", "stamp_slots"))) return rc;
  if ((rc = sk_check_list_n(n, "stamp_slots"))) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  const hipError_t e = (hipError_t)sk_launch_slot_stamps(d_slots, n, d_count_or_null, slot_voices, voice_mask, b->n_voices, stamps,
                                                         b->d_ro, b->d_rw, b->g.synth_sample_count, b->d_mask[b->mask_p], (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "stamp_slots launch -> %s", hipGetErrorString(e));
  sk_touched(b, slot_touched(n, voice_mask));
  return SKRED_OK;
}

/* ---- slot stealing, plain and matched (the victims of ONE channel: include/skred_amd.h, section "channel polyphony") ---- */

#define SK_SLOT_STEAL_FLAGS (SKRED_STEAL_RELEASED_FIRST | SKRED_STEAL_RELEASED_ONLY)

static int slot_steal_check(const skred_slot_steal_query_t *q, int n_voices, const char *who) {
  if (!q) return fail(SKRED_E_BAD_ARG, "%s: no query", who);
  if (q->policy != SKRED_STEAL_OLDEST && q->policy != SKRED_STEAL_QUIETEST) return fail(SKRED_E_BAD_ARG, "%s: unknown policy %u", who, q->policy);
  if ((q->flags & SKRED_STEAL_UNNAMED) || (q->exclude_idle & SKRED_IDLE_UNNAMED))
    return fail(SKRED_E_BAD_ARG, "%s: UNNAMED -- the voices of a patch name one another by design", who);
  if (q->flags & ~(uint32_t)SK_SLOT_STEAL_FLAGS) return fail(SKRED_E_BAD_ARG, "%s: unknown bits in flags = 0x%x", who, q->flags);
  if (q->exclude_idle & ~(uint32_t)SK_SLOT_CRITERIA) return fail(SKRED_E_BAD_ARG, "%s: unknown bits in exclude_idle = 0x%x", who, q->exclude_idle);
  if (q->reserved[0] || q->reserved[1]) return fail(SKRED_E_BAD_ARG, "%s: reserved words must be 0", who);
  if (q->max_out < 0 || q->max_out > SKRED_STEAL_MAX) return fail(SKRED_E_BAD_ARG, "%s: max_out %d outside [0, %d]", who, q->max_out, SKRED_STEAL_MAX);
  if (!(q->settle_level >= 0.0f) || isinf(q->settle_level)) return fail(SKRED_E_BAD_ARG, "%s: settle_level %g", who, (double)q->settle_level);
  const int rc = sk_check_slot_shape(q->slot_voices, q->member_mask, "member_mask", who);
  if (rc) return rc;
  if (n_voices <= 0) return fail(SKRED_E_BAD_ARG, "%s: a bank of %d voices", who, n_voices);
  return sk_check_slot_range(n_voices, q->first, q->count, q->slot_voices, 0, who);
}

int skred_slot_steal_check(const skred_slot_steal_query_t *q, int n_voices) { return slot_steal_check(q, n_voices, "slot_steal_check"); }

/* `matched`: the query is one channel's, `m` its match (checked here, behind the query; the query's refusals then carry the public
 * check's name) */
static int slot_steal_check_bank(const skred_bank_t *b, const skred_slot_steal_query_t *q, int matched, const skred_owner_match_t *m,
                                 const void *slots, const void *count, const char *who) {
  if (!b || !q) return fail(SKRED_E_BAD_ARG, "%s: no bank or no query", who);
  if (!count) return fail(SKRED_E_BAD_ARG, "%s: nowhere to put the counts", who);
  int rc = slot_steal_check(q, b->n_voices, matched ? "slot_steal_check" : who);
  if (rc) return rc;
  if (matched && (rc = skred_owner_match_check(m))) return rc;
  if (q->max_out > 0 && !slots) return fail(SKRED_E_BAD_ARG, "%s: max_out %d and no list to fill", who, q->max_out);
  return SKRED_OK;
}

/* the voice query's arguments (its scratch, `now`) around the slot key pass.  m != NULL: the matched key pass over the owner array
 * (allocated here by the first call that needs it); d_count then takes three words */
static int slot_steal_launch(skred_bank_t *b, const skred_slot_steal_query_t *q, const skred_owner_match_t *m, int32_t *d_slots,
                             uint32_t *d_count, hipStream_t s) {
  int rc;
  if (m) {
    HIP_TRY(hipSetDevice(b->device));
    if ((rc = sk_owner_ensure(b))) return rc;
  }
  const skred_steal_query_t vq = { q->first, q->count, q->policy, q->flags, q->min_age, q->exclude_idle, q->settle_level, q->max_out, 0 };
  sk_steal_args_t a;
  if ((rc = sk_steal_prepare(b, &vq, d_slots, d_count, s, &a))) return rc;
  const hipError_t e = (hipError_t)sk_launch_slot_steal(&a, q->member_mask, q->slot_voices, m ? b->d_owner : NULL, m ? m->value : 0,
                                                        m ? m->mask : 0, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "find_steal_slots%s launch -> %s", m ? "_match" : "", hipGetErrorString(e));
  return SKRED_OK;
}

/* the query into the bank's own d_steal_out: the counts in front (2; matched: 3), the victims behind them */
static int slot_steal_counts(const skred_owner_match_t *m) { return m ? 3 : 2; }

static int slot_steal_into_scratch(skred_bank_t *b, const skred_slot_steal_query_t *q, const skred_owner_match_t *m, hipStream_t s) {
  HIP_TRY(hipSetDevice(b->device));
  const int rc = sk_steal_out_buffers(b);
  if (rc) return rc;
  return slot_steal_launch(b, q, m, b->d_steal_out + slot_steal_counts(m), (uint32_t *)b->d_steal_out, s);
}

/* ... and from there to the caller: the entries written, or an error; h_steal_out holds the counts */
static int slot_steal_host(skred_bank_t *b, const skred_slot_steal_query_t *q, const skred_owner_match_t *m, int32_t *slots, hipStream_t s,
                           const char *who) {
  const int rc = slot_steal_into_scratch(b, q, m, s);
  if (rc) return rc;
  return sk_read_back(b->d_steal_out, b->h_steal_out, slot_steal_counts(m), q->max_out, q->max_out, slots, s, who);
}

int skred_bank_find_steal_slots(skred_bank_t *b, const skred_slot_steal_query_t *q, int32_t *d_slots, uint32_t *d_count, void *stream) {
  const int rc = slot_steal_check_bank(b, q, 0, NULL, d_slots, d_count, "find_steal_slots");
  if (rc) return rc;
  return slot_steal_launch(b, q, NULL, d_slots, d_count, (hipStream_t)stream);
}

int skred_bank_find_steal_slots_host(skred_bank_t *b, const skred_slot_steal_query_t *q, int32_t *slots, int *total_out, void *stream) {
  int dummy = 0;
  const int rc = slot_steal_check_bank(b, q, 0, NULL, slots, &dummy, "find_steal_slots_host");
  if (rc) return rc;
  const int written = slot_steal_host(b, q, NULL, slots, (hipStream_t)stream, "find_steal_slots_host");
  if (written >= 0 && total_out) *total_out = b->h_steal_out[1];
  return written;
}

int skred_bank_find_steal_slots_match(skred_bank_t *b, const skred_slot_steal_query_t *q, const skred_owner_match_t *m, int32_t *d_slots,
                                      uint32_t *d_count, void *stream) {
  const int rc = slot_steal_check_bank(b, q, 1, m, d_slots, d_count, "find_steal_slots_match");
  if (rc) return rc;
  return slot_steal_launch(b, q, m, d_slots, d_count, (hipStream_t)stream);
}

int skred_bank_find_steal_slots_match_host(skred_bank_t *b, const skred_slot_steal_query_t *q, const skred_owner_match_t *m, int32_t *slots,
                                           int *total_out, int *sounding_out, void *stream) {
  int dummy = 0;
  const int rc = slot_steal_check_bank(b, q, 1, m, slots, &dummy, "find_steal_slots_match_host");
  if (rc) return rc;
  const int written = slot_steal_host(b, q, m, slots, (hipStream_t)stream, "find_steal_slots_match_host");
  if (written >= 0 && total_out) *total_out = b->h_steal_out[1];
  if (written >= 0 && sounding_out) *sounding_out = b->h_steal_out[2];
  return written;
}

/* ---- note-on bursts that steal: the idle slots first, the victims behind them ---- */

/* the two queries as a burst runs them: the idle query lists at most n slots, the steal query excludes what the idle query lists
 * and returns at most n victims */
static void slot_burst_queries(const skred_slot_query_t *idle_q, const skred_slot_steal_query_t *steal_q, int n, skred_slot_query_t *iq,
                               skred_slot_steal_query_t *sq) {
  *iq = *idle_q;
  iq->max_out = n;
  *sq = *steal_q;
  sq->exclude_idle = idle_q->which;
  sq->settle_level = idle_q->settle_level;
  sq->max_out = n < SKRED_STEAL_MAX ? n : SKRED_STEAL_MAX;
}

int skred_bank_note_on_steal_slots(skred_bank_t *b, const skred_slot_query_t *idle_q, const skred_slot_steal_query_t *steal_q,
                                   const skred_note_t *notes, int n, uint64_t voice_mask, int32_t *d_assigned, uint32_t *d_result,
                                   void *stream) {
  if (!b || !idle_q || !steal_q || !notes || !d_result) return fail(SKRED_E_BAD_ARG, "note_on_steal_slots: no bank, query, notes or result");
  if (n < 0) return fail(SKRED_E_BAD_ARG, "note_on_steal_slots: n = %d", n);
  if (idle_q->which & SKRED_IDLE_AMP_ZERO)
    return fail(SKRED_E_BAD_ARG, "note_on_steal_slots: SKRED_IDLE_AMP_ZERO -- a note-on leaves voice_amp alone: the slot would stay silent and be listed again");
  skred_slot_query_t iq;
  skred_slot_steal_query_t sq;
  slot_burst_queries(idle_q, steal_q, n, &iq, &sq);
  int rc = slots_check(b, &iq, b, b, "note_on_steal_slots");   /* (the lists and the counts go into the bank's own scratch) */
  if (rc) return rc;
  if ((rc = slot_steal_check_bank(b, &sq, 0, NULL, b, b, "note_on_steal_slots"))) return rc;
  if (iq.slot_voices != sq.slot_voices || iq.member_mask != sq.member_mask)   /* (each range is made of whole slots of that K: checked above) */
    return fail(SKRED_E_BAD_ARG, "note_on_steal_slots: the idle query has K = %d, mask 0x%llx, the steal query K = %d, mask 0x%llx", iq.slot_voices,
                (unsigned long long)iq.member_mask, sq.slot_voices, (unsigned long long)sq.member_mask);
  if ((rc = slot_notes_check(notes, n, iq.slot_voices, voice_mask, "note_on_steal_slots"))) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_note_list_room(b, n))) return rc;
  uint32_t *d_idle_count = b->d_note_list, *d_joined = b->d_note_list + 2;
  int32_t *d_list = (int32_t *)(b->d_note_list + SK_NOTE_LIST_WORDS);
  if ((rc = slots_launch(b, &iq, d_list, d_idle_count, s))) return rc;
  if ((rc = slot_steal_into_scratch(b, &sq, NULL, s))) return rc;
  /* the victims behind the idle slots, as far as the burst reaches; d_result[2]: the notes that will land on them (every entry of
   * the joined list names a slot, and the list is no longer than the burst) */
  const hipError_t e = (hipError_t)sk_launch_list_append(d_list, d_idle_count, b->d_steal_out + 2, (const uint32_t *)b->d_steal_out, n,
                                                         d_joined, d_result + 2, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "list append launch -> %s", hipGetErrorString(e));
  return slot_notes_launch(b, notes, n, iq.slot_voices, voice_mask, d_list, d_joined, 0, d_assigned, d_result, s);
}

/* ---- channel polyphony: the capped, tagged burst ---- */

_Static_assert(sizeof(skred_owner_match_t) == 8, "skred_owner_match_t is (value, mask)");
_Static_assert(SKRED_CHAN_NO_CAP == 0xFFFFFFFFu, "no cap: the largest count a word holds");

int skred_chan_check(const skred_slot_query_t *idle_q, const skred_slot_steal_query_t *steal_q, const skred_owner_match_t *m, uint32_t cap,
                     const uint32_t *tags, int n, int n_voices) {
  (void)cap;                                               /* every cap is one: 0 lets nobody take an idle slot */
  if (!idle_q || !steal_q) return fail(SKRED_E_BAD_ARG, "chan_check: no idle query or no steal query");
  if (n < 0) return fail(SKRED_E_BAD_ARG, "chan_check: n = %d", n);
  if (idle_q->which & SKRED_IDLE_AMP_ZERO)
    return fail(SKRED_E_BAD_ARG, "chan_check: SKRED_IDLE_AMP_ZERO -- a note-on leaves voice_amp alone: the slot would stay silent and be listed again");
  skred_slot_query_t iq;
  skred_slot_steal_query_t sq;
  slot_burst_queries(idle_q, steal_q, n, &iq, &sq);
  int rc = skred_slot_query_check(&iq, n_voices);
  if (rc) return rc;
  if ((rc = skred_slot_steal_check(&sq, n_voices))) return rc;
  if (iq.slot_voices != sq.slot_voices || iq.member_mask != sq.member_mask)   /* (each range is made of whole slots of that K: checked above) */
    return fail(SKRED_E_BAD_ARG, "chan_check: the idle query has K = %d, mask 0x%llx, the steal query K = %d, mask 0x%llx", iq.slot_voices,
                (unsigned long long)iq.member_mask, sq.slot_voices, (unsigned long long)sq.member_mask);
  if ((rc = skred_owner_match_check(m))) return rc;
  if ((rc = skred_owner_tags_check(tags, n, SKRED_OWNER_ALLOW_ZERO))) return rc;   /* (what skred_bank_tag_slots asks of tags and n ...) */
  if ((rc = sk_check_list_n(n, "chan_check"))) return rc;
  for (int k = 0; k < n; k++) {                            /* ... and what only a channel asks: the note must count towards it */
    if (!tags[k]) return fail(SKRED_E_BAD_ARG, "chan_check: tag %d is 0 (0 means nobody: the note would belong to no channel)", k);
    if ((tags[k] & m->mask) != m->value)
      return fail(SKRED_E_BAD_ARG, "chan_check: tag %d = 0x%x does not satisfy the match (value 0x%x, mask 0x%x)", k, tags[k], m->value, m->mask);
  }
  return SKRED_OK;
}

/* skred_bank_note_on_steal_slots with the matched query, the join in place of the append, and the tags behind the notes.  The tags
 * change no class, counter, lane word or report: the owner array is no part of the bank the planner knows */
int skred_bank_note_on_channel(skred_bank_t *b, const skred_slot_query_t *idle_q, const skred_slot_steal_query_t *steal_q,
                               const skred_owner_match_t *m, uint32_t cap, const skred_note_t *notes, const uint32_t *tags, int n,
                               uint64_t voice_mask, int32_t *d_assigned, uint32_t *d_result, void *stream) {
  if (!b || !notes || !d_result) return fail(SKRED_E_BAD_ARG, "note_on_channel: no bank, notes or result");
  int rc = skred_chan_check(idle_q, steal_q, m, cap, tags, n, b->n_voices);
  if (rc) return rc;
  skred_slot_query_t iq;
  skred_slot_steal_query_t sq;
  slot_burst_queries(idle_q, steal_q, n, &iq, &sq);
  const int K = iq.slot_voices;
  if ((rc = skred_slot_notes_check(notes, n, K, voice_mask))) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_note_list_room(b, n))) return rc;
  uint32_t *d_idle_count = b->d_note_list, *d_joined = b->d_note_list + 2;
  int32_t *d_list = (int32_t *)(b->d_note_list + SK_NOTE_LIST_WORDS);
  /* 1. the idle slots, at most n;  2. the channel's victims and its sounding count */
  if ((rc = slots_launch(b, &iq, d_list, d_idle_count, s))) return rc;
  if ((rc = slot_steal_into_scratch(b, &sq, m, s))) return rc;
  /* 3. how many notes take idle slots, how many steal; the victims behind the idle slots that are used; d_result[2..3] */
  const hipError_t e = (hipError_t)sk_launch_chan_join(d_list, d_idle_count, b->d_steal_out + slot_steal_counts(m),
                                                       (const uint32_t *)b->d_steal_out, n, cap, d_joined, d_result, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "note_on_channel: join launch -> %s", hipGetErrorString(e));
  /* 4. the notes on the joined list: d_assigned, d_result[0..1] (an upper bound goes to touched_total: the cap and the channel can
   * only take notes away);  5. their tags: entry k of the joined list gets tags[k] (every entry is a slot of the bank) */
  if ((rc = slot_notes_launch(b, notes, n, K, voice_mask, d_list, d_joined, 0, d_assigned, d_result, s))) return rc;
  return sk_owner_tag_launch(b, d_list, tags, n, d_joined, K, NULL, "note_on_channel: tags", s);
}
