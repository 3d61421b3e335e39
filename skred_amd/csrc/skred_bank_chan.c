/*
 * skred_bank_chan.c -- channel polyphony: the victim query of one channel and the capped, tagged note-on (include/skred_amd.h:
 * skred_chan_check, skred_bank_find_steal_slots_match / _find_steal_slots_match_host / _note_on_channel).
 *
 * The host side of skred_chan_kernels.hip, on the pieces the other control calls are made of: the public checks of the two queries,
 * the match and the notes (made before anything touches the device), the steal scratch of skred_bank_steal.c, the idle scratch and
 * the answer buffers of skred_bank_idle.c, the list scratch of skred_bank_notes.c, the owner array of skred_bank_owner.c, the batch
 * path of skred_bank_stage.c, and the launchers of the idle-slot query, the slot notes and the owner tags as they are.  Nothing here
 * waits for the device except the _host query, which waits for its stream, and the allocation of a scratch by the first call that
 * needs it.  What a burst tells the bank is what skred_bank_note_on_steal_slots tells it: n * popcount(voice_mask) more voices may
 * be on the motion list (an upper bound: the cap and the channel can only take notes away), and earlier launches' reports are out
 * of date.  The tags change no class, counter, lane word or report: the owner array is no part of the bank the planner knows.
 *
 * The fixed-point bank's twin is skred_fx_chan.c.  Out of scope: shards beyond skred_shard_bank(), the drop-in mode, deferred items and
 * pattern steps.
 */
#include <stddef.h>
#include <string.h>

#include "skred_bank_priv.h"
#include "skred_chan.h"

_Static_assert(sizeof(skred_owner_match_t) == 8, "skred_owner_match_t is (value, mask)");
_Static_assert(SKRED_CHAN_NO_CAP == 0xFFFFFFFFu, "no cap: the largest count a word holds");

/* the two queries as the burst runs them: the idle query lists at most n slots, the steal query excludes what the idle query
 * lists and returns at most n victims */
static void chan_queries(const skred_slot_query_t *idle_q, const skred_slot_steal_query_t *steal_q, int n, skred_slot_query_t *iq,
                         skred_slot_steal_query_t *sq) {
  *iq = *idle_q;
  iq->max_out = n;
  *sq = *steal_q;
  sq->exclude_idle = idle_q->which;
  sq->settle_level = idle_q->settle_level;
  sq->max_out = n < SKRED_STEAL_MAX ? n : SKRED_STEAL_MAX;
}

int skred_chan_check(const skred_slot_query_t *idle_q, const skred_slot_steal_query_t *steal_q, const skred_owner_match_t *m, uint32_t cap,
                     const uint32_t *tags, int n, int n_voices) {
  (void)cap;                                               /* every cap is one: 0 lets nobody take an idle slot */
  if (!idle_q || !steal_q) return fail(SKRED_E_BAD_ARG, "chan_check: no idle query or no steal query");
  if (n < 0) return fail(SKRED_E_BAD_ARG, "chan_check: n = %d", n);
  if (idle_q->which & SKRED_IDLE_AMP_ZERO)
    return fail(SKRED_E_BAD_ARG, "chan_check: SKRED_IDLE_AMP_ZERO -- a note-on leaves voice_amp alone: the slot would stay silent and be listed again");
  skred_slot_query_t iq;
  skred_slot_steal_query_t sq;
  chan_queries(idle_q, steal_q, n, &iq, &sq);
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

/* ---- the matched victim query ---- */

static int match_query_check(const skred_bank_t *b, const skred_slot_steal_query_t *q, const skred_owner_match_t *m, const void *slots,
                             const void *count, const char *who) {
  if (!b || !q) return fail(SKRED_E_BAD_ARG, "%s: no bank or no query", who);
  if (!count) return fail(SKRED_E_BAD_ARG, "%s: nowhere to put the counts", who);
  int rc = skred_slot_steal_check(q, b->n_voices);
  if (rc) return rc;
  if ((rc = skred_owner_match_check(m))) return rc;
  if (q->max_out > 0 && !slots) return fail(SKRED_E_BAD_ARG, "%s: max_out %d and no list to fill", who, q->max_out);
  return SKRED_OK;
}

/* the voice query's arguments (its scratch, `now`) around the matched key pass */
static int match_query_launch(skred_bank_t *b, const skred_slot_steal_query_t *q, const skred_owner_match_t *m, int32_t *d_slots,
                              uint32_t *d_count, hipStream_t s) {
  int rc = sk_owner_ensure(b);
  if (rc) return rc;
  const skred_steal_query_t vq = { q->first, q->count, q->policy, q->flags, q->min_age, q->exclude_idle, q->settle_level, q->max_out, 0 };
  sk_steal_args_t a;
  if ((rc = sk_steal_prepare(b, &vq, d_slots, d_count, s, &a))) return rc;
  const hipError_t e = (hipError_t)sk_launch_chan_steal(&a, q->member_mask, q->slot_voices, b->d_owner, m->value, m->mask, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "find_steal_slots_match launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_bank_find_steal_slots_match(skred_bank_t *b, const skred_slot_steal_query_t *q, const skred_owner_match_t *m, int32_t *d_slots,
                                      uint32_t *d_count, void *stream) {
  const int rc = match_query_check(b, q, m, d_slots, d_count, "find_steal_slots_match");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(b->device));
  return match_query_launch(b, q, m, d_slots, d_count, (hipStream_t)stream);
}

/* the bank's answer buffer (skred_bank_idle.c: two words and a list) holds the three counts and SKRED_STEAL_MAX victims */
#define SK_CHAN_OUT_ENTRIES ((size_t)SKRED_STEAL_MAX + 1)
#define SK_CHAN_OUT_COUNTS 3

int skred_bank_find_steal_slots_match_host(skred_bank_t *b, const skred_slot_steal_query_t *q, const skred_owner_match_t *m, int32_t *slots,
                                           int *total_out, int *sounding_out, void *stream) {
  int dummy = 0;
  int rc = match_query_check(b, q, m, slots, &dummy, "find_steal_slots_match_host");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_idle_out_room(b, SK_CHAN_OUT_ENTRIES))) return rc;
  int32_t *d = b->d_idle_out, *h = b->h_idle_out;
  if ((rc = match_query_launch(b, q, m, d + SK_CHAN_OUT_COUNTS, (uint32_t *)d, s))) return rc;
  HIP_TRY(hipMemcpyAsync(h, d, (SK_CHAN_OUT_COUNTS + (size_t)q->max_out) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[0] < 0 || h[0] > q->max_out)
    return fail(SKRED_E_NO_DEVICE, "find_steal_slots_match_host: the device reported %d of at most %d", h[0], q->max_out);
  if (h[0] > 0) memcpy(slots, h + SK_CHAN_OUT_COUNTS, (size_t)h[0] * sizeof(int32_t));
  if (total_out) *total_out = h[1];
  if (sounding_out) *sounding_out = h[2];
  return h[0];
}

/* ---- the capped, tagged note-on ---- */

int skred_bank_note_on_channel(skred_bank_t *b, const skred_slot_query_t *idle_q, const skred_slot_steal_query_t *steal_q,
                               const skred_owner_match_t *m, uint32_t cap, const skred_note_t *notes, const uint32_t *tags, int n,
                               uint64_t voice_mask, int32_t *d_assigned, uint32_t *d_result, void *stream) {
  if (!b || !notes || !d_result) return fail(SKRED_E_BAD_ARG, "note_on_channel: no bank, notes or result");
  int rc = skred_chan_check(idle_q, steal_q, m, cap, tags, n, b->n_voices);
  if (rc) return rc;
  skred_slot_query_t iq;
  skred_slot_steal_query_t sq;
  chan_queries(idle_q, steal_q, n, &iq, &sq);
  const int K = iq.slot_voices;
  if ((rc = skred_slot_notes_check(notes, n, K, voice_mask))) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_note_list_room(b, n))) return rc;
  if ((rc = sk_idle_out_room(b, SK_CHAN_OUT_ENTRIES))) return rc;
  if ((rc = sk_idle_scratch(b, s))) return rc;
  uint32_t *d_idle_count = b->d_note_list, *d_joined = b->d_note_list + 2;
  int32_t *d_list = (int32_t *)(b->d_note_list + SK_NOTE_LIST_WORDS);
  uint32_t *d_victim_count = (uint32_t *)b->d_idle_out;
  int32_t *d_victims = b->d_idle_out + SK_CHAN_OUT_COUNTS;
  /* 1. the idle slots, at most n */
  sk_slot_args_t ia;
  memset(&ia, 0, sizeof(ia));
  sk_idle_args(b, &ia.idle, iq.first, iq.count, iq.from, iq.max_out, iq.which, iq.settle_level, d_list, d_idle_count);
  ia.member_mask = iq.member_mask;
  ia.slot_voices = K;
  hipError_t e = (hipError_t)sk_launch_slots(&ia, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "note_on_channel: idle query launch -> %s", hipGetErrorString(e));
  /* 2. the channel's victims and its sounding count */
  if ((rc = match_query_launch(b, &sq, m, d_victims, d_victim_count, s))) return rc;
  /* 3. how many notes take idle slots, how many steal; the victims behind the idle slots that are used; d_result[2..3] */
  e = (hipError_t)sk_launch_chan_join(d_list, d_idle_count, d_victims, d_victim_count, n, cap, d_joined, d_result, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "note_on_channel: join launch -> %s", hipGetErrorString(e));
  /* 4. the notes on the joined list: d_assigned, d_result[0..1] */
  const size_t note_bytes = (size_t)n * (size_t)K * sizeof(skred_note_t);
  sk_batch_t bt;
  if ((rc = sk_batch_begin(b, note_bytes, s, &bt))) return rc;
  memcpy(bt.h, notes, note_bytes);
  const sk_note_t *src = (const sk_note_t *)sk_batch_send(b, &bt, note_bytes, 0, s);
  if (!src) return SKRED_E_NO_DEVICE;
  e = (hipError_t)sk_launch_slot_notes(src, n, K, voice_mask, d_list, d_joined, 0, b->n_voices, b->d_ro, b->d_rw, b->g.synth_sample_count,
                                       b->d_mask[b->mask_p], d_assigned, d_result, bt.cnt, bt.done, bt.seq, s);
  if ((rc = sk_batch_end(&bt, e, "note_on_channel: slot notes", s))) return rc;
  sk_touched(b, (uint64_t)n * (uint64_t)__builtin_popcountll(voice_mask));
  /* 5. the tags of the placed notes: entry k of the joined list gets tags[k] (every entry is a slot of the bank) */
  const size_t tag_bytes = (size_t)n * sizeof(uint32_t);
  if ((rc = sk_batch_begin(b, tag_bytes, s, &bt))) return rc;
  memcpy(bt.h, tags, tag_bytes);
  const uint32_t *tsrc = (const uint32_t *)sk_batch_send(b, &bt, tag_bytes, 0, s);
  if (!tsrc) return SKRED_E_NO_DEVICE;
  e = (hipError_t)sk_launch_owner_tag(b->d_owner, d_list, tsrc, n, d_joined, K, b->n_voices, NULL, bt.cnt, bt.done, bt.seq, s);
  return sk_batch_end(&bt, e, "note_on_channel: tags", s);
}
