/*
 * skred_fx_chan.c -- channel polyphony on the fixed-point bank: the victim query of one channel and the capped, tagged note-on
 * (include/skred_amd_fxpt.h: skred_fx_chan_check, skred_fxbank_find_steal_match / _find_steal_match_host / _note_on_channel).
 *
 * The host side of skred_fx_chan_kernels.hip, on the pieces the other control calls of this bank are made of: the public checks of the
 * two queries, the match and the notes (made before anything touches the device), the steal scratch and the query's arguments of
 * skred_fx_steal.c, the idle query, the list scratch and the note placement of skred_fx_live.c, the owner array of skred_fx_owner.c,
 * the staging ring, and the float bank's bank-agnostic launchers of the join and of the owner tags (at K = 1, as skred_fxbank_tag_list
 * enters it).  The three count words and the victims have a device and a pinned buffer of their own (d_chan_out / h_chan_out): the
 * layout of d_steal_out stays what skred_fxbank_note_on_steal knows.  Nothing here waits for the device except the _host query, which
 * waits for its stream, and the allocation of a scratch by the first call that needs it.  The tags change nothing a render reads.
 */
#include <stddef.h>
#include <string.h>

#include "skred_fx_chan.h"
#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

_Static_assert(sizeof(skred_owner_match_t) == 8, "skred_owner_match_t is (value, mask)");
_Static_assert(SKRED_CHAN_NO_CAP == 0xFFFFFFFFu, "no cap: the largest count a word holds");

#define SKX_CHAN_OUT_COUNTS 3
#define SKX_CHAN_OUT_ENTRIES ((size_t)SKX_CHAN_OUT_COUNTS + SK_STEAL_MAX)

void skx_chan_free(skred_fxbank_t *fx) {
  if (fx->d_chan_out) hipFree(fx->d_chan_out);
  if (fx->h_chan_out) hipHostFree(fx->h_chan_out);
  fx->d_chan_out = NULL; fx->h_chan_out = NULL;
}

static int chan_out_room(skred_fxbank_t *fx) {
  if (!fx->d_chan_out) HIP_TRY(hipMalloc((void **)&fx->d_chan_out, SKX_CHAN_OUT_ENTRIES * sizeof(int32_t)));
  if (!fx->h_chan_out) HIP_TRY(hipHostMalloc((void **)&fx->h_chan_out, SKX_CHAN_OUT_ENTRIES * sizeof(int32_t), hipHostMallocDefault));
  return SKRED_OK;
}

/* the two queries as the burst runs them: the idle query lists at most n voices, the steal query excludes what the idle query
 * lists and returns at most n victims */
static void chan_queries(const skred_fx_idle_query_t *idle_q, const skred_fx_steal_query_t *steal_q, int n, skred_fx_idle_query_t *iq,
                         skred_fx_steal_query_t *sq) {
  *iq = *idle_q;
  iq->max_out = n;
  *sq = *steal_q;
  sq->exclude_idle = idle_q->which;
  sq->settle_q15 = idle_q->settle_q15;
  sq->max_out = n < SKRED_STEAL_MAX ? n : SKRED_STEAL_MAX;
}

int skred_fx_chan_check(const skred_fx_idle_query_t *idle_q, const skred_fx_steal_query_t *steal_q, const skred_owner_match_t *m, uint32_t cap,
                        const uint32_t *tags, int n, int n_voices) {
  (void)cap;                                               /* every cap is one: 0 lets nobody take an idle voice */
  if (!idle_q || !steal_q) return fail(SKRED_E_BAD_ARG, "fx chan_check: no idle query or no steal query");
  if (n < 0) return fail(SKRED_E_BAD_ARG, "fx chan_check: n = %d", n);
  if (idle_q->which & SKRED_IDLE_AMP_ZERO)
    return fail(SKRED_E_BAD_ARG, "fx chan_check: SKRED_IDLE_AMP_ZERO -- a note-on leaves amp_q15 alone: the voice would stay silent and be listed again");
  skred_fx_idle_query_t iq;
  skred_fx_steal_query_t sq;
  chan_queries(idle_q, steal_q, n, &iq, &sq);
  int rc = skred_fx_idle_check(&iq, n_voices);
  if (rc) return rc;
  if ((rc = skred_fx_steal_check(&sq, n_voices))) return rc;
  if ((rc = skred_owner_match_check(m))) return rc;
  if ((rc = skred_owner_tags_check(tags, n, SKRED_OWNER_ALLOW_ZERO))) return rc;   /* (what skred_fxbank_tag_list asks of tags and n ...) */
  if ((rc = sk_check_list_n(n, "fx chan_check"))) return rc;
  for (int k = 0; k < n; k++) {                            /* ... and what only a channel asks: the note must count towards it */
    if (!tags[k]) return fail(SKRED_E_BAD_ARG, "fx chan_check: tag %d is 0 (0 means nobody: the note would belong to no channel)", k);
    if ((tags[k] & m->mask) != m->value)
      return fail(SKRED_E_BAD_ARG, "fx chan_check: tag %d = 0x%x does not satisfy the match (value 0x%x, mask 0x%x)", k, tags[k], m->value, m->mask);
  }
  return SKRED_OK;
}

/* ---- the matched victim query ---- */

static int match_query_check(const skred_fxbank_t *fx, const skred_fx_steal_query_t *q, const skred_owner_match_t *m, const void *voices,
                             const void *count, const char *who) {
  if (!fx || !q) return fail(SKRED_E_BAD_ARG, "%s: no bank or no query", who);
  if (!count) return fail(SKRED_E_BAD_ARG, "%s: nowhere to put the counts", who);
  int rc = skred_fx_steal_check(q, fx->n_voices);
  if (rc) return rc;
  if ((rc = skred_owner_match_check(m))) return rc;
  if (q->max_out > 0 && !voices) return fail(SKRED_E_BAD_ARG, "%s: max_out %d and no list to fill", who, q->max_out);
  return SKRED_OK;
}

/* the plain query's arguments (its scratch, `now`) around the matched key pass */
static int match_query_launch(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, const skred_owner_match_t *m, int32_t *d_voices,
                              uint32_t *d_count, hipStream_t s) {
  int rc = skx_owner_ensure(fx);
  if (rc) return rc;
  skx_steal_args_t a;
  if ((rc = skx_steal_prepare(fx, q, d_voices, d_count, s, &a))) return rc;
  const hipError_t e = (hipError_t)skx_launch_chan_steal(&a, fx->d_owner, m->value, m->mask, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx find_steal_match launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_find_steal_match(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, const skred_owner_match_t *m, int32_t *d_voices,
                                  uint32_t *d_count, void *stream) {
  const int rc = match_query_check(fx, q, m, d_voices, d_count, "fx find_steal_match");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(fx->device));
  return match_query_launch(fx, q, m, d_voices, d_count, (hipStream_t)stream);
}

int skred_fxbank_find_steal_match_host(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, const skred_owner_match_t *m, int32_t *voices,
                                       int *total_out, int *sounding_out, void *stream) {
  int dummy = 0;
  int rc = match_query_check(fx, q, m, voices, &dummy, "fx find_steal_match_host");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = chan_out_room(fx))) return rc;
  int32_t *d = fx->d_chan_out, *h = fx->h_chan_out;
  if ((rc = match_query_launch(fx, q, m, d + SKX_CHAN_OUT_COUNTS, (uint32_t *)d, s))) return rc;
  HIP_TRY(hipMemcpyAsync(h, d, (SKX_CHAN_OUT_COUNTS + (size_t)q->max_out) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[0] < 0 || h[0] > q->max_out)
    return fail(SKRED_E_NO_DEVICE, "fx find_steal_match_host: the device reported %d of at most %d", h[0], q->max_out);
  if (h[0] > 0) memcpy(voices, h + SKX_CHAN_OUT_COUNTS, (size_t)h[0] * sizeof(int32_t));
  if (total_out) *total_out = h[1];
  if (sounding_out) *sounding_out = h[2];
  return h[0];
}

/* ---- the capped, tagged note-on ---- */

int skred_fxbank_note_on_channel(skred_fxbank_t *fx, const skred_fx_idle_query_t *idle_q, const skred_fx_steal_query_t *steal_q,
                                 const skred_owner_match_t *m, uint32_t cap, const skred_fx_note_t *notes, const uint32_t *tags, int n,
                                 int32_t *d_assigned, uint32_t *d_result, void *stream) {
  if (!fx || !notes || !d_result) return fail(SKRED_E_BAD_ARG, "fx note_on_channel: no bank, notes or result");
  int rc = skred_fx_chan_check(idle_q, steal_q, m, cap, tags, n, fx->n_voices);
  if (rc) return rc;
  if ((rc = skred_fx_notes_check(notes, n))) return rc;
  if (n == 0) return SKRED_OK;
  skred_fx_idle_query_t iq;
  skred_fx_steal_query_t sq;
  chan_queries(idle_q, steal_q, n, &iq, &sq);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_note_list_room(fx, n))) return rc;
  if ((rc = chan_out_room(fx))) return rc;
  uint32_t *d_idle_count = fx->d_note_list, *d_joined = fx->d_note_list + 2;
  int32_t *d_list = (int32_t *)(fx->d_note_list + SKX_NOTE_LIST_WORDS);
  uint32_t *d_victim_count = (uint32_t *)fx->d_chan_out;
  int32_t *d_victims = fx->d_chan_out + SKX_CHAN_OUT_COUNTS;
  /* 1. the idle voices, at most n */
  if ((rc = skx_idle_launch(fx, &iq, d_list, d_idle_count, s))) return rc;
  /* 2. the channel's victims and its sounding count */
  if ((rc = match_query_launch(fx, &sq, m, d_victims, d_victim_count, s))) return rc;
  /* 3. how many notes take idle voices, how many steal; the victims behind the idle voices that are used; d_result[2..3] */
  hipError_t e = (hipError_t)sk_launch_chan_join(d_list, d_idle_count, d_victims, d_victim_count, n, cap, d_joined, d_result, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx note_on_channel: join launch -> %s", hipGetErrorString(e));
  /* 4. the notes on the joined list: d_assigned, d_result[0..1] */
  if ((rc = skx_notes_launch(fx, notes, n, d_list, d_joined, 0, d_assigned, d_result, s))) return rc;
  /* 5. the tags of the placed notes: entry k of the joined list gets tags[k] (every entry is a voice of the bank) */
  const size_t tag_bytes = (size_t)n * sizeof(uint32_t);
  skx_slot_t *sl;
  if ((rc = skx_ring_take(fx, tag_bytes, &sl))) return rc;
  memcpy(sl->h, tags, tag_bytes);
  if ((rc = skx_ring_send(sl, tag_bytes, s))) return rc;
  e = (hipError_t)sk_launch_owner_tag(fx->d_owner, d_list, (const uint32_t *)sl->d, n, d_joined, 1, fx->n_voices, NULL, NULL, NULL, 0, s);
  rc = skx_ring_guard(sl, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx note_on_channel: tags launch -> %s", hipGetErrorString(e));
  return rc;
}
