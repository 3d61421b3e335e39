/*
 * skred_fx_steal.c -- voice stealing on the fixed-point bank (include/skred_amd_fxpt.h: skred_fx_steal_check,
 * skred_fxbank_find_steal / _find_steal_host / _note_on_steal), and channel polyphony on it (skred_fx_chan_check,
 * skred_fxbank_find_steal_match / _find_steal_match_host / _note_on_channel): the same query restricted to one owner match -- the
 * matched instantiation of the key pass over the owner array of skred_fx_owner.c --, and the capped, tagged burst on top of it.
 *
 * Argument checks (made before anything touches the device), the bank's scratch -- laid out as the float bank's
 * (skred_bank_steal.c), because everything behind the key pass is the float bank's select -- and the launches.  The query travels
 * in the launch arguments: it takes no staging slot.  skred_fxbank_note_on_steal stages its notes through the batch path exactly as
 * skred_fxbank_notes_on_list does.  Everything is queued on the caller's stream; only the host variant waits, for that stream alone.
 */
#include <string.h>

#include "skred_fx_steal.h"
#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

_Static_assert(SK_STEAL_MAX == SKRED_STEAL_MAX && SK_STEAL_OLDEST == SKRED_STEAL_OLDEST && SK_STEAL_QUIETEST == SKRED_STEAL_QUIETEST &&
               SK_STEAL_RELEASED_FIRST == SKRED_STEAL_RELEASED_FIRST && SK_STEAL_RELEASED_ONLY == SKRED_STEAL_RELEASED_ONLY,
               "device query bits must equal the public SKRED_STEAL_* values");
_Static_assert(sizeof(skred_fx_steal_query_t) == 40, "skred_fx_steal_query_t is 40 bytes (skred_amd/fxbank.py: FxStealQueryC)");

#define SKX_STEAL_FLAGS (SKRED_STEAL_RELEASED_FIRST | SKRED_STEAL_RELEASED_ONLY)
#define SKX_STEAL_EXCLUDE (SKRED_IDLE_FINISHED | SKRED_IDLE_ENV_DONE | SKRED_IDLE_AMP_ZERO)

void skx_steal_free(skred_fxbank_t *fx) {
  if (fx->d_steal) hipFree(fx->d_steal);
  if (fx->d_steal_out) hipFree(fx->d_steal_out);
  if (fx->h_steal_out) hipHostFree(fx->h_steal_out);
  fx->d_steal = NULL; fx->d_steal_out = NULL; fx->h_steal_out = NULL;
  fx->steal_wgs = 0;
}

static int steal_check(const skred_fx_steal_query_t *q, int n_voices, const char *who) {
  if (!q) return fail(SKRED_E_BAD_ARG, "%s: no query", who);
  if (q->policy != SKRED_STEAL_OLDEST && q->policy != SKRED_STEAL_QUIETEST) return fail(SKRED_E_BAD_ARG, "%s: unknown policy %u", who, q->policy);
  if (q->flags & SKRED_STEAL_UNNAMED) return fail(SKRED_E_BAD_ARG, "%s: SKRED_STEAL_UNNAMED -- the fixed-point definition has no modulators", who);
  if (q->flags & ~(uint32_t)SKX_STEAL_FLAGS) return fail(SKRED_E_BAD_ARG, "%s: unknown bits in flags = 0x%x", who, q->flags);
  if (q->exclude_idle & SKRED_IDLE_UNNAMED) return fail(SKRED_E_BAD_ARG, "%s: SKRED_IDLE_UNNAMED -- the fixed-point definition has no modulators", who);
  if (q->exclude_idle & ~(uint32_t)SKX_STEAL_EXCLUDE) return fail(SKRED_E_BAD_ARG, "%s: unknown bits in exclude_idle = 0x%x", who, q->exclude_idle);
  if (q->reserved != 0) return fail(SKRED_E_BAD_ARG, "%s: reserved = %d must be 0", who, q->reserved);
  if (q->max_out < 0 || q->max_out > SKRED_STEAL_MAX) return fail(SKRED_E_BAD_ARG, "%s: max_out %d outside [0, %d]", who, q->max_out, SKRED_STEAL_MAX);
  if (q->settle_q15 < 0) return fail(SKRED_E_BAD_ARG, "%s: settle_q15 %d", who, q->settle_q15);
  if (n_voices <= 0) return fail(SKRED_E_BAD_ARG, "%s: a bank of %d voices", who, n_voices);
  return sk_check_slot_range(n_voices, q->first, q->count, 1, 0, who);
}

int skred_fx_steal_check(const skred_fx_steal_query_t *q, int n_voices) { return steal_check(q, n_voices, "fx steal_check"); }

/* `matched`: the query is one channel's, `m` its match (checked here, behind the query; the query's refusals then carry the public
 * check's name) */
static int steal_check_bank(const skred_fxbank_t *fx, const skred_fx_steal_query_t *q, int matched, const skred_owner_match_t *m,
                            const void *voices, const void *count, const char *who) {
  if (!fx || !q) return fail(SKRED_E_BAD_ARG, "%s: no bank or no query", who);
  if (!count) return fail(SKRED_E_BAD_ARG, "%s: nowhere to put the counts", who);
  int rc = steal_check(q, fx->n_voices, matched ? "fx steal_check" : who);
  if (rc) return rc;
  if (matched && (rc = skred_owner_match_check(m))) return rc;
  if (q->max_out > 0 && !voices) return fail(SKRED_E_BAD_ARG, "%s: max_out %d and no list to fill", who, q->max_out);
  return SKRED_OK;
}

/* the bank's scratch (allocated by the first query, its words zeroed on `s`) and a checked query as the key pass takes it --
 * everything but base, digit and the idle range, which the launcher fills */
static int steal_prepare(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, int32_t *d_voices, uint32_t *d_count, hipStream_t s,
                         skx_steal_args_t *out) {
  HIP_TRY(hipSetDevice(fx->device));
  /* the scratch, sized once for the whole bank from any `first` (as the idle query's): words and histogram | four words per
   * workgroup | the winners' keys, then their voices | one key per voice of the spans */
  const int wgs = fx->d_steal ? fx->steal_wgs : sk_idle_workgroups(63, fx->n_padded);
  const size_t head = (size_t)SK_STEAL_W_COUNT + SK_STEAL_BINS;                    /* uint32 words, a multiple of 4 */
  const size_t per_wg = head + 4 * (size_t)wgs;
  const size_t win_at = (per_wg * sizeof(uint32_t) + 15) & ~(size_t)15;            /* bytes */
  const size_t keys_at = win_at + (size_t)SK_STEAL_MAX * (sizeof(uint64_t) + sizeof(int32_t));
  if (!fx->d_steal) {
    HIP_TRY(hipMalloc((void **)&fx->d_steal, keys_at + (size_t)wgs * SK_IDLE_SPAN * sizeof(uint64_t)));
    fx->steal_wgs = wgs;
    HIP_TRY(hipMemsetAsync(fx->d_steal, 0, head * sizeof(uint32_t), s));   /* ticket and histogram: zero once, re-armed by every last arriver */
  }
  skx_steal_args_t a;
  memset(&a, 0, sizeof(a));
  a.idle.osc = fx->d_ro[SKX_OSC];
  a.idle.rw0 = fx->d_rw[0];
  a.idle.which = q->exclude_idle;
  a.idle.settle_q15 = q->settle_q15;
  a.time = fx->d_ro[SKX_TIME];
  a.s.words = fx->d_steal;
  a.s.hist = fx->d_steal + SK_STEAL_W_COUNT;
  a.s.cnt_lt = fx->d_steal + head;
  a.s.cnt_eq = a.s.cnt_lt + wgs;
  a.s.off_lt = a.s.cnt_eq + wgs;
  a.s.off_eq = a.s.off_lt + wgs;
  a.s.win_keys = (unsigned long long *)((char *)fx->d_steal + win_at);
  a.s.win_voices = (int32_t *)(a.s.win_keys + SK_STEAL_MAX);
  a.s.keys = (unsigned long long *)((char *)fx->d_steal + keys_at);
  a.s.d_voices = d_voices;
  a.s.d_count = d_count;
  a.s.now = fx->count;
  a.s.min_age = q->min_age;
  a.s.first = q->first;
  a.s.end = q->first + q->count;
  a.s.max_out = q->max_out;
  a.s.policy = q->policy;
  a.s.flags = q->flags;
  if (sk_idle_workgroups(a.s.first, q->count) > wgs) return fail(SKRED_E_RANGE, "fx find_steal: scratch too small");   /* (unreachable: sized above) */
  *out = a;
  return SKRED_OK;
}

/* m != NULL: the matched key pass over the owner array (allocated here by the first call that needs it); d_count then takes three words */
static int steal_launch(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, const skred_owner_match_t *m, int32_t *d_voices,
                        uint32_t *d_count, hipStream_t s) {
  int rc;
  if (m) {
    HIP_TRY(hipSetDevice(fx->device));
    if ((rc = skx_owner_ensure(fx))) return rc;
  }
  skx_steal_args_t a;
  if ((rc = steal_prepare(fx, q, d_voices, d_count, s, &a))) return rc;
  const hipError_t e = (hipError_t)skx_launch_steal(&a, m ? fx->d_owner : NULL, m ? m->value : 0, m ? m->mask : 0, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx find_steal%s launch -> %s", m ? "_match" : "", hipGetErrorString(e));
  return SKRED_OK;
}

/* the query into the bank's own d_steal_out: the counts in front (2; matched: 3), the victims behind them */
static int steal_counts(const skred_owner_match_t *m) { return m ? 3 : 2; }

static int steal_into_scratch(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, const skred_owner_match_t *m, hipStream_t s) {
  HIP_TRY(hipSetDevice(fx->device));
  if (!fx->d_steal_out) HIP_TRY(hipMalloc((void **)&fx->d_steal_out, (3 + SK_STEAL_MAX) * sizeof(int32_t)));
  if (!fx->h_steal_out) HIP_TRY(hipHostMalloc((void **)&fx->h_steal_out, (3 + SK_STEAL_MAX) * sizeof(int32_t), hipHostMallocDefault));
  return steal_launch(fx, q, m, fx->d_steal_out + steal_counts(m), (uint32_t *)fx->d_steal_out, s);
}

/* ... and from there to the caller: the entries written, or an error; h_steal_out holds the counts */
static int steal_host(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, const skred_owner_match_t *m, int32_t *voices, hipStream_t s,
                      const char *who) {
  const int rc = steal_into_scratch(fx, q, m, s);
  if (rc) return rc;
  return sk_read_back(fx->d_steal_out, fx->h_steal_out, steal_counts(m), q->max_out, q->max_out, voices, s, who);
}

int skred_fxbank_find_steal(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, int32_t *d_voices, uint32_t *d_count, void *stream) {
  const int rc = steal_check_bank(fx, q, 0, NULL, d_voices, d_count, "fx find_steal");
  if (rc) return rc;
  return steal_launch(fx, q, NULL, d_voices, d_count, (hipStream_t)stream);
}

int skred_fxbank_find_steal_host(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, int32_t *voices, int *total_out, void *stream) {
  int dummy = 0;
  const int rc = steal_check_bank(fx, q, 0, NULL, voices, &dummy, "fx find_steal_host");
  if (rc) return rc;
  const int written = steal_host(fx, q, NULL, voices, (hipStream_t)stream, "fx find_steal_host");
  if (written >= 0 && total_out) *total_out = fx->h_steal_out[1];
  return written;
}

int skred_fxbank_find_steal_match(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, const skred_owner_match_t *m, int32_t *d_voices,
                                  uint32_t *d_count, void *stream) {
  const int rc = steal_check_bank(fx, q, 1, m, d_voices, d_count, "fx find_steal_match");
  if (rc) return rc;
  return steal_launch(fx, q, m, d_voices, d_count, (hipStream_t)stream);
}

int skred_fxbank_find_steal_match_host(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, const skred_owner_match_t *m, int32_t *voices,
                                       int *total_out, int *sounding_out, void *stream) {
  int dummy = 0;
  const int rc = steal_check_bank(fx, q, 1, m, voices, &dummy, "fx find_steal_match_host");
  if (rc) return rc;
  const int written = steal_host(fx, q, m, voices, (hipStream_t)stream, "fx find_steal_match_host");
  if (written >= 0 && total_out) *total_out = fx->h_steal_out[1];
  if (written >= 0 && sounding_out) *sounding_out = fx->h_steal_out[2];
  return written;
}

/* ---- note-on bursts that steal: the idle voices first, the victims behind them ---- */

/* the two queries as a burst runs them: the idle query lists at most n voices, the steal query excludes what the idle query lists
 * and returns at most n victims */
static void burst_queries(const skred_fx_idle_query_t *idle_q, const skred_fx_steal_query_t *steal_q, int n, skred_fx_idle_query_t *iq,
                          skred_fx_steal_query_t *sq) {
  *iq = *idle_q;
  iq->max_out = n;
  *sq = *steal_q;
  sq->exclude_idle = idle_q->which;
  sq->settle_q15 = idle_q->settle_q15;
  sq->max_out = n < SKRED_STEAL_MAX ? n : SKRED_STEAL_MAX;
}

int skred_fxbank_note_on_steal(skred_fxbank_t *fx, const skred_fx_idle_query_t *idle_q, const skred_fx_steal_query_t *steal_q,
                               const skred_fx_note_t *notes, int n, int32_t *d_assigned, uint32_t *d_result, void *stream) {
  if (!fx || !idle_q || !steal_q || !notes || !d_result) return fail(SKRED_E_BAD_ARG, "fx note_on_steal: no bank, query, notes or result");
  if (n < 0) return fail(SKRED_E_BAD_ARG, "fx note_on_steal: n = %d", n);
  if (idle_q->which & SKRED_IDLE_AMP_ZERO)
    return fail(SKRED_E_BAD_ARG, "fx note_on_steal: SKRED_IDLE_AMP_ZERO -- a note-on leaves amp_q15 alone: the voice would stay silent and be listed again");
  skred_fx_idle_query_t iq;
  skred_fx_steal_query_t sq;
  burst_queries(idle_q, steal_q, n, &iq, &sq);
  int rc = skred_fx_idle_check(&iq, fx->n_voices);
  if (rc) return rc;
  if ((rc = steal_check(&sq, fx->n_voices, "fx note_on_steal"))) return rc;
  if (n == 0) return SKRED_OK;
  if ((rc = skred_fx_notes_check(notes, n))) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_note_list_room(fx, n))) return rc;
  uint32_t *d_idle_count = fx->d_note_list, *d_joined = fx->d_note_list + 2;
  int32_t *d_list = (int32_t *)(fx->d_note_list + SKX_NOTE_LIST_WORDS);
  if ((rc = skx_idle_launch(fx, &iq, d_list, d_idle_count, s))) return rc;
  if ((rc = steal_into_scratch(fx, &sq, NULL, s))) return rc;
  /* the victims behind the idle entries, as far as the batch reaches; d_result[2]: the notes that will land on them (every entry
   * of the joined list names a voice, and the list is no longer than the batch) */
  const hipError_t e = (hipError_t)sk_launch_list_append(d_list, d_idle_count, fx->d_steal_out + 2, (const uint32_t *)fx->d_steal_out, n,
                                                         d_joined, d_result + 2, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx list append launch -> %s", hipGetErrorString(e));
  return skx_notes_launch(fx, notes, n, d_list, d_joined, 0, d_assigned, d_result, "fx note_on_steal", s);
}

/* ---- channel polyphony: the capped, tagged burst ---- */

_Static_assert(sizeof(skred_owner_match_t) == 8, "skred_owner_match_t is (value, mask)");
_Static_assert(SKRED_CHAN_NO_CAP == 0xFFFFFFFFu, "no cap: the largest count a word holds");

int skred_fx_chan_check(const skred_fx_idle_query_t *idle_q, const skred_fx_steal_query_t *steal_q, const skred_owner_match_t *m, uint32_t cap,
                        const uint32_t *tags, int n, int n_voices) {
  (void)cap;                                               /* every cap is one: 0 lets nobody take an idle voice */
  if (!idle_q || !steal_q) return fail(SKRED_E_BAD_ARG, "fx chan_check: no idle query or no steal query");
  if (n < 0) return fail(SKRED_E_BAD_ARG, "fx chan_check: n = %d", n);
  if (idle_q->which & SKRED_IDLE_AMP_ZERO)
    return fail(SKRED_E_BAD_ARG, "fx chan_check: SKRED_IDLE_AMP_ZERO -- a note-on leaves amp_q15 alone: the voice would stay silent and be listed again");
  skred_fx_idle_query_t iq;
  skred_fx_steal_query_t sq;
  burst_queries(idle_q, steal_q, n, &iq, &sq);
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

/* skred_fxbank_note_on_steal with the matched query, the join in place of the append, and the tags behind the notes.  The tags change
 * nothing a render reads */
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
  burst_queries(idle_q, steal_q, n, &iq, &sq);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_note_list_room(fx, n))) return rc;
  uint32_t *d_idle_count = fx->d_note_list, *d_joined = fx->d_note_list + 2;
  int32_t *d_list = (int32_t *)(fx->d_note_list + SKX_NOTE_LIST_WORDS);
  /* 1. the idle voices, at most n;  2. the channel's victims and its sounding count */
  if ((rc = skx_idle_launch(fx, &iq, d_list, d_idle_count, s))) return rc;
  if ((rc = steal_into_scratch(fx, &sq, m, s))) return rc;
  /* 3. how many notes take idle voices, how many steal; the victims behind the idle voices that are used; d_result[2..3] */
  const hipError_t e = (hipError_t)sk_launch_chan_join(d_list, d_idle_count, fx->d_steal_out + steal_counts(m),
                                                       (const uint32_t *)fx->d_steal_out, n, cap, d_joined, d_result, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx note_on_channel: join launch -> %s", hipGetErrorString(e));
  /* 4. the notes on the joined list: d_assigned, d_result[0..1];  5. their tags: entry k of the joined list gets tags[k] (every entry
   * is a voice of the bank) */
  if ((rc = skx_notes_launch(fx, notes, n, d_list, d_joined, 0, d_assigned, d_result, "fx note_on_channel", s))) return rc;
  return skx_owner_tag_launch(fx, d_list, tags, n, d_joined, NULL, "fx note_on_channel: tags", s);
}
