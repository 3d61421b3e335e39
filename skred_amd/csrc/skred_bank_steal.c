/*
 * skred_bank_steal.c -- voice stealing (include/skred_amd.h: skred_steal_check, skred_bank_find_steal / _find_steal_host).
 *
 * Argument checks (made before anything touches the device), the bank's scratch, the lazily rebuilt named set (shared with
 * skred_bank_idle.c) and the launches of skred_steal_kernels.hip.  Everything is queued on the caller's stream; the host variant
 * waits for that stream alone.  skred_bank_note_on_steal (skred_bank_notes.c) runs the query into d_steal_out.
 */
#include <math.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(SK_STEAL_MAX == SKRED_STEAL_MAX && SK_STEAL_OLDEST == SKRED_STEAL_OLDEST && SK_STEAL_QUIETEST == SKRED_STEAL_QUIETEST &&
               SK_STEAL_RELEASED_FIRST == SKRED_STEAL_RELEASED_FIRST && SK_STEAL_RELEASED_ONLY == SKRED_STEAL_RELEASED_ONLY &&
               SK_STEAL_UNNAMED == SKRED_STEAL_UNNAMED,
               "device query bits must equal the public SKRED_STEAL_* values");
_Static_assert(sizeof(skred_steal_query_t) == 40, "skred_steal_query_t is 40 bytes (skred_amd/device.py: StealQueryC)");

#define SK_STEAL_FLAGS (SKRED_STEAL_RELEASED_FIRST | SKRED_STEAL_RELEASED_ONLY | SKRED_STEAL_UNNAMED)
#define SK_STEAL_EXCLUDE (SKRED_IDLE_FINISHED | SKRED_IDLE_ENV_DONE | SKRED_IDLE_AMP_ZERO | SKRED_IDLE_UNNAMED)

void sk_steal_free(skred_bank_t *b) {
  if (b->d_steal) hipFree(b->d_steal);
  if (b->d_steal_out) hipFree(b->d_steal_out);
  if (b->h_steal_out) hipHostFree(b->h_steal_out);
  b->d_steal = NULL; b->d_steal_out = NULL; b->h_steal_out = NULL;
  b->steal_wgs = 0;
}

static int steal_check(const skred_steal_query_t *q, int n_voices, const char *who) {
  if (!q) return fail(SKRED_E_BAD_ARG, "%s: no query", who);
  if (q->policy != SKRED_STEAL_OLDEST && q->policy != SKRED_STEAL_QUIETEST) return fail(SKRED_E_BAD_ARG, "%s: unknown policy %u", who, q->policy);
  if (q->flags & ~(uint32_t)SK_STEAL_FLAGS) return fail(SKRED_E_BAD_ARG, "%s: unknown bits in flags = 0x%x", who, q->flags);
  if (q->exclude_idle & ~(uint32_t)SK_STEAL_EXCLUDE) return fail(SKRED_E_BAD_ARG, "%s: unknown bits in exclude_idle = 0x%x", who, q->exclude_idle);
  if (q->reserved != 0) return fail(SKRED_E_BAD_ARG, "%s: reserved = %d must be 0", who, q->reserved);
  if (q->max_out < 0 || q->max_out > SKRED_STEAL_MAX) return fail(SKRED_E_BAD_ARG, "%s: max_out %d outside [0, %d]", who, q->max_out, SKRED_STEAL_MAX);
  if (!(q->settle_level >= 0.0f) || isinf(q->settle_level)) return fail(SKRED_E_BAD_ARG, "%s: settle_level %g", who, (double)q->settle_level);
  if (n_voices <= 0) return fail(SKRED_E_BAD_ARG, "%s: a bank of %d voices", who, n_voices);
  return sk_check_slot_range(n_voices, q->first, q->count, 1, 0, who);
}

int skred_steal_check(const skred_steal_query_t *q, int n_voices) { return steal_check(q, n_voices, "steal_check"); }

int sk_steal_check_bank(const skred_bank_t *b, const skred_steal_query_t *q, const void *voices, const void *count, const char *who) {
  if (!b || !q) return fail(SKRED_E_BAD_ARG, "%s: no bank or no query", who);
  if (!count) return fail(SKRED_E_BAD_ARG, "%s: nowhere to put the counts", who);
  const int rc = steal_check(q, b->n_voices, who);
  if (rc) return rc;
  if (q->max_out > 0 && !voices) return fail(SKRED_E_BAD_ARG, "%s: max_out %d and no list to fill", who, q->max_out);
  return SKRED_OK;
}

int sk_steal_prepare(skred_bank_t *b, const skred_steal_query_t *q, int32_t *d_voices, uint32_t *d_count, hipStream_t s, sk_steal_args_t *out) {
  HIP_TRY(hipSetDevice(b->device));
  /* the scratch, sized once for the whole bank from any `first` (as the idle query's): words and histogram | four words per
   * workgroup | the winners' keys, then their voices | one key per voice of the spans */
  const int wgs = b->d_steal ? b->steal_wgs : sk_idle_workgroups(63, b->n_padded);
  const size_t head = (size_t)SK_STEAL_W_COUNT + SK_STEAL_BINS;                    /* uint32 words, a multiple of 4 */
  const size_t per_wg = head + 4 * (size_t)wgs;
  const size_t win_at = (per_wg * sizeof(uint32_t) + 15) & ~(size_t)15;            /* bytes */
  const size_t keys_at = win_at + (size_t)SK_STEAL_MAX * (sizeof(uint64_t) + sizeof(int32_t));
  if (!b->d_steal) {
    HIP_TRY(hipMalloc((void **)&b->d_steal, keys_at + (size_t)wgs * SK_IDLE_SPAN * sizeof(uint64_t)));
    b->steal_wgs = wgs;
    HIP_TRY(hipMemsetAsync(b->d_steal, 0, head * sizeof(uint32_t), s));   /* ticket and histogram: zero once, re-armed by every last arriver */
  }
  const int need_named = ((q->flags & SKRED_STEAL_UNNAMED) || (q->exclude_idle & SKRED_IDLE_UNNAMED)) ? 1 : 0;
  if (need_named) {
    const int rc = sk_named_ensure(b, s);
    if (rc) return rc;
  }
  sk_steal_args_t a;
  memset(&a, 0, sizeof(a));
  a.idle.osc_ro = b->d_ro[SKP_OSC];
  a.idle.tab = b->d_ro[SKP_TAB];
  a.idle.osc_rw = b->d_rw[SKS_OSC];
  a.idle.filt = b->d_rw[SKS_FILT];
  a.idle.named = need_named ? b->d_named : NULL;
  a.idle.which = q->exclude_idle;
  a.idle.settle_level = q->settle_level;
  a.env_s = b->d_ro[SKP_ENV_S];
  a.words = b->d_steal;
  a.hist = b->d_steal + SK_STEAL_W_COUNT;
  a.cnt_lt = b->d_steal + head;
  a.cnt_eq = a.cnt_lt + wgs;
  a.off_lt = a.cnt_eq + wgs;
  a.off_eq = a.off_lt + wgs;
  a.win_keys = (unsigned long long *)((char *)b->d_steal + win_at);
  a.win_voices = (int32_t *)(a.win_keys + SK_STEAL_MAX);
  a.keys = (unsigned long long *)((char *)b->d_steal + keys_at);
  a.d_voices = d_voices;
  a.d_count = d_count;
  a.now = b->g.synth_sample_count;
  a.min_age = q->min_age;
  a.first = q->first;
  a.end = q->first + q->count;
  a.max_out = q->max_out;
  a.policy = q->policy;
  a.flags = q->flags;
  if (sk_idle_workgroups(a.first, q->count) > wgs) return fail(SKRED_E_RANGE, "steal query: scratch too small");   /* (unreachable: sized above) */
  *out = a;
  return SKRED_OK;
}

static int steal_launch(skred_bank_t *b, const skred_steal_query_t *q, int32_t *d_voices, uint32_t *d_count, hipStream_t s) {
  sk_steal_args_t a;
  const int rc = sk_steal_prepare(b, q, d_voices, d_count, s, &a);
  if (rc) return rc;
  const hipError_t e = (hipError_t)sk_launch_steal(&a, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "find_steal launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_bank_find_steal(skred_bank_t *b, const skred_steal_query_t *q, int32_t *d_voices, uint32_t *d_count, void *stream) {
  const int rc = sk_steal_check_bank(b, q, d_voices, d_count, "find_steal");
  if (rc) return rc;
  return steal_launch(b, q, d_voices, d_count, (hipStream_t)stream);
}

int sk_steal_out_buffers(skred_bank_t *b) {
  if (!b->d_steal_out) HIP_TRY(hipMalloc((void **)&b->d_steal_out, (3 + SK_STEAL_MAX) * sizeof(int32_t)));
  if (!b->h_steal_out) HIP_TRY(hipHostMalloc((void **)&b->h_steal_out, (3 + SK_STEAL_MAX) * sizeof(int32_t), hipHostMallocDefault));
  return SKRED_OK;
}

int sk_steal_into_scratch(skred_bank_t *b, const skred_steal_query_t *q, hipStream_t s) {
  HIP_TRY(hipSetDevice(b->device));
  const int rc = sk_steal_out_buffers(b);
  if (rc) return rc;
  return steal_launch(b, q, b->d_steal_out + 2, (uint32_t *)b->d_steal_out, s);
}

int skred_bank_find_steal_host(skred_bank_t *b, const skred_steal_query_t *q, int32_t *voices, int *total_out, void *stream) {
  int dummy = 0;
  int rc = sk_steal_check_bank(b, q, voices, &dummy, "find_steal_host");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = sk_steal_into_scratch(b, q, s))) return rc;
  const int written = sk_read_back(b->d_steal_out, b->h_steal_out, 2, q->max_out, q->max_out, voices, s, "find_steal_host");
  if (written >= 0 && total_out) *total_out = b->h_steal_out[1];
  return written;
}
