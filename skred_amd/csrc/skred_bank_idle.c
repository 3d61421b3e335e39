/*
 * skred_bank_idle.c -- the free-voice query (include/skred_amd.h: skred_bank_find_idle / _find_idle_host).
 *
 * Argument checks, the bank's scratch, the lazily rebuilt named set and the launches of skred_idle_kernels.hip.  Everything
 * is queued on the caller's stream; the host variant waits for that stream alone.
 */
#include <math.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(SK_IDLE_FINISHED == SKRED_IDLE_FINISHED && SK_IDLE_ENV_DONE == SKRED_IDLE_ENV_DONE &&
               SK_IDLE_AMP_ZERO == SKRED_IDLE_AMP_ZERO && SK_IDLE_UNNAMED == SKRED_IDLE_UNNAMED,
               "device query bits must equal the public SKRED_IDLE_* values");

#define SK_IDLE_CRITERIA (SKRED_IDLE_FINISHED | SKRED_IDLE_ENV_DONE | SKRED_IDLE_AMP_ZERO)

void sk_idle_free(skred_bank_t *b) {
  if (b->d_idle) hipFree(b->d_idle);
  if (b->d_named) hipFree(b->d_named);
  if (b->d_idle_out) hipFree(b->d_idle_out);
  if (b->h_idle_out) hipHostFree(b->h_idle_out);
  b->d_idle = NULL; b->d_named = NULL; b->d_idle_out = NULL; b->h_idle_out = NULL;
  b->idle_wgs = 0; b->idle_out_cap = 0;
}

/* everything that can be said without the device */
int sk_idle_check(const skred_bank_t *b, const skred_idle_query_t *q, const void *voices, const void *count, const char *who) {
  if (!b || !q) return fail(SKRED_E_BAD_ARG, "%s: no bank or no query", who);
  if (!count) return fail(SKRED_E_BAD_ARG, "%s: nowhere to put the counts", who);
  if (q->max_out < 0) return fail(SKRED_E_BAD_ARG, "%s: max_out %d", who, q->max_out);
  if (q->max_out > 0 && !voices) return fail(SKRED_E_BAD_ARG, "%s: max_out %d and no list to fill", who, q->max_out);
  if (q->which & ~(uint32_t)(SK_IDLE_CRITERIA | SKRED_IDLE_UNNAMED)) return fail(SKRED_E_BAD_ARG, "%s: unknown bits in which = 0x%x", who, q->which);
  if (!(q->which & SK_IDLE_CRITERIA)) return fail(SKRED_E_BAD_ARG, "%s: which = 0x%x selects no criterion", who, q->which);
  if (!(q->settle_level >= 0.0f) || isinf(q->settle_level)) return fail(SKRED_E_BAD_ARG, "%s: settle_level %g", who, (double)q->settle_level);
  const int rc = sk_check_slot_range(b->n_voices, q->first, q->count, 1, 0, who);
  if (rc) return rc;
  if (q->from < q->first || q->from - q->first >= q->count)
    return fail(SKRED_E_RANGE, "%s: from = %d outside the range [%d,+%d)", who, q->from, q->first, q->count);
  return SKRED_OK;
}

/* the named set, rebuilt on `s` when the routing changed since it was built (shared with skred_bank_steal.c) */
int sk_named_ensure(skred_bank_t *b, hipStream_t s) {
  if (!b->d_named) {
    HIP_TRY(hipMalloc((void **)&b->d_named, (size_t)(b->n_padded / 64) * sizeof(uint64_t)));
    b->named_dirty = 1;
  }
  if (b->named_dirty) {
    const hipError_t e = (hipError_t)sk_launch_named(b->d_ro[SKP_TAB], b->d_ro[SKP_MODI], b->n_padded, b->n_voices, b->d_named, s);
    if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "named-set launch -> %s", hipGetErrorString(e));
    b->named_dirty = 0;
  }
  return SKRED_OK;
}

/* the bank's scratch of both list queries (this one and skred_bank_slots.c's), allocated on first use */
int sk_idle_scratch(skred_bank_t *b, hipStream_t s) {
  if (b->d_idle) return SKRED_OK;
  /* sized once, for the whole bank from any `first` (a range's spans start at `first` rounded down to 64) */
  const int wgs = sk_idle_workgroups(63, b->n_padded);
  HIP_TRY(hipMalloc((void **)&b->d_idle, ((size_t)SK_IDLE_W_COUNT + 2 * (size_t)wgs) * sizeof(uint32_t)));
  b->idle_wgs = wgs;
  HIP_TRY(hipMemsetAsync(b->d_idle, 0, (size_t)SK_IDLE_W_COUNT * sizeof(uint32_t), s));   /* the ticket: zero once, re-armed by every last arriver */
  return SKRED_OK;
}

/* the kernels' view of a query on this bank: planes, scratch, range and criteria (`named` stays NULL) */
void sk_idle_args(const skred_bank_t *b, sk_idle_args_t *a, int first, int count, int from, int max_out, uint32_t which,
                  float settle_level, int32_t *d_voices, uint32_t *d_count) {
  memset(a, 0, sizeof(*a));
  a->osc_ro = b->d_ro[SKP_OSC];
  a->tab = b->d_ro[SKP_TAB];
  a->osc_rw = b->d_rw[SKS_OSC];
  a->filt = b->d_rw[SKS_FILT];
  a->words = b->d_idle;
  a->counts = b->d_idle + SK_IDLE_W_COUNT;
  a->offsets = a->counts + b->idle_wgs;
  a->d_voices = d_voices;
  a->d_count = d_count;
  a->first = first;
  a->end = first + count;
  a->from = from;
  a->max_out = max_out;
  a->which = which;
  a->settle_level = settle_level;
}

static int idle_launch(skred_bank_t *b, const skred_idle_query_t *q, int32_t *d_voices, uint32_t *d_count, hipStream_t s) {
  HIP_TRY(hipSetDevice(b->device));
  int rc = sk_idle_scratch(b, s);
  if (rc) return rc;
  if (q->which & SKRED_IDLE_UNNAMED) {
    rc = sk_named_ensure(b, s);
    if (rc) return rc;
  }
  sk_idle_args_t a;
  sk_idle_args(b, &a, q->first, q->count, q->from, q->max_out, q->which, q->settle_level, d_voices, d_count);
  a.named = (q->which & SKRED_IDLE_UNNAMED) ? b->d_named : NULL;
  if (sk_idle_workgroups(a.first, q->count) > b->idle_wgs) return fail(SKRED_E_RANGE, "find_idle: scratch too small");   /* (unreachable: sized above) */
  const hipError_t e = (hipError_t)sk_launch_idle(&a, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "find_idle launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

/* room for `need` entries behind the two counts in d_idle_out and its pinned twin (the _host forms of both list queries) */
int sk_idle_out_room(skred_bank_t *b, size_t need) {
  return sk_answer_room((void **)&b->d_idle_out, (void **)&b->h_idle_out, &b->idle_out_cap, 2, need);
}

int skred_bank_find_idle(skred_bank_t *b, const skred_idle_query_t *q, int32_t *d_voices, uint32_t *d_count, void *stream) {
  const int rc = sk_idle_check(b, q, d_voices, d_count, "find_idle");
  if (rc) return rc;
  return idle_launch(b, q, d_voices, d_count, (hipStream_t)stream);
}

int skred_bank_find_idle_host(skred_bank_t *b, const skred_idle_query_t *q, int32_t *voices, int *total_out, void *stream) {
  int dummy = 0;
  int rc = sk_idle_check(b, q, voices, &dummy, "find_idle_host");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_idle_out_room(b, (size_t)q->max_out))) return rc;
  rc = idle_launch(b, q, b->d_idle_out + 2, (uint32_t *)b->d_idle_out, s);
  if (rc) return rc;
  const int written = sk_read_back(b->d_idle_out, b->h_idle_out, 2, q->max_out, q->max_out, voices, s, "find_idle_host");
  if (written >= 0 && total_out) *total_out = b->h_idle_out[1];
  return written;
}
