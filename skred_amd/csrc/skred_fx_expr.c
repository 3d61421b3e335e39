/*
 * skred_fx_expr.c -- channels and per-note expression on the fixed-point bank: masked owner matches and per-entry controller values
 * (include/skred_amd_fxpt.h: skred_fx_ctl_each_check, skred_fxbank_find_match / _find_match_host / _stamp_match / _ctl_match /
 * _ctl_owned_each / _ctl_tags_each), and per-note timbre: the same two calls with per-entry filter coefficients
 * (skred_fx_filter_each_check, skred_fxbank_ctl_owned_each_filter / _ctl_tags_each_filter).
 *
 * The host side of skred_fx_expr_kernels.hip, built like skred_fx_ctl.c and skred_fx_owner.c: the checks (made before anything
 * touches the device; the match's own through the float bank's skred_owner_match_check, the record's through skred_fx_ctl_check, the
 * shared ones of skred_bank_checks.c), the record's, entries' and tags' way through the batch path (skred_fx_stage.c), the launches.  The ordered list
 * of the matches is the float bank's count and scatter, entered through sk_launch_match_find at slot_voices = 1 on this bank's query
 * scratch, which has the shape they need (skred_fx_live.c: skx_idle_scratch).  Nothing here waits for the device except
 * _find_match_host, which waits for its stream, and the allocation of the owner array by the first call that needs it.  The bank
 * keeps no shadow of the voices and its render path has no planner to tell: a call ends with its launch.
 *
 * Out of scope: slots (K > 1), the deferred queue and pattern steps, the drop-in mode.
 */
#include <stddef.h>
#include <string.h>

#include "skred_launch.h"
#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

_Static_assert(sizeof(skred_fx_ctl_each_t) == sizeof(skx_each_t) && sizeof(skred_fx_ctl_each_t) == 32 && offsetof(skred_fx_ctl_each_t, set) == 4 * SKX_EACH_SET &&
               offsetof(skred_fx_ctl_each_t, inc_scale_q16) == 4 * SKX_EACH_W_INC_SCALE && offsetof(skred_fx_ctl_each_t, amp_scale_q16) == 4 * SKX_EACH_W_AMP_SCALE &&
               offsetof(skred_fx_ctl_each_t, velocity_q15) == 4 * SKX_EACH_W_VELOCITY && offsetof(skred_fx_ctl_each_t, pan_left_q15) == 4 * SKX_EACH_W_PAN_LEFT &&
               offsetof(skred_fx_ctl_each_t, pan_right_q15) == 4 * SKX_EACH_W_PAN_RIGHT && offsetof(skred_fx_ctl_each_t, reserved) == 24,
               "the device's per-entry record must be skred_fx_ctl_each_t word for word");
_Static_assert(SKX_EACH_INC_SCALE == SKRED_EACH_INC_SCALE && SKX_EACH_AMP_SCALE == SKRED_EACH_AMP_SCALE && SKX_EACH_VELOCITY == SKRED_EACH_VELOCITY &&
               SKX_EACH_PAN == SKRED_EACH_PAN, "device per-entry bits must equal the public SKRED_EACH_* values");
_Static_assert(sizeof(skx_ctl_t) % 16 == 0, "the entries behind the record stay 16-byte aligned");
_Static_assert(sizeof(skred_fx_filter_each_t) == sizeof(skx_filt_each_t) && sizeof(skred_fx_filter_each_t) == 32 &&
               offsetof(skred_fx_filter_each_t, b0_q30) == 4 * SKX_FILT_W_B0 && offsetof(skred_fx_filter_each_t, b1_q30) == 4 * SKX_FILT_W_B1 &&
               offsetof(skred_fx_filter_each_t, b2_q30) == 4 * SKX_FILT_W_B2 && offsetof(skred_fx_filter_each_t, a1_q30) == 4 * SKX_FILT_W_A1 &&
               offsetof(skred_fx_filter_each_t, a2_q30) == 4 * SKX_FILT_W_A2 && offsetof(skred_fx_filter_each_t, reserved) == 20,
               "the device's per-entry filter record must be skred_fx_filter_each_t word for word");
/* the float bank's count and scatter run on this bank's query scratch */
_Static_assert((int)SKX_IDLE_W_TICKET == (int)SK_IDLE_W_TICKET && (int)SKX_IDLE_W_PART == (int)SK_IDLE_W_PART &&
               (int)SKX_IDLE_W_RANK == (int)SK_IDLE_W_RANK && (int)SKX_IDLE_W_TOTAL == (int)SK_IDLE_W_TOTAL &&
               (int)SKX_IDLE_W_COUNT == (int)SK_IDLE_W_COUNT && SKX_IDLE_SPAN == SK_CONTROL_SPAN,
               "the fixed-point query scratch must have the shape sk_launch_match_find needs");

static int each_check(const skred_fx_ctl_each_t *each, int n, const skred_fx_ctl_t *ctl, const char *who) {
  if (!each) return fail(SKRED_E_BAD_ARG, "%s: no entries", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  int rc;
  if (ctl && (rc = skred_fx_ctl_check(ctl))) return rc;
  const uint32_t which = ctl ? ctl->which : 0u;
  for (int k = 0; k < n; k++) {
    const skred_fx_ctl_each_t *e = &each[k];
    if (e->set & ~(uint32_t)SKX_EACH_ALL) return fail(SKRED_E_BAD_ARG, "%s: entry %d: unknown bits in set = 0x%x", who, k, e->set);
    if (!e->set) return fail(SKRED_E_BAD_ARG, "%s: entry %d: set is 0", who, k);
    if (e->reserved[0] || e->reserved[1]) return fail(SKRED_E_BAD_ARG, "%s: entry %d: the reserved words must be 0", who, k);
    if ((e->set & SKRED_EACH_VELOCITY) && (e->velocity_q15 < 0 || e->velocity_q15 > 65535))
      return fail(SKRED_E_BAD_ARG, "%s: entry %d: velocity_q15 %d outside 0..65535", who, k, e->velocity_q15);
    if ((e->set & SKRED_EACH_PAN) && (e->pan_left_q15 < 0 || e->pan_left_q15 > 65535 || e->pan_right_q15 < 0 || e->pan_right_q15 > 65535))
      return fail(SKRED_E_BAD_ARG, "%s: entry %d: pan (%d, %d) outside 0..65535", who, k, e->pan_left_q15, e->pan_right_q15);
    if (e->set & SKRED_EACH_AMP_SCALE) {
      /* amp 0 would take the voice out of the voices that can sound (skred_fx_ctl.c) */
      if (e->amp_scale_q16 == 0) return fail(SKRED_E_BAD_ARG, "%s: entry %d: amp_scale_q16 == 0", who, k);
      if (!(which & SKRED_CTL_AMP)) return fail(SKRED_E_BAD_ARG, "%s: entry %d: SKRED_EACH_AMP_SCALE and no record that names SKRED_CTL_AMP", who, k);
    }
    if ((e->set & SKRED_EACH_INC_SCALE) && (which & (SKRED_CTL_PHASE_INC | SKRED_CTL_INC_SCALE)))
      return fail(SKRED_E_BAD_ARG, "%s: entry %d: SKRED_EACH_INC_SCALE and a record that names an increment", who, k);
  }
  return SKRED_OK;
}

int skred_fx_ctl_each_check(const skred_fx_ctl_each_t *each, int n, const skred_fx_ctl_t *ctl) { return each_check(each, n, ctl, "fx ctl_each_check"); }

void skx_each_pack(const skred_fx_ctl_each_t *each, int n, const uint32_t *perm, skx_each_t *out) {
  memset(out, 0, (size_t)n * sizeof(skx_each_t));
  for (int j = 0; j < n; j++) {
    const skred_fx_ctl_each_t *e = &each[perm ? perm[j] : (uint32_t)j];
    uint32_t *w = out[j].w;
    w[SKX_EACH_SET] = e->set;
    if (e->set & SKRED_EACH_INC_SCALE) w[SKX_EACH_W_INC_SCALE] = e->inc_scale_q16;
    if (e->set & SKRED_EACH_AMP_SCALE) w[SKX_EACH_W_AMP_SCALE] = e->amp_scale_q16;
    if (e->set & SKRED_EACH_VELOCITY) w[SKX_EACH_W_VELOCITY] = (uint32_t)e->velocity_q15;
    if (e->set & SKRED_EACH_PAN) { w[SKX_EACH_W_PAN_LEFT] = (uint32_t)e->pan_left_q15; w[SKX_EACH_W_PAN_RIGHT] = (uint32_t)e->pan_right_q15; }
  }
}

/* the record first (what each_check looks at before its entries), then the coefficients: any int32 is a coefficient */
static int filter_check(const skred_fx_filter_each_t *filt, int n, const skred_fx_ctl_t *ctl, const char *who) {
  if (!filt) return fail(SKRED_E_BAD_ARG, "%s: no coefficients", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  int rc;
  if (ctl && (rc = skred_fx_ctl_check(ctl))) return rc;
  if (ctl && (ctl->which & SKRED_CTL_FILTER)) return fail(SKRED_E_BAD_ARG, "%s: the record names SKRED_CTL_FILTER too: two sets of coefficients", who);
  for (int k = 0; k < n; k++)
    if (filt[k].reserved[0] || filt[k].reserved[1] || filt[k].reserved[2])
      return fail(SKRED_E_BAD_ARG, "%s: coefficients %d: the reserved words must be 0", who, k);
  return SKRED_OK;
}

int skred_fx_filter_each_check(const skred_fx_filter_each_t *filt, int n, const skred_fx_ctl_t *ctl) {
  return filter_check(filt, n, ctl, "fx filter_each_check");
}

void skx_filt_pack(const skred_fx_filter_each_t *filt, int n, const uint32_t *perm, skx_filt_each_t *out) {
  memset(out, 0, (size_t)n * sizeof(skx_filt_each_t));
  for (int j = 0; j < n; j++) memcpy(out[j].w, &filt[perm ? perm[j] : (uint32_t)j], 5 * sizeof(uint32_t));
}

/* ---- A. masked matches ---- */

static int match_check(const skred_owner_match_t *m, const char *who) {
  if (!m) return fail(SKRED_E_BAD_ARG, "%s: no match", who);
  return skred_owner_match_check(m);     /* the float bank's check, as it is */
}

static int find_match_check(const skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, int max_out, const void *voices,
                            const void *total, const char *who) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  int rc = match_check(m, who);
  if (rc) return rc;
  if (!total) return fail(SKRED_E_BAD_ARG, "%s: nowhere to put the count", who);
  if (max_out < 0) return fail(SKRED_E_BAD_ARG, "%s: max_out %d", who, max_out);
  if (max_out > 0 && !voices) return fail(SKRED_E_BAD_ARG, "%s: max_out %d and no list to fill", who, max_out);
  return sk_check_slot_range(fx->n_voices, first, count, 1, 0, who);   /* at least one voice, inside the bank */
}

/* count and scatter of the matching voices of a checked range; the count pass's (written, total) pair goes to the words behind the
 * owner array, the total where the caller wants it */
static int find_match_launch(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, int max_out, int32_t *d_voices,
                             uint32_t *d_total, hipStream_t s) {
  int rc = skx_owner_ensure(fx);
  if (rc) return rc;
  if ((rc = skx_idle_scratch(fx, s))) return rc;
  /* one lane per voice from `first`: (count + 255) / 256 workgroups, never more than a query of the whole bank takes */
  if ((count + SK_CONTROL_SPAN - 1) / SK_CONTROL_SPAN > fx->idle_wgs) return fail(SKRED_E_RANGE, "fx find_match: scratch too small");   /* (unreachable) */
  sk_match_args_t a;
  memset(&a, 0, sizeof(a));
  a.idle.words = fx->d_idle;
  a.idle.counts = fx->d_idle + SKX_IDLE_W_COUNT;
  a.idle.offsets = a.idle.counts + fx->idle_wgs;
  a.idle.d_voices = d_voices;
  a.idle.d_count = fx->d_match_pair;
  a.idle.max_out = max_out;
  a.owner = fx->d_owner;
  a.d_total = d_total;
  a.value = m->value;
  a.mask = m->mask;
  const hipError_t e = (hipError_t)sk_launch_match_find(&a, first, count, 1, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx find_match launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_find_match(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, int max_out, int32_t *d_voices,
                            uint32_t *d_count, void *stream) {
  const int rc = find_match_check(fx, first, count, m, max_out, d_voices, d_count, "fx find_match");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(fx->device));
  return find_match_launch(fx, first, count, m, max_out, d_voices, d_count, (hipStream_t)stream);
}

int skred_fxbank_find_match_host(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, int max_out, int32_t *voices,
                                 int *total_out, void *stream) {
  int dummy = 0;
  int rc = find_match_check(fx, first, count, m, max_out, voices, &dummy, "fx find_match_host");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_idle_out_room(fx, (size_t)max_out))) return rc;
  /* word 0: the total; the list from word 2, as the idle query lays its answer out */
  if ((rc = find_match_launch(fx, first, count, m, max_out, fx->d_idle_out + 2, (uint32_t *)fx->d_idle_out, s))) return rc;
  const int written = sk_read_back(fx->d_idle_out, fx->h_idle_out, 2, max_out, count, voices, s, "fx find_match_host");
  if (written >= 0 && total_out) *total_out = fx->h_idle_out[0];
  return written;
}

int skred_fxbank_stamp_match(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, uint32_t stamps, uint32_t *d_result,
                             void *stream) {
  if (!fx || !d_result) return fail(SKRED_E_BAD_ARG, "fx stamp_match: no bank or no result");
  int rc = match_check(m, "fx stamp_match");
  if (rc) return rc;
  if ((rc = sk_check_stamps(stamps, "fx stamp_match"))) return rc;
  if ((rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, "fx stamp_match"))) return rc;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_owner_ensure(fx))) return rc;
  const hipError_t e = (hipError_t)skx_launch_match_stamps(fx->d_owner, m->value, m->mask, first, count, stamps, fx->d_ro[SKX_TIME], fx->d_rw[0],
                                                           fx->count, d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx stamp_match launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_ctl_match(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, int first, int count, const skred_owner_match_t *m,
                           uint32_t *d_result, void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx ctl_match: no bank");
  int rc = skred_fx_ctl_check(ctl);
  if (rc) return rc;
  if ((rc = match_check(m, "fx ctl_match"))) return rc;
  if ((rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, "fx ctl_match"))) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_owner_ensure(fx))) return rc;
  skx_batch_t bt;
  if ((rc = skx_batch_begin(fx, sizeof(skx_ctl_t), &bt))) return rc;
  skx_ctl_pack(ctl, (skx_ctl_t *)bt.h);
  /* the device twin: a bank-wide range is thousands of workgroups reading the record */
  const skx_ctl_t *src = (const skx_ctl_t *)skx_batch_send(&bt, sizeof(skx_ctl_t), s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)skx_launch_ctl_match(src, first, count, fx->d_owner, m->value, m->mask, fx->d_ro, d_result, s);
  return skx_batch_end(&bt, e, "fx ctl_match", s);
}

/* ---- B. per-entry controller values ---- */

/* with_filter: a call of section C, where `each` may be NULL and the coefficients are checked behind the entries */
static int owned_each_check(const skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const skred_fx_ctl_each_t *each, const skred_fx_filter_each_t *filt,
                            int with_filter, const uint32_t *tags, int n, uint32_t tag_flags, const char *who) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  int rc = skred_owner_tags_check(tags, n, tag_flags);
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, who))) return rc;
  if (!with_filter) return each_check(each, n, ctl, who);
  if (each && (rc = each_check(each, n, ctl, who))) return rc;
  return filter_check(filt, n, ctl, who);
}

/* the record (zeros without `ctl`), the n entries (each[perm[j]]; perm NULL: as they stand), with `filt` the n sets of coefficients
 * (permuted likewise; then `each` may be NULL and no entries travel) and the n tags in one staging slot: one kernel reads them all,
 * from the slot's device twin */
static int owned_each_launch(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const skred_fx_ctl_each_t *each, const skred_fx_filter_each_t *filt,
                             const uint32_t *perm, const int32_t *d_voices, const uint32_t *tags, int n, const uint32_t *d_count,
                             uint32_t *d_result, const char *who, hipStream_t s) {
  const size_t each_bytes = each ? (size_t)n * sizeof(skx_each_t) : 0, filt_bytes = filt ? (size_t)n * sizeof(skx_filt_each_t) : 0;
  const size_t tags_at = sizeof(skx_ctl_t) + each_bytes + filt_bytes, bytes = tags_at + (size_t)n * sizeof(uint32_t);
  skx_batch_t bt;
  const int rc = skx_batch_begin(fx, bytes, &bt);
  if (rc) return rc;
  char *h = (char *)bt.h;
  if (ctl) skx_ctl_pack(ctl, (skx_ctl_t *)h);
  else memset(h, 0, sizeof(skx_ctl_t));
  if (each) skx_each_pack(each, n, perm, (skx_each_t *)(h + sizeof(skx_ctl_t)));
  if (filt) skx_filt_pack(filt, n, perm, (skx_filt_each_t *)(h + sizeof(skx_ctl_t) + each_bytes));
  memcpy(h + tags_at, tags, (size_t)n * sizeof(uint32_t));
  const char *src = (const char *)skx_batch_send(&bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)skx_launch_ctl_owned_each_filter((const skx_ctl_t *)src, each ? (const skx_each_t *)(src + sizeof(skx_ctl_t)) : NULL,
                                                                    filt ? (const skx_filt_each_t *)(src + sizeof(skx_ctl_t) + each_bytes) : NULL,
                                                                    d_voices, (const uint32_t *)(src + tags_at), fx->d_owner, n, d_count,
                                                                    fx->n_voices, fx->d_ro, d_result, s);
  return skx_batch_end(&bt, e, who, s);
}

static int owned_each_call(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const skred_fx_ctl_each_t *each, const skred_fx_filter_each_t *filt,
                           int with_filter, const int32_t *d_voices, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                           uint32_t *d_result, const char *who, void *stream) {
  if (!d_voices) return fail(SKRED_E_BAD_ARG, "%s: no list", who);
  int rc = owned_each_check(fx, ctl, each, filt, with_filter, tags, n, 0, who);
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_owner_ensure(fx))) return rc;
  return owned_each_launch(fx, ctl, each, filt, NULL, d_voices, tags, n, d_count_or_null, d_result, who, (hipStream_t)stream);
}

static int tags_each_call(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const skred_fx_ctl_each_t *each, const skred_fx_filter_each_t *filt,
                          int with_filter, int first, int count, const uint32_t *tags, int n, uint32_t *d_result, const char *who, void *stream) {
  int rc = owned_each_check(fx, ctl, each, filt, with_filter, tags, n, SKRED_OWNER_UNIQUE, who);
  if (rc) return rc;
  if ((rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, who))) return rc;
  if (n == 0) return SKRED_OK;
  /* the tags travel sorted (the find pass searches them), and each[k] and filt[k] stay with tags[k]: entry j of the list is the voice
   * of the j-th smallest tag, and receives each[perm[j]] and filt[perm[j]] */
  uint32_t sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  (void)sk_owner_pack(tags, n, sorted, perm);
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_owner_ensure(fx))) return rc;
  if ((rc = skred_fxbank_find_owned(fx, first, count, sorted, n, fx->d_owner_found, stream))) return rc;
  /* entry j is the lowest voice that carries sorted[j], or -1: the guard holds on every entry that is a voice */
  return owned_each_launch(fx, ctl, each, filt, perm, fx->d_owner_found, sorted, n, NULL, d_result, who, (hipStream_t)stream);
}

int skred_fxbank_ctl_owned_each(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const skred_fx_ctl_each_t *each, const int32_t *d_voices,
                                const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  return owned_each_call(fx, ctl, each, NULL, 0, d_voices, tags, n, d_count_or_null, d_result, "fx ctl_owned_each", stream);
}

int skred_fxbank_ctl_tags_each(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const skred_fx_ctl_each_t *each, int first, int count,
                               const uint32_t *tags, int n, uint32_t *d_result, void *stream) {
  return tags_each_call(fx, ctl, each, NULL, 0, first, count, tags, n, d_result, "fx ctl_tags_each", stream);
}

/* ---- C. per-entry filter coefficients ---- */

int skred_fxbank_ctl_owned_each_filter(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const skred_fx_ctl_each_t *each,
                                       const skred_fx_filter_each_t *filt, const int32_t *d_voices, const uint32_t *tags, int n,
                                       const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  return owned_each_call(fx, ctl, each, filt, 1, d_voices, tags, n, d_count_or_null, d_result, "fx ctl_owned_each_filter", stream);
}

int skred_fxbank_ctl_tags_each_filter(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const skred_fx_ctl_each_t *each,
                                      const skred_fx_filter_each_t *filt, int first, int count, const uint32_t *tags, int n, uint32_t *d_result,
                                      void *stream) {
  return tags_each_call(fx, ctl, each, filt, 1, first, count, tags, n, d_result, "fx ctl_tags_each_filter", stream);
}
