/*
 * skred_bank_fenv.c -- filter envelope: per-note cutoff contours that follow the gate, eight words per voice beside the cutoff array
 * (include/skred_amd.h: skred_fenv_check, skred_bank_fenv_match / _fenv_owned_each / _fenv_tags_each / _download_fenv).
 *
 * The host side of skred_fenv_kernels.hip, on the pieces of skred_bank_checks.c and skred_bank_stage.c, on the owner array and find
 * pass of skred_bank_owner.c and on the cutoff array of skred_bank_cutoff.c: the checks (made before anything touches the device, in
 * the order the header documents), the records' and tags' way through the batch path, the launches.  Nothing here waits for the
 * device except the download and the allocation of the arrays by the first record call.  The contour is stepped by
 * skred_bank_cutoff_advance (skred_bank_cutoff.c hands the array to the launch), ended by the cutoff calls and by the hook in
 * skred_bank_owner.c (sk_owner_tag_launch) that clears a re-tagged slot's words.  The calls tell the bank nothing: they store finite
 * coefficient words only, and FILTER lists nobody.
 *
 * Out of scope: the drop-in mode, deferred items and pattern steps.
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(sizeof(skred_fenv_t) == sizeof(sk_fenv_each_t) && sizeof(skred_fenv_t) == 32 && offsetof(skred_fenv_t, set) == 4 * SK_FENV_E_SET &&
               offsetof(skred_fenv_t, start) == 4 * SK_FENV_E_START && offsetof(skred_fenv_t, peak) == 4 * SK_FENV_E_PEAK &&
               offsetof(skred_fenv_t, sustain) == 4 * SK_FENV_E_SUSTAIN && offsetof(skred_fenv_t, end) == 4 * SK_FENV_E_END &&
               offsetof(skred_fenv_t, rate_attack) == 4 * SK_FENV_E_RATE_ATTACK && offsetof(skred_fenv_t, rate_decay) == 4 * SK_FENV_E_RATE_DECAY &&
               offsetof(skred_fenv_t, rate_release) == 4 * SK_FENV_E_RATE_RELEASE, "the device's record must be skred_fenv_t word for word");
_Static_assert(SK_FENV_ABS == SKRED_FENV_ABS && SK_FENV_REL == SKRED_FENV_REL && SK_FENV_START == SKRED_FENV_START, "the envelope bits travel as they are");
_Static_assert(sizeof(sk_fenv_t) == 32 && sizeof(sk_fenv_t) == sizeof(sk_cut_t), "two 16-byte loads per voice");

static int in_box(float x, float lo, float hi) { return isfinite(x) && x >= lo && x <= hi; }

static int mask_check(uint64_t mask, int K, const char *what, const char *who) {
  if (!mask || (K < 64 && (mask >> K))) return fail(SKRED_E_BAD_ARG, "%s: %s = 0x%llx (not 0, bits below K = %d)", who, what, (unsigned long long)mask, K);
  return SKRED_OK;
}

/* the header's order: the array and n, K, the two masks, (n_voices >= 0: the range), the records, filter_mask inside voice_mask */
static int fenv_check(const skred_fenv_t *rec, int n, int K, uint64_t voice_mask, uint64_t filter_mask, int n_voices, int first, int count,
                      const char *who) {
  if (!rec) return fail(SKRED_E_BAD_ARG, "%s: no records", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  int rc = sk_check_slot_shape(K, voice_mask, "voice_mask", who);
  if (rc) return rc;
  if ((rc = mask_check(filter_mask, K, "filter_mask", who))) return rc;
  if (n_voices >= 0 && (rc = sk_check_slot_range(n_voices, first, count, K, 0, who))) return rc;
  for (int k = 0; k < n; k++) {
    const skred_fenv_t *e = &rec[k];
    const uint32_t how = e->set & (SKRED_FENV_ABS | SKRED_FENV_REL);
    const int start = (e->set & SKRED_FENV_START) != 0;
    const float level[4] = { e->start, e->peak, e->sustain, e->end }, rate[3] = { e->rate_attack, e->rate_decay, e->rate_release };
    if (e->set & ~(uint32_t)SK_FENV_ALL) return fail(SKRED_E_BAD_ARG, "%s: record %d: unknown bits in set = 0x%x", who, k, e->set);
    if (how != SKRED_FENV_ABS && how != SKRED_FENV_REL)
      return fail(SKRED_E_BAD_ARG, "%s: record %d: set = 0x%x (exactly one of SKRED_FENV_ABS and SKRED_FENV_REL)", who, k, e->set);
    if (!start && !(e->start == 0.0f))
      return fail(SKRED_E_BAD_ARG, "%s: record %d: start = %g without SKRED_FENV_START (must be 0)", who, k, (double)e->start);
    for (int j = start ? 0 : 1; j < 4; j++)
      if (!isfinite(level[j])) return fail(SKRED_E_BAD_ARG, "%s: record %d: level %d is %g", who, k, j, (double)level[j]);
    for (int j = 0; j < 3; j++)
      if (!isfinite(rate[j])) return fail(SKRED_E_BAD_ARG, "%s: record %d: rate %d is %g", who, k, j, (double)rate[j]);
    for (int j = start ? 0 : 1; j < 4; j++) {
      if (how == SKRED_FENV_ABS && !in_box(level[j], SKRED_CUTOFF_W_MIN, SKRED_CUTOFF_W_MAX))
        return fail(SKRED_E_RANGE, "%s: record %d: level %d = %g outside the box", who, k, j, (double)level[j]);
      if (how == SKRED_FENV_REL && !(level[j] > 0.0f)) return fail(SKRED_E_RANGE, "%s: record %d: a relative level %d of %g (above 0)", who, k, j, (double)level[j]);
    }
    for (int j = 0; j < 3; j++)
      if (!in_box(rate[j], SKRED_CUTOFF_RATE_MIN, SKRED_CUTOFF_RATE_MAX))
        return fail(SKRED_E_RANGE, "%s: record %d: rate %d = %g outside the box", who, k, j, (double)rate[j]);
    for (int j = 0; j < 3; j++)
      if (rate[j] == 1.0f) return fail(SKRED_E_BAD_ARG, "%s: record %d: rate %d is 1 (a stage must move)", who, k, j);
  }
  if (filter_mask & ~voice_mask) return fail(SKRED_E_BAD_ARG, "%s: filter_mask = 0x%llx has bits outside voice_mask = 0x%llx", who,
                                             (unsigned long long)filter_mask, (unsigned long long)voice_mask);
  return SKRED_OK;
}

int skred_fenv_check(const skred_fenv_t *rec, int n, int slot_voices, uint64_t voice_mask, uint64_t filter_mask) {
  return fenv_check(rec, n, slot_voices, voice_mask, filter_mask, -1, 0, 0, "fenv_check");
}

/* The checked records as they travel: out[j] = rec[perm[j]] (perm NULL: j), word for word.  Pure host */
void sk_fenv_pack(const skred_fenv_t *rec, int n, const uint32_t *perm, sk_fenv_each_t *out) {
  for (int j = 0; j < n; j++) memcpy(out[j].w, &rec[perm ? perm[j] : (uint32_t)j], sizeof(sk_fenv_each_t));
}

/* the array, allocated and zeroed by the first record call (the cutoff and owner arrays first, when they do not exist yet) */
static int fenv_ensure(skred_bank_t *b) {
  if (b->d_fenv) return SKRED_OK;
  const int rc = sk_cutoff_ensure(b);
  if (rc) return rc;
  return sk_side_alloc((void **)&b->d_fenv, (size_t)b->n_voices * sizeof(sk_fenv_t), "filter-envelope array");
}

void sk_fenv_free(skred_bank_t *b) {
  if (b->d_fenv) (void)hipFree(b->d_fenv);
  b->d_fenv = NULL;
}

/* the pointers and n, K and the mask, (ranged: the range), the records, then the tags, then the list's length */
static int each_check(const skred_bank_t *b, const skred_fenv_t *recs, int K, uint64_t filter_mask, const uint32_t *tags, int n, uint32_t tag_flags,
                      int ranged, int first, int count, const char *who) {
  if (!b) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  if (!tags) return fail(SKRED_E_BAD_ARG, "%s: no tags", who);
  int rc = fenv_check(recs, n, K, sk_all_lanes(K), filter_mask, ranged ? b->n_voices : -1, first, count, who);
  if (rc) return rc;
  for (int k = 0; k < n; k++)
    if (!tags[k]) return fail(SKRED_E_BAD_ARG, "%s: tag %d is 0 (0 means nobody)", who, k);
  if ((rc = skred_owner_tags_check(tags, n, tag_flags))) return rc;     /* UNIQUE: n > SKRED_OWNER_MAX_TAGS, a tag twice */
  return sk_check_list_n(n, who);
}

/* the n records (recs[perm[j]]; perm NULL: as they stand) and the n tags in one staging slot: one kernel reads both */
static int each_launch(skred_bank_t *b, const skred_fenv_t *recs, const uint32_t *perm, int K, uint64_t filter_mask, const int32_t *d_slots,
                       const uint32_t *tags, int n, const uint32_t *d_count, uint32_t *d_result, const char *who, hipStream_t s) {
  const size_t rec_bytes = (size_t)n * sizeof(sk_fenv_each_t), bytes = rec_bytes + (size_t)n * sizeof(uint32_t);
  sk_batch_t bt;
  int rc = sk_batch_begin(b, bytes, s, &bt);
  if (rc) return rc;
  char *h = (char *)bt.h;
  sk_fenv_pack(recs, n, perm, (sk_fenv_each_t *)h);
  memcpy(h + rec_bytes, tags, (size_t)n * sizeof(uint32_t));
  const char *src = (const char *)sk_batch_send(b, &bt, bytes, 0, s);   /* (every byte is read by one workgroup) */
  if (!src) return SKRED_E_NO_DEVICE;
  const sk_cut_planes_t p = sk_cutoff_planes(b);
  const hipError_t e = (hipError_t)sk_launch_fenv_each(b->d_fenv, b->d_cut, (const sk_fenv_each_t *)src, K, filter_mask, d_slots,
                                                       (const uint32_t *)(src + rec_bytes), b->d_owner, n, d_count, b->n_voices, &p, d_result,
                                                       bt.cnt, bt.done, bt.seq, s);
  return sk_batch_end(&bt, e, who, s);                    /* (FILTER lists nobody: the planner's reports stand) */
}

int skred_bank_fenv_match(skred_bank_t *b, int first, int count, int slot_voices, uint64_t filter_mask, const skred_owner_match_t *m,
                          const skred_fenv_t *rec, uint32_t *d_result, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "fenv_match: no bank");
  if (!m) return fail(SKRED_E_BAD_ARG, "fenv_match: no match");
  int rc = fenv_check(rec, 1, slot_voices, sk_all_lanes(slot_voices), filter_mask, b->n_voices, first, count, "fenv_match");
  if (rc) return rc;
  if ((rc = skred_owner_match_check(m))) return rc;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = fenv_ensure(b))) return rc;
  sk_fenv_each_t r;
  sk_fenv_pack(rec, 1, NULL, &r);
  const sk_cut_planes_t p = sk_cutoff_planes(b);
  const hipError_t e = (hipError_t)sk_launch_fenv_match(b->d_fenv, b->d_cut, &r, slot_voices, filter_mask, first, count, b->d_owner, m->value,
                                                        m->mask, &p, d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fenv_match launch -> %s", hipGetErrorString(e));
  return SKRED_OK;                                         /* (finite coefficients only: the planner's reports stand) */
}

int skred_bank_fenv_owned_each(skred_bank_t *b, const skred_fenv_t *recs, int slot_voices, uint64_t filter_mask, const int32_t *d_slots,
                               const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  if (!b || !d_slots) return fail(SKRED_E_BAD_ARG, "fenv_owned_each: no bank or no list");
  int rc = each_check(b, recs, slot_voices, filter_mask, tags, n, 0, 0, 0, 0, "fenv_owned_each");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = fenv_ensure(b))) return rc;
  return each_launch(b, recs, NULL, slot_voices, filter_mask, d_slots, tags, n, d_count_or_null, d_result, "fenv_owned_each", (hipStream_t)stream);
}

int skred_bank_fenv_tags_each(skred_bank_t *b, const skred_fenv_t *recs, int first, int count, int slot_voices, uint64_t filter_mask,
                              const uint32_t *tags, int n, uint32_t *d_result, void *stream) {
  int rc = each_check(b, recs, slot_voices, filter_mask, tags, n, SKRED_OWNER_UNIQUE, 1, first, count, "fenv_tags_each");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  /* the tags travel sorted (the find pass searches them), and recs[k] stays with tags[k]: entry j of the list is the slot of the
   * j-th smallest tag, and receives recs[perm[j]] */
  uint32_t sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  (void)sk_owner_pack(tags, n, sorted, perm);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = fenv_ensure(b))) return rc;
  if ((rc = sk_owner_find_launch(b, first, count, slot_voices, sorted, n, b->d_owner_slots, s))) return rc;
  /* entry j is the lowest slot that carries sorted[j], or -1: the guard holds on every entry that is a slot */
  return each_launch(b, recs, perm, slot_voices, filter_mask, b->d_owner_slots, sorted, n, NULL, d_result, "fenv_tags_each", s);
}

int skred_bank_download_fenv(skred_bank_t *b, uint32_t *host_u32x8, int first, int count) {
  if (!b || !host_u32x8 || count < 0) return fail(SKRED_E_BAD_ARG, "download_fenv: bad arguments");
  return sk_side_download(b->d_fenv, sizeof(sk_fenv_t), b->device, b->n_voices, host_u32x8, first, count, "download_fenv");
}
