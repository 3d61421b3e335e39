/*
 * skred_bank_cutoff.c -- filter cutoff on the device: key-tracked cutoffs that glide and land, eight words per voice beside the bend
 * array (include/skred_amd.h: skred_filter_coeffs_w, skred_cutoff_check, skred_bank_cutoff_match / _cutoff_owned_each /
 * _cutoff_tags_each / _cutoff_advance / _cutoff_stop / _download_cutoff).
 *
 * The host side of skred_cutoff_kernels.hip, on the pieces of skred_bank_checks.c and skred_bank_stage.c and on the owner array and
 * find pass of skred_bank_owner.c: the checks (made before anything touches the device, in the order the header documents), the
 * records' and tags' way through the batch path, the launches; and skred_filter_coeffs_w, the host twin of skred_cutoff_common.hpp
 * (the Makefile builds this file with -ffp-contract=off: every operation below is rounded on its own).  Nothing here waits for the
 * device except the download and the allocation of the array by the first call that sets a cutoff.  The cutoff array is no part of
 * the bank the planner knows, and the calls tell the bank nothing: they store finite coefficient words only, and FILTER lists nobody
 * (skred_bank_expr.c, section C).  The hook that clears a re-tagged slot's words is in skred_bank_owner.c (sk_owner_tag_launch).
 * On a bank that has a filter-envelope array (skred_bank_fenv.c) the launches receive it: a cutoff call ends the contours of the
 * voices it sets, starts or stops, and the advance pass steps the others.
 *
 * Out of scope: the fixed-point bank, the drop-in mode, deferred items and pattern steps.
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(sizeof(skred_cutoff_t) == sizeof(sk_cut_each_t) && sizeof(skred_cutoff_t) == 32 && offsetof(skred_cutoff_t, set) == 4 * SK_CUT_E_SET &&
               offsetof(skred_cutoff_t, value) == 4 * SK_CUT_E_VALUE && offsetof(skred_cutoff_t, q) == 4 * SK_CUT_E_Q &&
               offsetof(skred_cutoff_t, mode) == 4 * SK_CUT_E_MODE && offsetof(skred_cutoff_t, rate_up) == 4 * SK_CUT_E_RATE_UP &&
               offsetof(skred_cutoff_t, rate_down) == 4 * SK_CUT_E_RATE_DOWN && offsetof(skred_cutoff_t, reserved) == 24,
               "the device's record must be skred_cutoff_t word for word");
_Static_assert(SK_CUTOFF_ABS == SKRED_CUTOFF_ABS && SK_CUTOFF_TRACK == SKRED_CUTOFF_TRACK && SK_CUTOFF_GLIDE == SKRED_CUTOFF_GLIDE &&
               SK_CUTOFF_Q == SKRED_CUTOFF_Q && SK_CUTOFF_MODE == SKRED_CUTOFF_MODE, "the cutoff bits travel as they are");
_Static_assert(sizeof(sk_cut_t) == 32, "two 16-byte loads per voice");
_Static_assert(SK_CUTOFF_W_MIN == SKRED_CUTOFF_W_MIN && SK_CUTOFF_W_MAX == SKRED_CUTOFF_W_MAX && SK_CUTOFF_HALF_PI == SKRED_CUTOFF_HALF_PI &&
               SK_CUTOFF_PI_HI == SKRED_CUTOFF_PI_HI && SK_CUTOFF_PI_LO == SKRED_CUTOFF_PI_LO && SK_CUTOFF_S1 == SKRED_CUTOFF_S1 &&
               SK_CUTOFF_S2 == SKRED_CUTOFF_S2 && SK_CUTOFF_S3 == SKRED_CUTOFF_S3 && SK_CUTOFF_S4 == SKRED_CUTOFF_S4 &&
               SK_CUTOFF_C1 == SKRED_CUTOFF_C1 && SK_CUTOFF_C2 == SKRED_CUTOFF_C2 && SK_CUTOFF_C3 == SKRED_CUTOFF_C3 &&
               SK_CUTOFF_C4 == SKRED_CUTOFF_C4 && SK_CUTOFF_C5 == SKRED_CUTOFF_C5, "the device's constants are the header's");

static int in_box(float x, float lo, float hi) { return isfinite(x) && x >= lo && x <= hi; }

/* THE ARITHMETIC of the header, operation by operation (skred_cutoff_common.hpp: sk_cutoff_sincos, sk_cutoff_coeffs) */
int skred_filter_coeffs_w(int mode, float w, float q, float out5[5]) {
  if (!out5) return fail(SKRED_E_BAD_ARG, "filter_coeffs_w: nowhere to put the coefficients");
  if (mode < 0 || mode > 5) return fail(SKRED_E_BAD_ARG, "filter_coeffs_w: mode = %d (0 .. 5)", mode);
  if (mode == 0) return 1;                                    /* bypassed: nothing computed */
  if (!in_box(w, SKRED_CUTOFF_W_MIN, SKRED_CUTOFF_W_MAX)) return fail(SKRED_E_RANGE, "filter_coeffs_w: w = %g outside the box", (double)w);
  if (!in_box(q, SKRED_CUTOFF_Q_MIN, SKRED_CUTOFF_Q_MAX)) return fail(SKRED_E_RANGE, "filter_coeffs_w: q = %g outside the box", (double)q);
  const int upper = w > SKRED_CUTOFF_HALF_PI;
  float r = w;
  if (upper) { r = SKRED_CUTOFF_PI_HI - w; r = r + SKRED_CUTOFF_PI_LO; }
  const float z = r * r;
  float p = SKRED_CUTOFF_S4;
  p = p * z; p = p + SKRED_CUTOFF_S3;
  p = p * z; p = p + SKRED_CUTOFF_S2;
  p = p * z; p = p + SKRED_CUTOFF_S1;
  float t = r * z;
  t = t * p;
  const float sn = r + t;
  float c = SKRED_CUTOFF_C5;
  c = c * z; c = c + SKRED_CUTOFF_C4;
  c = c * z; c = c + SKRED_CUTOFF_C3;
  c = c * z; c = c + SKRED_CUTOFF_C2;
  c = c * z; c = c + SKRED_CUTOFF_C1;
  c = z * c;
  c = 1.0f + c;
  const float cs = upper ? -c : c;
  /* skred_filter_coeffs (skred_bank_expr.c) from here on */
  const float alpha = sn / (2.0f * q);
  const float a0 = 1.0f + alpha;
  float b0, b1, b2;
  switch (mode) {
    case 2:  b0 = (1.0f + cs) / 2.0f; b1 = -(1.0f + cs); b2 = (1.0f + cs) / 2.0f; break;
    case 3:  b0 = alpha; b1 = 0.0f; b2 = -alpha; break;
    case 4:  b0 = 1.0f; b1 = -2.0f * cs; b2 = 1.0f; break;
    case 5:  b0 = 1.0f - alpha; b1 = -2.0f * cs; b2 = 1.0f + alpha; break;
    default: b0 = (1.0f - cs) / 2.0f; b1 = 1.0f - cs; b2 = (1.0f - cs) / 2.0f; break;
  }
  out5[0] = b0 / a0; out5[1] = b1 / a0; out5[2] = b2 / a0;
  out5[3] = (-2.0f * cs) / a0;
  out5[4] = (1.0f - alpha) / a0;
  return SKRED_OK;
}

static int mask_check(uint64_t mask, int K, const char *what, const char *who) {
  if (!mask || (K < 64 && (mask >> K))) return fail(SKRED_E_BAD_ARG, "%s: %s = 0x%llx (not 0, bits below K = %d)", who, what, (unsigned long long)mask, K);
  return SKRED_OK;
}

/* the header's order: the array and n, K, the two masks, (n_voices >= 0: the range), the records, filter_mask inside voice_mask */
static int cut_check(const skred_cutoff_t *rec, int n, int K, uint64_t voice_mask, uint64_t filter_mask, int first_time, int n_voices, int first,
                     int count, const char *who) {
  if (!rec) return fail(SKRED_E_BAD_ARG, "%s: no records", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  int rc = sk_check_slot_shape(K, voice_mask, "voice_mask", who);
  if (rc) return rc;
  if ((rc = mask_check(filter_mask, K, "filter_mask", who))) return rc;
  if (n_voices >= 0 && (rc = sk_check_slot_range(n_voices, first, count, K, 0, who))) return rc;
  for (int k = 0; k < n; k++) {
    const skred_cutoff_t *e = &rec[k];
    const uint32_t how = e->set & (SKRED_CUTOFF_ABS | SKRED_CUTOFF_TRACK);
    if (e->set & ~(uint32_t)SK_CUTOFF_ALL) return fail(SKRED_E_BAD_ARG, "%s: record %d: unknown bits in set = 0x%x", who, k, e->set);
    if (how != SKRED_CUTOFF_ABS && how != SKRED_CUTOFF_TRACK)
      return fail(SKRED_E_BAD_ARG, "%s: record %d: set = 0x%x (exactly one of SKRED_CUTOFF_ABS and SKRED_CUTOFF_TRACK)", who, k, e->set);
    if (first_time && (e->set & (SKRED_CUTOFF_Q | SKRED_CUTOFF_MODE)) != (SKRED_CUTOFF_Q | SKRED_CUTOFF_MODE))
      return fail(SKRED_E_BAD_ARG, "%s: record %d: a voice's first cutoff names SKRED_CUTOFF_Q and SKRED_CUTOFF_MODE", who, k);
    if (e->reserved[0] || e->reserved[1]) return fail(SKRED_E_BAD_ARG, "%s: record %d: the reserved words must be 0", who, k);
    const int glide = (e->set & SKRED_CUTOFF_GLIDE) != 0;
    if (!isfinite(e->value) || ((e->set & SKRED_CUTOFF_Q) && !isfinite(e->q)) || (glide && (!isfinite(e->rate_up) || !isfinite(e->rate_down))))
      return fail(SKRED_E_BAD_ARG, "%s: record %d holds %g %g %g %g", who, k, (double)e->value, (double)e->q, (double)e->rate_up, (double)e->rate_down);
    if ((e->set & SKRED_CUTOFF_Q) && !in_box(e->q, SKRED_CUTOFF_Q_MIN, SKRED_CUTOFF_Q_MAX))
      return fail(SKRED_E_RANGE, "%s: record %d: q = %g outside the box", who, k, (double)e->q);
    if (how == SKRED_CUTOFF_ABS && !in_box(e->value, SKRED_CUTOFF_W_MIN, SKRED_CUTOFF_W_MAX))
      return fail(SKRED_E_RANGE, "%s: record %d: value = %g outside the box", who, k, (double)e->value);
    if (how == SKRED_CUTOFF_TRACK && !(e->value > 0.0f)) return fail(SKRED_E_RANGE, "%s: record %d: a tracking value of %g (above 0)", who, k, (double)e->value);
    if ((e->set & SKRED_CUTOFF_MODE) && (e->mode < 1 || e->mode > 5)) return fail(SKRED_E_RANGE, "%s: record %d: mode = %u (1 .. 5)", who, k, e->mode);
    if (glide) {
      if (!in_box(e->rate_up, SKRED_CUTOFF_RATE_MIN, SKRED_CUTOFF_RATE_MAX) || !in_box(e->rate_down, SKRED_CUTOFF_RATE_MIN, SKRED_CUTOFF_RATE_MAX))
        return fail(SKRED_E_RANGE, "%s: record %d: rates %g, %g outside the box", who, k, (double)e->rate_up, (double)e->rate_down);
      if (!(e->rate_up > 1.0f)) return fail(SKRED_E_BAD_ARG, "%s: record %d: rate_up = %g (above 1)", who, k, (double)e->rate_up);
      if (!(e->rate_down < 1.0f)) return fail(SKRED_E_BAD_ARG, "%s: record %d: rate_down = %g (below 1)", who, k, (double)e->rate_down);
    }
  }
  if (filter_mask & ~voice_mask) return fail(SKRED_E_BAD_ARG, "%s: filter_mask = 0x%llx has bits outside voice_mask = 0x%llx", who,
                                             (unsigned long long)filter_mask, (unsigned long long)voice_mask);
  return SKRED_OK;
}

int skred_cutoff_check(const skred_cutoff_t *rec, int n, int slot_voices, uint64_t voice_mask, uint64_t filter_mask, int first_time) {
  return cut_check(rec, n, slot_voices, voice_mask, filter_mask, first_time, -1, 0, 0, "cutoff_check");
}

/* every lane of a slot: what the entry points hold filter_mask against */
uint64_t sk_all_lanes(int K) { return K >= 1 && K < 64 ? (1ull << K) - 1ull : ~0ull; }

/* The checked records as they travel: out[j] = rec[perm[j]] (perm NULL: j), set and value as they stand, q, mode and the rates where
 * named, the rest zero.  Pure host */
void sk_cutoff_pack(const skred_cutoff_t *rec, int n, const uint32_t *perm, sk_cut_each_t *out) {
  memset(out, 0, (size_t)n * sizeof(sk_cut_each_t));
  for (int j = 0; j < n; j++) {
    const skred_cutoff_t *e = &rec[perm ? perm[j] : (uint32_t)j];
    uint32_t *w = out[j].w;
    w[SK_CUT_E_SET] = e->set;
    memcpy(&w[SK_CUT_E_VALUE], &e->value, 4);
    if (e->set & SKRED_CUTOFF_Q) memcpy(&w[SK_CUT_E_Q], &e->q, 4);
    if (e->set & SKRED_CUTOFF_MODE) w[SK_CUT_E_MODE] = e->mode;
    if (e->set & SKRED_CUTOFF_GLIDE) { memcpy(&w[SK_CUT_E_RATE_UP], &e->rate_up, 4); memcpy(&w[SK_CUT_E_RATE_DOWN], &e->rate_down, 4); }
  }
}

/* the array, allocated and zeroed by the first call that sets a cutoff (the owner array first, when no owner call came before) */
int sk_cutoff_ensure(skred_bank_t *b) {
  if (b->d_cut) return SKRED_OK;
  const int rc = sk_owner_ensure(b);
  if (rc) return rc;
  return sk_side_alloc((void **)&b->d_cut, (size_t)b->n_voices * sizeof(sk_cut_t), "cutoff array");
}

void sk_cutoff_free(skred_bank_t *b) {
  if (b->d_cut) (void)hipFree(b->d_cut);
  b->d_cut = NULL;
}

sk_cut_planes_t sk_cutoff_planes(const skred_bank_t *b) {
  const sk_cut_planes_t p = { b->d_ro[SKP_OSC], b->d_ro[SKP_GAIN], b->d_ro[SKP_FILT] };
  return p;
}

/* the pointers and n, K and the mask, (ranged: the range), the records, then the tags, then the list's length */
static int each_check(const skred_bank_t *b, const skred_cutoff_t *recs, int K, uint64_t filter_mask, const uint32_t *tags, int n, uint32_t tag_flags,
                      int ranged, int first, int count, const char *who) {
  if (!b) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  if (!tags) return fail(SKRED_E_BAD_ARG, "%s: no tags", who);
  int rc = cut_check(recs, n, K, sk_all_lanes(K), filter_mask, 0, ranged ? b->n_voices : -1, first, count, who);
  if (rc) return rc;
  for (int k = 0; k < n; k++)
    if (!tags[k]) return fail(SKRED_E_BAD_ARG, "%s: tag %d is 0 (0 means nobody)", who, k);
  if ((rc = skred_owner_tags_check(tags, n, tag_flags))) return rc;     /* UNIQUE: n > SKRED_OWNER_MAX_TAGS, a tag twice */
  return sk_check_list_n(n, who);
}

/* the n records (recs[perm[j]]; perm NULL: as they stand) and the n tags in one staging slot: one kernel reads both */
static int each_launch(skred_bank_t *b, const skred_cutoff_t *recs, const uint32_t *perm, int K, uint64_t filter_mask, const int32_t *d_slots,
                       const uint32_t *tags, int n, const uint32_t *d_count, uint32_t *d_result, const char *who, hipStream_t s) {
  const size_t rec_bytes = (size_t)n * sizeof(sk_cut_each_t), bytes = rec_bytes + (size_t)n * sizeof(uint32_t);
  sk_batch_t bt;
  int rc = sk_batch_begin(b, bytes, s, &bt);
  if (rc) return rc;
  char *h = (char *)bt.h;
  sk_cutoff_pack(recs, n, perm, (sk_cut_each_t *)h);
  memcpy(h + rec_bytes, tags, (size_t)n * sizeof(uint32_t));
  const char *src = (const char *)sk_batch_send(b, &bt, bytes, 0, s);   /* (every byte is read by one workgroup) */
  if (!src) return SKRED_E_NO_DEVICE;
  const sk_cut_planes_t p = sk_cutoff_planes(b);
  const hipError_t e = (hipError_t)sk_launch_cutoff_each(b->d_cut, b->d_bend, b->d_fenv, (const sk_cut_each_t *)src, K, filter_mask, d_slots,
                                                         (const uint32_t *)(src + rec_bytes), b->d_owner, n, d_count, b->n_voices, &p, d_result,
                                                         bt.cnt, bt.done, bt.seq, s);
  return sk_batch_end(&bt, e, who, s);                    /* (FILTER lists nobody: the planner's reports stand) */
}

int skred_bank_cutoff_match(skred_bank_t *b, int first, int count, int slot_voices, uint64_t filter_mask, const skred_owner_match_t *m,
                            const skred_cutoff_t *rec, uint32_t *d_result, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "cutoff_match: no bank");
  if (!m) return fail(SKRED_E_BAD_ARG, "cutoff_match: no match");
  int rc = cut_check(rec, 1, slot_voices, sk_all_lanes(slot_voices), filter_mask, 0, b->n_voices, first, count, "cutoff_match");
  if (rc) return rc;
  if ((rc = skred_owner_match_check(m))) return rc;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_cutoff_ensure(b))) return rc;
  sk_cut_each_t r;
  sk_cutoff_pack(rec, 1, NULL, &r);
  const sk_cut_planes_t p = sk_cutoff_planes(b);
  const hipError_t e = (hipError_t)sk_launch_cutoff_match(b->d_cut, b->d_bend, b->d_fenv, &r, slot_voices, filter_mask, first, count, b->d_owner,
                                                          m->value, m->mask, &p, d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "cutoff_match launch -> %s", hipGetErrorString(e));
  return SKRED_OK;                                         /* (finite coefficients only: the planner's reports stand) */
}

int skred_bank_cutoff_owned_each(skred_bank_t *b, const skred_cutoff_t *recs, int slot_voices, uint64_t filter_mask, const int32_t *d_slots,
                                 const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  if (!b || !d_slots) return fail(SKRED_E_BAD_ARG, "cutoff_owned_each: no bank or no list");
  int rc = each_check(b, recs, slot_voices, filter_mask, tags, n, 0, 0, 0, 0, "cutoff_owned_each");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_cutoff_ensure(b))) return rc;
  return each_launch(b, recs, NULL, slot_voices, filter_mask, d_slots, tags, n, d_count_or_null, d_result, "cutoff_owned_each", (hipStream_t)stream);
}

int skred_bank_cutoff_tags_each(skred_bank_t *b, const skred_cutoff_t *recs, int first, int count, int slot_voices, uint64_t filter_mask,
                                const uint32_t *tags, int n, uint32_t *d_result, void *stream) {
  int rc = each_check(b, recs, slot_voices, filter_mask, tags, n, SKRED_OWNER_UNIQUE, 1, first, count, "cutoff_tags_each");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  /* the tags travel sorted (the find pass searches them), and recs[k] stays with tags[k]: entry j of the list is the slot of the
   * j-th smallest tag, and receives recs[perm[j]] */
  uint32_t sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  (void)sk_owner_pack(tags, n, sorted, perm);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_cutoff_ensure(b))) return rc;
  if ((rc = sk_owner_find_launch(b, first, count, slot_voices, sorted, n, b->d_owner_slots, s))) return rc;
  /* entry j is the lowest slot that carries sorted[j], or -1: the guard holds on every entry that is a slot */
  return each_launch(b, recs, perm, slot_voices, filter_mask, b->d_owner_slots, sorted, n, NULL, d_result, "cutoff_tags_each", s);
}

int skred_bank_cutoff_advance(skred_bank_t *b, int first, int count, int num_frames, uint32_t *d_result, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "cutoff_advance: no bank");
  if (num_frames < 1 || num_frames > 65536) return fail(SKRED_E_BAD_ARG, "cutoff_advance: num_frames = %d (1 .. 65536)", num_frames);
  const int rc = sk_check_slot_range(b->n_voices, first, count, 1, 0, "cutoff_advance");
  if (rc) return rc;
  if (!b->d_cut) {                                         /* (no cutoff was ever set: nobody moves, nobody arrives) */
    if (!d_result) return SKRED_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), (hipStream_t)stream));
    return SKRED_OK;
  }
  HIP_TRY(hipSetDevice(b->device));
  const sk_cut_planes_t p = sk_cutoff_planes(b);
  const hipError_t e = (hipError_t)sk_launch_cutoff_advance(b->d_cut, b->d_fenv, b->d_ro[SKP_ENV_S], &p, first, count, num_frames, d_result,
                                                            (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "cutoff_advance launch -> %s", hipGetErrorString(e));
  return SKRED_OK;                                         /* (finite coefficients only: the planner's reports stand) */
}

int skred_bank_cutoff_stop(skred_bank_t *b, int first, int count, int snap, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "cutoff_stop: no bank");
  const int rc = sk_check_window(b->n_voices, first, count, "cutoff_stop");
  if (rc) return rc;
  if (count == 0 || !b->d_cut) return SKRED_OK;            /* (no cutoff was ever set: nothing moves) */
  HIP_TRY(hipSetDevice(b->device));
  const sk_cut_planes_t p = sk_cutoff_planes(b);
  const hipError_t e = (hipError_t)sk_launch_cutoff_stop(b->d_cut, b->d_fenv, &p, first, count, snap != 0, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "cutoff_stop launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_bank_download_cutoff(skred_bank_t *b, uint32_t *host_u32x8, int first, int count) {
  if (!b || !host_u32x8 || count < 0) return fail(SKRED_E_BAD_ARG, "download_cutoff: bad arguments");
  return sk_side_download(b->d_cut, sizeof(sk_cut_t), b->device, b->n_voices, host_u32x8, first, count, "download_cutoff");
}
