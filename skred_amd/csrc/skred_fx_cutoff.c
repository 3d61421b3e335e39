/*
 * skred_fx_cutoff.c -- filter cutoff on the fixed-point bank: key-tracked cutoffs that glide and land, eight words per voice beside
 * the owner, pedal, glide and bend arrays (include/skred_amd_fxpt.h: skred_fx_filter_coeffs_w, skred_fx_cutoff_check,
 * skred_fxbank_cutoff_match / _cutoff_owned_each / _cutoff_tags_each / _cutoff_advance / _cutoff_stop / _download_cutoff).
 *
 * The host side of skred_fx_cutoff_kernels.hip, built like skred_fx_bend.c: the checks (made before anything touches the device, in
 * the order the header documents; the shared ones of skred_bank_checks.c, the tags' and the match's own through the float bank's
 * skred_owner_tags_check and skred_owner_match_check), the cutoff array, the records' and tags' way through the batch path
 * (skred_fx_stage.c), the launches; and skred_fx_filter_coeffs_w, the host twin of skred_fx_cutoff_common.hpp -- integers only, so no
 * compiler flag can move a bit of it.  The channel sweep's record is a kernel argument; it, the advance and the stop ship no bytes
 * and so take no slot of the ring.  Nothing here waits for the device except the download and the allocation of the array by the
 * first call that sets a cutoff.  The hook that clears a re-tagged voice's words is in skred_fx_owner.c (skx_owner_tag_launch).
 * Every launch here takes the bank's filter-envelope array (skred_fx_fenv.c; NULL on a bank that has none): a cutoff record or a stop
 * ends the contours it touches, and the advance steps them.
 *
 * Out of scope: the drop-in mode, deferred items and pattern steps.
 */
#include <stddef.h>
#include <string.h>

#include "skred_launch.h"
#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

_Static_assert(sizeof(skred_fx_cutoff_t) == sizeof(skx_cut_each_t) && sizeof(skred_fx_cutoff_t) == 32 &&
               offsetof(skred_fx_cutoff_t, set) == 4 * SKX_CUT_E_SET && offsetof(skred_fx_cutoff_t, value) == 4 * SKX_CUT_E_VALUE &&
               offsetof(skred_fx_cutoff_t, q_q16) == 4 * SKX_CUT_E_Q && offsetof(skred_fx_cutoff_t, mode) == 4 * SKX_CUT_E_MODE &&
               offsetof(skred_fx_cutoff_t, up_q32) == 4 * SKX_CUT_E_UP && offsetof(skred_fx_cutoff_t, down_q32) == 4 * SKX_CUT_E_DOWN &&
               offsetof(skred_fx_cutoff_t, reserved) == 24,
               "the device's record must be skred_fx_cutoff_t word for word");
_Static_assert(SKX_CUTOFF_ABS == SKRED_FX_CUTOFF_ABS && SKX_CUTOFF_TRACK == SKRED_FX_CUTOFF_TRACK && SKX_CUTOFF_GLIDE == SKRED_FX_CUTOFF_GLIDE &&
               SKX_CUTOFF_Q == SKRED_FX_CUTOFF_Q && SKX_CUTOFF_MODE == SKRED_FX_CUTOFF_MODE, "the cutoff bits travel as they are");
_Static_assert(sizeof(skx_cut_t) == 32 && sizeof(skx_cut_t) == sizeof(sk_cut_t), "two 16-byte loads per voice; the float bank's clear kernel serves the array");
_Static_assert(SKX_CUTOFF_W_MIN == SKRED_FX_CUTOFF_W_MIN && SKX_CUTOFF_W_MAX == SKRED_FX_CUTOFF_W_MAX && SKX_CUTOFF_PI_Q29 == SKRED_FX_CUTOFF_PI_Q29 &&
               SKX_CUTOFF_HALF_PI_Q29 == SKRED_FX_CUTOFF_HALF_PI_Q29 && SKX_CUTOFF_S1 == SKRED_FX_CUTOFF_S1 && SKX_CUTOFF_S2 == SKRED_FX_CUTOFF_S2 &&
               SKX_CUTOFF_S3 == SKRED_FX_CUTOFF_S3 && SKX_CUTOFF_S4 == SKRED_FX_CUTOFF_S4 && SKX_CUTOFF_S5 == SKRED_FX_CUTOFF_S5 &&
               SKX_CUTOFF_C2 == SKRED_FX_CUTOFF_C2 && SKX_CUTOFF_C3 == SKRED_FX_CUTOFF_C3 && SKX_CUTOFF_C4 == SKRED_FX_CUTOFF_C4 &&
               SKX_CUTOFF_C5 == SKRED_FX_CUTOFF_C5 && SKX_CUTOFF_C6 == SKRED_FX_CUTOFF_C6, "the device's constants are the header's");
_Static_assert((-1ll >> 1) == -1ll, "the rounding of signed products is stated on an arithmetic shift");

/* (p * z + 2^31) >> 32 on an arithmetic shift: |p| < 2^31, z < 2^32 */
static int64_t cut_mul(int64_t p, uint32_t z) { return (p * (int64_t)z + (1ll << 31)) >> 32; }

/* round(|num| * 2^(s + 2) / a0), ties away from zero, the sign put back, clamped to int32 (skx_cut_quot) */
static int32_t cut_quot(int64_t num, uint64_t a0, int s) {
  const uint64_t n = (uint64_t)(num < 0 ? -num : num) << s;
  const uint64_t qa = n / a0, ra = n - qa * a0;
  const uint64_t mag = (qa << 2) + ((ra << 2) + (a0 >> 1)) / a0;
  if (num < 0) return mag > 0x80000000ull ? INT32_MIN : (int32_t)-(int64_t)mag;
  return mag > 0x7fffffffull ? INT32_MAX : (int32_t)mag;
}

/* THE ARITHMETIC of the header, step by step (skred_fx_cutoff_common.hpp: skx_cutoff_coeffs) */
int skred_fx_filter_coeffs_w(int mode, uint32_t w, uint32_t q, int32_t out5[5]) {
  if (!out5) return fail(SKRED_E_BAD_ARG, "fx filter_coeffs_w: nowhere to put the coefficients");
  if (mode < 0 || mode > 5) return fail(SKRED_E_BAD_ARG, "fx filter_coeffs_w: mode = %d (0 .. 5)", mode);
  if (mode == 0) return 1;                                    /* bypassed: nothing computed */
  if (w < SKRED_FX_CUTOFF_W_MIN || w > SKRED_FX_CUTOFF_W_MAX) return fail(SKRED_E_RANGE, "fx filter_coeffs_w: w_q29 = %u outside the box", w);
  if (q < SKRED_FX_CUTOFF_Q_MIN || q > SKRED_FX_CUTOFF_Q_MAX) return fail(SKRED_E_RANGE, "fx filter_coeffs_w: q_q16 = %u outside the box", q);
  const int upper = w > SKRED_FX_CUTOFF_HALF_PI_Q29;
  const uint32_t r = upper ? SKRED_FX_CUTOFF_PI_Q29 - w : w;
  const uint32_t z = (uint32_t)(((uint64_t)r * r + (1ull << 27)) >> 28);
  int64_t p = SKRED_FX_CUTOFF_S5;
  p = cut_mul(p, z) + SKRED_FX_CUTOFF_S4;
  p = cut_mul(p, z) + SKRED_FX_CUTOFF_S3;
  p = cut_mul(p, z) + SKRED_FX_CUTOFF_S2;
  p = cut_mul(p, z) + SKRED_FX_CUTOFF_S1;
  const uint64_t sinc = (uint64_t)((1ll << 31) + cut_mul(p, z));
  const uint64_t rs = (uint64_t)r * sinc;
  int64_t c = SKRED_FX_CUTOFF_C6;
  c = cut_mul(c, z) + SKRED_FX_CUTOFF_C5;
  c = cut_mul(c, z) + SKRED_FX_CUTOFF_C4;
  c = cut_mul(c, z) + SKRED_FX_CUTOFF_C3;
  c = cut_mul(c, z) + SKRED_FX_CUTOFF_C2;
  const int64_t t = cut_mul(c, z);
  const int64_t cosr = (1ll << 31) - (int64_t)z + cut_mul(t, z);
  const int64_t cs = upper ? -cosr : cosr;
  const uint64_t den = (uint64_t)q << 15;
  const uint64_t alpha = (rs + (den >> 1)) / den;
  const uint64_t a0 = (1ull << 30) + alpha;
  const int64_t one = 1ll << 30, one31 = 1ll << 31, ia = (int64_t)alpha;
  int32_t b0, b1, b2;
  switch (mode) {
    case 2:  b0 = cut_quot(one31 + cs, a0, 26); b1 = cut_quot(-(one31 + cs), a0, 27); b2 = b0; break;
    case 3:  b0 = cut_quot(ia, a0, 28); b1 = 0; b2 = cut_quot(-ia, a0, 28); break;
    case 4:  b0 = cut_quot(one, a0, 28); b1 = cut_quot(-cs, a0, 28); b2 = b0; break;
    case 5:  b0 = cut_quot(one - ia, a0, 28); b1 = cut_quot(-cs, a0, 28); b2 = cut_quot((int64_t)a0, a0, 28); break;
    default: b0 = cut_quot(one31 - cs, a0, 26); b1 = cut_quot(one31 - cs, a0, 27); b2 = b0; break;
  }
  out5[0] = b0; out5[1] = b1; out5[2] = b2;
  out5[3] = cut_quot(-cs, a0, 28);
  out5[4] = cut_quot(one - ia, a0, 28);
  return SKRED_OK;
}

/* the header's order: the array and n, then record by record */
static int cut_check(const skred_fx_cutoff_t *rec, int n, int first_time, const char *who) {
  if (!rec) return fail(SKRED_E_BAD_ARG, "%s: no records", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  for (int k = 0; k < n; k++) {
    const skred_fx_cutoff_t *e = &rec[k];
    const uint32_t how = e->set & (SKRED_FX_CUTOFF_ABS | SKRED_FX_CUTOFF_TRACK);
    if (e->set & ~(uint32_t)SKX_CUTOFF_ALL) return fail(SKRED_E_BAD_ARG, "%s: record %d: unknown bits in set = 0x%x", who, k, e->set);
    if (how != SKRED_FX_CUTOFF_ABS && how != SKRED_FX_CUTOFF_TRACK)
      return fail(SKRED_E_BAD_ARG, "%s: record %d: set = 0x%x (exactly one of SKRED_FX_CUTOFF_ABS and SKRED_FX_CUTOFF_TRACK)", who, k, e->set);
    if (first_time && (e->set & (SKRED_FX_CUTOFF_Q | SKRED_FX_CUTOFF_MODE)) != (SKRED_FX_CUTOFF_Q | SKRED_FX_CUTOFF_MODE))
      return fail(SKRED_E_BAD_ARG, "%s: record %d: a voice's first cutoff names SKRED_FX_CUTOFF_Q and SKRED_FX_CUTOFF_MODE", who, k);
    if (e->reserved[0] || e->reserved[1]) return fail(SKRED_E_BAD_ARG, "%s: record %d: the reserved words must be 0", who, k);
    if ((e->set & SKRED_FX_CUTOFF_Q) && (e->q_q16 < SKRED_FX_CUTOFF_Q_MIN || e->q_q16 > SKRED_FX_CUTOFF_Q_MAX))
      return fail(SKRED_E_RANGE, "%s: record %d: q_q16 = %u outside the box", who, k, e->q_q16);
    if (how == SKRED_FX_CUTOFF_ABS && (e->value < SKRED_FX_CUTOFF_W_MIN || e->value > SKRED_FX_CUTOFF_W_MAX))
      return fail(SKRED_E_RANGE, "%s: record %d: value = %u outside the box", who, k, e->value);
    if (how == SKRED_FX_CUTOFF_TRACK && !e->value) return fail(SKRED_E_RANGE, "%s: record %d: a tracking value of 0", who, k);
    if ((e->set & SKRED_FX_CUTOFF_MODE) && (e->mode < 1 || e->mode > 5)) return fail(SKRED_E_RANGE, "%s: record %d: mode = %u (1 .. 5)", who, k, e->mode);
    if ((e->set & SKRED_FX_CUTOFF_GLIDE) && (!e->up_q32 || !e->down_q32))
      return fail(SKRED_E_BAD_ARG, "%s: record %d: up_q32 = %u, down_q32 = %u (both above 0)", who, k, e->up_q32, e->down_q32);
  }
  return SKRED_OK;
}

int skred_fx_cutoff_check(const skred_fx_cutoff_t *rec, int n, int first_time) { return cut_check(rec, n, first_time, "fx cutoff_check"); }

/* The checked records as they travel: out[j] = rec[perm[j]] (perm NULL: j), set and value as they stand, q_q16, mode and the rates where
 * named, the rest zero.  Pure host */
void skx_cutoff_pack(const skred_fx_cutoff_t *rec, int n, const uint32_t *perm, skx_cut_each_t *out) {
  memset(out, 0, (size_t)n * sizeof(skx_cut_each_t));
  for (int j = 0; j < n; j++) {
    const skred_fx_cutoff_t *e = &rec[perm ? perm[j] : (uint32_t)j];
    uint32_t *w = out[j].w;
    w[SKX_CUT_E_SET] = e->set;
    w[SKX_CUT_E_VALUE] = e->value;
    if (e->set & SKRED_FX_CUTOFF_Q) w[SKX_CUT_E_Q] = e->q_q16;
    if (e->set & SKRED_FX_CUTOFF_MODE) w[SKX_CUT_E_MODE] = e->mode;
    if (e->set & SKRED_FX_CUTOFF_GLIDE) { w[SKX_CUT_E_UP] = e->up_q32; w[SKX_CUT_E_DOWN] = e->down_q32; }
  }
}

/* the array beside the bend array, allocated and zeroed by the first call that sets a cutoff (the owner array first, when no owner call
 * came before); skred_fx_fenv.c enters it ahead of its own array */
int skx_cutoff_ensure(skred_fxbank_t *fx) {
  if (fx->d_cut) return SKRED_OK;
  const int rc = skx_owner_ensure(fx);
  if (rc) return rc;
  return sk_side_alloc((void **)&fx->d_cut, (size_t)fx->n_voices * sizeof(skx_cut_t), "fx cutoff array");
}

void skx_cutoff_free(skred_fxbank_t *fx) {
  if (fx->d_cut) (void)hipFree(fx->d_cut);
  fx->d_cut = NULL;
}

/* the bank, then the tags, then n, then the records: skred_fxbank_bend_owned_each's order */
static int each_check(const skred_fxbank_t *fx, const skred_fx_cutoff_t *recs, const uint32_t *tags, int n, uint32_t tag_flags, const char *who) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  int rc = skred_owner_tags_check(tags, n, tag_flags);
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, who))) return rc;
  return cut_check(recs, n, 0, who);
}

int skred_fxbank_cutoff_match(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, const skred_fx_cutoff_t *rec,
                              uint32_t *d_result, void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx cutoff_match: no bank");
  if (!m) return fail(SKRED_E_BAD_ARG, "fx cutoff_match: no match");
  int rc = cut_check(rec, 1, 0, "fx cutoff_match");
  if (rc) return rc;
  if ((rc = skred_owner_match_check(m))) return rc;
  if ((rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, "fx cutoff_match"))) return rc;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_cutoff_ensure(fx))) return rc;
  skx_cut_each_t r;
  skx_cutoff_pack(rec, 1, NULL, &r);
  const hipError_t e = (hipError_t)skx_launch_cutoff_match(fx->d_cut, fx->d_bend, fx->d_fenv, &r, first, count, fx->d_owner, m->value, m->mask, fx->d_ro,
                                                           d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx cutoff_match launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_cutoff_owned_each(skred_fxbank_t *fx, const skred_fx_cutoff_t *recs, const int32_t *d_voices, const uint32_t *tags, int n,
                                   const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  if (!d_voices) return fail(SKRED_E_BAD_ARG, "fx cutoff_owned_each: no list");
  int rc = each_check(fx, recs, tags, n, 0, "fx cutoff_owned_each");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_cutoff_ensure(fx))) return rc;
  /* the n records and the n tags in one staging slot: one kernel reads both */
  const size_t rec_bytes = (size_t)n * sizeof(skx_cut_each_t), bytes = rec_bytes + (size_t)n * sizeof(uint32_t);
  skx_batch_t bt;
  if ((rc = skx_batch_begin(fx, bytes, &bt))) return rc;
  char *h = (char *)bt.h;
  skx_cutoff_pack(recs, n, NULL, (skx_cut_each_t *)h);
  memcpy(h + rec_bytes, tags, (size_t)n * sizeof(uint32_t));
  const char *src = (const char *)skx_batch_send(&bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)skx_launch_cutoff_each(fx->d_cut, fx->d_bend, fx->d_fenv, (const skx_cut_each_t *)src, d_voices,
                                                          (const uint32_t *)(src + rec_bytes), fx->d_owner, n, d_count_or_null, fx->n_voices,
                                                          fx->d_ro, d_result, s);
  return skx_batch_end(&bt, e, "fx cutoff_owned_each", s);
}

int skred_fxbank_cutoff_tags_each(skred_fxbank_t *fx, const skred_fx_cutoff_t *recs, int first, int count, const uint32_t *tags, int n,
                                  uint32_t *d_result, void *stream) {
  int rc = each_check(fx, recs, tags, n, SKRED_OWNER_UNIQUE, "fx cutoff_tags_each");
  if (rc) return rc;
  if ((rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, "fx cutoff_tags_each"))) return rc;
  if (n == 0) return SKRED_OK;
  /* the tags travel sorted (the find pass searches them), and recs[k] stays with tags[k]: entry j of the list is the voice of the
   * j-th smallest tag, and receives recs[perm[j]] */
  uint32_t sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  (void)sk_owner_pack(tags, n, sorted, perm);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_cutoff_ensure(fx))) return rc;
  skx_batch_t find, ent;
  hipError_t e = hipSuccess;
  /* the find pass's slot: sorted | the identity | sorted again, the third of which the record kernel reads as its tags */
  if ((rc = skx_owner_find_launch(fx, first, count, sorted, n, 1, fx->d_owner_found, s, &find, &e))) return rc;
  const size_t bytes = (size_t)n * sizeof(skx_cut_each_t);
  if ((rc = skx_batch_begin(fx, bytes, &ent))) {
    (void)skx_batch_end(&find, hipSuccess, "fx cutoff_tags_each", s);
    return rc;
  }
  skx_cutoff_pack(recs, n, perm, (skx_cut_each_t *)ent.h);
  const skx_cut_each_t *src = (const skx_cut_each_t *)skx_batch_send(&ent, bytes, s);
  /* entry j is the lowest voice that carries sorted[j], or -1: the guard holds on every entry that is a voice */
  if (src && e == hipSuccess)
    e = (hipError_t)skx_launch_cutoff_each(fx->d_cut, fx->d_bend, fx->d_fenv, src, fx->d_owner_found, (const uint32_t *)find.sl->d + 2 * (size_t)n, fx->d_owner,
                                           n, NULL, fx->n_voices, fx->d_ro, d_result, s);
  rc = skx_batch_end(&ent, e, "fx cutoff_tags_each", s);
  const int rc_find = skx_batch_end(&find, hipSuccess, "fx cutoff_tags_each", s);
  if (!src) return SKRED_E_NO_DEVICE;
  return rc ? rc : rc_find;
}

int skred_fxbank_cutoff_advance(skred_fxbank_t *fx, int first, int count, int num_frames, uint32_t *d_result, void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx cutoff_advance: no bank");
  if (num_frames < 1 || num_frames > 65536) return fail(SKRED_E_BAD_ARG, "fx cutoff_advance: num_frames = %d (1 .. 65536)", num_frames);
  const int rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, "fx cutoff_advance");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(fx->device));
  if (!fx->d_cut) {                                          /* (no cutoff was ever set: nobody moves, nobody arrives) */
    if (d_result) HIP_TRY(hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), (hipStream_t)stream));
    return SKRED_OK;
  }
  const hipError_t e = (hipError_t)skx_launch_cutoff_advance(fx->d_cut, fx->d_fenv, fx->d_ro, first, count, num_frames, d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx cutoff_advance launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_cutoff_stop(skred_fxbank_t *fx, int first, int count, int snap, void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx cutoff_stop: no bank");
  const int rc = sk_check_window(fx->n_voices, first, count, "fx cutoff_stop");
  if (rc) return rc;
  if (count == 0 || !fx->d_cut) return SKRED_OK;             /* (no cutoff was ever set: nothing moves) */
  HIP_TRY(hipSetDevice(fx->device));
  const hipError_t e = (hipError_t)skx_launch_cutoff_stop(fx->d_cut, fx->d_fenv, fx->d_ro, first, count, snap != 0, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx cutoff_stop launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_download_cutoff(skred_fxbank_t *fx, uint32_t *host_u32x8, int first, int count) {
  if (!fx || !host_u32x8 || count < 0) return fail(SKRED_E_BAD_ARG, "fx download_cutoff: bad arguments");
  return sk_side_download(fx->d_cut, sizeof(skx_cut_t), fx->device, fx->n_voices, host_u32x8, first, count, "fx download_cutoff");
}
