/*
 * skred_fx_fenv.c -- the filter envelope on the fixed-point bank: per-note cutoff contours that follow the gate, eight words per voice
 * beside the cutoff array (include/skred_amd_fxpt.h: skred_fx_fenv_check, skred_fxbank_fenv_match / _fenv_owned_each / _fenv_tags_each
 * / _download_fenv).
 *
 * The host side of skred_fx_fenv_kernels.hip, built like skred_fx_cutoff.c: the checks (made before anything touches the device, in
 * the order the header documents; the shared ones of skred_bank_checks.c, the tags' and the match's own through the float bank's
 * skred_owner_tags_check and skred_owner_match_check), the fenv array, the records' and tags' way through the batch path
 * (skred_fx_stage.c), the launches.  The channel sweep's record is a kernel argument and takes no slot of the ring.  Nothing here
 * waits for the device except the download and the allocation of the arrays by the first record call.  The contour is stepped by
 * skred_fxbank_cutoff_advance (skred_fx_cutoff.c hands the array to the launch), ended by the cutoff calls and by the hook in
 * skred_fx_owner.c (skx_owner_tag_launch) that clears a re-tagged voice's words.
 *
 * Out of scope: the drop-in mode, deferred items and pattern steps.
 */
#include <stddef.h>
#include <string.h>

#include "skred_launch.h"
#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

_Static_assert(sizeof(skred_fx_fenv_t) == sizeof(skx_fenv_each_t) && sizeof(skred_fx_fenv_t) == 32 &&
               offsetof(skred_fx_fenv_t, set) == 4 * SKX_FENV_E_SET && offsetof(skred_fx_fenv_t, start) == 4 * SKX_FENV_E_START &&
               offsetof(skred_fx_fenv_t, peak) == 4 * SKX_FENV_E_PEAK && offsetof(skred_fx_fenv_t, sustain) == 4 * SKX_FENV_E_SUSTAIN &&
               offsetof(skred_fx_fenv_t, end) == 4 * SKX_FENV_E_END && offsetof(skred_fx_fenv_t, rate_attack_q32) == 4 * SKX_FENV_E_RATE_ATTACK &&
               offsetof(skred_fx_fenv_t, rate_decay_q32) == 4 * SKX_FENV_E_RATE_DECAY &&
               offsetof(skred_fx_fenv_t, rate_release_q32) == 4 * SKX_FENV_E_RATE_RELEASE,
               "the device's record must be skred_fx_fenv_t word for word");
_Static_assert(SKX_FENV_ABS == SKRED_FX_FENV_ABS && SKX_FENV_REL == SKRED_FX_FENV_REL && SKX_FENV_START == SKRED_FX_FENV_START,
               "the envelope bits travel as they are");
_Static_assert(sizeof(skx_fenv_t) == 32 && sizeof(skx_fenv_t) == sizeof(sk_fenv_t) && sizeof(skx_fenv_t) == sizeof(skx_cut_t),
               "two 16-byte loads per voice; the float bank's clear kernel serves the array");
/* the header's words: stage | w_peak | w_sustain | w_end, then rate_attack_q32 | rate_decay_q32 | rate_release_q32 | 0; stages 0 .. 4 */
_Static_assert(SKX_FENV_STAGE == 0 && SKX_FENV_W_PEAK == 1 && SKX_FENV_W_SUSTAIN == 2 && SKX_FENV_W_END == 3 && SKX_FENV_RATE_ATTACK == 4 &&
               SKX_FENV_RATE_DECAY == 5 && SKX_FENV_RATE_RELEASE == 6 && SKX_FENV_RESERVED == 7 && SKX_FENV_WORDS == 8,
               "the SKX_FENV_* words are the header's");
_Static_assert(SKX_FENV_OFF == 0 && SKX_FENV_ATTACK == 1 && SKX_FENV_DECAY == 2 && SKX_FENV_SUSTAIN == 3 && SKX_FENV_RELEASE == 4,
               "the stage values are the header's");
_Static_assert((int)SKX_FENV_STAGE == (int)SK_FENV_STAGE && (int)SKX_FENV_RATE_ATTACK == (int)SK_FENV_RATE_ATTACK &&
               (int)SKX_FENV_WORDS == (int)SK_FENV_WORDS,
               "the array has the float bank's shape");

/* the header's order: the array and n, then record by record */
static int fenv_check(const skred_fx_fenv_t *rec, int n, const char *who) {
  if (!rec) return fail(SKRED_E_BAD_ARG, "%s: no records", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  for (int k = 0; k < n; k++) {
    const skred_fx_fenv_t *e = &rec[k];
    const uint32_t how = e->set & (SKRED_FX_FENV_ABS | SKRED_FX_FENV_REL);
    const int start = (e->set & SKRED_FX_FENV_START) != 0;
    const uint32_t level[4] = { e->start, e->peak, e->sustain, e->end };
    if (e->set & ~(uint32_t)SKX_FENV_ALL) return fail(SKRED_E_BAD_ARG, "%s: record %d: unknown bits in set = 0x%x", who, k, e->set);
    if (how != SKRED_FX_FENV_ABS && how != SKRED_FX_FENV_REL)
      return fail(SKRED_E_BAD_ARG, "%s: record %d: set = 0x%x (exactly one of SKRED_FX_FENV_ABS and SKRED_FX_FENV_REL)", who, k, e->set);
    if (!start && e->start) return fail(SKRED_E_BAD_ARG, "%s: record %d: start = %u without SKRED_FX_FENV_START (must be 0)", who, k, e->start);
    if (how == SKRED_FX_FENV_ABS)
      for (int j = start ? 0 : 1; j < 4; j++)
        if (level[j] < SKRED_FX_CUTOFF_W_MIN || level[j] > SKRED_FX_CUTOFF_W_MAX)
          return fail(SKRED_E_RANGE, "%s: record %d: level %d = %u outside the box", who, k, j, level[j]);
    if (how == SKRED_FX_FENV_REL)
      for (int j = start ? 0 : 1; j < 4; j++)
        if (!level[j]) return fail(SKRED_E_RANGE, "%s: record %d: a relative level %d of 0", who, k, j);
    if (!e->rate_attack_q32 || !e->rate_decay_q32 || !e->rate_release_q32)
      return fail(SKRED_E_BAD_ARG, "%s: record %d: rates %u, %u, %u (all above 0: a stage must move)", who, k, e->rate_attack_q32, e->rate_decay_q32,
                  e->rate_release_q32);
  }
  return SKRED_OK;
}

int skred_fx_fenv_check(const skred_fx_fenv_t *recs, int n) { return fenv_check(recs, n, "fx fenv_check"); }

/* The checked records as they travel: out[j] = rec[perm[j]] (perm NULL: j), word for word.  Pure host */
void skx_fenv_pack(const skred_fx_fenv_t *rec, int n, const uint32_t *perm, skx_fenv_each_t *out) {
  for (int j = 0; j < n; j++) memcpy(out[j].w, &rec[perm ? perm[j] : (uint32_t)j], sizeof(skx_fenv_each_t));
}

/* the array beside the cutoff array, allocated and zeroed by the first record call (the owner and cutoff arrays first, when they do
 * not exist yet) */
static int fenv_ensure(skred_fxbank_t *fx) {
  if (fx->d_fenv) return SKRED_OK;
  const int rc = skx_cutoff_ensure(fx);
  if (rc) return rc;
  return sk_side_alloc((void **)&fx->d_fenv, (size_t)fx->n_voices * sizeof(skx_fenv_t), "fx filter-envelope array");
}

void skx_fenv_free(skred_fxbank_t *fx) {
  if (fx->d_fenv) (void)hipFree(fx->d_fenv);
  fx->d_fenv = NULL;
}

/* the bank, then the tags, then n, then the records: skred_fxbank_cutoff_owned_each's order */
static int each_check(const skred_fxbank_t *fx, const skred_fx_fenv_t *recs, const uint32_t *tags, int n, uint32_t tag_flags, const char *who) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  int rc = skred_owner_tags_check(tags, n, tag_flags);
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, who))) return rc;
  return fenv_check(recs, n, who);
}

int skred_fxbank_fenv_match(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, const skred_fx_fenv_t *rec,
                            uint32_t *d_result, void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx fenv_match: no bank");
  if (!m) return fail(SKRED_E_BAD_ARG, "fx fenv_match: no match");
  int rc = fenv_check(rec, 1, "fx fenv_match");
  if (rc) return rc;
  if ((rc = skred_owner_match_check(m))) return rc;
  if ((rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, "fx fenv_match"))) return rc;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = fenv_ensure(fx))) return rc;
  skx_fenv_each_t r;
  skx_fenv_pack(rec, 1, NULL, &r);
  const hipError_t e = (hipError_t)skx_launch_fenv_match(fx->d_fenv, fx->d_cut, &r, first, count, fx->d_owner, m->value, m->mask, fx->d_ro, d_result,
                                                         (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx fenv_match launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_fenv_owned_each(skred_fxbank_t *fx, const skred_fx_fenv_t *recs, const int32_t *d_voices, const uint32_t *tags, int n,
                                 const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  if (!d_voices) return fail(SKRED_E_BAD_ARG, "fx fenv_owned_each: no list");
  int rc = each_check(fx, recs, tags, n, 0, "fx fenv_owned_each");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = fenv_ensure(fx))) return rc;
  /* the n records and the n tags in one staging slot: one kernel reads both */
  const size_t rec_bytes = (size_t)n * sizeof(skx_fenv_each_t), bytes = rec_bytes + (size_t)n * sizeof(uint32_t);
  skx_batch_t bt;
  if ((rc = skx_batch_begin(fx, bytes, &bt))) return rc;
  char *h = (char *)bt.h;
  skx_fenv_pack(recs, n, NULL, (skx_fenv_each_t *)h);
  memcpy(h + rec_bytes, tags, (size_t)n * sizeof(uint32_t));
  const char *src = (const char *)skx_batch_send(&bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)skx_launch_fenv_each(fx->d_fenv, fx->d_cut, (const skx_fenv_each_t *)src, d_voices,
                                                        (const uint32_t *)(src + rec_bytes), fx->d_owner, n, d_count_or_null, fx->n_voices,
                                                        fx->d_ro, d_result, s);
  return skx_batch_end(&bt, e, "fx fenv_owned_each", s);
}

int skred_fxbank_fenv_tags_each(skred_fxbank_t *fx, const skred_fx_fenv_t *recs, int first, int count, const uint32_t *tags, int n,
                                uint32_t *d_result, void *stream) {
  int rc = each_check(fx, recs, tags, n, SKRED_OWNER_UNIQUE, "fx fenv_tags_each");
  if (rc) return rc;
  if ((rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, "fx fenv_tags_each"))) return rc;
  if (n == 0) return SKRED_OK;
  /* the tags travel sorted (the find pass searches them), and recs[k] stays with tags[k]: entry j of the list is the voice of the
   * j-th smallest tag, and receives recs[perm[j]] */
  uint32_t sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  (void)sk_owner_pack(tags, n, sorted, perm);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = fenv_ensure(fx))) return rc;
  skx_batch_t find, ent;
  hipError_t e = hipSuccess;
  /* the find pass's slot: sorted | the identity | sorted again, the third of which the record kernel reads as its tags */
  if ((rc = skx_owner_find_launch(fx, first, count, sorted, n, 1, fx->d_owner_found, s, &find, &e))) return rc;
  const size_t bytes = (size_t)n * sizeof(skx_fenv_each_t);
  if ((rc = skx_batch_begin(fx, bytes, &ent))) {
    (void)skx_batch_end(&find, hipSuccess, "fx fenv_tags_each", s);
    return rc;
  }
  skx_fenv_pack(recs, n, perm, (skx_fenv_each_t *)ent.h);
  const skx_fenv_each_t *src = (const skx_fenv_each_t *)skx_batch_send(&ent, bytes, s);
  /* entry j is the lowest voice that carries sorted[j], or -1: the guard holds on every entry that is a voice */
  if (src && e == hipSuccess)
    e = (hipError_t)skx_launch_fenv_each(fx->d_fenv, fx->d_cut, src, fx->d_owner_found, (const uint32_t *)find.sl->d + 2 * (size_t)n, fx->d_owner, n,
                                         NULL, fx->n_voices, fx->d_ro, d_result, s);
  rc = skx_batch_end(&ent, e, "fx fenv_tags_each", s);
  const int rc_find = skx_batch_end(&find, hipSuccess, "fx fenv_tags_each", s);
  if (!src) return SKRED_E_NO_DEVICE;
  return rc ? rc : rc_find;
}

int skred_fxbank_download_fenv(skred_fxbank_t *fx, uint32_t *host_u32x8, int first, int count) {
  if (!fx || !host_u32x8 || count < 0) return fail(SKRED_E_BAD_ARG, "fx download_fenv: bad arguments");
  return sk_side_download(fx->d_fenv, sizeof(skx_fenv_t), fx->device, fx->n_voices, host_u32x8, first, count, "fx download_fenv");
}
