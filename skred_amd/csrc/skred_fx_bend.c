/*
 * skred_fx_bend.c -- the pitch wheel of the fixed-point bank: bends that return to the key's bits and compose with glides, two words
 * per voice beside the owner, pedal and glide arrays (include/skred_amd_fxpt.h: skred_fx_bend_check, skred_fxbank_bend_match /
 * _bend_owned_each / _bend_tags_each / _bend_clear / _download_bend).
 *
 * The host side of skred_fx_bend_kernels.hip, built like skred_fx_glide.c: the checks (made before anything touches the device, in the
 * order the header documents; the shared ones of skred_bank_checks.c, the tags' and the match's own through the float bank's
 * skred_owner_tags_check and skred_owner_match_check), the bend array, the ratios' and tags' way through the batch path
 * (skred_fx_stage.c), the launches.  The two per-note calls ship their ratios and tags in batches; the channel wheel's ratio is a
 * kernel argument, and it and the clear ship no bytes and so take no slot of the ring.  Nothing here waits for the device except the
 * download and the allocation of the array by the first call that bends.  The hook that clears a re-tagged voice's words is in
 * skred_fx_owner.c (skx_owner_tag_launch); the glide launches of skred_fx_glide.c take the array once it exists.
 *
 * Out of scope: the drop-in mode, deferred items and pattern steps.
 */
#include <stddef.h>
#include <string.h>

#include "skred_launch.h"
#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

_Static_assert(sizeof(skx_bend_t) == 8 && sizeof(skx_bend_t) == sizeof(sk_bend_t) && (int)SKX_BEND_KEY == (int)SK_BEND_KEY &&
               (int)SKX_BEND_RATIO == (int)SK_BEND_RATIO,
               "one 8-byte load per voice; the float bank's clear kernel serves the array");
_Static_assert(SKX_BEND_ONE == SKRED_FX_BEND_ONE, "the centre travels as it is");

static int bend_check(const uint32_t *ratios_q24, int n, const char *who) {
  if (!ratios_q24) return fail(SKRED_E_BAD_ARG, "%s: no ratios", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  for (int k = 0; k < n; k++)
    if (!ratios_q24[k]) return fail(SKRED_E_BAD_ARG, "%s: ratio %d is 0 (%u is the centre)", who, k, SKRED_FX_BEND_ONE);
  return SKRED_OK;
}

int skred_fx_bend_check(const uint32_t *ratios_q24, int n) { return bend_check(ratios_q24, n, "fx bend_check"); }

void skx_bend_pack(const uint32_t *ratios_q24, int n, const uint32_t *perm, uint32_t *out) {
  for (int j = 0; j < n; j++) out[j] = ratios_q24[perm ? perm[j] : (uint32_t)j];
}

/* the array beside the glide array, allocated and zeroed by the first call that bends (the owner array first, when no owner call came
 * before) */
static int skx_bend_ensure(skred_fxbank_t *fx) {
  if (fx->d_bend) return SKRED_OK;
  const int rc = skx_owner_ensure(fx);
  if (rc) return rc;
  return sk_side_alloc((void **)&fx->d_bend, (size_t)fx->n_voices * sizeof(skx_bend_t), "fx bend array");
}

void skx_bend_free(skred_fxbank_t *fx) {
  if (fx->d_bend) (void)hipFree(fx->d_bend);
  fx->d_bend = NULL;
}

/* the bank, then the tags, then n, then the ratios: skred_fxbank_glide_owned's order */
static int each_check(const skred_fxbank_t *fx, const uint32_t *ratios_q24, const uint32_t *tags, int n, uint32_t tag_flags, const char *who) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  int rc = skred_owner_tags_check(tags, n, tag_flags);
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, who))) return rc;
  return bend_check(ratios_q24, n, who);
}

int skred_fxbank_bend_match(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, uint32_t ratio_q24, uint32_t *d_result,
                            void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx bend_match: no bank");
  if (!m) return fail(SKRED_E_BAD_ARG, "fx bend_match: no match");
  int rc = bend_check(&ratio_q24, 1, "fx bend_match");
  if (rc) return rc;
  if ((rc = skred_owner_match_check(m))) return rc;
  if ((rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, "fx bend_match"))) return rc;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_bend_ensure(fx))) return rc;
  const hipError_t e = (hipError_t)skx_launch_bend_match(fx->d_bend, ratio_q24, first, count, fx->d_owner, m->value, m->mask, fx->d_ro[SKX_OSC],
                                                         d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx bend_match launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_bend_owned_each(skred_fxbank_t *fx, const uint32_t *ratios_q24, const int32_t *d_voices, const uint32_t *tags, int n,
                                 const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  if (!d_voices) return fail(SKRED_E_BAD_ARG, "fx bend_owned_each: no list");
  int rc = each_check(fx, ratios_q24, tags, n, 0, "fx bend_owned_each");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_bend_ensure(fx))) return rc;
  /* the n ratios and the n tags in one staging slot: one kernel reads both */
  const size_t words = (size_t)n * sizeof(uint32_t), bytes = 2 * words;
  skx_batch_t bt;
  if ((rc = skx_batch_begin(fx, bytes, &bt))) return rc;
  char *h = (char *)bt.h;
  skx_bend_pack(ratios_q24, n, NULL, (uint32_t *)h);
  memcpy(h + words, tags, words);
  const char *src = (const char *)skx_batch_send(&bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)skx_launch_bend_each(fx->d_bend, (const uint32_t *)src, d_voices, (const uint32_t *)(src + words), fx->d_owner,
                                                        n, d_count_or_null, fx->n_voices, fx->d_ro[SKX_OSC], d_result, s);
  return skx_batch_end(&bt, e, "fx bend_owned_each", s);
}

int skred_fxbank_bend_tags_each(skred_fxbank_t *fx, const uint32_t *ratios_q24, int first, int count, const uint32_t *tags, int n,
                                uint32_t *d_result, void *stream) {
  int rc = each_check(fx, ratios_q24, tags, n, SKRED_OWNER_UNIQUE, "fx bend_tags_each");
  if (rc) return rc;
  if ((rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, "fx bend_tags_each"))) return rc;
  if (n == 0) return SKRED_OK;
  /* the tags travel sorted (the find pass searches them), and ratios[k] stays with tags[k]: entry j of the list is the voice of the
   * j-th smallest tag, and receives ratios[perm[j]] */
  uint32_t sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  (void)sk_owner_pack(tags, n, sorted, perm);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_bend_ensure(fx))) return rc;
  skx_batch_t find, ent;
  hipError_t e = hipSuccess;
  /* the find pass's slot: sorted | the identity | sorted again, the third of which the bend kernel reads as its tags */
  if ((rc = skx_owner_find_launch(fx, first, count, sorted, n, 1, fx->d_owner_found, s, &find, &e))) return rc;
  const size_t bytes = (size_t)n * sizeof(uint32_t);
  if ((rc = skx_batch_begin(fx, bytes, &ent))) {
    (void)skx_batch_end(&find, hipSuccess, "fx bend_tags_each", s);
    return rc;
  }
  skx_bend_pack(ratios_q24, n, perm, (uint32_t *)ent.h);
  const uint32_t *src = (const uint32_t *)skx_batch_send(&ent, bytes, s);
  /* entry j is the lowest voice that carries sorted[j], or -1: the guard holds on every entry that is a voice */
  if (src && e == hipSuccess)
    e = (hipError_t)skx_launch_bend_each(fx->d_bend, src, fx->d_owner_found, (const uint32_t *)find.sl->d + 2 * (size_t)n, fx->d_owner, n, NULL,
                                         fx->n_voices, fx->d_ro[SKX_OSC], d_result, s);
  rc = skx_batch_end(&ent, e, "fx bend_tags_each", s);
  const int rc_find = skx_batch_end(&find, hipSuccess, "fx bend_tags_each", s);
  if (!src) return SKRED_E_NO_DEVICE;
  return rc ? rc : rc_find;
}

int skred_fxbank_bend_clear(skred_fxbank_t *fx, int first, int count, int snap, void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx bend_clear: no bank");
  const int rc = sk_check_window(fx->n_voices, first, count, "fx bend_clear");
  if (rc) return rc;
  if (count == 0 || !fx->d_bend) return SKRED_OK;          /* (no voice was ever bent: every word is 0 already) */
  HIP_TRY(hipSetDevice(fx->device));
  const hipError_t e = (hipError_t)skx_launch_bend_range_clear(fx->d_bend, fx->d_ro[SKX_OSC], first, count, snap != 0, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx bend_clear launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_download_bend(skred_fxbank_t *fx, uint32_t *host_u32x2, int first, int count) {
  if (!fx || !host_u32x2 || count < 0) return fail(SKRED_E_BAD_ARG, "fx download_bend: bad arguments");
  return sk_side_download(fx->d_bend, sizeof(skx_bend_t), fx->device, fx->n_voices, host_u32x2, first, count, "fx download_bend");
}
