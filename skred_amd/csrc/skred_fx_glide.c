/*
 * skred_fx_glide.c -- portamento on the fixed-point bank: pitch glides that advance and land on the device, four words per voice beside
 * the owner and pedal arrays (include/skred_amd_fxpt.h: skred_fx_glide_check, skred_fxbank_glide_owned / _glide_tags / _glide_advance /
 * _glide_stop / _download_glide).
 *
 * The host side of skred_fx_glide_kernels.hip, built like skred_fx_pedal.c: the checks (made before anything touches the device; the
 * shared ones of skred_bank_checks.c, the tags' own through the float bank's skred_owner_tags_check), the glide array, the entries'
 * and tags' way through the batch path (skred_fx_stage.c), the launches.  The two starting calls ship their entries and tags in
 * batches; the advance and the stop ship no bytes and so take no slot of the ring.  Nothing here waits for the device except the
 * download and the allocation of the array by the first call that starts a glide.  The hook that clears a re-tagged voice's words is in
 * skred_fx_owner.c (skx_owner_tag_launch).  Every glide launch takes the bank's pitch-wheel array (skred_fx_bend.c; NULL on a bank that
 * never bent, and then the kernels are the ones they were).
 *
 * Out of scope: the drop-in mode, deferred items, pattern steps and per-frame glides.
 */
#include <stddef.h>
#include <string.h>

#include "skred_launch.h"
#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

_Static_assert(sizeof(skred_fx_glide_t) == sizeof(skx_glide_each_t) && sizeof(skred_fx_glide_t) == 32 &&
               offsetof(skred_fx_glide_t, set) == 4 * SKX_GLIDE_E_SET && offsetof(skred_fx_glide_t, up_q32) == 4 * SKX_GLIDE_E_UP &&
               offsetof(skred_fx_glide_t, down_q32) == 4 * SKX_GLIDE_E_DOWN && offsetof(skred_fx_glide_t, scale_q16) == 4 * SKX_GLIDE_E_SCALE &&
               offsetof(skred_fx_glide_t, target_inc) == 4 * SKX_GLIDE_E_TARGET_INC && offsetof(skred_fx_glide_t, reserved) == 20,
               "the device's per-entry record must be skred_fx_glide_t word for word");
_Static_assert(SKX_GLIDE_FROM_SCALE == SKRED_FX_GLIDE_FROM_SCALE && SKX_GLIDE_TO_SCALE == SKRED_FX_GLIDE_TO_SCALE &&
               SKX_GLIDE_TO_INC == SKRED_FX_GLIDE_TO_INC, "the glide bits travel as they are");
_Static_assert(sizeof(skx_glide_t) == 16 && sizeof(skx_glide_t) == sizeof(sk_glide_t), "one 16-byte load per voice; the float bank's clear kernel serves the array");

static int glide_check(const skred_fx_glide_t *glide, int n, const char *who) {
  if (!glide) return fail(SKRED_E_BAD_ARG, "%s: no entries", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  for (int k = 0; k < n; k++) {
    const skred_fx_glide_t *e = &glide[k];
    if (e->set != SKRED_FX_GLIDE_FROM_SCALE && e->set != SKRED_FX_GLIDE_TO_SCALE && e->set != SKRED_FX_GLIDE_TO_INC)
      return fail(SKRED_E_BAD_ARG, "%s: entry %d: set = 0x%x (exactly one of SKRED_FX_GLIDE_FROM_SCALE, _TO_SCALE and _TO_INC)", who, k, e->set);
    if (e->reserved[0] || e->reserved[1] || e->reserved[2]) return fail(SKRED_E_BAD_ARG, "%s: entry %d: the reserved words must be 0", who, k);
    if (!e->up_q32 || !e->down_q32)
      return fail(SKRED_E_BAD_ARG, "%s: entry %d: up_q32 = %u, down_q32 = %u (both above 0)", who, k, e->up_q32, e->down_q32);
    if (e->set == SKRED_FX_GLIDE_TO_INC) {
      if (!e->target_inc) return fail(SKRED_E_BAD_ARG, "%s: entry %d: target_inc = 0 (a voice without pitch is no target)", who, k);
    } else if (!e->scale_q16) {
      return fail(SKRED_E_BAD_ARG, "%s: entry %d: scale_q16 = 0 (65536 is 1.0)", who, k);
    }
  }
  return SKRED_OK;
}

int skred_fx_glide_check(const skred_fx_glide_t *glide, int n) { return glide_check(glide, n, "fx glide_check"); }

void skx_glide_pack(const skred_fx_glide_t *glide, int n, const uint32_t *perm, skx_glide_each_t *out) {
  memset(out, 0, (size_t)n * sizeof(skx_glide_each_t));
  for (int j = 0; j < n; j++) memcpy(out[j].w, &glide[perm ? perm[j] : (uint32_t)j], 5 * sizeof(uint32_t));
}

/* the array beside the owner array, allocated and zeroed by the first call that starts a glide (the owner array first, when no owner
 * call came before) */
static int skx_glide_ensure(skred_fxbank_t *fx) {
  if (fx->d_glide) return SKRED_OK;
  const int rc = skx_owner_ensure(fx);
  if (rc) return rc;
  return sk_side_alloc((void **)&fx->d_glide, (size_t)fx->n_voices * sizeof(skx_glide_t), "fx glide array");
}

void skx_glide_free(skred_fxbank_t *fx) {
  if (fx->d_glide) (void)hipFree(fx->d_glide);
  fx->d_glide = NULL;
}

static int start_check(const skred_fxbank_t *fx, const skred_fx_glide_t *glide, const uint32_t *tags, int n, uint32_t tag_flags,
                       const char *who) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  int rc = skred_owner_tags_check(tags, n, tag_flags);
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, who))) return rc;
  return glide_check(glide, n, who);
}

int skred_fxbank_glide_owned(skred_fxbank_t *fx, const skred_fx_glide_t *glide, const int32_t *d_voices, const uint32_t *tags, int n,
                             const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  if (!d_voices) return fail(SKRED_E_BAD_ARG, "fx glide_owned: no list");
  int rc = start_check(fx, glide, tags, n, 0, "fx glide_owned");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_glide_ensure(fx))) return rc;
  /* the n entries and the n tags in one staging slot: one kernel reads both */
  const size_t each_bytes = (size_t)n * sizeof(skx_glide_each_t), bytes = each_bytes + (size_t)n * sizeof(uint32_t);
  skx_batch_t bt;
  if ((rc = skx_batch_begin(fx, bytes, &bt))) return rc;
  char *h = (char *)bt.h;
  skx_glide_pack(glide, n, NULL, (skx_glide_each_t *)h);
  memcpy(h + each_bytes, tags, (size_t)n * sizeof(uint32_t));
  const char *src = (const char *)skx_batch_send(&bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)skx_launch_glide_start(fx->d_glide, fx->d_bend, (const skx_glide_each_t *)src, d_voices, (const uint32_t *)(src + each_bytes),
                                                          fx->d_owner, n, d_count_or_null, fx->n_voices, fx->d_ro[SKX_OSC], d_result, s);
  return skx_batch_end(&bt, e, "fx glide_owned", s);
}

int skred_fxbank_glide_tags(skred_fxbank_t *fx, const skred_fx_glide_t *glide, int first, int count, const uint32_t *tags, int n,
                            uint32_t *d_result, void *stream) {
  int rc = start_check(fx, glide, tags, n, SKRED_OWNER_UNIQUE, "fx glide_tags");
  if (rc) return rc;
  if ((rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, "fx glide_tags"))) return rc;
  if (n == 0) return SKRED_OK;
  /* the tags travel sorted (the find pass searches them), and glide[k] stays with tags[k]: entry j of the list is the voice of the
   * j-th smallest tag, and receives glide[perm[j]] */
  uint32_t sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  (void)sk_owner_pack(tags, n, sorted, perm);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_glide_ensure(fx))) return rc;
  skx_batch_t find, ent;
  hipError_t e = hipSuccess;
  /* the find pass's slot: sorted | the identity | sorted again, the third of which the start kernel reads as its tags */
  if ((rc = skx_owner_find_launch(fx, first, count, sorted, n, 1, fx->d_owner_found, s, &find, &e))) return rc;
  const size_t bytes = (size_t)n * sizeof(skx_glide_each_t);
  if ((rc = skx_batch_begin(fx, bytes, &ent))) {
    (void)skx_batch_end(&find, hipSuccess, "fx glide_tags", s);
    return rc;
  }
  skx_glide_pack(glide, n, perm, (skx_glide_each_t *)ent.h);
  const skx_glide_each_t *src = (const skx_glide_each_t *)skx_batch_send(&ent, bytes, s);
  /* entry j is the lowest voice that carries sorted[j], or -1: the guard holds on every entry that is a voice */
  if (src && e == hipSuccess)
    e = (hipError_t)skx_launch_glide_start(fx->d_glide, fx->d_bend, src, fx->d_owner_found, (const uint32_t *)find.sl->d + 2 * (size_t)n, fx->d_owner, n,
                                           NULL, fx->n_voices, fx->d_ro[SKX_OSC], d_result, s);
  rc = skx_batch_end(&ent, e, "fx glide_tags", s);
  const int rc_find = skx_batch_end(&find, hipSuccess, "fx glide_tags", s);
  if (!src) return SKRED_E_NO_DEVICE;
  return rc ? rc : rc_find;
}

int skred_fxbank_glide_advance(skred_fxbank_t *fx, int first, int count, int num_frames, uint32_t *d_result, void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx glide_advance: no bank");
  if (num_frames < 1 || num_frames > 65536) return fail(SKRED_E_BAD_ARG, "fx glide_advance: num_frames = %d (1 .. 65536)", num_frames);
  const int rc = sk_check_slot_range(fx->n_voices, first, count, 1, 0, "fx glide_advance");
  if (rc) return rc;
  if (!fx->d_glide) {                                      /* (no glide was ever started: nobody glides, nobody arrives) */
    if (!d_result) return SKRED_OK;
    HIP_TRY(hipSetDevice(fx->device));
    HIP_TRY(hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), (hipStream_t)stream));
    return SKRED_OK;
  }
  HIP_TRY(hipSetDevice(fx->device));
  const hipError_t e = (hipError_t)skx_launch_glide_advance(fx->d_glide, fx->d_bend, fx->d_ro[SKX_OSC], first, count, num_frames, d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx glide_advance launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_glide_stop(skred_fxbank_t *fx, int first, int count, int snap, void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx glide_stop: no bank");
  const int rc = sk_check_window(fx->n_voices, first, count, "fx glide_stop");
  if (rc) return rc;
  if (count == 0 || !fx->d_glide) return SKRED_OK;         /* (no glide was ever started: every word is 0 already) */
  HIP_TRY(hipSetDevice(fx->device));
  const hipError_t e = (hipError_t)skx_launch_glide_stop(fx->d_glide, fx->d_bend, fx->d_ro[SKX_OSC], first, count, snap != 0, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx glide_stop launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_download_glide(skred_fxbank_t *fx, uint32_t *host_u32x4, int first, int count) {
  if (!fx || !host_u32x4 || count < 0) return fail(SKRED_E_BAD_ARG, "fx download_glide: bad arguments");
  return sk_side_download(fx->d_glide, sizeof(skx_glide_t), fx->device, fx->n_voices, host_u32x4, first, count, "fx download_glide");
}
