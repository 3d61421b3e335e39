/*
 * skred_fx_pedal.c -- pedals on the fixed-point bank: note-offs the sustain and sostenuto pedals hold back, remembered per voice on
 * the device (include/skred_amd_fxpt.h: skred_fx_pedal_check, skred_fxbank_stamp_owned_pedal / _release_tags_pedal / _pedal_latch /
 * _pedal_up / _pedal_clear / _download_pedals).
 *
 * The host side of skred_fx_pedal_kernels.hip, built like skred_fx_owner.c: the checks (the float bank's skred_pedal_check at one
 * voice per slot, made before anything touches the device), the pedal array, the tags' way through the batch path
 * (skred_fx_stage.c), the launches.  The two list calls ship their tags in a batch; the two range calls ship no bytes -- the match
 * travels as kernel arguments, as skred_fxbank_stamp_match's does -- and so take no slot of the ring.  Nothing here waits for the
 * device except the download and the allocation of the array by the first call that needs it.  The hook that clears a re-tagged
 * voice's word is in skred_fx_owner.c (skx_owner_tag_launch).
 *
 * Out of scope: the drop-in mode, deferred items and pattern steps.
 */
#include <string.h>

#include "skred_launch.h"
#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

_Static_assert(SK_PEDAL_PENDING == SKRED_PEDAL_PENDING && SK_PEDAL_LATCHED == SKRED_PEDAL_LATCHED, "the pedal bits travel as they are");
_Static_assert(SK_PEDAL_LIFT_SUSTAIN == SKRED_PEDAL_LIFT_SUSTAIN && SK_PEDAL_LIFT_SOSTENUTO == SKRED_PEDAL_LIFT_SOSTENUTO &&
               SK_PEDAL_SUSTAIN_DOWN == SKRED_PEDAL_SUSTAIN_DOWN, "the pedal-up flags travel as they are");

int skred_fx_pedal_check(int call, int n_voices, int first, int count, const skred_owner_match_t *m, uint32_t flags, const uint32_t *tags,
                         int n) {
  return skred_pedal_check(call, n_voices, first, count, 1, 1, m, flags, tags, n);
}

/* the array beside the owner array, allocated and zeroed by the first call that needs it (the owner array first, when no owner call
 * came before) */
static int skx_pedal_ensure(skred_fxbank_t *fx) {
  if (fx->d_pedal) return SKRED_OK;
  const int rc = skx_owner_ensure(fx);
  if (rc) return rc;
  return sk_side_alloc((void **)&fx->d_pedal, (size_t)fx->n_voices * sizeof(uint32_t), "fx pedal array");
}

void skx_pedal_free(skred_fxbank_t *fx) {
  if (fx->d_pedal) (void)hipFree(fx->d_pedal);
  fx->d_pedal = NULL;
}

int skred_fxbank_stamp_owned_pedal(skred_fxbank_t *fx, const int32_t *d_voices, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                                   int hold_all, uint32_t *d_result, void *stream) {
  if (!fx || !d_voices || !d_result) return fail(SKRED_E_BAD_ARG, "fx stamp_owned_pedal: no bank, list or result");
  int rc = skred_fx_pedal_check(SKRED_PEDAL_CALL_STAMP_OWNED, fx->n_voices, 0, 0, NULL, 0, tags, n);
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_pedal_ensure(fx))) return rc;
  const size_t bytes = (size_t)n * sizeof(uint32_t);
  skx_batch_t bt;
  if ((rc = skx_batch_begin(fx, bytes, &bt))) return rc;
  memcpy(bt.h, tags, bytes);
  const uint32_t *src = (const uint32_t *)skx_batch_send(&bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)skx_launch_pedal_stamps(fx->d_owner, fx->d_pedal, d_voices, src, n, d_count_or_null, fx->n_voices, hold_all,
                                                           fx->d_ro[SKX_TIME], fx->d_rw[0], fx->count, d_result, s);
  return skx_batch_end(&bt, e, "fx stamp_owned_pedal", s);
}

int skred_fxbank_release_tags_pedal(skred_fxbank_t *fx, int first, int count, const uint32_t *tags, int n, int hold_all, uint32_t *d_result,
                                    void *stream) {
  if (!fx || !d_result) return fail(SKRED_E_BAD_ARG, "fx release_tags_pedal: no bank or no result");
  int rc = skred_fx_pedal_check(SKRED_PEDAL_CALL_RELEASE_TAGS, fx->n_voices, first, count, NULL, 0, tags, n);
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_pedal_ensure(fx))) return rc;
  skx_batch_t bt;
  hipError_t e = hipSuccess;
  if ((rc = skx_owner_find_launch(fx, first, count, tags, n, 1, fx->d_owner_found, s, &bt, &e))) return rc;
  /* entry k is the lowest voice that carries tags[k], or -1: the guard holds on every entry that is a voice */
  if (e == hipSuccess)
    e = (hipError_t)skx_launch_pedal_stamps(fx->d_owner, fx->d_pedal, fx->d_owner_found, (const uint32_t *)bt.sl->d + 2 * (size_t)n, n, NULL,
                                            fx->n_voices, hold_all, fx->d_ro[SKX_TIME], fx->d_rw[0], fx->count, d_result, s);
  return skx_batch_end(&bt, e, "fx release_tags_pedal", s);
}

int skred_fxbank_pedal_latch(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, uint32_t *d_result, void *stream) {
  if (!fx || !d_result) return fail(SKRED_E_BAD_ARG, "fx pedal_latch: no bank or no result");
  int rc = skred_fx_pedal_check(SKRED_PEDAL_CALL_LATCH, fx->n_voices, first, count, m, 0, NULL, 0);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_pedal_ensure(fx))) return rc;
  const hipError_t e = (hipError_t)skx_launch_pedal_latch(fx->d_owner, fx->d_pedal, m->value, m->mask, first, count, fx->d_ro[SKX_OSC],
                                                          fx->d_ro[SKX_TIME], fx->d_rw[0], d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx pedal_latch launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_pedal_up(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, uint32_t flags, uint32_t *d_result,
                          void *stream) {
  if (!fx || !d_result) return fail(SKRED_E_BAD_ARG, "fx pedal_up: no bank or no result");
  int rc = skred_fx_pedal_check(SKRED_PEDAL_CALL_UP, fx->n_voices, first, count, m, flags, NULL, 0);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_pedal_ensure(fx))) return rc;
  const hipError_t e = (hipError_t)skx_launch_pedal_up(fx->d_owner, fx->d_pedal, m->value, m->mask, first, count, flags, fx->d_ro[SKX_TIME],
                                                       fx->d_rw[0], fx->count, d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx pedal_up launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_pedal_clear(skred_fxbank_t *fx, int first, int count, void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx pedal_clear: no bank");
  return sk_side_clear(fx->d_pedal, sizeof(uint32_t), fx->device, fx->n_voices, first, count, (hipStream_t)stream, "fx pedal_clear");
}

int skred_fxbank_download_pedals(skred_fxbank_t *fx, uint32_t *host_u32, int first, int count) {
  if (!fx || !host_u32 || count < 0) return fail(SKRED_E_BAD_ARG, "fx download_pedals: bad arguments");
  return sk_side_download(fx->d_pedal, sizeof(uint32_t), fx->device, fx->n_voices, host_u32, first, count, "fx download_pedals");
}
