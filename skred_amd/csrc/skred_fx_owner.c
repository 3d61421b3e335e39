/*
 * skred_fx_owner.c -- note owners of the fixed-point bank: one 32-bit tag per voice on the device, and note-offs that carry the tag
 * they expect to find (include/skred_amd_fxpt.h: skred_fxbank_tag_list / _find_owned / _stamp_owned / _release_tags / _owner_clear /
 * _download_owners, and skred_fxbank_download_params).
 *
 * The host side, built like skred_fx_live.c: the checks (made before anything touches the device; the tags' own through the float
 * bank's skred_owner_tags_check, the shared ones of skred_bank_checks.c), the tags' way through the batch path (skred_fx_stage.c),
 * the launches.  The tag and the find pass are the float bank's kernels, entered through their launchers at slot_voices = 1 without a
 * batch-done word (skred_launch.h: this ring guards a slot with an event); the guarded stamp is skred_fx_owner_kernels.hip.  Nothing here waits for the device except the two downloads
 * and the allocation of the array by the first call that needs it.  The bank has no slots: every call is per voice.
 */
#include <stdlib.h>
#include <string.h>

#include "skred_launch.h"
#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

_Static_assert(SK_OWNER_MAX_TAGS == SKRED_OWNER_MAX_TAGS, "the find kernel's LDS holds SKRED_OWNER_MAX_TAGS tags");

int skx_owner_ensure(skred_fxbank_t *fx) {
  if (fx->d_owner) return SKRED_OK;
  uint32_t *p = NULL;
  const size_t words = (size_t)fx->n_voices + SKRED_OWNER_MAX_TAGS + 2;   /* the owners, _release_tags' list, _find_match's pair */
  const int rc = sk_side_alloc((void **)&p, words * sizeof(uint32_t), "fx owner array");
  if (rc) return rc;
  fx->d_owner = p;
  fx->d_owner_found = (int32_t *)(p + fx->n_voices);
  fx->d_match_pair = p + fx->n_voices + SKRED_OWNER_MAX_TAGS;
  return SKRED_OK;
}

void skx_owner_free(skred_fxbank_t *fx) {
  if (fx->d_owner) (void)hipFree(fx->d_owner);
  fx->d_owner = NULL;
  fx->d_owner_found = NULL;
  fx->d_match_pair = NULL;
}

/* n >= 1 checked tags -> a staging slot -> the float bank's tag kernel at K = 1: entry k of the list gets tags[k] (the bank's device
 * is current) */
int skx_owner_tag_launch(skred_fxbank_t *fx, const int32_t *d_voices, const uint32_t *tags, int n, const uint32_t *d_count,
                         uint32_t *d_result, const char *who, hipStream_t s) {
  int rc = skx_owner_ensure(fx);
  if (rc) return rc;
  const size_t bytes = (size_t)n * sizeof(uint32_t);
  skx_batch_t bt;
  if ((rc = skx_batch_begin(fx, bytes, &bt))) return rc;
  memcpy(bt.h, tags, bytes);
  const uint32_t *src = (const uint32_t *)skx_batch_send(&bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  hipError_t e = (hipError_t)sk_launch_owner_tag(fx->d_owner, d_voices, src, n, d_count, 1, fx->n_voices, d_result, NULL, NULL, 0, s);
  /* a new note clears its voice's pedal word (skred_fx_pedal.c): the same list under the same rule, once the bank has the array */
  if (e == hipSuccess && fx->d_pedal) e = (hipError_t)sk_launch_pedal_clear(fx->d_pedal, d_voices, n, d_count, 1, fx->n_voices, s);
  /* ... and does not inherit a glide (skred_fx_glide.c): the float bank's clear kernel, the array's shape being the same */
  if (e == hipSuccess && fx->d_glide) e = (hipError_t)sk_launch_glide_clear((sk_glide_t *)fx->d_glide, d_voices, n, d_count, 1, fx->n_voices, s);
  /* ... nor a bend (skred_fx_bend.c): a thief's first bend would take its victim's key, and the centre would restore it */
  if (e == hipSuccess && fx->d_bend) e = (hipError_t)sk_launch_bend_clear((sk_bend_t *)fx->d_bend, d_voices, n, d_count, 1, fx->n_voices, s);
  /* ... nor a cutoff word (skred_fx_cutoff.c): a thief or a key struck again does not inherit a moving cutoff; the coefficients stay */
  if (e == hipSuccess && fx->d_cut) e = (hipError_t)sk_launch_cutoff_clear((sk_cut_t *)fx->d_cut, d_voices, n, d_count, 1, fx->n_voices, s);
  /* ... nor a contour (skred_fx_fenv.c): the float bank's clear kernel again, the fenv array's shape being the same */
  if (e == hipSuccess && fx->d_fenv) e = (hipError_t)sk_launch_fenv_clear((sk_fenv_t *)fx->d_fenv, d_voices, n, d_count, 1, fx->n_voices, s);
  return skx_batch_end(&bt, e, who, s);
}

int skred_fxbank_tag_list(skred_fxbank_t *fx, const int32_t *d_voices, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                          uint32_t *d_result, void *stream) {
  if (!fx || !d_voices) return fail(SKRED_E_BAD_ARG, "fx tag_list: no bank or no list");
  int rc = skred_owner_tags_check(tags, n, SKRED_OWNER_ALLOW_ZERO);
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, "fx tag_list"))) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(fx->device));
  return skx_owner_tag_launch(fx, d_voices, tags, n, d_count_or_null, d_result, "fx tag_list", (hipStream_t)stream);
}

/* Begins the batch `bt` with sorted | perm (| the tags as given, with_tags) of n checked tags and queues the find pass over a checked
 * range into d_out: *err is that launch's verdict.  The caller queues what else reads the slot (bt->sl->d), then ends the batch.
 * (skred_fx_pedal.c enters it too.) */
int skx_owner_find_launch(skred_fxbank_t *fx, int first, int count, const uint32_t *tags, int n, int with_tags, int32_t *d_out, hipStream_t s,
                          skx_batch_t *bt, hipError_t *err) {
  const size_t words = (size_t)(with_tags ? 3 : 2) * (size_t)n, bytes = words * sizeof(uint32_t);
  const int rc = skx_batch_begin(fx, bytes, bt);
  if (rc) return rc;
  uint32_t *sorted = (uint32_t *)bt->h, *perm = sorted + n;
  (void)sk_owner_pack(tags, n, sorted, perm);
  if (with_tags) memcpy(perm + n, tags, (size_t)n * sizeof(uint32_t));
  const uint32_t *src = (const uint32_t *)skx_batch_send(bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  *err = (hipError_t)sk_launch_owner_find(fx->d_owner, first, count, 1, src, src + n, n, d_out, NULL, NULL, 0, s);
  return SKRED_OK;
}

static int find_check(const skred_fxbank_t *fx, int first, int count, const uint32_t *tags, int n, const char *who) {
  const int rc = skred_owner_tags_check(tags, n, SKRED_OWNER_UNIQUE);
  if (rc) return rc;
  return sk_check_slot_range(fx->n_voices, first, count, 1, 0, who);   /* at least one voice, inside the bank */
}

int skred_fxbank_find_owned(skred_fxbank_t *fx, int first, int count, const uint32_t *tags, int n, int32_t *d_voices_out, void *stream) {
  if (!fx || !d_voices_out) return fail(SKRED_E_BAD_ARG, "fx find_owned: no bank or nowhere to put the voices");
  int rc = find_check(fx, first, count, tags, n, "fx find_owned");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_owner_ensure(fx))) return rc;
  skx_batch_t bt;
  hipError_t e = hipSuccess;
  if ((rc = skx_owner_find_launch(fx, first, count, tags, n, 0, d_voices_out, s, &bt, &e))) return rc;
  return skx_batch_end(&bt, e, "fx find_owned", s);
}

int skred_fxbank_stamp_owned(skred_fxbank_t *fx, const int32_t *d_voices, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                             uint32_t stamps, uint32_t *d_result, void *stream) {
  if (!fx || !d_voices || !d_result) return fail(SKRED_E_BAD_ARG, "fx stamp_owned: no bank, list or result");
  int rc = skred_owner_tags_check(tags, n, 0);
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, "fx stamp_owned"))) return rc;
  if ((rc = sk_check_stamps(stamps, "fx stamp_owned"))) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_owner_ensure(fx))) return rc;
  const size_t bytes = (size_t)n * sizeof(uint32_t);
  skx_batch_t bt;
  if ((rc = skx_batch_begin(fx, bytes, &bt))) return rc;
  memcpy(bt.h, tags, bytes);
  const uint32_t *src = (const uint32_t *)skx_batch_send(&bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)skx_launch_stamp_owned(fx->d_owner, d_voices, src, n, d_count_or_null, fx->n_voices, stamps,
                                                          fx->d_ro[SKX_TIME], fx->d_rw[0], fx->count, d_result, s);
  return skx_batch_end(&bt, e, "fx stamp_owned", s);
}

int skred_fxbank_release_tags(skred_fxbank_t *fx, int first, int count, const uint32_t *tags, int n, uint32_t stamps, uint32_t *d_result,
                              void *stream) {
  if (!fx || !d_result) return fail(SKRED_E_BAD_ARG, "fx release_tags: no bank or no result");
  int rc = find_check(fx, first, count, tags, n, "fx release_tags");
  if (rc) return rc;
  if ((rc = sk_check_stamps(stamps, "fx release_tags"))) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_owner_ensure(fx))) return rc;
  skx_batch_t bt;
  hipError_t e = hipSuccess;
  if ((rc = skx_owner_find_launch(fx, first, count, tags, n, 1, fx->d_owner_found, s, &bt, &e))) return rc;
  /* entry k is the lowest voice that carries tags[k], or -1: the guard holds on every entry that is a voice */
  if (e == hipSuccess)
    e = (hipError_t)skx_launch_stamp_owned(fx->d_owner, fx->d_owner_found, (const uint32_t *)bt.sl->d + 2 * (size_t)n, n, NULL, fx->n_voices,
                                           stamps, fx->d_ro[SKX_TIME], fx->d_rw[0], fx->count, d_result, s);
  return skx_batch_end(&bt, e, "fx release_tags", s);
}

int skred_fxbank_owner_clear(skred_fxbank_t *fx, int first, int count, void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx owner_clear: no bank");
  return sk_side_clear(fx->d_owner, sizeof(uint32_t), fx->device, fx->n_voices, first, count, (hipStream_t)stream, "fx owner_clear");
}

int skred_fxbank_download_owners(skred_fxbank_t *fx, uint32_t *host_u32, int first, int count) {
  if (!fx || !host_u32 || count < 0) return fail(SKRED_E_BAD_ARG, "fx download_owners: bad arguments");
  return sk_side_download(fx->d_owner, sizeof(uint32_t), fx->device, fx->n_voices, host_u32, first, count, "fx download_owners");
}

int skred_fxbank_download_params(skred_fxbank_t *fx, skred_fxpt_bank_t *h, uint32_t *recip_out, int src_first, int dst_first, int count) {
  if (!fx || !h || count < 0) return fail(SKRED_E_BAD_ARG, "fx download_params: bad arguments");
  int bad = sk_check_window(fx->n_voices, src_first, count, "fx download_params");
  if (bad || (bad = sk_check_window(h->n_voices, dst_first, count, "fx download_params into the host view"))) return bad;
  if (count == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(fx->device));
  skx_plane_t *st = (skx_plane_t *)malloc((size_t)SKX_COUNT * (size_t)count * sizeof(skx_plane_t));
  if (!st) return fail(SKRED_E_NO_MEM, "fx download_params staging");
  hipError_t e = hipDeviceSynchronize();
  for (int p = 0; p < SKX_COUNT && e == hipSuccess; p++)
    e = hipMemcpy(st + (size_t)p * count, fx->d_ro[p] + src_first, (size_t)count * sizeof(skx_plane_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) { free(st); HIP_TRY(e); }
  for (int i = 0; i < count; i++) {
    const int v = dst_first + i;
    const skx_plane_t *osc = &st[(size_t)SKX_OSC * count + i], *gn = &st[(size_t)SKX_GAIN * count + i], *env = &st[(size_t)SKX_ENV * count + i];
    const skx_plane_t *rc = &st[(size_t)SKX_RECIP * count + i], *tm = &st[(size_t)SKX_TIME * count + i];
    const skx_plane_t *f = &st[(size_t)SKX_FILT * count + i], *f2 = &st[(size_t)SKX_FILT2 * count + i];
    const uint32_t flags = osc->w[2] >> 8;
    h->phase_inc[v] = osc->w[0]; h->table_offset[v] = (int32_t)osc->w[1]; h->log2_size[v] = (int32_t)(osc->w[2] & 0xFFu);
    h->amp_q15[v] = (int32_t)osc->w[3];
    h->use_envelope[v] = (flags & SKXF_USE_ENV) != 0; h->smoother_enable[v] = (flags & SKXF_SMOOTH) != 0;
    h->disconnect[v] = (flags & SKXF_MUTED) != 0;
    if (h->filter_mode) h->filter_mode[v] = (flags & SKXF_FILTER) != 0;
    if (h->one_shot) h->one_shot[v] = (flags & SKXF_ONE_SHOT) != 0;
    h->pan_left_q15[v] = (int32_t)gn->w[0]; h->pan_right_q15[v] = (int32_t)gn->w[1];
    h->smoother_k_q15[v] = (int32_t)gn->w[2]; h->velocity_q15[v] = (int32_t)gn->w[3];
    h->attack_frames[v] = env->w[0]; h->decay_frames[v] = env->w[1]; h->release_frames[v] = env->w[2]; h->sustain_q15[v] = (int32_t)env->w[3];
    h->sample_start[v] = (uint64_t)tm->w[0] | (uint64_t)tm->w[1] << 32;
    h->sample_release[v] = (uint64_t)tm->w[2] | (uint64_t)tm->w[3] << 32;
    if (h->b0_q30) h->b0_q30[v] = (int32_t)f->w[0];
    if (h->b1_q30) h->b1_q30[v] = (int32_t)f->w[1];
    if (h->b2_q30) h->b2_q30[v] = (int32_t)f->w[2];
    if (h->a1_q30) h->a1_q30[v] = (int32_t)f->w[3];
    if (h->a2_q30) h->a2_q30[v] = (int32_t)f2->w[0];
    if (recip_out) { recip_out[3 * (size_t)i] = rc->w[0]; recip_out[3 * (size_t)i + 1] = rc->w[1]; recip_out[3 * (size_t)i + 2] = rc->w[2]; }
  }
  free(st);
  return SKRED_OK;
}
