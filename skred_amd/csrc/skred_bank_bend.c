/*
 * skred_bank_bend.c -- the pitch wheel: bends that return to the key's bits and compose with glides, two words per voice beside the
 * glide array (include/skred_amd.h: skred_bend_check, skred_bank_bend_match / _bend_owned_each / _bend_tags_each / _bend_clear /
 * _download_bend).
 *
 * The host side of skred_bend_kernels.hip, on the pieces of skred_bank_checks.c and skred_bank_stage.c and on the owner array and
 * find pass of skred_bank_owner.c: the checks (made before anything touches the device, in the order the header documents), the
 * ratios' and tags' way through the batch path, the launches.  Nothing here waits for the device except the download and the
 * allocation of the array by the first call that bends.  The bend array is no part of the bank the planner knows: no class, counter,
 * lane word or report depends on it.  The calls tell the bank nothing either: the one plane word they store is voice_phase_inc, they
 * store finite non-zero values only, and an increment lists nobody (skred_bank_ctl.c has the measurement behind
 * SKRED_CTL_INC_SCALE's rule).  The hook that clears a re-tagged slot's words is in skred_bank_owner.c (sk_owner_tag_launch); the
 * glide launches of skred_bank_glide.c take the array once it exists.
 *
 * Out of scope: the fixed-point bank, the drop-in mode, deferred items and pattern steps.
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(sizeof(sk_bend_t) == 8, "one 8-byte load per voice");

static int ratio_check(float r, int k, const char *who) {
  if (!isfinite(r) || !(r > 0.0f)) return fail(SKRED_E_BAD_ARG, "%s: ratio %d = %g (finite and above 0)", who, k, (double)r);
  return SKRED_OK;
}

/* K, the mask, the ratios: what every bending call checks between its pointers and its tags */
static int bend_check(const float *ratios, int n, int slot_voices, uint64_t voice_mask, const char *who) {
  if (!ratios) return fail(SKRED_E_BAD_ARG, "%s: no ratios", who);
  int rc = sk_check_slot_shape(slot_voices, voice_mask, "voice_mask", who);
  if (rc) return rc;
  for (int k = 0; k < n; k++)
    if ((rc = ratio_check(ratios[k], k, who))) return rc;
  return SKRED_OK;
}

int skred_bend_check(const float *ratios, int n, int slot_voices, uint64_t voice_mask) {
  const int rc = bend_check(ratios, n, slot_voices, voice_mask, "bend_check");
  if (rc) return rc;
  if (n < 0) return fail(SKRED_E_BAD_ARG, "bend_check: n = %d", n);
  return SKRED_OK;
}

/* The checked ratios as they travel: out[j] = the bits of ratios[perm[j]] (perm NULL: j).  Pure host */
void sk_bend_pack(const float *ratios, int n, const uint32_t *perm, uint32_t *out) {
  for (int j = 0; j < n; j++) memcpy(&out[j], &ratios[perm ? perm[j] : (uint32_t)j], sizeof(uint32_t));
}

/* the array, allocated and zeroed by the first call that bends (the owner array first, when no owner call came before) */
static int bend_ensure(skred_bank_t *b) {
  if (b->d_bend) return SKRED_OK;
  const int rc = sk_owner_ensure(b);
  if (rc) return rc;
  return sk_side_alloc((void **)&b->d_bend, (size_t)b->n_voices * sizeof(sk_bend_t), "bend array");
}

void sk_bend_free(skred_bank_t *b) {
  if (b->d_bend) (void)hipFree(b->d_bend);
  b->d_bend = NULL;
}

/* the pointers, then K, mask and ratios, then the tags, then n: the header's order */
static int each_check(const skred_bank_t *b, const float *ratios, int slot_voices, uint64_t voice_mask, const uint32_t *tags, int n,
                      uint32_t tag_flags, const char *who) {
  if (!b) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  if (!tags) return fail(SKRED_E_BAD_ARG, "%s: no tags", who);
  int rc = bend_check(ratios, n, slot_voices, voice_mask, who);
  if (rc) return rc;
  for (int k = 0; k < n; k++)
    if (!tags[k]) return fail(SKRED_E_BAD_ARG, "%s: tag %d is 0 (0 means nobody)", who, k);
  if ((rc = skred_owner_tags_check(tags, n, tag_flags))) return rc;     /* n < 0; UNIQUE: n > SKRED_OWNER_MAX_TAGS, a tag twice */
  return sk_check_list_n(n, who);
}

/* the n ratios (ratios[perm[j]]; perm NULL: as they stand) and the n tags in one staging slot: one kernel reads both */
static int each_launch(skred_bank_t *b, const float *ratios, const uint32_t *perm, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                       const uint32_t *tags, int n, const uint32_t *d_count, uint32_t *d_result, const char *who, hipStream_t s) {
  const size_t words = (size_t)n * sizeof(uint32_t), bytes = 2 * words;
  sk_batch_t bt;
  int rc = sk_batch_begin(b, bytes, s, &bt);
  if (rc) return rc;
  char *h = (char *)bt.h;
  sk_bend_pack(ratios, n, perm, (uint32_t *)h);
  memcpy(h + words, tags, words);
  const char *src = (const char *)sk_batch_send(b, &bt, bytes, 0, s);   /* (every byte is read by one workgroup) */
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)sk_launch_bend_each(b->d_bend, (const uint32_t *)src, slot_voices, voice_mask, d_slots,
                                                       (const uint32_t *)(src + words), b->d_owner, n, d_count, b->n_voices,
                                                       b->d_ro[SKP_OSC], d_result, bt.cnt, bt.done, bt.seq, s);
  return sk_batch_end(&bt, e, who, s);                    /* (an increment lists nobody: the planner's reports stand) */
}

int skred_bank_bend_match(skred_bank_t *b, int first, int count, int slot_voices, uint64_t voice_mask, const skred_owner_match_t *m,
                          float ratio, uint32_t *d_result, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "bend_match: no bank");
  if (!m) return fail(SKRED_E_BAD_ARG, "bend_match: no match");
  int rc = sk_check_slot_shape(slot_voices, voice_mask, "voice_mask", "bend_match");
  if (rc) return rc;
  if ((rc = ratio_check(ratio, 0, "bend_match"))) return rc;
  if ((rc = skred_owner_match_check(m))) return rc;
  if ((rc = sk_check_slot_range(b->n_voices, first, count, slot_voices, 0, "bend_match"))) return rc;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = bend_ensure(b))) return rc;
  uint32_t bits;
  memcpy(&bits, &ratio, sizeof(bits));
  const hipError_t e = (hipError_t)sk_launch_bend_match(b->d_bend, bits, slot_voices, voice_mask, first, count, b->d_owner, m->value, m->mask,
                                                        b->d_ro[SKP_OSC], d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "bend_match launch -> %s", hipGetErrorString(e));
  return SKRED_OK;                                         /* (finite increments only: the planner's reports stand) */
}

int skred_bank_bend_owned_each(skred_bank_t *b, const float *ratios, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                               const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  if (!b || !d_slots) return fail(SKRED_E_BAD_ARG, "bend_owned_each: no bank or no list");
  int rc = each_check(b, ratios, slot_voices, voice_mask, tags, n, 0, "bend_owned_each");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = bend_ensure(b))) return rc;
  return each_launch(b, ratios, NULL, slot_voices, voice_mask, d_slots, tags, n, d_count_or_null, d_result, "bend_owned_each", (hipStream_t)stream);
}

int skred_bank_bend_tags_each(skred_bank_t *b, const float *ratios, int first, int count, int slot_voices, uint64_t voice_mask,
                              const uint32_t *tags, int n, uint32_t *d_result, void *stream) {
  int rc = each_check(b, ratios, slot_voices, voice_mask, tags, n, SKRED_OWNER_UNIQUE, "bend_tags_each");
  if (rc) return rc;
  if ((rc = sk_check_slot_range(b->n_voices, first, count, slot_voices, 0, "bend_tags_each"))) return rc;
  if (n == 0) return SKRED_OK;
  /* the tags travel sorted (the find pass searches them), and ratios[k] stays with tags[k]: entry j of the list is the slot of the
   * j-th smallest tag, and receives ratios[perm[j]] */
  uint32_t sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  (void)sk_owner_pack(tags, n, sorted, perm);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = bend_ensure(b))) return rc;
  if ((rc = sk_owner_find_launch(b, first, count, slot_voices, sorted, n, b->d_owner_slots, s))) return rc;
  /* entry j is the lowest slot that carries sorted[j], or -1: the guard holds on every entry that is a slot */
  return each_launch(b, ratios, perm, slot_voices, voice_mask, b->d_owner_slots, sorted, n, NULL, d_result, "bend_tags_each", s);
}

int skred_bank_bend_clear(skred_bank_t *b, int first, int count, int snap, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "bend_clear: no bank");
  const int rc = sk_check_window(b->n_voices, first, count, "bend_clear");
  if (rc) return rc;
  if (count == 0 || !b->d_bend) return SKRED_OK;           /* (no voice was ever bent: every word is 0 already) */
  HIP_TRY(hipSetDevice(b->device));
  const hipError_t e = (hipError_t)sk_launch_bend_range_clear(b->d_bend, b->d_ro[SKP_OSC], first, count, snap != 0, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "bend_clear launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_bank_download_bend(skred_bank_t *b, uint32_t *host_u32x2, int first, int count) {
  if (!b || !host_u32x2 || count < 0) return fail(SKRED_E_BAD_ARG, "download_bend: bad arguments");
  return sk_side_download(b->d_bend, sizeof(sk_bend_t), b->device, b->n_voices, host_u32x2, first, count, "download_bend");
}
