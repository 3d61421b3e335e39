/*
 * skred_bank_owner.c -- note owners: one 32-bit tag per slot on the device, and note-offs and controllers that carry the tag they
 * expect to find (include/skred_amd.h: skred_owner_tags_check, skred_bank_tag_slots / _find_owned / _stamp_owned / _release_tags /
 * _ctl_owned / _owner_clear / _download_owners / _download_env_clocks).
 *
 * The host side of skred_owner_kernels.hip and of sk_ctl_owned_kernel, on the pieces of skred_bank_checks.c and skred_bank_stage.c:
 * the checks (made before anything touches the device), the tags' way through the batch path, the launches.
 * Nothing here waits for the device except the two downloads and the allocation of the array by the first call that needs it.  The
 * owner array is no part of the bank the planner knows: no class, counter, lane word or report depends on it.  What a guarded stamp
 * or controller tells the bank is what its unguarded twin tells it -- n * popcount(mask) more voices may be on the motion list (an
 * upper bound: the guard can only take voices away), and earlier launches' reports are out of date.
 *
 * Out of scope: the fixed-point bank, the drop-in mode, deferred items and pattern steps.
 */
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(SK_OWNER_MAX_TAGS == SKRED_OWNER_MAX_TAGS, "the find kernel's LDS holds SKRED_OWNER_MAX_TAGS tags");
_Static_assert(SKU_STAMP_TRIGGER == SKRED_STAMP_TRIGGER && SKU_STAMP_RELEASE == SKRED_STAMP_RELEASE, "stamp bits travel as they are");

#define SK_OWNER_FLAGS (SKRED_OWNER_ALLOW_ZERO | SKRED_OWNER_UNIQUE)

/* (tag, where it stood) ascending by tag as UNSIGNED numbers, ties by position */
typedef struct { uint32_t tag, at; } owner_pair_t;
static int owner_pair_cmp(const void *x, const void *y) {
  const owner_pair_t *a = (const owner_pair_t *)x, *b = (const owner_pair_t *)y;
  if (a->tag != b->tag) return a->tag < b->tag ? -1 : 1;
  return a->at < b->at ? -1 : a->at > b->at;
}

/* The find pass's view of n <= SKRED_OWNER_MAX_TAGS tags: sorted[j] ascending, perm[j] = the index tags' j-th smallest has in the
 * caller's array.  Returns 0, or 1 + the index of a tag that appears earlier in the array too.  Pure host */
int sk_owner_pack(const uint32_t *tags, int n, uint32_t *sorted, uint32_t *perm) {
  owner_pair_t pairs[SKRED_OWNER_MAX_TAGS];
  for (int k = 0; k < n; k++) { pairs[k].tag = tags[k]; pairs[k].at = (uint32_t)k; }
  qsort(pairs, (size_t)n, sizeof(pairs[0]), owner_pair_cmp);
  int dup = 0;
  for (int j = 0; j < n; j++) {
    sorted[j] = pairs[j].tag;
    perm[j] = pairs[j].at;
    if (j > 0 && !dup && pairs[j].tag == pairs[j - 1].tag) dup = 1 + (int)pairs[j].at;
  }
  return dup;
}

static int tags_check(const uint32_t *tags, int n, uint32_t flags, const char *who) {
  if (!tags) return fail(SKRED_E_BAD_ARG, "%s: no tags", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  if (flags & ~(uint32_t)SK_OWNER_FLAGS) return fail(SKRED_E_BAD_ARG, "%s: unknown bits in flags = 0x%x", who, flags);
  if ((flags & SKRED_OWNER_UNIQUE) && n > SKRED_OWNER_MAX_TAGS)
    return fail(SKRED_E_BAD_ARG, "%s: n = %d tags (at most SKRED_OWNER_MAX_TAGS = %d)", who, n, SKRED_OWNER_MAX_TAGS);
  if (!(flags & SKRED_OWNER_ALLOW_ZERO))
    for (int k = 0; k < n; k++)
      if (!tags[k]) return fail(SKRED_E_BAD_ARG, "%s: tag %d is 0 (0 means nobody)", who, k);
  if (flags & SKRED_OWNER_UNIQUE) {
    uint32_t sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
    const int dup = sk_owner_pack(tags, n, sorted, perm);
    if (dup) return fail(SKRED_E_BAD_ARG, "%s: tag %d = 0x%x appears twice", who, dup - 1, tags[dup - 1]);
  }
  return SKRED_OK;
}

int skred_owner_tags_check(const uint32_t *tags, int n, uint32_t flags) { return tags_check(tags, n, flags, "owner_tags_check"); }

/* the array, the scratch of skred_bank_release_tags and the two words of skred_bank_find_match (skred_bank_expr.c), allocated and
 * zeroed by the first call that needs them */
int sk_owner_ensure(skred_bank_t *b) {
  if (b->d_owner) return SKRED_OK;
  uint32_t *p = NULL;
  const size_t words = (size_t)b->n_voices + SKRED_OWNER_MAX_TAGS + 2;
  const int rc = sk_side_alloc((void **)&p, words * sizeof(uint32_t), "owner array");
  if (rc) return rc;
  b->d_owner = p;
  b->d_owner_slots = (int32_t *)(p + b->n_voices);
  b->d_match_pair = p + b->n_voices + SKRED_OWNER_MAX_TAGS;
  return SKRED_OK;
}

void sk_owner_free(skred_bank_t *b) {
  if (b->d_owner) (void)hipFree(b->d_owner);
  b->d_owner = NULL;
  b->d_owner_slots = NULL;
  b->d_match_pair = NULL;
}

/* n >= 1 checked tags -> a staging slot -> the tag kernel: entry k of the list gets tags[k] (the bank's device is current).  A bank
 * that has a pedal array (skred_bank_pedal.c) clears the tagged slots' pedal words right behind it: a new note starts with no bit
 * of the note it replaces; a bank that has a glide array (skred_bank_glide.c) clears the glide words of the slots' voices likewise,
 * and one that has a bend array (skred_bank_bend.c) the bend words: a thief's first bend must not restore its victim's key; one that
 * has a cutoff array (skred_bank_cutoff.c) the cutoff words: a thief does not inherit a moving cutoff; one that has a filter-envelope
 * array (skred_bank_fenv.c) the fenv words: nor a contour */
int sk_owner_tag_launch(skred_bank_t *b, const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count, int slot_voices,
                        uint32_t *d_result, const char *who, hipStream_t s) {
  int rc = sk_owner_ensure(b);
  if (rc) return rc;
  const size_t bytes = (size_t)n * sizeof(uint32_t);
  sk_batch_t bt;
  if ((rc = sk_batch_begin(b, bytes, s, &bt))) return rc;
  memcpy(bt.h, tags, bytes);
  const uint32_t *src = (const uint32_t *)sk_batch_send(b, &bt, bytes, 0, s);
  if (!src) return SKRED_E_NO_DEVICE;
  hipError_t e = (hipError_t)sk_launch_owner_tag(b->d_owner, d_slots, src, n, d_count, slot_voices, b->n_voices, d_result, bt.cnt, bt.done,
                                                 bt.seq, s);
  if (e == hipSuccess && b->d_pedal) e = (hipError_t)sk_launch_pedal_clear(b->d_pedal, d_slots, n, d_count, slot_voices, b->n_voices, s);
  if (e == hipSuccess && b->d_glide) e = (hipError_t)sk_launch_glide_clear(b->d_glide, d_slots, n, d_count, slot_voices, b->n_voices, s);
  if (e == hipSuccess && b->d_bend) e = (hipError_t)sk_launch_bend_clear(b->d_bend, d_slots, n, d_count, slot_voices, b->n_voices, s);
  if (e == hipSuccess && b->d_cut) e = (hipError_t)sk_launch_cutoff_clear(b->d_cut, d_slots, n, d_count, slot_voices, b->n_voices, s);
  if (e == hipSuccess && b->d_fenv) e = (hipError_t)sk_launch_fenv_clear(b->d_fenv, d_slots, n, d_count, slot_voices, b->n_voices, s);
  return sk_batch_end(&bt, e, who, s);
}

int skred_bank_tag_slots(skred_bank_t *b, const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                         int slot_voices, uint32_t *d_result, void *stream) {
  if (!b || !d_slots) return fail(SKRED_E_BAD_ARG, "tag_slots: no bank or no list");
  int rc = tags_check(tags, n, SKRED_OWNER_ALLOW_ZERO, "tag_slots");
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, "tag_slots"))) return rc;
  if ((rc = sk_check_slot_shape(slot_voices, 0, NULL, "tag_slots"))) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  return sk_owner_tag_launch(b, d_slots, tags, n, d_count_or_null, slot_voices, d_result, "tag_slots", (hipStream_t)stream);
}

/* the find pass of n checked tags over a checked range into d_out (on the device); skred_bank_pedal.c runs it too */
int sk_owner_find_launch(skred_bank_t *b, int first, int count, int slot_voices, const uint32_t *tags, int n, int32_t *d_out, hipStream_t s) {
  const size_t bytes = 2 * (size_t)n * sizeof(uint32_t);
  /* one workgroup per 256 slots stages the tags: beyond a handful of workgroups they read the slot's device twin, not the bus */
  const int wide = (count / slot_voices) > 64 * SK_CONTROL_SPAN;
  sk_batch_t bt;
  const int rc = sk_batch_begin(b, bytes, s, &bt);
  if (rc) return rc;
  uint32_t *sorted = (uint32_t *)bt.h, *perm = sorted + n;
  (void)sk_owner_pack(tags, n, sorted, perm);
  const uint32_t *src = (const uint32_t *)sk_batch_send(b, &bt, bytes, wide, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)sk_launch_owner_find(b->d_owner, first, count, slot_voices, src, src + n, n, d_out, bt.cnt, bt.done, bt.seq, s);
  return sk_batch_end(&bt, e, "find_owned", s);
}

static int find_check(const skred_bank_t *b, int first, int count, int slot_voices, const uint32_t *tags, int n, const char *who) {
  int rc = tags_check(tags, n, SKRED_OWNER_UNIQUE, who);
  if (rc) return rc;
  if ((rc = sk_check_slot_shape(slot_voices, 0, NULL, who))) return rc;
  return sk_check_slot_range(b->n_voices, first, count, slot_voices, 0, who);
}

int skred_bank_find_owned(skred_bank_t *b, int first, int count, int slot_voices, const uint32_t *tags, int n, int32_t *d_slots_out,
                          void *stream) {
  if (!b || !d_slots_out) return fail(SKRED_E_BAD_ARG, "find_owned: no bank or nowhere to put the slots");
  int rc = find_check(b, first, count, slot_voices, tags, n, "find_owned");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_owner_ensure(b))) return rc;
  return sk_owner_find_launch(b, first, count, slot_voices, tags, n, d_slots_out, (hipStream_t)stream);
}

/* the guarded stamps of n checked tags on a list in device memory */
static int stamp_launch(skred_bank_t *b, const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count, int slot_voices,
                        uint64_t voice_mask, uint32_t stamps, uint32_t *d_result, hipStream_t s) {
  const size_t bytes = (size_t)n * sizeof(uint32_t);
  sk_batch_t bt;
  int rc = sk_batch_begin(b, bytes, s, &bt);
  if (rc) return rc;
  memcpy(bt.h, tags, bytes);
  const uint32_t *src = (const uint32_t *)sk_batch_send(b, &bt, bytes, 0, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)sk_launch_owner_stamps(b->d_owner, d_slots, src, n, d_count, slot_voices, voice_mask, b->n_voices, stamps,
                                                          b->d_ro, b->d_rw, b->g.synth_sample_count, b->d_mask[b->mask_p], d_result,
                                                          bt.cnt, bt.done, bt.seq, s);
  if ((rc = sk_batch_end(&bt, e, "stamp_owned", s))) return rc;
  sk_touched(b, (uint64_t)n * (uint64_t)__builtin_popcountll(voice_mask));
  return SKRED_OK;
}

int skred_bank_stamp_owned(skred_bank_t *b, const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                           int slot_voices, uint64_t voice_mask, uint32_t stamps, uint32_t *d_result, void *stream) {
  if (!b || !d_slots || !d_result) return fail(SKRED_E_BAD_ARG, "stamp_owned: no bank, list or result");
  int rc = tags_check(tags, n, 0, "stamp_owned");
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, "stamp_owned"))) return rc;
  if ((rc = sk_check_stamps(stamps, "stamp_owned"))) return rc;
  if ((rc = sk_check_slot_shape(slot_voices, voice_mask, "voice_mask", "stamp_owned"))) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_owner_ensure(b))) return rc;
  return stamp_launch(b, d_slots, tags, n, d_count_or_null, slot_voices, voice_mask, stamps, d_result, (hipStream_t)stream);
}

int skred_bank_release_tags(skred_bank_t *b, int first, int count, int slot_voices, uint64_t voice_mask, const uint32_t *tags, int n,
                            uint32_t stamps, uint32_t *d_result, void *stream) {
  if (!b || !d_result) return fail(SKRED_E_BAD_ARG, "release_tags: no bank or no result");
  int rc = find_check(b, first, count, slot_voices, tags, n, "release_tags");
  if (rc) return rc;
  if ((rc = sk_check_stamps(stamps, "release_tags"))) return rc;
  if ((rc = sk_check_slot_shape(slot_voices, voice_mask, "voice_mask", "release_tags"))) return rc;   /* (K passed find_check: the mask) */
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_owner_ensure(b))) return rc;
  if ((rc = sk_owner_find_launch(b, first, count, slot_voices, tags, n, b->d_owner_slots, s))) return rc;
  /* entry k is the lowest slot that carries tags[k], or -1: the guard holds on every entry that is a slot */
  return stamp_launch(b, b->d_owner_slots, tags, n, NULL, slot_voices, voice_mask, stamps, d_result, s);
}

int skred_bank_ctl_owned(skred_bank_t *b, const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                         const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  if (!b || !d_slots) return fail(SKRED_E_BAD_ARG, "ctl_owned: no bank or no list");
  int rc = tags_check(tags, n, 0, "ctl_owned");
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, "ctl_owned"))) return rc;
  if ((rc = skred_ctl_check(ctl, slot_voices, voice_mask))) return rc;
  if (n == 0) return SKRED_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_owner_ensure(b))) return rc;
  /* the K records, then the n tags, in one staging slot: one kernel reads both */
  const size_t rec_bytes = (size_t)slot_voices * sizeof(sk_ctl_t), bytes = rec_bytes + (size_t)n * sizeof(uint32_t);
  const int wide = (int64_t)n * slot_voices > 64 * 256;    /* (skred_bank_ctl.c: beyond 64 workgroups the records are read from the device) */
  sk_batch_t bt;
  if ((rc = sk_batch_begin(b, bytes, s, &bt))) return rc;
  const uint64_t lists = sk_ctl_pack(ctl, slot_voices, voice_mask, (sk_ctl_t *)bt.h);
  memcpy((char *)bt.h + rec_bytes, tags, (size_t)n * sizeof(uint32_t));
  const char *src = (const char *)sk_batch_send(b, &bt, bytes, wide, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)sk_launch_ctl_owned((const sk_ctl_t *)src, slot_voices, voice_mask, d_slots, (const uint32_t *)(src + rec_bytes),
                                                       b->d_owner, n, d_count_or_null, b->n_voices, b->d_ro, b->d_rw, b->d_mask[b->mask_p],
                                                       d_result, bt.cnt, bt.done, bt.seq, s);
  if ((rc = sk_batch_end(&bt, e, "ctl_owned", s))) return rc;
  if (lists) sk_touched(b, (uint64_t)n * (uint64_t)__builtin_popcountll(lists));   /* (skred_bank_ctl.c: a controller that lists nobody leaves the reports alone) */
  return SKRED_OK;
}

int skred_bank_owner_clear(skred_bank_t *b, int first, int count, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "owner_clear: no bank");
  return sk_side_clear(b->d_owner, sizeof(uint32_t), b->device, b->n_voices, first, count, (hipStream_t)stream, "owner_clear");
}

int skred_bank_download_owners(skred_bank_t *b, uint32_t *host_u32, int first, int count) {
  if (!b || !host_u32 || count < 0) return fail(SKRED_E_BAD_ARG, "download_owners: bad arguments");
  return sk_side_download(b->d_owner, sizeof(uint32_t), b->device, b->n_voices, host_u32, first, count, "download_owners");
}

int skred_bank_download_env_clocks(skred_bank_t *b, uint64_t *sample_start, uint64_t *sample_release, int first, int count) {
  if (!b || count < 0) return fail(SKRED_E_BAD_ARG, "download_env_clocks: bad arguments");
  const int rc = sk_check_window(b->n_voices, first, count, "download_env_clocks");
  if (rc) return rc;
  if (count == 0 || (!sample_start && !sample_release)) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  sk_plane_t *st = (sk_plane_t *)malloc((size_t)count * sizeof(sk_plane_t));
  if (!st) return fail(SKRED_E_NO_MEM, "download_env_clocks staging");
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(st, b->d_ro[SKP_ENV_S] + first, (size_t)count * sizeof(sk_plane_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) { free(st); HIP_TRY(e); }
  for (int i = 0; i < count; i++) {
    if (sample_start) sample_start[i] = (uint64_t)st[i].w[0] | (uint64_t)st[i].w[1] << 32;
    if (sample_release) sample_release[i] = (uint64_t)st[i].w[2] | (uint64_t)st[i].w[3] << 32;
  }
  free(st);
  return SKRED_OK;
}
