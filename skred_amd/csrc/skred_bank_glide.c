/*
 * skred_bank_glide.c -- portamento: pitch glides that advance and land on the device, four words per voice beside the owner array
 * (include/skred_amd.h: skred_glide_check, skred_bank_glide_owned / _glide_tags / _glide_advance / _glide_stop / _download_glide).
 *
 * The host side of skred_glide_kernels.hip, on the pieces of skred_bank_checks.c and skred_bank_stage.c and on the owner array and
 * find pass of skred_bank_owner.c: the checks (made before anything touches the device), the entries' and tags' way through the batch
 * path, the launches.  Nothing here waits for the device except the download and the allocation of the array by the first call that
 * starts a glide.  The glide array is no part of the bank the planner knows: no class, counter, lane word or report depends on it.
 * The calls tell the bank nothing either: the one plane word they store is voice_phase_inc, they store finite values only, and an
 * increment lists nobody (skred_bank_ctl.c has the measurement behind SKRED_CTL_INC_SCALE's rule).  The hook that clears a re-tagged
 * slot's words is in skred_bank_owner.c (sk_owner_tag_launch).  On a bank that has a pitch-wheel array (skred_bank_bend.c) the three
 * launches take it, and a bent voice's glide runs on its key.
 *
 * Out of scope: the fixed-point bank, the drop-in mode, deferred items and pattern steps.
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(sizeof(skred_glide_t) == sizeof(sk_glide_each_t) && sizeof(skred_glide_t) == 32 && offsetof(skred_glide_t, set) == 4 * SK_GLIDE_E_SET &&
               offsetof(skred_glide_t, rate_up) == 4 * SK_GLIDE_E_RATE_UP && offsetof(skred_glide_t, rate_down) == 4 * SK_GLIDE_E_RATE_DOWN &&
               offsetof(skred_glide_t, scale) == 4 * SK_GLIDE_E_SCALE && offsetof(skred_glide_t, reserved) == 16,
               "the device's per-entry record must be skred_glide_t word for word");
_Static_assert(SK_GLIDE_FROM_SCALE == SKRED_GLIDE_FROM_SCALE && SK_GLIDE_TO_SCALE == SKRED_GLIDE_TO_SCALE, "the glide bits travel as they are");
_Static_assert(sizeof(sk_glide_t) == 16, "one 16-byte load per voice");

static int glide_check(const skred_glide_t *glide, int n, int slot_voices, uint64_t voice_mask, const char *who) {
  if (!glide) return fail(SKRED_E_BAD_ARG, "%s: no entries", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  const int rc = sk_check_slot_shape(slot_voices, voice_mask, "voice_mask", who);
  if (rc) return rc;
  for (int k = 0; k < n; k++) {
    const skred_glide_t *e = &glide[k];
    if (e->set != SKRED_GLIDE_FROM_SCALE && e->set != SKRED_GLIDE_TO_SCALE)
      return fail(SKRED_E_BAD_ARG, "%s: entry %d: set = 0x%x (exactly one of SKRED_GLIDE_FROM_SCALE and SKRED_GLIDE_TO_SCALE)", who, k, e->set);
    if (e->reserved[0] || e->reserved[1] || e->reserved[2] || e->reserved[3])
      return fail(SKRED_E_BAD_ARG, "%s: entry %d: the reserved words must be 0", who, k);
    if (!isfinite(e->rate_up) || !isfinite(e->rate_down) || !isfinite(e->scale))
      return fail(SKRED_E_BAD_ARG, "%s: entry %d holds %g %g %g", who, k, (double)e->rate_up, (double)e->rate_down, (double)e->scale);
    if (!(e->rate_up > 1.0f)) return fail(SKRED_E_BAD_ARG, "%s: entry %d: rate_up = %g (above 1)", who, k, (double)e->rate_up);
    if (!(e->rate_down < 1.0f) || !(e->rate_down > 0.0f))
      return fail(SKRED_E_BAD_ARG, "%s: entry %d: rate_down = %g (between 0 and 1)", who, k, (double)e->rate_down);
    if (!(e->scale > 0.0f)) return fail(SKRED_E_BAD_ARG, "%s: entry %d: scale = %g (above 0)", who, k, (double)e->scale);
  }
  return SKRED_OK;
}

int skred_glide_check(const skred_glide_t *glide, int n, int slot_voices, uint64_t voice_mask) {
  return glide_check(glide, n, slot_voices, voice_mask, "glide_check");
}

/* The checked entries as they travel: out[j] = glide[perm[j]] (perm NULL: j), the four named words as they stand, the rest zero.
 * Pure host */
void sk_glide_pack(const skred_glide_t *glide, int n, const uint32_t *perm, sk_glide_each_t *out) {
  memset(out, 0, (size_t)n * sizeof(sk_glide_each_t));
  for (int j = 0; j < n; j++) memcpy(out[j].w, &glide[perm ? perm[j] : (uint32_t)j], 4 * sizeof(uint32_t));
}

/* the array behind the owner array, allocated and zeroed by the first call that starts a glide (the owner array first, when no owner
 * call came before) */
static int glide_ensure(skred_bank_t *b) {
  if (b->d_glide) return SKRED_OK;
  const int rc = sk_owner_ensure(b);
  if (rc) return rc;
  return sk_side_alloc((void **)&b->d_glide, (size_t)b->n_voices * sizeof(sk_glide_t), "glide array");
}

void sk_glide_free(skred_bank_t *b) {
  if (b->d_glide) (void)hipFree(b->d_glide);
  b->d_glide = NULL;
}

static int start_check(const skred_bank_t *b, const skred_glide_t *glide, int slot_voices, uint64_t voice_mask, const uint32_t *tags, int n,
                       uint32_t tag_flags, const char *who) {
  if (!b) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  int rc = skred_owner_tags_check(tags, n, tag_flags);
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, who))) return rc;
  return glide_check(glide, n, slot_voices, voice_mask, who);
}

/* the n entries (glide[perm[j]]; perm NULL: as they stand) and the n tags in one staging slot: one kernel reads both */
static int start_launch(skred_bank_t *b, const skred_glide_t *glide, const uint32_t *perm, int slot_voices, uint64_t voice_mask,
                        const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count, uint32_t *d_result, const char *who,
                        hipStream_t s) {
  const size_t each_bytes = (size_t)n * sizeof(sk_glide_each_t), bytes = each_bytes + (size_t)n * sizeof(uint32_t);
  sk_batch_t bt;
  int rc = sk_batch_begin(b, bytes, s, &bt);
  if (rc) return rc;
  char *h = (char *)bt.h;
  sk_glide_pack(glide, n, perm, (sk_glide_each_t *)h);
  memcpy(h + each_bytes, tags, (size_t)n * sizeof(uint32_t));
  const char *src = (const char *)sk_batch_send(b, &bt, bytes, 0, s);   /* (every byte is read by one workgroup) */
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)sk_launch_glide_start(b->d_glide, b->d_bend, (const sk_glide_each_t *)src, slot_voices, voice_mask, d_slots,
                                                         (const uint32_t *)(src + each_bytes), b->d_owner, n, d_count, b->n_voices,
                                                         b->d_ro[SKP_OSC], d_result, bt.cnt, bt.done, bt.seq, s);
  return sk_batch_end(&bt, e, who, s);                    /* (an increment lists nobody: the planner's reports stand) */
}

int skred_bank_glide_owned(skred_bank_t *b, const skred_glide_t *glide, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                           const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  if (!d_slots) return fail(SKRED_E_BAD_ARG, "glide_owned: no list");
  int rc = start_check(b, glide, slot_voices, voice_mask, tags, n, 0, "glide_owned");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = glide_ensure(b))) return rc;
  return start_launch(b, glide, NULL, slot_voices, voice_mask, d_slots, tags, n, d_count_or_null, d_result, "glide_owned", (hipStream_t)stream);
}

int skred_bank_glide_tags(skred_bank_t *b, const skred_glide_t *glide, int first, int count, int slot_voices, uint64_t voice_mask,
                          const uint32_t *tags, int n, uint32_t *d_result, void *stream) {
  int rc = start_check(b, glide, slot_voices, voice_mask, tags, n, SKRED_OWNER_UNIQUE, "glide_tags");
  if (rc) return rc;
  if ((rc = sk_check_slot_range(b->n_voices, first, count, slot_voices, 0, "glide_tags"))) return rc;
  if (n == 0) return SKRED_OK;
  /* the tags travel sorted (the find pass searches them), and glide[k] stays with tags[k]: entry j of the list is the slot of the
   * j-th smallest tag, and receives glide[perm[j]] */
  uint32_t sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  (void)sk_owner_pack(tags, n, sorted, perm);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = glide_ensure(b))) return rc;
  if ((rc = sk_owner_find_launch(b, first, count, slot_voices, sorted, n, b->d_owner_slots, s))) return rc;
  /* entry j is the lowest slot that carries sorted[j], or -1: the guard holds on every entry that is a slot */
  return start_launch(b, glide, perm, slot_voices, voice_mask, b->d_owner_slots, sorted, n, NULL, d_result, "glide_tags", s);
}

int skred_bank_glide_advance(skred_bank_t *b, int first, int count, int num_frames, uint32_t *d_result, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "glide_advance: no bank");
  if (num_frames < 1 || num_frames > 65536) return fail(SKRED_E_BAD_ARG, "glide_advance: num_frames = %d (1 .. 65536)", num_frames);
  const int rc = sk_check_slot_range(b->n_voices, first, count, 1, 0, "glide_advance");
  if (rc) return rc;
  if (!b->d_glide) {                                       /* (no glide was ever started: nobody glides, nobody arrives) */
    if (!d_result) return SKRED_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), (hipStream_t)stream));
    return SKRED_OK;
  }
  HIP_TRY(hipSetDevice(b->device));
  const hipError_t e = (hipError_t)sk_launch_glide_advance(b->d_glide, b->d_bend, b->d_ro[SKP_OSC], first, count, num_frames, d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "glide_advance launch -> %s", hipGetErrorString(e));
  return SKRED_OK;                                         /* (finite increments only: the planner's reports stand) */
}

int skred_bank_glide_stop(skred_bank_t *b, int first, int count, int snap, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "glide_stop: no bank");
  const int rc = sk_check_window(b->n_voices, first, count, "glide_stop");
  if (rc) return rc;
  if (count == 0 || !b->d_glide) return SKRED_OK;          /* (no glide was ever started: every word is 0 already) */
  HIP_TRY(hipSetDevice(b->device));
  const hipError_t e = (hipError_t)sk_launch_glide_stop(b->d_glide, b->d_bend, b->d_ro[SKP_OSC], first, count, snap != 0, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "glide_stop launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_bank_download_glide(skred_bank_t *b, uint32_t *host_u32x4, int first, int count) {
  if (!b || !host_u32x4 || count < 0) return fail(SKRED_E_BAD_ARG, "download_glide: bad arguments");
  return sk_side_download(b->d_glide, sizeof(sk_glide_t), b->device, b->n_voices, host_u32x4, first, count, "download_glide");
}
