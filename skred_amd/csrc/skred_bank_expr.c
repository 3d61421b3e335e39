/*
 * skred_bank_expr.c -- channels and per-note expression: masked owner matches and per-entry controller values
 * (include/skred_amd.h: skred_owner_match_check, skred_ctl_each_check, skred_bank_find_match / _find_match_host / _stamp_match /
 * _ctl_match / _ctl_owned_each / _ctl_tags_each), and per-note timbre: the same two calls with per-entry filter coefficients
 * (skred_filter_each_check, skred_bank_ctl_owned_each_filter / _ctl_tags_each_filter, skred_filter_coeffs).
 *
 * The host side of skred_expr_kernels.hip, on the pieces of skred_bank_checks.c and skred_bank_stage.c (and the owner array of
 * skred_bank_owner.c): the checks (made before anything touches the device), the records', entries' and tags' way through the batch
 * path, the launches.  Nothing here waits for the device except _find_match_host, which waits for its stream, and the allocation of the
 * owner array by the first call that needs it.  What the two range calls tell the bank is what their unguarded twins tell it about
 * the same range -- the host cannot know how many slots match, and the bound behind the in-place rule only has to hold: stamp_match
 * always grows it, ctl_match only when a record names a listing word, and a controller that lists nobody leaves the reports alone
 * (skred_bank_ctl.c has the measurement behind that).
 *
 * Out of scope: the fixed-point bank, the drop-in mode, deferred items and pattern steps.
 */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(sizeof(skred_ctl_each_t) == sizeof(sk_each_t) && sizeof(skred_ctl_each_t) == 32 && offsetof(skred_ctl_each_t, set) == 4 * SK_EACH_SET &&
               offsetof(skred_ctl_each_t, inc_scale) == 4 * SK_EACH_W_INC_SCALE && offsetof(skred_ctl_each_t, amp_scale) == 4 * SK_EACH_W_AMP_SCALE &&
               offsetof(skred_ctl_each_t, velocity) == 4 * SK_EACH_W_VELOCITY && offsetof(skred_ctl_each_t, pan_left) == 4 * SK_EACH_W_PAN_LEFT &&
               offsetof(skred_ctl_each_t, pan_right) == 4 * SK_EACH_W_PAN_RIGHT && offsetof(skred_ctl_each_t, reserved) == 24,
               "the device's per-entry record must be skred_ctl_each_t word for word");
_Static_assert(SK_EACH_INC_SCALE == SKRED_EACH_INC_SCALE && SK_EACH_AMP_SCALE == SKRED_EACH_AMP_SCALE && SK_EACH_VELOCITY == SKRED_EACH_VELOCITY &&
               SK_EACH_PAN == SKRED_EACH_PAN, "device per-entry bits must equal the public SKRED_EACH_* values");
_Static_assert(sizeof(sk_ctl_t) % 32 == 0, "the entries behind the K records stay 16-byte aligned");

_Static_assert(sizeof(skred_filter_each_t) == sizeof(sk_filt_each_t) && sizeof(skred_filter_each_t) == 32 && offsetof(skred_filter_each_t, b0) == 4 * SK_FILT_W_B0 &&
               offsetof(skred_filter_each_t, b1) == 4 * SK_FILT_W_B1 && offsetof(skred_filter_each_t, b2) == 4 * SK_FILT_W_B2 &&
               offsetof(skred_filter_each_t, a1) == 4 * SK_FILT_W_A1 && offsetof(skred_filter_each_t, a2) == 4 * SK_FILT_W_A2 &&
               offsetof(skred_filter_each_t, reserved) == 20, "the device's per-entry filter record must be skred_filter_each_t word for word");

/* the entry bits that put a voice on the motion list (AMP_SCALE stores voice_amp, VELOCITY the envelope's velocity) */
#define SK_EACH_LISTS (SKRED_EACH_AMP_SCALE | SKRED_EACH_VELOCITY)

static int match_check(const skred_owner_match_t *m, const char *who) {
  if (!m) return fail(SKRED_E_BAD_ARG, "%s: no match", who);
  if (m->value & ~m->mask) return fail(SKRED_E_BAD_ARG, "%s: value = 0x%x has bits outside mask = 0x%x: no owner word can give it", who, m->value, m->mask);
  return SKRED_OK;
}

int skred_owner_match_check(const skred_owner_match_t *m) { return match_check(m, "owner_match_check"); }

static int each_check(const skred_ctl_each_t *each, int n, const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask, const char *who) {
  if (!each) return fail(SKRED_E_BAD_ARG, "%s: no entries", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  int rc;
  if (ctl) { if ((rc = skred_ctl_check(ctl, slot_voices, voice_mask))) return rc; }
  else if ((rc = sk_check_slot_shape(slot_voices, voice_mask, "voice_mask", who))) return rc;
  /* what the masked records name: every one (AMP_SCALE needs AMP on all of them), any one (INC_SCALE needs no increment on any) */
  uint32_t all = ctl ? ~0u : 0u, any = 0;
  for (int l = 0; ctl && l < slot_voices; l++)
    if ((voice_mask >> l) & 1) { all &= ctl[l].set; any |= ctl[l].set; }
  for (int k = 0; k < n; k++) {
    const skred_ctl_each_t *e = &each[k];
    if (e->set & ~(uint32_t)SK_EACH_ALL) return fail(SKRED_E_BAD_ARG, "%s: entry %d: unknown bits in set = 0x%x", who, k, e->set);
    if (!e->set) return fail(SKRED_E_BAD_ARG, "%s: entry %d: set is 0", who, k);
    if (e->reserved[0] || e->reserved[1]) return fail(SKRED_E_BAD_ARG, "%s: entry %d: the reserved words must be 0", who, k);
    if ((e->set & SKRED_EACH_INC_SCALE) && !isfinite(e->inc_scale)) return fail(SKRED_E_BAD_ARG, "%s: entry %d: inc_scale holds %g", who, k, (double)e->inc_scale);
    if ((e->set & SKRED_EACH_AMP_SCALE) && !isfinite(e->amp_scale)) return fail(SKRED_E_BAD_ARG, "%s: entry %d: amp_scale holds %g", who, k, (double)e->amp_scale);
    if ((e->set & SKRED_EACH_VELOCITY) && !isfinite(e->velocity)) return fail(SKRED_E_BAD_ARG, "%s: entry %d: velocity holds %g", who, k, (double)e->velocity);
    if ((e->set & SKRED_EACH_PAN) && (!isfinite(e->pan_left) || !isfinite(e->pan_right)))
      return fail(SKRED_E_BAD_ARG, "%s: entry %d: pan holds %g, %g", who, k, (double)e->pan_left, (double)e->pan_right);
    if (e->set & SKRED_EACH_AMP_SCALE) {
      /* amp 0 would take the voice out of the voices that can sound without the planner knowing (skred_bank_ctl.c) */
      if (e->amp_scale == 0.0f) return fail(SKRED_E_BAD_ARG, "%s: entry %d: amp_scale == 0", who, k);
      if (!(all & SKRED_CTL_AMP)) return fail(SKRED_E_BAD_ARG, "%s: entry %d: SKRED_EACH_AMP_SCALE and a masked record without SKRED_CTL_AMP", who, k);
    }
    if ((e->set & SKRED_EACH_INC_SCALE) && (any & (SKRED_CTL_PHASE_INC | SKRED_CTL_INC_SCALE)))
      return fail(SKRED_E_BAD_ARG, "%s: entry %d: SKRED_EACH_INC_SCALE and a masked record that names an increment", who, k);
  }
  return SKRED_OK;
}

int skred_ctl_each_check(const skred_ctl_each_t *each, int n, const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask) {
  return each_check(each, n, ctl, slot_voices, voice_mask, "ctl_each_check");
}

/* The checked entries as they travel: out[j] = each[perm[j]] (perm NULL: j), the named values word for word, the others zeroed.
 * Returns the entry bits of all of them together.  Pure host */
uint32_t sk_each_pack(const skred_ctl_each_t *each, int n, const uint32_t *perm, sk_each_t *out) {
  uint32_t bits = 0;
  memset(out, 0, (size_t)n * sizeof(sk_each_t));
  for (int j = 0; j < n; j++) {
    const skred_ctl_each_t *e = &each[perm ? perm[j] : (uint32_t)j];
    uint32_t *w = out[j].w;
    w[SK_EACH_SET] = e->set;
    if (e->set & SKRED_EACH_INC_SCALE) memcpy(&w[SK_EACH_W_INC_SCALE], &e->inc_scale, 4);
    if (e->set & SKRED_EACH_AMP_SCALE) memcpy(&w[SK_EACH_W_AMP_SCALE], &e->amp_scale, 4);
    if (e->set & SKRED_EACH_VELOCITY) memcpy(&w[SK_EACH_W_VELOCITY], &e->velocity, 4);
    if (e->set & SKRED_EACH_PAN) { memcpy(&w[SK_EACH_W_PAN_LEFT], &e->pan_left, 4); memcpy(&w[SK_EACH_W_PAN_RIGHT], &e->pan_right, 4); }
    bits |= e->set;
  }
  return bits;
}

/* K, the two masks and the records first (what each_check looks at before its entries), then the coefficients */
static int filter_check(const skred_filter_each_t *filt, int n, const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask, uint64_t filter_mask,
                        const char *who) {
  if (!filt) return fail(SKRED_E_BAD_ARG, "%s: no coefficients", who);
  if (n < 0) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  int rc;
  if (ctl) { if ((rc = skred_ctl_check(ctl, slot_voices, voice_mask))) return rc; }
  else if ((rc = sk_check_slot_shape(slot_voices, voice_mask, "voice_mask", who))) return rc;
  if (!filter_mask) return fail(SKRED_E_BAD_ARG, "%s: filter_mask is 0", who);
  if (filter_mask & ~voice_mask) return fail(SKRED_E_BAD_ARG, "%s: filter_mask = 0x%llx has bits outside voice_mask = 0x%llx", who,
                                             (unsigned long long)filter_mask, (unsigned long long)voice_mask);
  for (int l = 0; ctl && l < slot_voices; l++)
    if (((filter_mask >> l) & 1) && (ctl[l].set & SKRED_CTL_FILTER))
      return fail(SKRED_E_BAD_ARG, "%s: record %d names SKRED_CTL_FILTER and bit %d of filter_mask is set: two sets of coefficients", who, l, l);
  for (int k = 0; k < n; k++) {
    const skred_filter_each_t *f = &filt[k];
    if (f->reserved[0] || f->reserved[1] || f->reserved[2]) return fail(SKRED_E_BAD_ARG, "%s: coefficients %d: the reserved words must be 0", who, k);
    if (!isfinite(f->b0) || !isfinite(f->b1) || !isfinite(f->b2) || !isfinite(f->a1) || !isfinite(f->a2))
      return fail(SKRED_E_BAD_ARG, "%s: coefficients %d hold %g %g %g %g %g", who, k, (double)f->b0, (double)f->b1, (double)f->b2, (double)f->a1,
                  (double)f->a2);
  }
  return SKRED_OK;
}

int skred_filter_each_check(const skred_filter_each_t *filt, int n, const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask,
                            uint64_t filter_mask) {
  return filter_check(filt, n, ctl, slot_voices, voice_mask, filter_mask, "filter_each_check");
}

/* The checked coefficients as they travel: out[j] = filt[perm[j]] (perm NULL: j), the five words as they stand, the rest zero.  Pure host */
void sk_filt_pack(const skred_filter_each_t *filt, int n, const uint32_t *perm, sk_filt_each_t *out) {
  memset(out, 0, (size_t)n * sizeof(sk_filt_each_t));
  for (int j = 0; j < n; j++) memcpy(out[j].w, &filt[perm ? perm[j] : (uint32_t)j], 5 * sizeof(uint32_t));
}

/* mmf_set_params' arithmetic (skred_synth_dropin.c calls this): fp32 throughout, every product, sum and quotient rounded on its own
 * -- the Makefile builds this file with -ffp-contract=off, as it builds the drop-in's */
int skred_filter_coeffs(int mode, float freq, float resonance, float sample_rate, float out5[5]) {
  if (!out5) return fail(SKRED_E_BAD_ARG, "filter_coeffs: nowhere to put the coefficients");
  if (mode == 0) return 1;                                    /* bypassed: nothing computed */
  const float w = 2.0f * (float)M_PI * freq / sample_rate;
  const float sn = sinf(w), cs = cosf(w);
  const float alpha = sn / (2.0f * resonance);
  const float a0 = 1.0f + alpha;
  float b0, b1, b2;
  switch (mode) {
    case 2:  b0 = (1.0f + cs) / 2.0f; b1 = -(1.0f + cs); b2 = (1.0f + cs) / 2.0f; break;   /* high-pass */
    case 3:  b0 = alpha; b1 = 0.0f; b2 = -alpha; break;                                    /* band-pass */
    case 4:  b0 = 1.0f; b1 = -2.0f * cs; b2 = 1.0f; break;                                 /* notch */
    case 5:  b0 = 1.0f - alpha; b1 = -2.0f * cs; b2 = 1.0f + alpha; break;                 /* all-pass */
    default: b0 = (1.0f - cs) / 2.0f; b1 = 1.0f - cs; b2 = (1.0f - cs) / 2.0f; break;      /* low-pass; also any unknown mode */
  }
  out5[0] = b0 / a0; out5[1] = b1 / a0; out5[2] = b2 / a0;
  out5[3] = (-2.0f * cs) / a0;
  out5[4] = (1.0f - alpha) / a0;
  return SKRED_OK;
}

/* ---- A. masked owner matches ---- */

static int find_match_check(const skred_bank_t *b, int first, int count, int K, const skred_owner_match_t *m, int max_out,
                            const void *slots, const void *total, const char *who) {
  if (!b) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  int rc = match_check(m, who);
  if (rc) return rc;
  if (!total) return fail(SKRED_E_BAD_ARG, "%s: nowhere to put the count", who);
  if (max_out < 0) return fail(SKRED_E_BAD_ARG, "%s: max_out %d", who, max_out);
  if (max_out > 0 && !slots) return fail(SKRED_E_BAD_ARG, "%s: max_out %d and no list to fill", who, max_out);
  if ((rc = sk_check_slot_shape(K, 0, NULL, who))) return rc;
  return sk_check_slot_range(b->n_voices, first, count, K, 0, who);
}

/* count and scatter of the matching slots of a checked range; the count pass's (written, total) pair goes to the words behind the
 * owner array, the total where the caller wants it */
static int find_match_launch(skred_bank_t *b, int first, int count, int K, const skred_owner_match_t *m, int max_out, int32_t *d_slots,
                             uint32_t *d_total, hipStream_t s) {
  int rc = sk_owner_ensure(b);
  if (rc) return rc;
  if ((rc = sk_idle_scratch(b, s))) return rc;
  sk_match_args_t a;
  memset(&a, 0, sizeof(a));
  sk_idle_args(b, &a.idle, first, count, first, max_out, 0, 0.0f, d_slots, b->d_match_pair);
  a.owner = b->d_owner;
  a.d_total = d_total;
  a.value = m->value;
  a.mask = m->mask;
  const hipError_t e = (hipError_t)sk_launch_match_find(&a, first, count, K, s);   /* (count / K lanes: never more workgroups than the scratch holds) */
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "find_match launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_bank_find_match(skred_bank_t *b, int first, int count, int slot_voices, const skred_owner_match_t *m, int max_out,
                          int32_t *d_slots, uint32_t *d_count, void *stream) {
  const int rc = find_match_check(b, first, count, slot_voices, m, max_out, d_slots, d_count, "find_match");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(b->device));
  return find_match_launch(b, first, count, slot_voices, m, max_out, d_slots, d_count, (hipStream_t)stream);
}

int skred_bank_find_match_host(skred_bank_t *b, int first, int count, int slot_voices, const skred_owner_match_t *m, int max_out,
                               int32_t *slots, int *total_out, void *stream) {
  int dummy = 0;
  int rc = find_match_check(b, first, count, slot_voices, m, max_out, slots, &dummy, "find_match_host");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_idle_out_room(b, (size_t)max_out))) return rc;
  /* word 0: the total; the list from word 2, as the idle queries lay their answer out */
  if ((rc = find_match_launch(b, first, count, slot_voices, m, max_out, b->d_idle_out + 2, (uint32_t *)b->d_idle_out, s))) return rc;
  const int written = sk_read_back(b->d_idle_out, b->h_idle_out, 2, max_out, count / slot_voices, slots, s, "find_match_host");
  if (written >= 0 && total_out) *total_out = b->h_idle_out[0];
  return written;
}

int skred_bank_stamp_match(skred_bank_t *b, int first, int count, int slot_voices, uint64_t voice_mask, const skred_owner_match_t *m,
                           uint32_t stamps, uint32_t *d_result, void *stream) {
  if (!b || !d_result) return fail(SKRED_E_BAD_ARG, "stamp_match: no bank or no result");
  int rc = match_check(m, "stamp_match");
  if (rc) return rc;
  if ((rc = sk_check_stamps(stamps, "stamp_match"))) return rc;
  if ((rc = sk_check_slot_shape(slot_voices, voice_mask, "voice_mask", "stamp_match"))) return rc;
  if ((rc = sk_check_slot_range(b->n_voices, first, count, slot_voices, 0, "stamp_match"))) return rc;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_owner_ensure(b))) return rc;
  const hipError_t e = (hipError_t)sk_launch_match_stamps(b->d_owner, m->value, m->mask, first, count, slot_voices, voice_mask, stamps, b->d_ro,
                                                          b->d_rw, b->g.synth_sample_count, b->d_mask[b->mask_p], d_result, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "stamp_match launch -> %s", hipGetErrorString(e));
  /* every slot of the range may match: what skred_bank_stamp_slots on all of them would add */
  sk_touched(b, (uint64_t)(count / slot_voices) * (uint64_t)__builtin_popcountll(voice_mask));
  return SKRED_OK;
}

int skred_bank_ctl_match(skred_bank_t *b, const skred_ctl_t *ctl, int first, int count, int slot_voices, uint64_t voice_mask,
                         const skred_owner_match_t *m, uint32_t *d_result, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "ctl_match: no bank");
  int rc = skred_ctl_check(ctl, slot_voices, voice_mask);
  if (rc) return rc;
  if ((rc = match_check(m, "ctl_match"))) return rc;
  if ((rc = sk_check_slot_range(b->n_voices, first, count, slot_voices, 0, "ctl_match"))) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_owner_ensure(b))) return rc;
  const size_t bytes = (size_t)slot_voices * sizeof(sk_ctl_t);
  sk_batch_t bt;
  if ((rc = sk_batch_begin(b, bytes, s, &bt))) return rc;
  const uint64_t lists = sk_ctl_pack(ctl, slot_voices, voice_mask, (sk_ctl_t *)bt.h);
  /* (skred_bank_ctl.c: beyond 64 workgroups the records are read from the device, not over the bus) */
  const sk_ctl_t *src = (const sk_ctl_t *)sk_batch_send(b, &bt, bytes, count > 64 * SK_CONTROL_SPAN, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)sk_launch_ctl_match(src, slot_voices, voice_mask, first, count, b->d_owner, m->value, m->mask, b->d_ro, b->d_rw,
                                                       b->d_mask[b->mask_p], d_result, bt.cnt, bt.done, bt.seq, s);
  if ((rc = sk_batch_end(&bt, e, "ctl_match", s))) return rc;
  /* (a controller that lists nobody leaves the reports alone: skred_bank_ctl.c) */
  if (lists) sk_touched(b, (uint64_t)(count / slot_voices) * (uint64_t)__builtin_popcountll(lists));
  return SKRED_OK;
}

/* ---- B. per-entry controller values ---- */

/* with_filter: a call of section C -- `each` may be NULL, `filt` may not, and the coefficients are checked behind the entries */
static int owned_each_check(const skred_bank_t *b, const skred_ctl_t *ctl, const skred_ctl_each_t *each, const skred_filter_each_t *filt,
                            int with_filter, int slot_voices, uint64_t voice_mask, uint64_t filter_mask, const uint32_t *tags, int n,
                            uint32_t tag_flags, const char *who) {
  if (!b) return fail(SKRED_E_BAD_ARG, "%s: no bank", who);
  int rc = skred_owner_tags_check(tags, n, tag_flags);
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, who))) return rc;
  if (!with_filter) return each_check(each, n, ctl, slot_voices, voice_mask, who);
  if (each && (rc = each_check(each, n, ctl, slot_voices, voice_mask, who))) return rc;
  return filter_check(filt, n, ctl, slot_voices, voice_mask, filter_mask, who);
}

/* the K records (zeros without `ctl`), the n entries (each[perm[j]]; perm NULL: as they stand), with `filt` the n sets of coefficients
 * (permuted likewise; then `each` may be NULL and no entries travel) and the n tags in one staging slot: one kernel reads them all */
static int owned_each_launch(skred_bank_t *b, const skred_ctl_t *ctl, const skred_ctl_each_t *each, const skred_filter_each_t *filt,
                             const uint32_t *perm, int slot_voices, uint64_t voice_mask, uint64_t filter_mask, const int32_t *d_slots,
                             const uint32_t *tags, int n, const uint32_t *d_count, uint32_t *d_result, const char *what, hipStream_t s) {
  const size_t rec_bytes = (size_t)slot_voices * sizeof(sk_ctl_t), each_bytes = each ? (size_t)n * sizeof(sk_each_t) : 0;
  const size_t filt_bytes = filt ? (size_t)n * sizeof(sk_filt_each_t) : 0;
  const size_t bytes = rec_bytes + each_bytes + filt_bytes + (size_t)n * sizeof(uint32_t);
  const int wide = (int64_t)n * slot_voices > 64 * SK_CONTROL_SPAN;
  sk_batch_t bt;
  int rc = sk_batch_begin(b, bytes, s, &bt);
  if (rc) return rc;
  char *h = (char *)bt.h;
  uint64_t lists = 0;
  if (ctl) lists = sk_ctl_pack(ctl, slot_voices, voice_mask, (sk_ctl_t *)h);
  else memset(h, 0, rec_bytes);
  const uint32_t bits = each ? sk_each_pack(each, n, perm, (sk_each_t *)(h + rec_bytes)) : 0u;
  if (filt) sk_filt_pack(filt, n, perm, (sk_filt_each_t *)(h + rec_bytes + each_bytes));
  memcpy(h + rec_bytes + each_bytes + filt_bytes, tags, (size_t)n * sizeof(uint32_t));
  const char *src = (const char *)sk_batch_send(b, &bt, bytes, wide, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)sk_launch_ctl_owned_each_filter((const sk_ctl_t *)src, each ? (const sk_each_t *)(src + rec_bytes) : NULL,
                                                                   filt ? (const sk_filt_each_t *)(src + rec_bytes + each_bytes) : NULL,
                                                                   slot_voices, voice_mask, filter_mask, d_slots,
                                                                   (const uint32_t *)(src + rec_bytes + each_bytes + filt_bytes), b->d_owner, n,
                                                                   d_count, b->n_voices, b->d_ro, b->d_rw, b->d_mask[b->mask_p], d_result,
                                                                   bt.cnt, bt.done, bt.seq, s);
  if ((rc = sk_batch_end(&bt, e, what, s))) return rc;
  if (lists || (bits & SK_EACH_LISTS)) sk_touched(b, (uint64_t)n * (uint64_t)__builtin_popcountll(voice_mask));
  return SKRED_OK;
}

static int owned_each_call(skred_bank_t *b, const skred_ctl_t *ctl, const skred_ctl_each_t *each, const skred_filter_each_t *filt, int with_filter,
                           int slot_voices, uint64_t voice_mask, uint64_t filter_mask, const int32_t *d_slots, const uint32_t *tags, int n,
                           const uint32_t *d_count_or_null, uint32_t *d_result, const char *who, void *stream) {
  if (!d_slots) return fail(SKRED_E_BAD_ARG, "%s: no list", who);
  int rc = owned_each_check(b, ctl, each, filt, with_filter, slot_voices, voice_mask, filter_mask, tags, n, 0, who);
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_owner_ensure(b))) return rc;
  return owned_each_launch(b, ctl, each, filt, NULL, slot_voices, voice_mask, filter_mask, d_slots, tags, n, d_count_or_null, d_result, who,
                           (hipStream_t)stream);
}

static int tags_each_call(skred_bank_t *b, const skred_ctl_t *ctl, const skred_ctl_each_t *each, const skred_filter_each_t *filt, int with_filter,
                          int first, int count, int slot_voices, uint64_t voice_mask, uint64_t filter_mask, const uint32_t *tags, int n,
                          uint32_t *d_result, const char *who, void *stream) {
  int rc = owned_each_check(b, ctl, each, filt, with_filter, slot_voices, voice_mask, filter_mask, tags, n, SKRED_OWNER_UNIQUE, who);
  if (rc) return rc;
  if ((rc = sk_check_slot_range(b->n_voices, first, count, slot_voices, 0, who))) return rc;
  if (n == 0) return SKRED_OK;
  /* the tags travel sorted (the find pass searches them), and each[k] and filt[k] stay with tags[k]: entry j of the list is the slot
   * of the j-th smallest tag, and receives each[perm[j]] and filt[perm[j]] */
  uint32_t sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  (void)sk_owner_pack(tags, n, sorted, perm);
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = sk_owner_ensure(b))) return rc;
  if ((rc = skred_bank_find_owned(b, first, count, slot_voices, sorted, n, b->d_owner_slots, stream))) return rc;
  /* entry j is the lowest slot that carries sorted[j], or -1: the guard holds on every entry that is a slot */
  return owned_each_launch(b, ctl, each, filt, perm, slot_voices, voice_mask, filter_mask, b->d_owner_slots, sorted, n, NULL, d_result, who,
                           (hipStream_t)stream);
}

int skred_bank_ctl_owned_each(skred_bank_t *b, const skred_ctl_t *ctl, const skred_ctl_each_t *each, int slot_voices, uint64_t voice_mask,
                              const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result,
                              void *stream) {
  return owned_each_call(b, ctl, each, NULL, 0, slot_voices, voice_mask, 0, d_slots, tags, n, d_count_or_null, d_result, "ctl_owned_each", stream);
}

int skred_bank_ctl_tags_each(skred_bank_t *b, const skred_ctl_t *ctl, const skred_ctl_each_t *each, int first, int count, int slot_voices,
                             uint64_t voice_mask, const uint32_t *tags, int n, uint32_t *d_result, void *stream) {
  return tags_each_call(b, ctl, each, NULL, 0, first, count, slot_voices, voice_mask, 0, tags, n, d_result, "ctl_tags_each", stream);
}

/* ---- C. per-entry filter coefficients ---- */

int skred_bank_ctl_owned_each_filter(skred_bank_t *b, const skred_ctl_t *ctl, const skred_ctl_each_t *each, const skred_filter_each_t *filt,
                                     int slot_voices, uint64_t voice_mask, uint64_t filter_mask, const int32_t *d_slots, const uint32_t *tags,
                                     int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  return owned_each_call(b, ctl, each, filt, 1, slot_voices, voice_mask, filter_mask, d_slots, tags, n, d_count_or_null, d_result,
                         "ctl_owned_each_filter", stream);
}

int skred_bank_ctl_tags_each_filter(skred_bank_t *b, const skred_ctl_t *ctl, const skred_ctl_each_t *each, const skred_filter_each_t *filt,
                                    int first, int count, int slot_voices, uint64_t voice_mask, uint64_t filter_mask, const uint32_t *tags,
                                    int n, uint32_t *d_result, void *stream) {
  return tags_each_call(b, ctl, each, filt, 1, first, count, slot_voices, voice_mask, filter_mask, tags, n, d_result, "ctl_tags_each_filter",
                        stream);
}
