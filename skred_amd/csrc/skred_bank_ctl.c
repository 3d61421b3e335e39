/*
 * skred_bank_ctl.c -- patch controllers: a few parameter words of every copy of a tiled patch, changed on the device
 * (include/skred_amd.h: skred_ctl_check, skred_bank_ctl_range / _ctl_slots / _download_ctl).
 *
 * The host side of skred_ctl_kernels.hip, on the pieces of skred_bank_checks.c and skred_bank_stage.c: the checks (made before anything
 * touches the device), the K records' way through the batch path, the launches.  Nothing here waits for the
 * device except the download.  The host's shadow of the bank (h_class, the counters, the lane words, the named set, the tape plan)
 * reads three things about the words a controller stores: whether voice_amp == 0 (SKC_LIVE), whether the increment is finite
 * (SKC_EXOTIC), and the routing.  The checks admit finite values only, the kernel keeps an amp of 0 at 0 and a scaled increment
 * finite, and no routing field can be named: the shadow stays right without the host knowing which voice holds what.  What a call
 * does tell the bank, when a record names a word the motion list depends on, is what every control action tells it: the voices it
 * may have put on the list (touched_total, an upper bound), and that earlier launches' reports are out of date.
 */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "skred_bank_priv.h"

_Static_assert(sizeof(skred_ctl_t) == sizeof(sk_ctl_t) && sizeof(skred_ctl_t) == 96 && offsetof(skred_ctl_t, set) == 4 * SK_CTL_SET &&
               offsetof(skred_ctl_t, phase_inc) == 4 * SK_CTL_W_PHASE_INC && offsetof(skred_ctl_t, inc_scale) == 4 * SK_CTL_W_INC_SCALE &&
               offsetof(skred_ctl_t, amp) == 4 * SK_CTL_W_AMP && offsetof(skred_ctl_t, pan_left) == 4 * SK_CTL_W_PAN_LEFT &&
               offsetof(skred_ctl_t, pan_right) == 4 * SK_CTL_W_PAN_RIGHT && offsetof(skred_ctl_t, b0) == 4 * SK_CTL_W_B0 &&
               offsetof(skred_ctl_t, b1) == 4 * SK_CTL_W_B1 && offsetof(skred_ctl_t, b2) == 4 * SK_CTL_W_B2 &&
               offsetof(skred_ctl_t, a1) == 4 * SK_CTL_W_A1 && offsetof(skred_ctl_t, a2) == 4 * SK_CTL_W_A2 &&
               offsetof(skred_ctl_t, attack_time) == 4 * SK_CTL_W_ATTACK && offsetof(skred_ctl_t, decay_time) == 4 * SK_CTL_W_DECAY &&
               offsetof(skred_ctl_t, sustain_level) == 4 * SK_CTL_W_SUSTAIN && offsetof(skred_ctl_t, release_time) == 4 * SK_CTL_W_RELEASE &&
               offsetof(skred_ctl_t, velocity) == 4 * SK_CTL_W_VELOCITY && offsetof(skred_ctl_t, smoothing) == 4 * SK_CTL_W_SMOOTHING &&
               offsetof(skred_ctl_t, fm_depth) == 4 * SK_CTL_W_FM_DEPTH && offsetof(skred_ctl_t, freq_scale) == 4 * SK_CTL_W_FREQ_SCALE &&
               offsetof(skred_ctl_t, am_depth) == 4 * SK_CTL_W_AM_DEPTH && offsetof(skred_ctl_t, pan_depth) == 4 * SK_CTL_W_PAN_DEPTH &&
               offsetof(skred_ctl_t, cz_depth) == 4 * SK_CTL_W_CZ_DEPTH && offsetof(skred_ctl_t, cz_dist) == 4 * SK_CTL_W_CZ_DIST &&
               offsetof(skred_ctl_t, reserved) == 4 * SK_CTL_W_RESERVED,
               "the device's controller record must be skred_ctl_t word for word");
_Static_assert(SK_CTL_PHASE_INC == SKRED_CTL_PHASE_INC && SK_CTL_INC_SCALE == SKRED_CTL_INC_SCALE && SK_CTL_AMP == SKRED_CTL_AMP &&
               SK_CTL_PAN == SKRED_CTL_PAN && SK_CTL_FILTER == SKRED_CTL_FILTER && SK_CTL_ENV_TIMES == SKRED_CTL_ENV_TIMES &&
               SK_CTL_VELOCITY == SKRED_CTL_VELOCITY && SK_CTL_SMOOTHING == SKRED_CTL_SMOOTHING && SK_CTL_FM_DEPTH == SKRED_CTL_FM_DEPTH &&
               SK_CTL_FREQ_SCALE == SKRED_CTL_FREQ_SCALE && SK_CTL_AM_DEPTH == SKRED_CTL_AM_DEPTH && SK_CTL_PAN_DEPTH == SKRED_CTL_PAN_DEPTH &&
               SK_CTL_CZ_DEPTH == SKRED_CTL_CZ_DEPTH && SK_CTL_CZ_DIST == SKRED_CTL_CZ_DIST,
               "device controller bits must equal the public SKRED_CTL_* values");

/* which words of a record a bit of `set` names (first word, how many) */
static const struct { uint32_t bit; int first, count; const char *name; } ctl_fields[] = {
  { SKRED_CTL_PHASE_INC, SK_CTL_W_PHASE_INC, 1, "phase_inc" }, { SKRED_CTL_INC_SCALE, SK_CTL_W_INC_SCALE, 1, "inc_scale" },
  { SKRED_CTL_AMP, SK_CTL_W_AMP, 1, "amp" },                   { SKRED_CTL_PAN, SK_CTL_W_PAN_LEFT, 2, "pan" },
  { SKRED_CTL_FILTER, SK_CTL_W_B0, 5, "filter" },              { SKRED_CTL_ENV_TIMES, SK_CTL_W_ATTACK, 4, "envelope times" },
  { SKRED_CTL_VELOCITY, SK_CTL_W_VELOCITY, 1, "velocity" },    { SKRED_CTL_SMOOTHING, SK_CTL_W_SMOOTHING, 1, "smoothing" },
  { SKRED_CTL_FM_DEPTH, SK_CTL_W_FM_DEPTH, 1, "fm_depth" },    { SKRED_CTL_FREQ_SCALE, SK_CTL_W_FREQ_SCALE, 1, "freq_scale" },
  { SKRED_CTL_AM_DEPTH, SK_CTL_W_AM_DEPTH, 1, "am_depth" },    { SKRED_CTL_PAN_DEPTH, SK_CTL_W_PAN_DEPTH, 1, "pan_depth" },
  { SKRED_CTL_CZ_DEPTH, SK_CTL_W_CZ_DEPTH, 1, "cz_depth" },    { SKRED_CTL_CZ_DIST, SK_CTL_W_CZ_DIST, 1, "cz_dist" },
};
#define CTL_FIELDS ((int)(sizeof(ctl_fields) / sizeof(ctl_fields[0])))

static int ctl_check_one(const skred_ctl_t *c, int l, const char *who) {
  if (c->set & ~(uint32_t)SK_CTL_ALL) return fail(SKRED_E_BAD_ARG, "%s: record %d: unknown bits in set = 0x%x", who, l, c->set);
  if (!c->set) return fail(SKRED_E_BAD_ARG, "%s: record %d: set is 0 and the voice's mask bit is set", who, l);
  if (c->reserved) return fail(SKRED_E_BAD_ARG, "%s: record %d: the reserved word must be 0", who, l);
  if ((c->set & SKRED_CTL_PHASE_INC) && (c->set & SKRED_CTL_INC_SCALE))
    return fail(SKRED_E_BAD_ARG, "%s: record %d: both SKRED_CTL_PHASE_INC and SKRED_CTL_INC_SCALE", who, l);
  const float *w = (const float *)c;
  for (int k = 0; k < CTL_FIELDS; k++) {
    if (!(c->set & ctl_fields[k].bit)) continue;
    /* a value that is not finite would change a voice's class (sk_pack_voice: SKC_EXOTIC) or poison its state behind the host's back */
    for (int i = 0; i < ctl_fields[k].count; i++)
      if (!isfinite(w[ctl_fields[k].first + i]))
        return fail(SKRED_E_BAD_ARG, "%s: record %d: %s holds %g", who, l, ctl_fields[k].name, (double)w[ctl_fields[k].first + i]);
  }
  /* amp 0 would take the voice out of the voices that can sound (SKC_LIVE) without the planner knowing */
  if ((c->set & SKRED_CTL_AMP) && c->amp == 0.0f) return fail(SKRED_E_BAD_ARG, "%s: record %d: amp == 0 under SKRED_CTL_AMP", who, l);
  return SKRED_OK;
}

static int ctl_check(const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask, const char *who) {
  if (!ctl) return fail(SKRED_E_BAD_ARG, "%s: no controller", who);
  const int rc = sk_check_slot_shape(slot_voices, voice_mask, "voice_mask", who);   /* (the rules of skred_slot_query_t) */
  if (rc) return rc;
  for (int l = 0; l < slot_voices; l++) {
    if (!((voice_mask >> l) & 1)) continue;                /* a record no voice receives is not looked at */
    const int rc1 = ctl_check_one(&ctl[l], l, who);
    if (rc1) return rc1;
  }
  return SKRED_OK;
}

int skred_ctl_check(const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask) { return ctl_check(ctl, slot_voices, voice_mask, "ctl_check"); }

/* The checked records as they travel: the masked ones word for word, the others zeroed (set == 0: what the caller left there is
 * never shipped).  Returns the mask of the voices whose record puts them on the motion list. */
uint64_t sk_ctl_pack(const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask, sk_ctl_t *out) {
  uint64_t lists = 0;
  memset(out, 0, (size_t)slot_voices * sizeof(sk_ctl_t));
  for (int l = 0; l < slot_voices; l++) {
    if (!((voice_mask >> l) & 1)) continue;
    memcpy(&out[l], &ctl[l], sizeof(sk_ctl_t));
    if (ctl[l].set & SK_CTL_LISTS) lists |= 1ull << l;
  }
  return lists;
}

/* the packed records -> a staging slot -> one of the two kernels (d_slots NULL: the range) */
static int ctl_launch(skred_bank_t *b, const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask, int first, int count,
                      const int32_t *d_slots, int n, const uint32_t *d_count, uint32_t *d_result, hipStream_t s) {
  HIP_TRY(hipSetDevice(b->device));
  const size_t bytes = (size_t)slot_voices * sizeof(sk_ctl_t);
  sk_batch_t bt;
  int rc = sk_batch_begin(b, bytes, s, &bt);
  if (rc) return rc;
  const uint64_t lists = sk_ctl_pack(ctl, slot_voices, voice_mask, (sk_ctl_t *)bt.h);
  /* up to 64 workgroups read these few KB from the pinned buffer itself; a bank-wide range is thousands of them, each staging the
   * records into its LDS: wide (skred_bank_stage.c has the measurement) */
  const int64_t lanes = d_slots ? (int64_t)n * slot_voices : (int64_t)count;
  const sk_ctl_t *src = (const sk_ctl_t *)sk_batch_send(b, &bt, bytes, lanes > 64 * 256, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = d_slots
    ? (hipError_t)sk_launch_ctl_slots(src, slot_voices, voice_mask, d_slots, n, d_count, b->n_voices, b->d_ro, b->d_rw,
                                      b->d_mask[b->mask_p], d_result, bt.cnt, bt.done, bt.seq, s)
    : (hipError_t)sk_launch_ctl_range(src, slot_voices, voice_mask, first, count, b->d_ro, b->d_rw, b->d_mask[b->mask_p], d_result,
                                      bt.cnt, bt.done, bt.seq, s);
  if ((rc = sk_batch_end(&bt, e, "controller", s))) return rc;
  /* every voice the call MAY have listed: the slots of the range (or the entries, whether or not each is a slot) times the voices
   * of a slot whose record names a listing word.  FILTER, PAN, the increments and the depths list nobody */
  const uint64_t slots = d_slots ? (uint64_t)n : (uint64_t)(count / slot_voices);
  if (lists) sk_touched(b, slots * (uint64_t)__builtin_popcountll(lists));
  /* (a controller that lists nobody leaves what earlier launches reported about envelope activity true: an empty motion list is
   * still empty, and the block behind a bank-wide filter sweep stays the steady block -- with sk_control_changed here it ran the
   * list's path on an empty list, 0.150 ms instead of 0.139 ms at 2^20 voices) */
  return SKRED_OK;
}

int skred_bank_ctl_range(skred_bank_t *b, const skred_ctl_t *ctl, int first, int count, int slot_voices, uint64_t voice_mask,
                         uint32_t *d_result, void *stream) {
  if (!b) return fail(SKRED_E_BAD_ARG, "ctl_range: no bank");
  int rc = ctl_check(ctl, slot_voices, voice_mask, "ctl_range");
  if (rc) return rc;
  if ((rc = sk_check_slot_range(b->n_voices, first, count, slot_voices, 1, "ctl_range"))) return rc;
  if (count == 0) return SKRED_OK;
  return ctl_launch(b, ctl, slot_voices, voice_mask, first, count, NULL, 0, NULL, d_result, (hipStream_t)stream);
}

int skred_bank_ctl_slots(skred_bank_t *b, const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask, const int32_t *d_slots, int n,
                         const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  if (!b || !d_slots) return fail(SKRED_E_BAD_ARG, "ctl_slots: no bank or no list");
  int rc = sk_check_list_n(n, "ctl_slots");
  if (rc) return rc;
  if ((rc = ctl_check(ctl, slot_voices, voice_mask, "ctl_slots"))) return rc;
  if (n == 0) return SKRED_OK;
  return ctl_launch(b, ctl, slot_voices, voice_mask, 0, 0, d_slots, n, d_count_or_null, d_result, (hipStream_t)stream);
}

static inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int skred_bank_download_ctl(skred_bank_t *b, skred_voice_bank_t *h, int src_first, int dst_first, int count) {
  if (!b || !h || count < 0) return fail(SKRED_E_BAD_ARG, "download_ctl: bad arguments");
  int rc = sk_check_window(b->n_voices, src_first, count, "download_ctl");
  if (rc || (rc = sk_check_window(h->n_voices, dst_first, count, "download_ctl into the host view"))) return rc;
  if (count == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  static const int planes[] = { SKP_OSC, SKP_ENV_T, SKP_GAIN, SKP_FILT, SKP_MODF, SKP_MODX };
  enum { N_RO = (int)(sizeof(planes) / sizeof(planes[0])) };
  sk_plane_t *st = (sk_plane_t *)malloc((size_t)(N_RO + 1) * (size_t)count * sizeof(sk_plane_t));
  if (!st) return fail(SKRED_E_NO_MEM, "download_ctl staging");
  const size_t bytes = (size_t)count * sizeof(sk_plane_t);
  hipError_t e = hipDeviceSynchronize();
  for (int k = 0; k < N_RO && e == hipSuccess; k++)
    e = hipMemcpy(st + (size_t)k * count, b->d_ro[planes[k]] + src_first, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(st + (size_t)N_RO * count, b->d_rw[SKS_MISC] + src_first, bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { free(st); HIP_TRY(e); }
  for (int i = 0; i < count; i++) {
    const int v = dst_first + i;
    const sk_plane_t *osc = &st[i], *et = &st[(size_t)count + i], *gn = &st[(size_t)2 * count + i], *fl = &st[(size_t)3 * count + i];
    const sk_plane_t *mf = &st[(size_t)4 * count + i], *mx = &st[(size_t)5 * count + i], *misc = &st[(size_t)6 * count + i];
    skred_envelope_t *env = &h->voice_amp_envelope[v];
    skred_mmf_t *f = &h->voice_filter[v];
    h->voice_phase_inc[v] = u2f(osc->w[0]); h->voice_amp[v] = u2f(osc->w[3]);
    env->attack_time = u2f(et->w[0]); env->decay_time = u2f(et->w[1]); env->sustain_level = u2f(et->w[2]); env->release_time = u2f(et->w[3]);
    env->velocity = u2f(gn->w[0]); h->voice_smoother_smoothing[v] = u2f(gn->w[1]);
    f->b0 = u2f(gn->w[2]); f->b1 = u2f(gn->w[3]); f->b2 = u2f(fl->w[0]); f->a1 = u2f(fl->w[1]); f->a2 = u2f(fl->w[2]);
    h->voice_cz_distortion[v] = u2f(fl->w[3]);
    h->voice_freq_mod_depth[v] = u2f(mf->w[0]); h->voice_freq_scale[v] = u2f(mf->w[1]);
    h->voice_amp_mod_depth[v] = u2f(mf->w[2]);  h->voice_pan_mod_depth[v] = u2f(mf->w[3]);
    h->voice_cz_mod_depth[v] = u2f(mx->w[0]);
    h->voice_pan_left[v] = u2f(misc->w[2]); h->voice_pan_right[v] = u2f(misc->w[3]);
  }
  free(st);
  return SKRED_OK;
}
