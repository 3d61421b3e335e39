/*
 * skred_fx_ctl.c -- controllers of the fixed-point bank: a few parameter words of resident voices, changed on the device
 * (include/skred_amd_fxpt.h: skred_fx_ctl_check, skred_fxbank_ctl_range / _ctl_list / _ctl_owned).
 *
 * The host side of skred_fx_ctl_kernels.hip, built like skred_fx_live.c: the checks (made before anything touches the device), the
 * record's -- and for the guarded form the tags' -- way through the batch path (skred_fx_stage.c), one launch.  Nothing here waits for the device.
 * The bank keeps no shadow of the voices; the one thing the host knows about them, n_filter (which selects the biquad
 * instantiation), counts voices with filter_mode != 0, and no controller can name filter_mode: it stays right by construction.
 * The bank has no slots: one record, every call per voice.
 */
#include <stddef.h>
#include <string.h>

#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

_Static_assert(sizeof(skred_fx_ctl_t) == sizeof(skx_ctl_t) && sizeof(skred_fx_ctl_t) == 80 && offsetof(skred_fx_ctl_t, which) == 4 * SKX_CTL_WHICH &&
               offsetof(skred_fx_ctl_t, phase_inc) == 4 * SKX_CTL_PHASE_INC && offsetof(skred_fx_ctl_t, inc_scale_q16) == 4 * SKX_CTL_INC_SCALE &&
               offsetof(skred_fx_ctl_t, amp_q15) == 4 * SKX_CTL_AMP && offsetof(skred_fx_ctl_t, pan_left_q15) == 4 * SKX_CTL_PAN_LEFT &&
               offsetof(skred_fx_ctl_t, pan_right_q15) == 4 * SKX_CTL_PAN_RIGHT && offsetof(skred_fx_ctl_t, b0_q30) == 4 * SKX_CTL_B0 &&
               offsetof(skred_fx_ctl_t, b1_q30) == 4 * SKX_CTL_B1 && offsetof(skred_fx_ctl_t, b2_q30) == 4 * SKX_CTL_B2 &&
               offsetof(skred_fx_ctl_t, a1_q30) == 4 * SKX_CTL_A1 && offsetof(skred_fx_ctl_t, a2_q30) == 4 * SKX_CTL_A2 &&
               offsetof(skred_fx_ctl_t, attack_frames) == 4 * SKX_CTL_ATTACK && offsetof(skred_fx_ctl_t, decay_frames) == 4 * SKX_CTL_DECAY &&
               offsetof(skred_fx_ctl_t, release_frames) == 4 * SKX_CTL_RELEASE && offsetof(skred_fx_ctl_t, sustain_q15) == 4 * SKX_CTL_SUSTAIN &&
               offsetof(skred_fx_ctl_t, velocity_q15) == 4 * SKX_CTL_VELOCITY && offsetof(skred_fx_ctl_t, smoother_k_q15) == 4 * SKX_CTL_SMOOTHING &&
               offsetof(skred_fx_ctl_t, reserved) == 4 * SKX_CTL_RECIP_A,
               "the device's controller record must be skred_fx_ctl_t word for word");
/* the kernels spell the public bits out (skred_fx_ctl_common.hpp: SKX_C_*) */
_Static_assert(SKRED_CTL_PHASE_INC == 1u << 0 && SKRED_CTL_INC_SCALE == 1u << 1 && SKRED_CTL_AMP == 1u << 2 && SKRED_CTL_PAN == 1u << 3 &&
               SKRED_CTL_FILTER == 1u << 4 && SKRED_CTL_ENV_TIMES == 1u << 5 && SKRED_CTL_VELOCITY == 1u << 6 && SKRED_CTL_SMOOTHING == 1u << 7,
               "device controller bits must equal the public SKRED_CTL_* values");

#define SKX_CTL_FIELDS (SKRED_CTL_PHASE_INC | SKRED_CTL_INC_SCALE | SKRED_CTL_AMP | SKRED_CTL_PAN | SKRED_CTL_FILTER | SKRED_CTL_ENV_TIMES | \
                        SKRED_CTL_VELOCITY | SKRED_CTL_SMOOTHING)
#define SKX_CTL_MODULATORS (SKRED_CTL_FM_DEPTH | SKRED_CTL_FREQ_SCALE | SKRED_CTL_AM_DEPTH | SKRED_CTL_PAN_DEPTH | SKRED_CTL_CZ_DEPTH | \
                            SKRED_CTL_CZ_DIST)

static int ctl_check(const skred_fx_ctl_t *c, const char *who) {
  if (!c) return fail(SKRED_E_BAD_ARG, "%s: no controller", who);
  if (c->which & SKX_CTL_MODULATORS)
    return fail(SKRED_E_BAD_ARG, "%s: which = 0x%x names a depth, scale or CZ field -- the fixed-point definition has no modulators", who, c->which);
  if (c->which & ~(uint32_t)SKX_CTL_FIELDS) return fail(SKRED_E_BAD_ARG, "%s: unknown bits in which = 0x%x", who, c->which);
  if (!c->which) return fail(SKRED_E_BAD_ARG, "%s: which is 0", who);
  if (c->reserved[0] || c->reserved[1] || c->reserved[2]) return fail(SKRED_E_BAD_ARG, "%s: reserved words must be 0", who);
  /* amp 0 would take the voice out of the voices that can sound; a voice whose amp is 0 keeps it (the kernel's guard) */
  if ((c->which & SKRED_CTL_AMP) && (c->amp_q15 < 1 || c->amp_q15 > 65535))
    return fail(SKRED_E_BAD_ARG, "%s: amp_q15 %d outside 1..65535", who, c->amp_q15);
  if ((c->which & SKRED_CTL_PAN) && (c->pan_left_q15 < 0 || c->pan_left_q15 > 65535 || c->pan_right_q15 < 0 || c->pan_right_q15 > 65535))
    return fail(SKRED_E_BAD_ARG, "%s: pan (%d, %d) outside 0..65535", who, c->pan_left_q15, c->pan_right_q15);
  if ((c->which & SKRED_CTL_ENV_TIMES) && (c->sustain_q15 < 0 || c->sustain_q15 > 32768))
    return fail(SKRED_E_BAD_ARG, "%s: sustain_q15 %d outside 0..32768", who, c->sustain_q15);
  if ((c->which & SKRED_CTL_VELOCITY) && (c->velocity_q15 < 0 || c->velocity_q15 > 65535))
    return fail(SKRED_E_BAD_ARG, "%s: velocity_q15 %d outside 0..65535", who, c->velocity_q15);
  if ((c->which & SKRED_CTL_SMOOTHING) && (c->smoother_k_q15 < 0 || c->smoother_k_q15 > 32768))
    return fail(SKRED_E_BAD_ARG, "%s: smoother_k_q15 %d outside 0..32768", who, c->smoother_k_q15);
  return SKRED_OK;
}

int skred_fx_ctl_check(const skred_fx_ctl_t *ctl) { return ctl_check(ctl, "fx ctl_check"); }

static uint32_t recip32(uint32_t x) { return x ? (uint32_t)(0x100000000ull / x) : 0u; }   /* (skred_fxbank.c: skx_pack_voice's) */

/* The checked record as it travels: `which` and the words it names, everything else zero (what the caller left in an unnamed field
 * is never shipped); under ENV_TIMES the reciprocals in the three reserved words. */
void skx_ctl_pack(const skred_fx_ctl_t *c, skx_ctl_t *out) {
  static const struct { uint32_t bit; int first, count; } fields[] = {
    { SKRED_CTL_PHASE_INC, SKX_CTL_PHASE_INC, 1 }, { SKRED_CTL_INC_SCALE, SKX_CTL_INC_SCALE, 1 }, { SKRED_CTL_AMP, SKX_CTL_AMP, 1 },
    { SKRED_CTL_PAN, SKX_CTL_PAN_LEFT, 2 },        { SKRED_CTL_FILTER, SKX_CTL_B0, 5 },           { SKRED_CTL_ENV_TIMES, SKX_CTL_ATTACK, 4 },
    { SKRED_CTL_VELOCITY, SKX_CTL_VELOCITY, 1 },   { SKRED_CTL_SMOOTHING, SKX_CTL_SMOOTHING, 1 },
  };
  const uint32_t *w = (const uint32_t *)c;
  memset(out, 0, sizeof(*out));
  out->w[SKX_CTL_WHICH] = c->which;
  for (size_t k = 0; k < sizeof(fields) / sizeof(fields[0]); k++)
    if (c->which & fields[k].bit)
      for (int i = 0; i < fields[k].count; i++) out->w[fields[k].first + i] = w[fields[k].first + i];
  if (c->which & SKRED_CTL_ENV_TIMES) {
    out->w[SKX_CTL_RECIP_A] = recip32(c->attack_frames);
    out->w[SKX_CTL_RECIP_D] = recip32(c->decay_frames);
    out->w[SKX_CTL_RECIP_R] = recip32(c->release_frames);
  }
}

/* the packed record (and, guarded, the n tags behind it) -> a staging slot -> one of the two kernels (d_voices NULL: the range) */
static int ctl_launch(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, int first, int count, const int32_t *d_voices, const uint32_t *tags, int n,
                      const uint32_t *d_count, uint32_t *d_result, const char *who, hipStream_t s) {
  HIP_TRY(hipSetDevice(fx->device));
  int rc;
  if (tags && (rc = skx_owner_ensure(fx))) return rc;
  const size_t bytes = sizeof(skx_ctl_t) + (tags ? (size_t)n * sizeof(uint32_t) : 0);
  skx_batch_t bt;
  if ((rc = skx_batch_begin(fx, bytes, &bt))) return rc;
  skx_ctl_pack(ctl, (skx_ctl_t *)bt.h);
  if (tags) memcpy((char *)bt.h + sizeof(skx_ctl_t), tags, (size_t)n * sizeof(uint32_t));
  const skx_ctl_t *src = (const skx_ctl_t *)skx_batch_send(&bt, bytes, s);   /* the device twin: a bank-wide range is thousands of workgroups reading it */
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = d_voices
    ? (hipError_t)skx_launch_ctl_list(src, d_voices, tags ? (const uint32_t *)(src + 1) : NULL, tags ? fx->d_owner : NULL, n, d_count,
                                      fx->n_voices, fx->d_ro, d_result, s)
    : (hipError_t)skx_launch_ctl_range(src, first, count, fx->d_ro, d_result, s);
  return skx_batch_end(&bt, e, who, s);
}

int skred_fxbank_ctl_range(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, int first, int count, uint32_t *d_result, void *stream) {
  if (!fx) return fail(SKRED_E_BAD_ARG, "fx ctl_range: no bank");
  int rc = ctl_check(ctl, "fx ctl_range");
  if (rc) return rc;
  if ((rc = sk_check_slot_range(fx->n_voices, first, count, 1, 1, "fx ctl_range"))) return rc;
  if (count == 0) return SKRED_OK;
  return ctl_launch(fx, ctl, first, count, NULL, NULL, 0, NULL, d_result, "fx ctl_range", (hipStream_t)stream);
}

int skred_fxbank_ctl_list(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const int32_t *d_voices, int n, const uint32_t *d_count_or_null,
                          uint32_t *d_result, void *stream) {
  if (!fx || !d_voices) return fail(SKRED_E_BAD_ARG, "fx ctl_list: no bank or no list");
  int rc = sk_check_list_n(n, "fx ctl_list");
  if (rc || (rc = ctl_check(ctl, "fx ctl_list"))) return rc;
  if (n == 0) return SKRED_OK;
  return ctl_launch(fx, ctl, 0, 0, d_voices, NULL, n, d_count_or_null, d_result, "fx ctl_list", (hipStream_t)stream);
}

int skred_fxbank_ctl_owned(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const int32_t *d_voices, const uint32_t *tags, int n,
                           const uint32_t *d_count_or_null, uint32_t *d_result, void *stream) {
  if (!fx || !d_voices) return fail(SKRED_E_BAD_ARG, "fx ctl_owned: no bank or no list");
  int rc = skred_owner_tags_check(tags, n, 0);
  if (rc) return rc;
  if ((rc = sk_check_list_n(n, "fx ctl_owned"))) return rc;
  if ((rc = ctl_check(ctl, "fx ctl_owned"))) return rc;
  if (n == 0) return SKRED_OK;
  return ctl_launch(fx, ctl, 0, 0, d_voices, tags, n, d_count_or_null, d_result, "fx ctl_owned", (hipStream_t)stream);
}
