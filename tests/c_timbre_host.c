/* The host side of per-note timbre on both banks without a device: skred_filter_each_check and skred_fx_filter_each_check, the
 * 32-byte packing of the coefficients (sk_filt_pack, skx_filt_pack), the permutation that keeps filt[k] beside tags[k] through the
 * sort of the tags, for n = 1, 2, 1023 and 1024, skred_filter_coeffs against a restatement of mmf_set_params' arithmetic, and every
 * refusal the four entry points make before anything touches the device, each with its return code, on banks that are nothing but their voice count (a refused call reads no other member).  One line per
 * case, "OK" last.  tests/test_timbre_cpu.py builds and runs it; built together with skred_amd/csrc/skred_bank_expr.c and
 * skred_amd/csrc/skred_fx_expr.c, the shared checks and the batch path they reach, under -fsanitize=address,undefined, it is the
 * sanitizer run of those two files' host code -- from the repository root, after the library is built (the program's own copy of
 * the four files takes the place of the library's; everything else it calls comes from the library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_timbre_host.c skred_amd/csrc/skred_bank_expr.c skred_amd/csrc/skred_fx_expr.c \
 *       skred_amd/csrc/skred_bank_checks.c skred_amd/csrc/skred_bank_stage.c -o /tmp/c_timbre_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_timbre_host_san */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_bank_priv.h"
#undef HIP_TRY                    /* (each bank's private header brings its own; this program calls neither) */
#include "skred_fxbank_priv.h"

static int failures;
#define CASE(name, cond) do { const int ok_ = (cond); printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); failures += !ok_; } while (0)
#define BAD SKRED_E_BAD_ARG
#define RNG SKRED_E_RANGE

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static skred_filter_each_t filt_of(float v) {
  skred_filter_each_t f;
  memset(&f, 0, sizeof(f));
  f.b0 = v; f.b1 = v + 1.0f; f.b2 = v + 2.0f; f.a1 = -v; f.a2 = 0.5f;
  return f;
}

static skred_fx_filter_each_t fx_filt_of(int32_t v) {
  skred_fx_filter_each_t f;
  memset(&f, 0, sizeof(f));
  f.b0_q30 = v; f.b1_q30 = v + 1; f.b2_q30 = -v; f.a1_q30 = INT32_MIN; f.a2_q30 = INT32_MAX;
  return f;
}

static skred_ctl_each_t each_of(uint32_t set, float v) {
  skred_ctl_each_t e;
  memset(&e, 0, sizeof(e));
  e.set = set; e.inc_scale = v; e.amp_scale = v; e.velocity = v; e.pan_left = v; e.pan_right = v;
  return e;
}

static uint32_t *make_tags(int n) {
  uint32_t *t = (uint32_t *)malloc((size_t)n * sizeof(uint32_t));
  for (int k = 0; k < n; k++) t[k] = (1u + ((uint32_t)k * 7919u) % 1031u) | ((k & 1) ? 0x80000000u : 0u);   /* (1031 is prime: distinct for k < 1031) */
  if (n > 1) t[0] = 0xFFFFFFFFu;
  return t;
}

/* what the _tags_each_filter calls ship: the tags sorted, filt[k] and each[k] still beside tags[k] -- on both banks */
static int perm_ok(int n) {
  uint32_t *tags = make_tags(n), *sorted = (uint32_t *)malloc((size_t)n * sizeof(uint32_t)), *perm = (uint32_t *)malloc((size_t)n * sizeof(uint32_t));
  skred_filter_each_t *filt = (skred_filter_each_t *)malloc((size_t)n * sizeof(*filt));
  skred_fx_filter_each_t *fxf = (skred_fx_filter_each_t *)malloc((size_t)n * sizeof(*fxf));
  skred_ctl_each_t *each = (skred_ctl_each_t *)malloc((size_t)n * sizeof(*each));
  sk_filt_each_t *out = (sk_filt_each_t *)malloc((size_t)n * sizeof(*out));
  skx_filt_each_t *fxo = (skx_filt_each_t *)malloc((size_t)n * sizeof(*fxo));
  sk_each_t *eo = (sk_each_t *)malloc((size_t)n * sizeof(*eo));
  for (int k = 0; k < n; k++) { filt[k] = filt_of((float)k); fxf[k] = fx_filt_of(k); each[k] = each_of(SKRED_EACH_VELOCITY, (float)k); }
  memset(out, 0xAB, (size_t)n * sizeof(*out));
  memset(fxo, 0xAB, (size_t)n * sizeof(*fxo));
  int ok = sk_owner_pack(tags, n, sorted, perm) == 0 && sk_each_pack(each, n, perm, eo) == SKRED_EACH_VELOCITY;
  sk_filt_pack(filt, n, perm, out);
  skx_filt_pack(fxf, n, perm, fxo);
  for (int j = 0; j < n && ok; j++) {
    const uint32_t k = perm[j];                           /* sorted[j] stood at k: the coefficients beside it must be filt[k] */
    ok = k < (uint32_t)n && sorted[j] == tags[k] && (j == 0 || sorted[j - 1] < sorted[j]) &&
         out[j].w[SK_FILT_W_B0] == bits_of((float)k) && out[j].w[SK_FILT_W_B1] == bits_of((float)k + 1.0f) &&
         out[j].w[SK_FILT_W_B2] == bits_of((float)k + 2.0f) && out[j].w[SK_FILT_W_A1] == bits_of(-(float)k) &&
         out[j].w[SK_FILT_W_A2] == bits_of(0.5f) && !out[j].w[5] && !out[j].w[6] && !out[j].w[7] &&
         eo[j].w[SK_EACH_W_VELOCITY] == bits_of((float)k) &&
         fxo[j].w[SKX_FILT_W_B0] == k && fxo[j].w[SKX_FILT_W_B1] == k + 1 && fxo[j].w[SKX_FILT_W_B2] == (uint32_t)-(int32_t)k &&
         fxo[j].w[SKX_FILT_W_A1] == 0x80000000u && fxo[j].w[SKX_FILT_W_A2] == 0x7FFFFFFFu && !fxo[j].w[5] && !fxo[j].w[6] && !fxo[j].w[7];
  }
  if (ok && n > 1) ok = out[n - 1].w[SK_FILT_W_B0] == bits_of(0.0f) && fxo[n - 1].w[SKX_FILT_W_B0] == 0;   /* 0xFFFFFFFF sorts last and brings entry 0 */
  free(eo); free(fxo); free(out); free(each); free(fxf); free(filt); free(perm); free(sorted); free(tags);
  return ok;
}

/* mmf_set_params' coefficient arithmetic as the drop-in stated it before it called skred_filter_coeffs (reference synth.c:929-1008),
 * written out again here so that the library's function is held to a statement that is not itself: fp32, the operations in this
 * order, the rate the drop-in's (this program is built with -ffp-contract=off, as the drop-in is) */
static void mmf_coeffs_restated(int mode, float f, float resonance, float out[5]) {
  const float w = 2.0f * (float)M_PI * f / (float)44100;
  const float sn = sinf(w), cs = cosf(w);
  const float alpha = sn / (2.0f * resonance);
  const float a0 = 1.0f + alpha;
  float b0 = (1.0f - cs) / 2.0f, b1 = 1.0f - cs, b2 = (1.0f - cs) / 2.0f;                      /* low-pass; also any unknown mode */
  if (mode == 2) { b0 = (1.0f + cs) / 2.0f; b1 = -(1.0f + cs); b2 = (1.0f + cs) / 2.0f; }      /* high-pass */
  if (mode == 3) { b0 = alpha; b1 = 0.0f; b2 = -alpha; }                                       /* band-pass */
  if (mode == 4) { b0 = 1.0f; b1 = -2.0f * cs; b2 = 1.0f; }                                    /* notch */
  if (mode == 5) { b0 = 1.0f - alpha; b1 = -2.0f * cs; b2 = 1.0f + alpha; }                    /* all-pass */
  out[0] = b0 / a0; out[1] = b1 / a0; out[2] = b2 / a0;
  out[3] = (-2.0f * cs) / a0;
  out[4] = (1.0f - alpha) / a0;
}

/* modes 1 .. 5 and two unknown ones, 64 frequencies from 20 Hz to 20.48 kHz, 8 resonances: bit for bit */
static int coeffs_sweep_ok(void) {
  const int modes[7] = { 1, 2, 3, 4, 5, 9, -3 };
  const float ress[8] = { 0.1f, 0.5f, 0.707f, 1.0f, 1.5f, 2.5f, 4.0f, 12.0f };
  for (int m = 0; m < 7; m++)
    for (int i = 0; i < 64; i++)
      for (int r = 0; r < 8; r++) {
        const float f = 20.0f * exp2f((float)i * (10.0f / 63.0f));
        float got[5], want[5];
        if (skred_filter_coeffs(modes[m], f, ress[r], 44100.0f, got) != SKRED_OK) return 0;
        mmf_coeffs_restated(modes[m], f, ress[r], want);
        if (memcmp(got, want, sizeof(got))) { printf("coeffs differ: mode %d f %g res %g\n", modes[m], (double)f, (double)ress[r]); return 0; }
      }
  return 1;
}

int main(void) {
  CASE("const/sizes", sizeof(skred_filter_each_t) == 32 && sizeof(sk_filt_each_t) == 32 && sizeof(skred_fx_filter_each_t) == 32 &&
                      sizeof(skx_filt_each_t) == 32);
  CASE("const/offsets", offsetof(skred_filter_each_t, b0) == 0 && offsetof(skred_filter_each_t, a1) == 12 && offsetof(skred_filter_each_t, a2) == 16 &&
                        offsetof(skred_filter_each_t, reserved) == 20 && offsetof(skred_fx_filter_each_t, b0_q30) == 0 &&
                        offsetof(skred_fx_filter_each_t, a2_q30) == 16 && offsetof(skred_fx_filter_each_t, reserved) == 20);

  /* ---- skred_filter_each_check ---- */
  skred_ctl_t k4[4];
  memset(k4, 0, sizeof(k4));
  for (int l = 0; l < 4; l++) { k4[l].set = SKRED_CTL_PAN; k4[l].pan_left = 0.25f; k4[l].pan_right = 0.75f; }
  skred_filter_each_t f2[2] = { filt_of(0.25f), filt_of(0.5f) }, bad;
  CASE("check/plain", skred_filter_each_check(f2, 2, k4, 4, 0xF, 0xF) == SKRED_OK);
  CASE("check/subset", skred_filter_each_check(f2, 2, k4, 4, 0xF, 0x5) == SKRED_OK);
  CASE("check/no_records", skred_filter_each_check(f2, 2, NULL, 4, 0x6, 0x2) == SKRED_OK);
  CASE("check/empty", skred_filter_each_check(f2, 0, k4, 4, 0xF, 0xF) == SKRED_OK);
  CASE("check/null", skred_filter_each_check(NULL, 2, k4, 4, 0xF, 0xF) == BAD);
  CASE("check/negative_n", skred_filter_each_check(f2, -1, k4, 4, 0xF, 0xF) == BAD);
  CASE("check/bad_k", skred_filter_each_check(f2, 2, k4, 3, 0x7, 0x7) == RNG);
  CASE("check/bad_k_no_records", skred_filter_each_check(f2, 2, NULL, 128, 0xF, 0xF) == RNG);
  CASE("check/voice_mask0", skred_filter_each_check(f2, 2, k4, 4, 0, 0) == BAD);
  CASE("check/voice_mask_high", skred_filter_each_check(f2, 2, NULL, 4, 0x10, 0x10) == BAD);
  CASE("check/filter_mask0", skred_filter_each_check(f2, 2, k4, 4, 0xF, 0) == BAD);
  CASE("check/filter_mask_outside_voice_mask", skred_filter_each_check(f2, 2, k4, 4, 0x3, 0x6) == BAD);
  CASE("check/filter_mask_outside_no_records", skred_filter_each_check(f2, 2, NULL, 4, 0x3, 0x4) == BAD);
  CASE("check/k64_full_masks", skred_filter_each_check(f2, 2, NULL, 64, ~0ull, 1ull << 63) == SKRED_OK);
  k4[1].set = 0;
  CASE("check/bad_record", skred_filter_each_check(f2, 2, k4, 4, 0xF, 0x1) == BAD);
  CASE("check/bad_record_unmasked", skred_filter_each_check(f2, 2, k4, 4, 0xD, 0x1) == SKRED_OK);
  k4[1].set = SKRED_CTL_PAN | SKRED_CTL_FILTER;
  CASE("check/record_names_filter_on_a_filter_lane", skred_filter_each_check(f2, 2, k4, 4, 0xF, 0x2) == BAD);
  CASE("check/record_names_filter_on_another_lane", skred_filter_each_check(f2, 2, k4, 4, 0xF, 0xD) == SKRED_OK);
  CASE("check/record_names_filter_unmasked", skred_filter_each_check(f2, 2, k4, 4, 0xD, 0xD) == SKRED_OK);
  k4[1].set = SKRED_CTL_PAN;
  for (int w = 0; w < 3; w++) {
    char name[32];
    snprintf(name, sizeof(name), "check/reserved%d", w);
    bad = filt_of(0.5f); bad.reserved[w] = 1;
    CASE(name, skred_filter_each_check(&bad, 1, k4, 4, 0xF, 0xF) == BAD);
  }
  const float nonfinite[3] = { INFINITY, -INFINITY, NAN };
  for (int c = 0; c < 5; c++) {
    char name[32];
    snprintf(name, sizeof(name), "check/not_finite%d", c);
    bad = filt_of(0.5f);
    ((float *)&bad)[c] = nonfinite[c % 3];
    CASE(name, skred_filter_each_check(&bad, 1, k4, 4, 0xF, 0xF) == BAD);
  }
  skred_filter_each_t second[2] = { filt_of(0.5f), filt_of(NAN) };
  CASE("check/second_entry", skred_filter_each_check(second, 2, k4, 4, 0xF, 0xF) == BAD && skred_filter_each_check(second, 1, k4, 4, 0xF, 0xF) == SKRED_OK);
  bad = filt_of(1e-45f);
  CASE("check/subnormal_is_finite", skred_filter_each_check(&bad, 1, k4, 4, 0xF, 0xF) == SKRED_OK);

  /* ---- skred_fx_filter_each_check ---- */
  skred_fx_ctl_t pan, fil;
  memset(&pan, 0, sizeof(pan));
  pan.which = SKRED_CTL_PAN; pan.pan_left_q15 = 1; pan.pan_right_q15 = 2;
  fil = pan;
  fil.which |= SKRED_CTL_FILTER;
  skred_fx_filter_each_t x2[2] = { fx_filt_of(5), fx_filt_of(-7) }, xbad;
  CASE("fxcheck/plain", skred_fx_filter_each_check(x2, 2, &pan) == SKRED_OK);
  CASE("fxcheck/no_record", skred_fx_filter_each_check(x2, 2, NULL) == SKRED_OK);
  CASE("fxcheck/empty", skred_fx_filter_each_check(x2, 0, NULL) == SKRED_OK);
  CASE("fxcheck/null", skred_fx_filter_each_check(NULL, 2, &pan) == BAD);
  CASE("fxcheck/negative_n", skred_fx_filter_each_check(x2, -1, &pan) == BAD);
  CASE("fxcheck/record_names_filter", skred_fx_filter_each_check(x2, 2, &fil) == BAD);
  fil.which = 0;
  CASE("fxcheck/bad_record", skred_fx_filter_each_check(x2, 2, &fil) == BAD);
  for (int w = 0; w < 3; w++) {
    char name[32];
    snprintf(name, sizeof(name), "fxcheck/reserved%d", w);
    xbad = fx_filt_of(3); xbad.reserved[w] = 1;
    CASE(name, skred_fx_filter_each_check(&xbad, 1, NULL) == BAD);
  }
  skred_fx_filter_each_t xsecond[2] = { fx_filt_of(1), fx_filt_of(2) };
  xsecond[1].reserved[2] = 9;
  CASE("fxcheck/second_entry", skred_fx_filter_each_check(xsecond, 2, NULL) == BAD && skred_fx_filter_each_check(xsecond, 1, NULL) == SKRED_OK);

  /* ---- the packing: five words as they stand, the rest zero ---- */
  skred_filter_each_t src[3] = { filt_of(1.25f), filt_of(-2.0f), filt_of(0.0f) };
  src[2].a2 = -0.0f;
  sk_filt_each_t out[3];
  memset(out, 0xAB, sizeof(out));
  sk_filt_pack(src, 3, NULL, out);
  CASE("pack/words", out[0].w[0] == bits_of(1.25f) && out[0].w[1] == bits_of(2.25f) && out[0].w[2] == bits_of(3.25f) && out[0].w[3] == bits_of(-1.25f) &&
                     out[0].w[4] == bits_of(0.5f) && !out[0].w[5] && !out[0].w[6] && !out[0].w[7]);
  CASE("pack/minus_zero_kept", out[2].w[4] == 0x80000000u && out[2].w[0] == 0 && !out[2].w[7]);
  const uint32_t rev[3] = { 2, 0, 1 };
  sk_filt_pack(src, 3, rev, out);
  CASE("pack/permuted", out[0].w[4] == 0x80000000u && out[1].w[0] == bits_of(1.25f) && out[2].w[0] == bits_of(-2.0f));
  skx_filt_each_t xo[2];
  memset(xo, 0xAB, sizeof(xo));
  skx_filt_pack(x2, 2, NULL, xo);
  CASE("pack/fx_words", xo[0].w[0] == 5 && xo[0].w[1] == 6 && xo[0].w[2] == (uint32_t)-5 && xo[0].w[3] == 0x80000000u && xo[0].w[4] == 0x7FFFFFFFu &&
                        !xo[0].w[5] && !xo[0].w[6] && !xo[0].w[7] && xo[1].w[0] == (uint32_t)-7);
  CASE("perm/1", perm_ok(1));
  CASE("perm/2", perm_ok(2));
  CASE("perm/1023", perm_ok(1023));
  CASE("perm/1024", perm_ok(1024));

  /* ---- the coefficient helper ---- */
  float c5[5] = { 7.0f, 7.0f, 7.0f, 7.0f, 7.0f };
  CASE("coeffs/null_out", skred_filter_coeffs(1, 1000.0f, 0.7f, 44100.0f, NULL) == BAD);
  CASE("coeffs/bypass", skred_filter_coeffs(0, 1000.0f, 0.7f, 44100.0f, c5) == 1 && c5[0] == 7.0f && c5[4] == 7.0f);
  CASE("coeffs/low_pass", skred_filter_coeffs(1, 1000.0f, 0.7f, 44100.0f, c5) == SKRED_OK && c5[0] > 0.0f && c5[1] == c5[0] + c5[0] && c5[2] == c5[0] && c5[3] < 0.0f);
  float u5[5];
  CASE("coeffs/unknown_mode_is_low_pass", skred_filter_coeffs(9, 1000.0f, 0.7f, 44100.0f, u5) == SKRED_OK && !memcmp(u5, c5, sizeof(c5)));
  CASE("coeffs/sweep_equals_the_restated_arithmetic", coeffs_sweep_ok());
  CASE("coeffs/resonance0_is_refused_later", skred_filter_coeffs(1, 1000.0f, 0.0f, 44100.0f, u5) == SKRED_OK && !isfinite(u5[4]));

  /* ---- the float bank's entry points: a bank that is nothing but its size ---- */
  skred_bank_t *b = (skred_bank_t *)calloc(1, sizeof(skred_bank_t));
  b->n_voices = 200;
  int32_t list[4] = { 0, 8, 16, 24 };
  skred_ctl_t k8[8], k8f[8];
  memset(k8, 0, sizeof(k8));
  for (int l = 0; l < 8; l++) { k8[l].set = SKRED_CTL_PAN; k8[l].pan_left = 0.25f; k8[l].pan_right = 0.75f; }
  memcpy(k8f, k8, sizeof(k8));
  k8f[3].set |= SKRED_CTL_FILTER;
  const uint32_t t4[4] = { 1, 2, 3, 0xFFFFFFFFu }, z4[4] = { 1, 0, 3, 4 }, d4[4] = { 1, 2, 1, 4 };
  skred_ctl_each_t e4[4] = { each_of(SKRED_EACH_VELOCITY, 0.5f), each_of(SKRED_EACH_INC_SCALE, 1.5f), each_of(SKRED_EACH_PAN, 0.5f), each_of(SKRED_EACH_VELOCITY, 0.25f) };
  skred_ctl_each_t a4[4] = { each_of(SKRED_EACH_AMP_SCALE, 0.5f), each_of(SKRED_EACH_AMP_SCALE, 0.5f), each_of(SKRED_EACH_AMP_SCALE, 0.5f), each_of(SKRED_EACH_AMP_SCALE, 0.5f) };
  skred_filter_each_t f4[4] = { filt_of(0.1f), filt_of(0.2f), filt_of(0.3f), filt_of(0.4f) }, n4[4], r4[4];
  memcpy(n4, f4, sizeof(f4)); n4[2].a1 = NAN;
  memcpy(r4, f4, sizeof(f4)); r4[3].reserved[1] = 1;
#define OWNED(bank, ctl, each, filt, K, vm, fm, lst, tags, n) skred_bank_ctl_owned_each_filter(bank, ctl, each, filt, K, vm, fm, lst, tags, n, NULL, NULL, NULL)
#define TAGS(bank, ctl, each, filt, first, count, K, vm, fm, tags, n) skred_bank_ctl_tags_each_filter(bank, ctl, each, filt, first, count, K, vm, fm, tags, n, NULL, NULL)
  CASE("owned/null_bank", OWNED(NULL, k8, e4, f4, 8, 0xFF, 0xFF, list, t4, 4) == BAD);
  CASE("owned/null_list", OWNED(b, k8, e4, f4, 8, 0xFF, 0xFF, NULL, t4, 4) == BAD);
  CASE("owned/null_tags", OWNED(b, k8, e4, f4, 8, 0xFF, 0xFF, list, NULL, 4) == BAD);
  CASE("owned/zero_tag", OWNED(b, k8, e4, f4, 8, 0xFF, 0xFF, list, z4, 4) == BAD);
  CASE("owned/negative_n", OWNED(b, k8, e4, f4, 8, 0xFF, 0xFF, list, t4, -1) == BAD);
  CASE("owned/huge_n", OWNED(b, k8, e4, f4, 8, 0xFF, 0xFF, list, t4, INT32_MAX / 64 + 1) == BAD);
  CASE("owned/null_filt", OWNED(b, k8, e4, NULL, 8, 0xFF, 0xFF, list, t4, 4) == BAD);
  CASE("owned/null_filt_and_each", OWNED(b, k8, NULL, NULL, 8, 0xFF, 0xFF, list, t4, 4) == BAD);
  CASE("owned/filter_mask0", OWNED(b, k8, e4, f4, 8, 0xFF, 0, list, t4, 4) == BAD);
  CASE("owned/filter_mask_outside", OWNED(b, k8, e4, f4, 8, 0x0F, 0x1F, list, t4, 4) == BAD);
  CASE("owned/reserved", OWNED(b, k8, e4, r4, 8, 0xFF, 0xFF, list, t4, 4) == BAD);
  CASE("owned/not_finite", OWNED(b, k8, e4, n4, 8, 0xFF, 0xFF, list, t4, 4) == BAD);
  CASE("owned/record_names_filter", OWNED(b, k8f, e4, f4, 8, 0xFF, 0x08, list, t4, 4) == BAD);
  CASE("owned/bad_k", OWNED(b, NULL, e4, f4, 5, 0x1F, 0x1F, list, t4, 4) == RNG);
  CASE("owned/bad_k_no_each", OWNED(b, NULL, NULL, f4, 5, 0x1F, 0x1F, list, t4, 4) == RNG);
  CASE("owned/mask0", OWNED(b, k8, e4, f4, 8, 0, 0, list, t4, 4) == BAD);
  CASE("owned/bad_entry", OWNED(b, k8, a4, f4, 8, 0xFF, 0xFF, list, t4, 4) == BAD);
  CASE("owned/empty", OWNED(b, k8, e4, f4, 8, 0xFF, 0xFF, list, t4, 0) == SKRED_OK);
  CASE("owned/empty_filter_only", OWNED(b, NULL, NULL, f4, 8, 0xFF, 0x01, list, t4, 0) == SKRED_OK);
  CASE("owned/empty_record_filter_on_another_lane", OWNED(b, k8f, NULL, f4, 8, 0xFF, 0xF7, list, t4, 0) == SKRED_OK);

  CASE("tags/null_bank", TAGS(NULL, k8, e4, f4, 0, 200, 8, 0xFF, 0xFF, t4, 4) == BAD);
  CASE("tags/null_tags", TAGS(b, k8, e4, f4, 0, 200, 8, 0xFF, 0xFF, NULL, 4) == BAD);
  CASE("tags/zero_tag", TAGS(b, k8, e4, f4, 0, 200, 8, 0xFF, 0xFF, z4, 4) == BAD);
  CASE("tags/dup_tag", TAGS(b, k8, e4, f4, 0, 200, 8, 0xFF, 0xFF, d4, 4) == BAD);
  uint32_t *many = (uint32_t *)malloc(1025 * sizeof(uint32_t));
  skred_filter_each_t *many_f = (skred_filter_each_t *)malloc(1025 * sizeof(skred_filter_each_t));
  for (int k = 0; k < 1025; k++) { many[k] = 1u + (uint32_t)k; many_f[k] = filt_of(0.5f); }
  CASE("tags/1025_tags", TAGS(b, k8, NULL, many_f, 0, 200, 8, 0xFF, 0xFF, many, 1025) == BAD);
  CASE("tags/null_filt", TAGS(b, k8, e4, NULL, 0, 200, 8, 0xFF, 0xFF, t4, 4) == BAD);
  CASE("tags/filter_mask0", TAGS(b, k8, e4, f4, 0, 200, 8, 0xFF, 0, t4, 4) == BAD);
  CASE("tags/filter_mask_outside", TAGS(b, k8, NULL, f4, 0, 200, 8, 0x0F, 0x10, t4, 4) == BAD);
  CASE("tags/reserved", TAGS(b, k8, NULL, r4, 0, 200, 8, 0xFF, 0xFF, t4, 4) == BAD);
  CASE("tags/not_finite", TAGS(b, NULL, NULL, n4, 0, 200, 8, 0xFF, 0xFF, t4, 4) == BAD);
  CASE("tags/record_names_filter", TAGS(b, k8f, NULL, f4, 0, 200, 8, 0xFF, 0xFF, t4, 4) == BAD);
  CASE("tags/bad_entry", TAGS(b, k8, a4, f4, 0, 200, 8, 0xFF, 0xFF, t4, 4) == BAD);
  CASE("tags/bad_k", TAGS(b, NULL, NULL, f4, 0, 200, 3, 0x7, 0x7, t4, 4) == RNG);
  CASE("tags/range_off_slot", TAGS(b, k8, e4, f4, 4, 8, 8, 0xFF, 0xFF, t4, 4) == RNG);
  CASE("tags/count_zero", TAGS(b, k8, e4, f4, 8, 0, 8, 0xFF, 0xFF, t4, 4) == RNG);
  CASE("tags/past_the_bank", TAGS(b, k8, e4, f4, 0, 208, 8, 0xFF, 0xFF, t4, 4) == RNG);
  CASE("tags/empty", TAGS(b, k8, e4, f4, 0, 200, 8, 0xFF, 0xFF, t4, 0) == SKRED_OK);
  /* the calls without coefficients keep their refusals: a NULL `each` is refused there and only there */
  CASE("plain/null_each_still_refused", skred_bank_ctl_owned_each(b, k8, NULL, 8, 0xFF, list, t4, 4, NULL, NULL, NULL) == BAD &&
                                        skred_bank_ctl_tags_each(b, k8, NULL, 0, 200, 8, 0xFF, t4, 4, NULL, NULL) == BAD);
  CASE("bank/untouched", b->touched_total == 0 && b->control_epoch == 0 && b->upd_seq == 0 && b->upd_head == 0 && !b->d_owner && !b->d_owner_slots &&
                         !b->d_match_pair && !b->d_idle);
  free(b);

  /* ---- the fixed-point bank's entry points ---- */
  skred_fxbank_t *fx = (skred_fxbank_t *)calloc(1, sizeof(skred_fxbank_t));
  fx->n_voices = 200;
  fil = pan;
  fil.which |= SKRED_CTL_FILTER;
  skred_fx_ctl_each_t xe4[4], xa4[4];
  memset(xe4, 0, sizeof(xe4));
  for (int k = 0; k < 4; k++) { xe4[k].set = SKRED_EACH_VELOCITY; xe4[k].velocity_q15 = 100 + k; }
  memcpy(xa4, xe4, sizeof(xe4));
  xa4[1].set = SKRED_EACH_AMP_SCALE; xa4[1].amp_scale_q16 = 65536;
  skred_fx_filter_each_t xf4[4] = { fx_filt_of(1), fx_filt_of(2), fx_filt_of(3), fx_filt_of(4) }, xr4[4];
  memcpy(xr4, xf4, sizeof(xf4)); xr4[0].reserved[0] = 1;
#define XOWNED(bank, ctl, each, filt, lst, tags, n) skred_fxbank_ctl_owned_each_filter(bank, ctl, each, filt, lst, tags, n, NULL, NULL, NULL)
#define XTAGS(bank, ctl, each, filt, first, count, tags, n) skred_fxbank_ctl_tags_each_filter(bank, ctl, each, filt, first, count, tags, n, NULL, NULL)
  CASE("fxowned/null_bank", XOWNED(NULL, &pan, xe4, xf4, list, t4, 4) == BAD);
  CASE("fxowned/null_list", XOWNED(fx, &pan, xe4, xf4, NULL, t4, 4) == BAD);
  CASE("fxowned/null_tags", XOWNED(fx, &pan, xe4, xf4, list, NULL, 4) == BAD);
  CASE("fxowned/zero_tag", XOWNED(fx, &pan, xe4, xf4, list, z4, 4) == BAD);
  CASE("fxowned/negative_n", XOWNED(fx, &pan, xe4, xf4, list, t4, -1) == BAD);
  CASE("fxowned/null_filt", XOWNED(fx, &pan, xe4, NULL, list, t4, 4) == BAD);
  CASE("fxowned/reserved", XOWNED(fx, &pan, xe4, xr4, list, t4, 4) == BAD);
  CASE("fxowned/record_names_filter", XOWNED(fx, &fil, NULL, xf4, list, t4, 4) == BAD);
  CASE("fxowned/bad_entry", XOWNED(fx, &pan, xa4, xf4, list, t4, 4) == BAD);
  CASE("fxowned/empty", XOWNED(fx, &pan, xe4, xf4, list, t4, 0) == SKRED_OK);
  CASE("fxowned/empty_filter_only", XOWNED(fx, NULL, NULL, xf4, list, t4, 0) == SKRED_OK);
  CASE("fxtags/null_bank", XTAGS(NULL, &pan, xe4, xf4, 0, 200, t4, 4) == BAD);
  CASE("fxtags/null_tags", XTAGS(fx, &pan, xe4, xf4, 0, 200, NULL, 4) == BAD);
  CASE("fxtags/dup_tag", XTAGS(fx, &pan, xe4, xf4, 0, 200, d4, 4) == BAD);
  skred_fx_filter_each_t *many_x = (skred_fx_filter_each_t *)calloc(1025, sizeof(skred_fx_filter_each_t));
  CASE("fxtags/1025_tags", XTAGS(fx, NULL, NULL, many_x, 0, 200, many, 1025) == BAD);
  CASE("fxtags/null_filt", XTAGS(fx, &pan, xe4, NULL, 0, 200, t4, 4) == BAD);
  CASE("fxtags/reserved", XTAGS(fx, NULL, NULL, xr4, 0, 200, t4, 4) == BAD);
  CASE("fxtags/record_names_filter", XTAGS(fx, &fil, xe4, xf4, 0, 200, t4, 4) == BAD);
  CASE("fxtags/past_the_bank", XTAGS(fx, &pan, xe4, xf4, 0, 201, t4, 4) == RNG);
  CASE("fxtags/count_zero", XTAGS(fx, &pan, xe4, xf4, 8, 0, t4, 4) == RNG);
  CASE("fxtags/empty", XTAGS(fx, &pan, xe4, xf4, 0, 200, t4, 0) == SKRED_OK);
  CASE("fxplain/null_each_still_refused", skred_fxbank_ctl_owned_each(fx, &pan, NULL, list, t4, 4, NULL, NULL, NULL) == BAD &&
                                          skred_fxbank_ctl_tags_each(fx, &pan, NULL, 0, 200, t4, 4, NULL, NULL) == BAD);
  CASE("fxbank/untouched", !fx->d_owner && !fx->d_idle);
  free(many_x); free(many_f); free(many);
  free(fx);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
