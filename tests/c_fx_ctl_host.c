/* The host side of the fixed-point bank's note owners and controllers without a device: skred_fx_ctl_check, the record's packing
 * (skx_ctl_pack), the sort-plus-permutation of the tags as the find pass gets them (sk_owner_pack) and every refusal the entry points
 * make before anything touches the device, on a skred_fxbank_t that is nothing but its voice count (a refused call reads no other
 * member), those of the live calls that share the batch path with them included (skred_fxbank_update, _stamp, _notes_on_list,
 * _note_on_idle, _find_idle_host).  One line per case, "OK" last.  tests/test_fx_ctl_cpu.py and tests/test_fx_owner_cpu.py build and
 * run it; built together with skred_amd/csrc/skred_fx_owner.c, skred_fx_ctl.c, skred_fx_live.c, skred_fx_stage.c and the checks they
 * share with the float bank under -fsanitize=address,undefined it is the sanitizer run of those files' host code -- from the
 * repository root, after the library is built (the program's own copy of those files takes the place of the library's; everything
 * else it calls comes from the library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_fx_ctl_host.c skred_amd/csrc/skred_fx_owner.c skred_amd/csrc/skred_fx_ctl.c \
 *       skred_amd/csrc/skred_fx_live.c skred_amd/csrc/skred_fx_stage.c skred_amd/csrc/skred_bank_checks.c -o /tmp/c_fx_ctl_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_fx_ctl_host_san */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_fxbank_priv.h"

static int failures;
#define CASE(name, cond) do { const int ok_ = (cond); printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); failures += !ok_; } while (0)
#define BAD SKRED_E_BAD_ARG
#define RNG SKRED_E_RANGE

static uint32_t *make_tags(int n) {
  uint32_t *t = (uint32_t *)malloc((size_t)(n > 0 ? n : 1) * sizeof(uint32_t));
  for (int k = 0; k < n; k++) t[k] = (1u + ((uint32_t)k * 7919u) % 1031u) | ((k & 1) ? 0x80000000u : 0u);   /* (1031 is prime: distinct for k < 1031) */
  if (n > 1) t[0] = 0xFFFFFFFFu;
  return t;
}

/* sorted ascending as UNSIGNED numbers, strictly; perm a permutation with sorted[j] == tags[perm[j]] */
static int pack_ok(int n) {
  uint32_t *t = make_tags(n);
  uint32_t *sorted = (uint32_t *)malloc((size_t)n * sizeof(uint32_t)), *perm = (uint32_t *)malloc((size_t)n * sizeof(uint32_t));
  unsigned char *seen = (unsigned char *)calloc((size_t)n, 1);
  int ok = sk_owner_pack(t, n, sorted, perm) == 0;
  for (int j = 0; j < n && ok; j++) {
    ok = perm[j] < (uint32_t)n && !seen[perm[j]] && sorted[j] == t[perm[j]] && (j == 0 || sorted[j - 1] < sorted[j]);
    if (ok) seen[perm[j]] = 1;
  }
  if (ok && n > 1) ok = sorted[n - 1] == 0xFFFFFFFFu && perm[n - 1] == 0;
  free(seen); free(perm); free(sorted); free(t);
  return ok;
}

static skred_fx_ctl_t all_fields(void) {
  skred_fx_ctl_t c;
  memset(&c, 0, sizeof(c));
  c.which = 255;
  c.phase_inc = 0xDEADBEEFu; c.inc_scale_q16 = 65536; c.amp_q15 = 65535; c.pan_left_q15 = 0; c.pan_right_q15 = 65535;
  c.b0_q30 = INT32_MIN; c.b1_q30 = INT32_MAX; c.b2_q30 = -1; c.a1_q30 = 7; c.a2_q30 = -7;
  c.attack_frames = 0; c.decay_frames = 1; c.release_frames = 3; c.sustain_q15 = 32768; c.velocity_q15 = 0; c.smoother_k_q15 = 32768;
  return c;
}

int main(void) {
  CASE("const/record", sizeof(skred_fx_ctl_t) == 80 && sizeof(skx_ctl_t) == 80 && SKX_CTL_WORDS == 20);
  CASE("const/bits", SKRED_CTL_PHASE_INC == 1 && SKRED_CTL_INC_SCALE == 2 && SKRED_CTL_AMP == 4 && SKRED_CTL_PAN == 8 && SKRED_CTL_FILTER == 16 &&
                     SKRED_CTL_ENV_TIMES == 32 && SKRED_CTL_VELOCITY == 64 && SKRED_CTL_SMOOTHING == 128);
  CASE("const/owner", SKRED_OWNER_MAX_TAGS == 1024 && SKRED_OWNER_ALLOW_ZERO == 1 && SKRED_OWNER_UNIQUE == 2);

  /* ---- skred_fx_ctl_check: every refusal beside the accepted edge */
  skred_fx_ctl_t c = all_fields();
  CASE("check/all_fields_at_their_edges", skred_fx_ctl_check(&c) == SKRED_OK);
  CASE("check/null", skred_fx_ctl_check(NULL) == BAD);
  c = all_fields(); c.which = 0;
  CASE("check/which0", skred_fx_ctl_check(&c) == BAD);
  c = all_fields(); c.which = 1u << 14;
  CASE("check/unknown_bit", skred_fx_ctl_check(&c) == BAD);
  int refused = 1;
  for (int bit = 8; bit <= 13; bit++) { c = all_fields(); c.which = SKRED_CTL_PAN | (1u << bit); refused = refused && skred_fx_ctl_check(&c) == BAD; }
  CASE("check/modulator_bits", refused);
  for (int k = 0; k < 3; k++) {
    char name[32];
    snprintf(name, sizeof(name), "check/reserved%d", k);
    c = all_fields(); c.reserved[k] = 1;
    CASE(name, skred_fx_ctl_check(&c) == BAD);
  }
  c = all_fields(); c.amp_q15 = 0;
  CASE("check/amp0", skred_fx_ctl_check(&c) == BAD);
  c.which &= ~(uint32_t)SKRED_CTL_AMP;
  CASE("check/amp0_unnamed", skred_fx_ctl_check(&c) == SKRED_OK);
  c = all_fields(); c.amp_q15 = 1;
  CASE("check/amp1", skred_fx_ctl_check(&c) == SKRED_OK);
  c = all_fields(); c.amp_q15 = 65536;
  CASE("check/amp65536", skred_fx_ctl_check(&c) == BAD);
  c = all_fields(); c.amp_q15 = -1;
  CASE("check/amp_negative", skred_fx_ctl_check(&c) == BAD);
  c = all_fields(); c.pan_left_q15 = 65536;
  CASE("check/pan_left_high", skred_fx_ctl_check(&c) == BAD);
  c = all_fields(); c.pan_right_q15 = -1;
  CASE("check/pan_right_negative", skred_fx_ctl_check(&c) == BAD);
  c.which &= ~(uint32_t)SKRED_CTL_PAN;
  CASE("check/pan_unnamed", skred_fx_ctl_check(&c) == SKRED_OK);
  c = all_fields(); c.sustain_q15 = 32769;
  CASE("check/sustain_high", skred_fx_ctl_check(&c) == BAD);
  c = all_fields(); c.sustain_q15 = -1;
  CASE("check/sustain_negative", skred_fx_ctl_check(&c) == BAD);
  c = all_fields(); c.attack_frames = c.decay_frames = c.release_frames = 0; c.sustain_q15 = 0;
  CASE("check/zero_length_stages", skred_fx_ctl_check(&c) == SKRED_OK);
  c = all_fields(); c.velocity_q15 = 65536;
  CASE("check/velocity_high", skred_fx_ctl_check(&c) == BAD);
  c = all_fields(); c.velocity_q15 = 65535;
  CASE("check/velocity_65535", skred_fx_ctl_check(&c) == SKRED_OK);
  c = all_fields(); c.velocity_q15 = -1;
  CASE("check/velocity_negative", skred_fx_ctl_check(&c) == BAD);
  c = all_fields(); c.smoother_k_q15 = 32769;
  CASE("check/smoothing_high", skred_fx_ctl_check(&c) == BAD);
  c = all_fields(); c.smoother_k_q15 = -1;
  CASE("check/smoothing_negative", skred_fx_ctl_check(&c) == BAD);
  c = all_fields(); c.which = SKRED_CTL_PHASE_INC | SKRED_CTL_INC_SCALE; c.inc_scale_q16 = 0xFFFFFFFFu;
  CASE("check/inc_and_scale_together", skred_fx_ctl_check(&c) == SKRED_OK);

  /* ---- the record as it travels */
  skx_ctl_t p;
  c = all_fields(); c.attack_frames = 48000; c.decay_frames = 1; c.release_frames = 0;
  skx_ctl_pack(&c, &p);
  int same = 1;
  for (int k = 0; k < SKX_CTL_RECIP_A; k++) same = same && p.w[k] == ((const uint32_t *)&c)[k];
  CASE("pack/word_for_word", same);
  CASE("pack/recips", p.w[SKX_CTL_RECIP_A] == (uint32_t)(0x100000000ull / 48000) && p.w[SKX_CTL_RECIP_D] == 0 /* 2^32 wraps */ && p.w[SKX_CTL_RECIP_R] == 0);
  c.which = SKRED_CTL_PAN;
  skx_ctl_pack(&c, &p);
  int clean = p.w[SKX_CTL_WHICH] == SKRED_CTL_PAN && p.w[SKX_CTL_PAN_LEFT] == 0 && p.w[SKX_CTL_PAN_RIGHT] == 65535;
  for (int k = 1; k < SKX_CTL_WORDS; k++) if (k != SKX_CTL_PAN_LEFT && k != SKX_CTL_PAN_RIGHT) clean = clean && p.w[k] == 0;
  CASE("pack/unnamed_words_never_travel", clean);
  c.which = SKRED_CTL_ENV_TIMES; c.attack_frames = 3; c.decay_frames = 0xFFFFFFFFu; c.release_frames = 2;
  skx_ctl_pack(&c, &p);
  CASE("pack/recips_edges", p.w[SKX_CTL_RECIP_A] == 0x55555555u && p.w[SKX_CTL_RECIP_D] == 1u && p.w[SKX_CTL_RECIP_R] == 0x80000000u &&
                             p.w[SKX_CTL_B0] == 0 && p.w[SKX_CTL_SUSTAIN] == 32768);

  CASE("sort/1", pack_ok(1));
  CASE("sort/2", pack_ok(2));
  CASE("sort/3", pack_ok(3));
  CASE("sort/1023", pack_ok(1023));
  CASE("sort/1024", pack_ok(1024));
  const uint32_t top[4] = { 0x80000000u, 1u, 0xFFFFFFFFu, 0x7FFFFFFFu };
  uint32_t s4[4], p4[4];
  CASE("sort/unsigned_order", sk_owner_pack(top, 4, s4, p4) == 0 && s4[0] == 1u && s4[1] == 0x7FFFFFFFu && s4[2] == 0x80000000u &&
                                s4[3] == 0xFFFFFFFFu && p4[0] == 1 && p4[1] == 3 && p4[2] == 0 && p4[3] == 2);

  /* ---- the entry points: a bank that is nothing but its size */
  skred_fxbank_t *fx = (skred_fxbank_t *)calloc(1, sizeof(skred_fxbank_t));
  fx->n_voices = 300;
  int32_t list[4] = { 0, 8, -1, 299 };
  uint32_t res[3] = { 0, 0, 0 };
  const uint32_t t4[4] = { 1, 2, 3, 0xFFFFFFFFu }, z4[4] = { 1, 0, 3, 4 }, d4[4] = { 1, 2, 1, 4 };
  const uint32_t REL = SKRED_STAMP_RELEASE;
  uint32_t *many = make_tags(1025);

  CASE("tag/null_bank", skred_fxbank_tag_list(NULL, list, t4, 4, NULL, NULL, NULL) == BAD);
  CASE("tag/null_list", skred_fxbank_tag_list(fx, NULL, t4, 4, NULL, NULL, NULL) == BAD);
  CASE("tag/null_tags", skred_fxbank_tag_list(fx, list, NULL, 4, NULL, NULL, NULL) == BAD);
  CASE("tag/negative_n", skred_fxbank_tag_list(fx, list, t4, -1, NULL, NULL, NULL) == BAD);
  CASE("tag/empty_with_zero_tags", skred_fxbank_tag_list(fx, list, z4, 0, NULL, NULL, NULL) == SKRED_OK);

  CASE("find/null_bank", skred_fxbank_find_owned(NULL, 0, 300, t4, 4, list, NULL) == BAD);
  CASE("find/null_out", skred_fxbank_find_owned(fx, 0, 300, t4, 4, NULL, NULL) == BAD);
  CASE("find/null_tags", skred_fxbank_find_owned(fx, 0, 300, NULL, 4, list, NULL) == BAD);
  CASE("find/negative_n", skred_fxbank_find_owned(fx, 0, 300, t4, -1, list, NULL) == BAD);
  CASE("find/zero_tag", skred_fxbank_find_owned(fx, 0, 300, z4, 4, list, NULL) == BAD);
  CASE("find/dup_tag", skred_fxbank_find_owned(fx, 0, 300, d4, 4, list, NULL) == BAD);
  CASE("find/1025_tags", skred_fxbank_find_owned(fx, 0, 300, many, 1025, list, NULL) == BAD);
  CASE("find/count_zero", skred_fxbank_find_owned(fx, 8, 0, t4, 4, list, NULL) == RNG);
  CASE("find/count_negative", skred_fxbank_find_owned(fx, 8, -8, t4, 4, list, NULL) == RNG);
  CASE("find/first_negative", skred_fxbank_find_owned(fx, -1, 8, t4, 4, list, NULL) == RNG);
  CASE("find/first_at_the_end", skred_fxbank_find_owned(fx, 300, 1, t4, 4, list, NULL) == RNG);
  CASE("find/past_the_bank", skred_fxbank_find_owned(fx, 299, 2, t4, 4, list, NULL) == RNG);
  CASE("find/huge_count", skred_fxbank_find_owned(fx, 8, INT32_MAX, t4, 4, list, NULL) == RNG);
  CASE("find/empty", skred_fxbank_find_owned(fx, 299, 1, t4, 0, list, NULL) == SKRED_OK);

  CASE("stamp/null_bank", skred_fxbank_stamp_owned(NULL, list, t4, 4, NULL, REL, res, NULL) == BAD);
  CASE("stamp/null_list", skred_fxbank_stamp_owned(fx, NULL, t4, 4, NULL, REL, res, NULL) == BAD);
  CASE("stamp/null_tags", skred_fxbank_stamp_owned(fx, list, NULL, 4, NULL, REL, res, NULL) == BAD);
  CASE("stamp/null_result", skred_fxbank_stamp_owned(fx, list, t4, 4, NULL, REL, NULL, NULL) == BAD);
  CASE("stamp/negative_n", skred_fxbank_stamp_owned(fx, list, t4, -1, NULL, REL, res, NULL) == BAD);
  CASE("stamp/zero_tag", skred_fxbank_stamp_owned(fx, list, z4, 4, NULL, REL, res, NULL) == BAD);
  CASE("stamp/no_stamp_bit", skred_fxbank_stamp_owned(fx, list, t4, 4, NULL, 0, res, NULL) == BAD);
  CASE("stamp/other_bits", skred_fxbank_stamp_owned(fx, list, t4, 4, NULL, REL | 1, res, NULL) == BAD);
  CASE("stamp/dup_tags_are_fine_but_empty", skred_fxbank_stamp_owned(fx, list, d4, 0, NULL, REL, res, NULL) == SKRED_OK);

  CASE("release/null_bank", skred_fxbank_release_tags(NULL, 0, 300, t4, 4, REL, res, NULL) == BAD);
  CASE("release/null_result", skred_fxbank_release_tags(fx, 0, 300, t4, 4, REL, NULL, NULL) == BAD);
  CASE("release/null_tags", skred_fxbank_release_tags(fx, 0, 300, NULL, 4, REL, res, NULL) == BAD);
  CASE("release/zero_tag", skred_fxbank_release_tags(fx, 0, 300, z4, 4, REL, res, NULL) == BAD);
  CASE("release/dup_tag", skred_fxbank_release_tags(fx, 0, 300, d4, 4, REL, res, NULL) == BAD);
  CASE("release/1025_tags", skred_fxbank_release_tags(fx, 0, 300, many, 1025, REL, res, NULL) == BAD);
  CASE("release/bad_stamps", skred_fxbank_release_tags(fx, 0, 300, t4, 4, 1024, res, NULL) == BAD);
  CASE("release/count_zero", skred_fxbank_release_tags(fx, 0, 0, t4, 4, REL, res, NULL) == RNG);
  CASE("release/past_the_bank", skred_fxbank_release_tags(fx, 0, 301, t4, 4, REL, res, NULL) == RNG);
  CASE("release/empty", skred_fxbank_release_tags(fx, 0, 300, t4, 0, REL, res, NULL) == SKRED_OK);

  /* the checks shared with the float bank (skred_bank_checks.c): the same codes, in the same order */
  CASE("stamp/stamps4", skred_fxbank_stamp_owned(fx, list, t4, 4, NULL, 4, res, NULL) == BAD);
  CASE("release/stamps4_count_zero", skred_fxbank_release_tags(fx, 300, 0, t4, 4, 4, res, NULL) == RNG);
  CASE("release/stamps0", skred_fxbank_release_tags(fx, 0, 300, t4, 4, 0, res, NULL) == BAD);
  CASE("find/count_zero_at_the_end", skred_fxbank_find_owned(fx, 300, 0, t4, 4, list, NULL) == RNG);

  CASE("clear/null_bank", skred_fxbank_owner_clear(NULL, 0, 8, NULL) == BAD);
  CASE("clear/negative", skred_fxbank_owner_clear(fx, 0, -1, NULL) == RNG);
  CASE("clear/past_the_bank", skred_fxbank_owner_clear(fx, 293, 8, NULL) == RNG);
  CASE("clear/never_tagged", skred_fxbank_owner_clear(fx, 0, 300, NULL) == SKRED_OK);
  uint32_t words[8];
  memset(words, 0xAB, sizeof(words));
  CASE("download/null", skred_fxbank_download_owners(NULL, words, 0, 8) == BAD && skred_fxbank_download_owners(fx, NULL, 0, 8) == BAD);
  CASE("download/negative", skred_fxbank_download_owners(fx, words, 0, -1) == BAD);
  CASE("download/past_the_bank", skred_fxbank_download_owners(fx, words, 296, 8) == RNG);
  int zeros = skred_fxbank_download_owners(fx, words, 292, 8) == SKRED_OK;
  for (int i = 0; i < 8; i++) zeros = zeros && words[i] == 0;
  CASE("download/never_tagged_is_zeros", zeros);
  skred_fxpt_bank_t view;
  memset(&view, 0, sizeof(view));
  view.n_voices = 300;
  CASE("download/params_null", skred_fxbank_download_params(NULL, &view, NULL, 0, 0, 8) == BAD && skred_fxbank_download_params(fx, NULL, NULL, 0, 0, 8) == BAD);
  CASE("download/params_past_the_bank", skred_fxbank_download_params(fx, &view, NULL, 296, 0, 8) == RNG && skred_fxbank_download_params(fx, &view, NULL, 0, 296, 8) == RNG);
  CASE("download/params_empty", skred_fxbank_download_params(fx, &view, NULL, 300, 300, 0) == SKRED_OK);

  skred_fx_ctl_t pan;
  memset(&pan, 0, sizeof(pan));
  pan.which = SKRED_CTL_PAN; pan.pan_left_q15 = 100; pan.pan_right_q15 = 200;
  skred_fx_ctl_t bad = pan;
  bad.which |= SKRED_CTL_FM_DEPTH;
  CASE("range/null_bank", skred_fxbank_ctl_range(NULL, &pan, 0, 300, NULL, NULL) == BAD);
  CASE("range/null_ctl", skred_fxbank_ctl_range(fx, NULL, 0, 300, NULL, NULL) == BAD);
  CASE("range/bad_ctl", skred_fxbank_ctl_range(fx, &bad, 0, 300, NULL, NULL) == BAD);
  CASE("range/count_negative", skred_fxbank_ctl_range(fx, &pan, 0, -1, NULL, NULL) == RNG);
  CASE("range/first_negative", skred_fxbank_ctl_range(fx, &pan, -1, 1, NULL, NULL) == RNG);
  CASE("range/past_the_bank", skred_fxbank_ctl_range(fx, &pan, 299, 2, NULL, NULL) == RNG);
  CASE("range/huge_count", skred_fxbank_ctl_range(fx, &pan, 8, INT32_MAX, NULL, NULL) == RNG);
  CASE("range/empty", skred_fxbank_ctl_range(fx, &pan, 300, 0, NULL, NULL) == SKRED_OK);
  CASE("range/empty_bad_ctl", skred_fxbank_ctl_range(fx, &bad, 300, 0, NULL, NULL) == BAD);

  CASE("list/null_bank", skred_fxbank_ctl_list(NULL, &pan, list, 4, NULL, NULL, NULL) == BAD);
  CASE("list/null_list", skred_fxbank_ctl_list(fx, &pan, NULL, 4, NULL, NULL, NULL) == BAD);
  CASE("list/null_ctl", skred_fxbank_ctl_list(fx, NULL, list, 4, NULL, NULL, NULL) == BAD);
  CASE("list/bad_ctl", skred_fxbank_ctl_list(fx, &bad, list, 4, NULL, NULL, NULL) == BAD);
  CASE("list/negative_n", skred_fxbank_ctl_list(fx, &pan, list, -1, NULL, NULL, NULL) == BAD);
  CASE("list/huge_n", skred_fxbank_ctl_list(fx, &pan, list, INT32_MAX / 64 + 1, NULL, NULL, NULL) == BAD);
  CASE("list/empty", skred_fxbank_ctl_list(fx, &pan, list, 0, NULL, NULL, NULL) == SKRED_OK);

  CASE("owned/null_bank", skred_fxbank_ctl_owned(NULL, &pan, list, t4, 4, NULL, NULL, NULL) == BAD);
  CASE("owned/null_list", skred_fxbank_ctl_owned(fx, &pan, NULL, t4, 4, NULL, NULL, NULL) == BAD);
  CASE("owned/null_tags", skred_fxbank_ctl_owned(fx, &pan, list, NULL, 4, NULL, NULL, NULL) == BAD);
  CASE("owned/null_ctl", skred_fxbank_ctl_owned(fx, NULL, list, t4, 4, NULL, NULL, NULL) == BAD);
  CASE("owned/bad_ctl", skred_fxbank_ctl_owned(fx, &bad, list, t4, 4, NULL, NULL, NULL) == BAD);
  CASE("owned/zero_tag", skred_fxbank_ctl_owned(fx, &pan, list, z4, 4, NULL, NULL, NULL) == BAD);
  CASE("owned/negative_n", skred_fxbank_ctl_owned(fx, &pan, list, t4, -1, NULL, NULL, NULL) == BAD);
  CASE("owned/empty", skred_fxbank_ctl_owned(fx, &pan, list, d4, 0, NULL, NULL, NULL) == SKRED_OK);

  /* the order of the checks, where two of them would answer differently */
  CASE("tag/null_tags_empty", skred_fxbank_tag_list(fx, list, NULL, 0, NULL, NULL, NULL) == BAD);
  CASE("tag/huge_n", skred_fxbank_tag_list(fx, list, t4, INT32_MAX / 64 + 1, NULL, NULL, NULL) == BAD);
  CASE("find/dup_tag_past_the_bank", skred_fxbank_find_owned(fx, 299, 2, d4, 4, list, NULL) == BAD);
  CASE("stamp/no_stamp_bit_empty", skred_fxbank_stamp_owned(fx, list, t4, 0, NULL, 0, res, NULL) == BAD);
  CASE("release/zero_tag_count_zero", skred_fxbank_release_tags(fx, 0, 0, z4, 4, REL, res, NULL) == BAD);
  CASE("release/bad_stamps_empty", skred_fxbank_release_tags(fx, 0, 300, t4, 0, 1024, res, NULL) == BAD);

  /* ---- the live calls that go through the same batch path (skred_fx_live.c, skred_fxbank_stamp): refused before the device */
  int32_t log2s[8] = { 3, 3, 3, 3, 3, 3, 3, 3 }, offs[8] = { 0 }, amps[8] = { 0 };
  const int32_t v01[2] = { 0, 1 }, v8[1] = { 8 }, v300[2] = { 0, 300 }, vneg[1] = { -1 };
  memset(&view, 0, sizeof(view));
  view.n_voices = 8; view.log2_size = log2s; view.table_offset = offs; view.amp_q15 = amps;
  const uint32_t PARAMS = SKRED_DIRTY_PARAMS;
  CASE("update/null_bank", skred_fxbank_update(NULL, &view, v01, 2, PARAMS, NULL) == BAD);
  CASE("update/null_view", skred_fxbank_update(fx, NULL, v01, 2, PARAMS, NULL) == BAD);
  CASE("update/null_voices", skred_fxbank_update(fx, &view, NULL, 2, PARAMS, NULL) == BAD);
  CASE("update/negative_n", skred_fxbank_update(fx, &view, v01, -1, PARAMS, NULL) == BAD);
  CASE("update/empty_before_the_mask", skred_fxbank_update(fx, &view, NULL, 0, 0, NULL) == SKRED_OK);
  CASE("update/dirty0", skred_fxbank_update(fx, &view, v01, 2, 0, NULL) == BAD);
  CASE("update/unknown_bit", skred_fxbank_update(fx, &view, v01, 2, 1u << 11, NULL) == BAD);
  CASE("update/hold", skred_fxbank_update(fx, &view, v01, 2, PARAMS | SKRED_DIRTY_HOLD, NULL) == BAD);
  CASE("update/mask_before_the_voices", skred_fxbank_update(fx, &view, v300, 2, 0, NULL) == BAD);
  CASE("update/voice_past_the_bank", skred_fxbank_update(fx, &view, v300, 2, PARAMS, NULL) == RNG);
  CASE("update/voice_past_the_view", skred_fxbank_update(fx, &view, v8, 1, PARAMS, NULL) == RNG);
  CASE("update/voice_negative", skred_fxbank_update(fx, &view, vneg, 1, PARAMS, NULL) == RNG);
  CASE("update/stamp_voice_past_the_bank", skred_fxbank_update(fx, &view, v300, 2, SKRED_STAMP_TRIGGER, NULL) == RNG);
  CASE("update/table_outside_the_pool", skred_fxbank_update(fx, &view, v01, 2, PARAMS, NULL) == RNG);      /* (a pool of 0 entries) */
  fx->table_entries = 64;
  amps[0] = 65536;
  CASE("update/amp_high", skred_fxbank_update(fx, &view, v01, 2, PARAMS, NULL) == RNG);
  log2s[0] = 16; amps[0] = 0;
  CASE("update/log2_size_high", skred_fxbank_update(fx, &view, v01, 2, PARAMS, NULL) == RNG);
  fx->table_entries = 0;
  CASE("ids/null_bank", skred_fxbank_stamp(NULL, v01, 2, 1, NULL) == BAD);
  CASE("ids/null_voices", skred_fxbank_stamp(fx, NULL, 2, 1, NULL) == BAD);
  CASE("ids/negative_n", skred_fxbank_stamp(fx, v01, -1, 1, NULL) == BAD);
  CASE("ids/which0", skred_fxbank_stamp(fx, v01, 2, 0, NULL) == BAD);
  CASE("ids/which4", skred_fxbank_stamp(fx, v01, 2, 4, NULL) == BAD);
  CASE("ids/which0_empty", skred_fxbank_stamp(fx, v01, 0, 0, NULL) == BAD);
  CASE("ids/voice_past_the_bank", skred_fxbank_stamp(fx, v300, 2, 3, NULL) == RNG);
  CASE("ids/empty", skred_fxbank_stamp(fx, NULL, 0, 3, NULL) == SKRED_OK);

  skred_fx_note_t note[2];
  memset(note, 0, sizeof(note));
  note[0].phase_inc = note[1].phase_inc = 3000017u; note[0].velocity_q15 = note[1].velocity_q15 = 9000;
  int32_t out4[4] = { -7, -7, -7, -7 };
#define NOTES(bank, nt, n, l, c, fe, r) skred_fxbank_notes_on_list(bank, nt, n, l, c, fe, out4, r, NULL)
  CASE("notes/null_bank", NOTES(NULL, note, 2, list, res, 0, res) == BAD);
  CASE("notes/null_notes", NOTES(fx, NULL, 2, list, res, 0, res) == BAD);
  CASE("notes/null_list", NOTES(fx, note, 2, NULL, res, 0, res) == BAD);
  CASE("notes/null_count", NOTES(fx, note, 2, list, NULL, 0, res) == BAD);
  CASE("notes/null_result", NOTES(fx, note, 2, list, res, 0, NULL) == BAD);
  CASE("notes/negative_n", NOTES(fx, note, -1, list, res, 0, res) == BAD);
  CASE("notes/negative_first_entry", NOTES(fx, note, 2, list, res, -1, res) == BAD);
  note[1].flags = 4;
  CASE("notes/unknown_flag", NOTES(fx, note, 2, list, res, 0, res) == BAD);
  CASE("notes/empty_before_the_notes", NOTES(fx, note, 0, list, res, 0, res) == SKRED_OK);
  note[1].flags = 0; note[1].reserved[0] = 1;
  CASE("notes/reserved", NOTES(fx, note, 2, list, res, 0, res) == BAD);
  note[1].reserved[0] = 0; note[0].velocity_q15 = 65536;
  CASE("notes/velocity_high", NOTES(fx, note, 2, list, res, 0, res) == BAD);
  note[0].velocity_q15 = 9000;

  skred_fx_idle_query_t q;
  memset(&q, 0, sizeof(q));
  q.first = 0; q.count = 300; q.which = SKRED_IDLE_ENV_DONE; q.from = 0; q.max_out = 4;
  skred_fx_idle_query_t qb;
  CASE("on_idle/null_bank", skred_fxbank_note_on_idle(NULL, &q, note, 2, out4, res, NULL) == BAD);
  CASE("on_idle/null_query", skred_fxbank_note_on_idle(fx, NULL, note, 2, out4, res, NULL) == BAD);
  CASE("on_idle/null_notes", skred_fxbank_note_on_idle(fx, &q, NULL, 2, out4, res, NULL) == BAD);
  CASE("on_idle/null_result", skred_fxbank_note_on_idle(fx, &q, note, 2, out4, NULL, NULL) == BAD);
  CASE("on_idle/negative_n", skred_fxbank_note_on_idle(fx, &q, note, -1, out4, res, NULL) == BAD);
  qb = q; qb.which |= SKRED_IDLE_AMP_ZERO;
  CASE("on_idle/amp_zero", skred_fxbank_note_on_idle(fx, &qb, note, 2, out4, res, NULL) == BAD);
  qb = q; qb.count = 301;
  CASE("on_idle/past_the_bank", skred_fxbank_note_on_idle(fx, &qb, note, 2, out4, res, NULL) == RNG);
  CASE("on_idle/past_the_bank_empty", skred_fxbank_note_on_idle(fx, &qb, note, 0, out4, res, NULL) == RNG);
  qb = q; qb.from = 300;
  CASE("on_idle/from_outside", skred_fxbank_note_on_idle(fx, &qb, note, 2, out4, res, NULL) == RNG);
  CASE("on_idle/empty", skred_fxbank_note_on_idle(fx, &q, note, 0, out4, res, NULL) == SKRED_OK);
  note[1].flags = 8;
  CASE("on_idle/unknown_flag", skred_fxbank_note_on_idle(fx, &q, note, 2, out4, res, NULL) == BAD);
  note[1].flags = 0;

  int idle_total = -5;
  CASE("idle_host/null_bank", skred_fxbank_find_idle_host(NULL, &q, out4, &idle_total, NULL) == BAD);
  CASE("idle_host/null_query", skred_fxbank_find_idle_host(fx, NULL, out4, &idle_total, NULL) == BAD);
  CASE("idle_host/null_list", skred_fxbank_find_idle_host(fx, &q, NULL, &idle_total, NULL) == BAD);
  qb = q; qb.max_out = -1;
  CASE("idle_host/negative_max_out", skred_fxbank_find_idle_host(fx, &qb, out4, &idle_total, NULL) == BAD);
  qb = q; qb.which = SKRED_IDLE_ENV_DONE | SKRED_IDLE_UNNAMED;
  CASE("idle_host/unnamed", skred_fxbank_find_idle_host(fx, &qb, out4, &idle_total, NULL) == BAD);
  qb = q; qb.which = 0;
  CASE("idle_host/no_criterion", skred_fxbank_find_idle_host(fx, &qb, out4, &idle_total, NULL) == BAD);
  qb = q; qb.count = 0;
  CASE("idle_host/empty_range", skred_fxbank_find_idle_host(fx, &qb, out4, &idle_total, NULL) == RNG);
  qb = q; qb.first = 299; qb.from = 299; qb.count = 2;
  CASE("idle_host/past_the_bank", skred_fxbank_find_idle_host(fx, &qb, out4, &idle_total, NULL) == RNG);
  CASE("idle_host/outputs_untouched", idle_total == -5 && out4[0] == -7 && out4[3] == -7 && res[0] == 0 && res[1] == 0 && res[2] == 0);

  int untouched = !fx->d_owner && !fx->d_owner_found && fx->ring_head == 0 && fx->n_filter == 0 && fx->count == 0 && !fx->upd_mark &&
                  !fx->d_idle && !fx->d_idle_out && !fx->h_idle_out && !fx->d_note_list;
  for (int i = 0; i < SKX_RING; i++) untouched = untouched && !fx->ring[i].h && !fx->ring[i].d && !fx->ring[i].ev && !fx->ring[i].in_flight;
  CASE("bank/untouched", untouched);
  free(many);
  free(fx);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
