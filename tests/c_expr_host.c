/* The host side of channels and per-note expression without a device: skred_owner_match_check, skred_ctl_each_check, the packing of
 * the per-entry records (sk_each_pack: named values word for word, the others zeroed), the permutation that keeps each[k] beside
 * tags[k] through the sort of the tags, and every refusal the entry points make before anything touches the device, on a skred_bank_t
 * that is nothing but its voice count (a refused call reads no other member).  One line per case, "OK" last.
 * tests/test_expr_cpu.py builds and runs it; built together with skred_amd/csrc/skred_bank_expr.c, the shared checks and the batch
 * path it reaches, and -fsanitize=address,undefined it is the sanitizer run of those files' host code -- from the repository root,
 * after the library is built (the program's own copy of skred_bank_expr.c, skred_bank_checks.c and skred_bank_stage.c takes the place
 * of the library's; everything else it calls comes from the library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_expr_host.c skred_amd/csrc/skred_bank_expr.c skred_amd/csrc/skred_bank_checks.c \
 *       skred_amd/csrc/skred_bank_stage.c -o /tmp/c_expr_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_expr_host_san */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_bank_priv.h"

static int failures;
#define CASE(name, cond) do { const int ok_ = (cond); printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); failures += !ok_; } while (0)

static skred_ctl_each_t each_of(uint32_t set, float v) {
  skred_ctl_each_t e;
  memset(&e, 0, sizeof(e));
  e.set = set; e.inc_scale = v; e.amp_scale = v; e.velocity = v; e.pan_left = v; e.pan_right = v;
  return e;
}

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* n distinct non-zero tags in no order (as tests/c_owner_host.c draws them), entry k marked with its own index */
static int perm_ok(int n) {
  uint32_t *tags = (uint32_t *)malloc((size_t)n * sizeof(uint32_t)), *sorted = (uint32_t *)malloc((size_t)n * sizeof(uint32_t));
  uint32_t *perm = (uint32_t *)malloc((size_t)n * sizeof(uint32_t));
  skred_ctl_each_t *each = (skred_ctl_each_t *)malloc((size_t)n * sizeof(skred_ctl_each_t));
  sk_each_t *out = (sk_each_t *)malloc((size_t)n * sizeof(sk_each_t));
  for (int k = 0; k < n; k++) {
    tags[k] = (1u + ((uint32_t)k * 7919u) % 1031u) | ((k & 1) ? 0x80000000u : 0u);
    each[k] = each_of(SKRED_EACH_VELOCITY, (float)k);     /* the entry knows which tag it came with */
  }
  if (n > 1) tags[0] = 0xFFFFFFFFu;
  int ok = sk_owner_pack(tags, n, sorted, perm) == 0 && sk_each_pack(each, n, perm, out) == SKRED_EACH_VELOCITY;
  for (int j = 0; j < n && ok; j++) {
    const uint32_t k = perm[j];                           /* sorted[j] stood at k: the entry beside it must be each[k] */
    ok = sorted[j] == tags[k] && (j == 0 || sorted[j - 1] < sorted[j]) && out[j].w[SK_EACH_W_VELOCITY] == bits_of((float)k);
  }
  if (ok && n > 1) ok = out[n - 1].w[SK_EACH_W_VELOCITY] == bits_of(0.0f);   /* 0xFFFFFFFF sorts last and brings entry 0 */
  free(out); free(each); free(perm); free(sorted); free(tags);
  return ok;
}

int main(void) {
  CASE("const/bits", SKRED_EACH_INC_SCALE == 1 && SKRED_EACH_AMP_SCALE == 2 && SKRED_EACH_VELOCITY == 4 && SKRED_EACH_PAN == 8 && SK_EACH_ALL == 15);
  CASE("const/sizes", sizeof(skred_ctl_each_t) == 32 && sizeof(sk_each_t) == 32 && sizeof(skred_owner_match_t) == 8);

  skred_owner_match_t all = { 0, 0 }, chan = { 0x03000000u, 0xFF000000u }, one = { 0xFFFFFFFFu, 0xFFFFFFFFu }, off = { 0x03000001u, 0xFF000000u };
  skred_owner_match_t off0 = { 1u, 0u };
  CASE("match/all", skred_owner_match_check(&all) == SKRED_OK);
  CASE("match/channel", skred_owner_match_check(&chan) == SKRED_OK);
  CASE("match/one_note", skred_owner_match_check(&one) == SKRED_OK);
  CASE("match/null", skred_owner_match_check(NULL) == SKRED_E_BAD_ARG);
  CASE("match/value_outside_mask", skred_owner_match_check(&off) == SKRED_E_BAD_ARG);
  CASE("match/value_with_mask0", skred_owner_match_check(&off0) == SKRED_E_BAD_ARG);

  skred_ctl_t k4[4], amp4[4], inc4[4];
  memset(k4, 0, sizeof(k4));
  for (int l = 0; l < 4; l++) { k4[l].set = SKRED_CTL_FILTER; k4[l].b0 = 0.5f; }
  memcpy(amp4, k4, sizeof(k4));
  memcpy(inc4, k4, sizeof(k4));
  for (int l = 0; l < 4; l++) { amp4[l].set |= SKRED_CTL_AMP; amp4[l].amp = 0.5f; }
  inc4[2].set |= SKRED_CTL_INC_SCALE; inc4[2].inc_scale = 1.5f;
  skred_ctl_each_t e2[2] = { each_of(SKRED_EACH_VELOCITY | SKRED_EACH_PAN, 0.5f), each_of(SKRED_EACH_INC_SCALE, 1.01f) };
  skred_ctl_each_t bad;
  CASE("each/plain", skred_ctl_each_check(e2, 2, k4, 4, 0xF) == SKRED_OK);
  CASE("each/no_records", skred_ctl_each_check(e2, 2, NULL, 4, 0xF) == SKRED_OK);
  CASE("each/null", skred_ctl_each_check(NULL, 2, k4, 4, 0xF) == SKRED_E_BAD_ARG);
  CASE("each/negative_n", skred_ctl_each_check(e2, -1, k4, 4, 0xF) == SKRED_E_BAD_ARG);
  CASE("each/empty", skred_ctl_each_check(e2, 0, k4, 4, 0xF) == SKRED_OK);
  CASE("each/bad_k", skred_ctl_each_check(e2, 2, k4, 3, 0x7) == SKRED_E_RANGE);
  CASE("each/bad_k_no_records", skred_ctl_each_check(e2, 2, NULL, 128, 0xF) == SKRED_E_RANGE);
  CASE("each/mask0", skred_ctl_each_check(e2, 2, k4, 4, 0) == SKRED_E_BAD_ARG);
  CASE("each/mask0_no_records", skred_ctl_each_check(e2, 2, NULL, 4, 0) == SKRED_E_BAD_ARG);
  CASE("each/mask_high_no_records", skred_ctl_each_check(e2, 2, NULL, 4, 0x10) == SKRED_E_BAD_ARG);
  k4[1].set = 0;
  CASE("each/bad_record", skred_ctl_each_check(e2, 2, k4, 4, 0xF) == SKRED_E_BAD_ARG);
  CASE("each/bad_record_unmasked", skred_ctl_each_check(e2, 2, k4, 4, 0xD) == SKRED_OK);
  k4[1].set = SKRED_CTL_FILTER;
  bad = each_of(16, 0.5f);
  CASE("each/unknown_bits", skred_ctl_each_check(&bad, 1, k4, 4, 0xF) == SKRED_E_BAD_ARG);
  bad = each_of(0, 0.5f);
  CASE("each/set0", skred_ctl_each_check(&bad, 1, k4, 4, 0xF) == SKRED_E_BAD_ARG);
  bad = each_of(SKRED_EACH_PAN, 0.5f); bad.reserved[1] = 1;
  CASE("each/reserved", skred_ctl_each_check(&bad, 1, k4, 4, 0xF) == SKRED_E_BAD_ARG);
  bad = each_of(SKRED_EACH_PAN, 0.5f); bad.reserved[0] = 1;
  CASE("each/reserved0", skred_ctl_each_check(&bad, 1, k4, 4, 0xF) == SKRED_E_BAD_ARG);
  bad = each_of(SKRED_EACH_INC_SCALE, INFINITY);
  CASE("each/inc_inf", skred_ctl_each_check(&bad, 1, k4, 4, 0xF) == SKRED_E_BAD_ARG);
  bad = each_of(SKRED_EACH_VELOCITY, NAN);
  CASE("each/velocity_nan", skred_ctl_each_check(&bad, 1, k4, 4, 0xF) == SKRED_E_BAD_ARG);
  bad = each_of(SKRED_EACH_PAN, 0.5f); bad.pan_right = -INFINITY;
  CASE("each/pan_inf", skred_ctl_each_check(&bad, 1, k4, 4, 0xF) == SKRED_E_BAD_ARG);
  bad = each_of(SKRED_EACH_PAN, 0.5f); bad.inc_scale = NAN; bad.amp_scale = INFINITY; bad.velocity = NAN;
  CASE("each/unnamed_values_are_not_looked_at", skred_ctl_each_check(&bad, 1, k4, 4, 0xF) == SKRED_OK);
  bad = each_of(SKRED_EACH_AMP_SCALE, 0.5f);
  CASE("each/amp_scale", skred_ctl_each_check(&bad, 1, amp4, 4, 0xF) == SKRED_OK);
  CASE("each/amp_scale_without_amp", skred_ctl_each_check(&bad, 1, k4, 4, 0xF) == SKRED_E_BAD_ARG);
  CASE("each/amp_scale_no_records", skred_ctl_each_check(&bad, 1, NULL, 4, 0xF) == SKRED_E_BAD_ARG);
  amp4[3].set &= ~(uint32_t)SKRED_CTL_AMP;
  CASE("each/amp_scale_one_record_lacks_amp", skred_ctl_each_check(&bad, 1, amp4, 4, 0xF) == SKRED_E_BAD_ARG);
  CASE("each/amp_scale_that_record_unmasked", skred_ctl_each_check(&bad, 1, amp4, 4, 0x7) == SKRED_OK);
  amp4[3].set |= SKRED_CTL_AMP;
  bad = each_of(SKRED_EACH_AMP_SCALE, 0.0f);
  CASE("each/amp_scale_zero", skred_ctl_each_check(&bad, 1, amp4, 4, 0xF) == SKRED_E_BAD_ARG);
  bad = each_of(SKRED_EACH_AMP_SCALE, -0.0f);
  CASE("each/amp_scale_minus_zero", skred_ctl_each_check(&bad, 1, amp4, 4, 0xF) == SKRED_E_BAD_ARG);
  bad = each_of(SKRED_EACH_AMP_SCALE, NAN);
  CASE("each/amp_scale_nan", skred_ctl_each_check(&bad, 1, amp4, 4, 0xF) == SKRED_E_BAD_ARG);
  bad = each_of(SKRED_EACH_INC_SCALE, 1.01f);
  CASE("each/inc_scale_over_inc_scale", skred_ctl_each_check(&bad, 1, inc4, 4, 0xF) == SKRED_E_BAD_ARG);
  CASE("each/inc_scale_that_record_unmasked", skred_ctl_each_check(&bad, 1, inc4, 4, 0xB) == SKRED_OK);
  inc4[2].set = SKRED_CTL_PHASE_INC; inc4[2].phase_inc = 0.1f;
  CASE("each/inc_scale_over_phase_inc", skred_ctl_each_check(&bad, 1, inc4, 4, 0xF) == SKRED_E_BAD_ARG);
  skred_ctl_each_t second[2] = { each_of(SKRED_EACH_PAN, 0.5f), each_of(SKRED_EACH_PAN | 32, 0.5f) };
  CASE("each/second_entry", skred_ctl_each_check(second, 2, k4, 4, 0xF) == SKRED_E_BAD_ARG && skred_ctl_each_check(second, 1, k4, 4, 0xF) == SKRED_OK);

  /* the packing: named values word for word, the others zeroed, the reserved words zero */
  skred_ctl_each_t src[3] = { each_of(SKRED_EACH_INC_SCALE, 1.25f), each_of(SKRED_EACH_PAN | SKRED_EACH_VELOCITY, 0.75f), each_of(SK_EACH_ALL, -2.0f) };
  src[1].pan_right = 0.125f;
  sk_each_t out[3];
  memset(out, 0xAB, sizeof(out));
  const uint32_t bits = sk_each_pack(src, 3, NULL, out);
  CASE("pack/bits", bits == SK_EACH_ALL);
  CASE("pack/inc_alone", out[0].w[0] == 1 && out[0].w[1] == bits_of(1.25f) && !out[0].w[2] && !out[0].w[3] && !out[0].w[4] && !out[0].w[5] && !out[0].w[6] && !out[0].w[7]);
  CASE("pack/pan_velocity", out[1].w[0] == 12 && !out[1].w[1] && !out[1].w[2] && out[1].w[3] == bits_of(0.75f) && out[1].w[4] == bits_of(0.75f) &&
                            out[1].w[5] == bits_of(0.125f) && !out[1].w[6] && !out[1].w[7]);
  CASE("pack/all", out[2].w[0] == 15 && out[2].w[1] == bits_of(-2.0f) && out[2].w[2] == bits_of(-2.0f) && out[2].w[5] == bits_of(-2.0f) && !out[2].w[6]);
  const uint32_t rev[3] = { 2, 0, 1 };
  CASE("pack/permuted", sk_each_pack(src, 3, rev, out) == SK_EACH_ALL && out[0].w[0] == 15 && out[1].w[0] == 1 && out[2].w[0] == 12);
  CASE("pack/one_bit", sk_each_pack(src, 1, NULL, out) == SKRED_EACH_INC_SCALE);
  CASE("perm/1", perm_ok(1));
  CASE("perm/2", perm_ok(2));
  CASE("perm/257", perm_ok(257));
  CASE("perm/1024", perm_ok(1024));

  /* the entry points: a bank that is nothing but its size */
  skred_bank_t *b = (skred_bank_t *)calloc(1, sizeof(skred_bank_t));
  b->n_voices = 200;
  int32_t list[4] = { 0, 8, 16, 24 };
  uint32_t res[3] = { 0, 0, 0 };
  int total = 0;
  const uint32_t REL = SKRED_STAMP_RELEASE;

  CASE("find/null_bank", skred_bank_find_match(NULL, 0, 200, 8, &chan, 4, list, res, NULL) == SKRED_E_BAD_ARG);
  CASE("find/null_match", skred_bank_find_match(b, 0, 200, 8, NULL, 4, list, res, NULL) == SKRED_E_BAD_ARG);
  CASE("find/bad_match", skred_bank_find_match(b, 0, 200, 8, &off, 4, list, res, NULL) == SKRED_E_BAD_ARG);
  CASE("find/null_count", skred_bank_find_match(b, 0, 200, 8, &chan, 4, list, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("find/negative_max_out", skred_bank_find_match(b, 0, 200, 8, &chan, -1, list, res, NULL) == SKRED_E_BAD_ARG);
  CASE("find/null_list", skred_bank_find_match(b, 0, 200, 8, &chan, 4, NULL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("find/bad_k", skred_bank_find_match(b, 0, 200, 3, &chan, 4, list, res, NULL) == SKRED_E_RANGE);
  CASE("find/first_off_slot", skred_bank_find_match(b, 4, 8, 8, &chan, 4, list, res, NULL) == SKRED_E_RANGE);
  CASE("find/count_off_slot", skred_bank_find_match(b, 8, 12, 8, &chan, 4, list, res, NULL) == SKRED_E_RANGE);
  CASE("find/count_zero", skred_bank_find_match(b, 8, 0, 8, &chan, 4, list, res, NULL) == SKRED_E_RANGE);
  CASE("find/past_the_bank", skred_bank_find_match(b, 192, 16, 8, &chan, 4, list, res, NULL) == SKRED_E_RANGE);
  CASE("find/huge_count", skred_bank_find_match(b, 8, INT32_MAX - 7, 8, &chan, 4, list, res, NULL) == SKRED_E_RANGE);
  CASE("find/first_negative", skred_bank_find_match(b, -8, 8, 8, &chan, 4, list, res, NULL) == SKRED_E_RANGE);
  CASE("find_host/null_bank", skred_bank_find_match_host(NULL, 0, 200, 8, &chan, 4, list, &total, NULL) == SKRED_E_BAD_ARG);
  CASE("find_host/null_list", skred_bank_find_match_host(b, 0, 200, 8, &chan, 4, NULL, &total, NULL) == SKRED_E_BAD_ARG);
  CASE("find_host/bad_match", skred_bank_find_match_host(b, 0, 200, 8, &off, 4, list, &total, NULL) == SKRED_E_BAD_ARG);
  CASE("find_host/range", skred_bank_find_match_host(b, 0, 208, 8, &chan, 4, list, &total, NULL) == SKRED_E_RANGE);

  CASE("stamp/null_bank", skred_bank_stamp_match(NULL, 0, 200, 8, 0xFF, &chan, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/null_result", skred_bank_stamp_match(b, 0, 200, 8, 0xFF, &chan, REL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/null_match", skred_bank_stamp_match(b, 0, 200, 8, 0xFF, NULL, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/bad_match", skred_bank_stamp_match(b, 0, 200, 8, 0xFF, &off0, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/no_stamp_bit", skred_bank_stamp_match(b, 0, 200, 8, 0xFF, &chan, 0, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/other_bits", skred_bank_stamp_match(b, 0, 200, 8, 0xFF, &chan, REL | 1, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/mask0", skred_bank_stamp_match(b, 0, 200, 8, 0, &chan, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/mask_high", skred_bank_stamp_match(b, 0, 200, 8, 0x100, &chan, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/bad_k", skred_bank_stamp_match(b, 0, 200, 6, 0x3F, &chan, REL, res, NULL) == SKRED_E_RANGE);
  CASE("stamp/range_off_slot", skred_bank_stamp_match(b, 4, 8, 8, 0xFF, &chan, REL, res, NULL) == SKRED_E_RANGE);
  CASE("stamp/count_zero", skred_bank_stamp_match(b, 8, 0, 8, 0xFF, &chan, REL, res, NULL) == SKRED_E_RANGE);
  CASE("stamp/past_the_bank", skred_bank_stamp_match(b, 0, 208, 8, 0xFF, &chan, REL, res, NULL) == SKRED_E_RANGE);

  /* the checks the entry points share (skred_bank_checks.c): a call that is wrong in several ways gets the code of its first check
   * (stamp_match looks at the stamps before K and the mask), and the matches refuse the empty range a controller accepts */
  CASE("stamp/k3_mask_at_k_stamps0", skred_bank_stamp_match(b, 0, 200, 3, 0x8, &chan, 0, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/k3_mask_at_k_stamps4", skred_bank_stamp_match(b, 0, 200, 3, 0x8, &chan, 4, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/k3_mask_at_k", skred_bank_stamp_match(b, 0, 200, 3, 0x8, &chan, REL, res, NULL) == SKRED_E_RANGE);
  CASE("stamp/count_zero_at_the_end", skred_bank_stamp_match(b, 200, 0, 8, 0xFF, &chan, REL, res, NULL) == SKRED_E_RANGE);
  CASE("find/count_zero_at_the_end", skred_bank_find_match(b, 200, 0, 8, &chan, 4, list, res, NULL) == SKRED_E_RANGE);

  skred_ctl_t k8[8];
  memset(k8, 0, sizeof(k8));
  for (int l = 0; l < 8; l++) { k8[l].set = SKRED_CTL_PAN; k8[l].pan_left = 0.25f; k8[l].pan_right = 0.75f; }
  CASE("ctl/count_zero_at_the_end", skred_bank_ctl_match(b, k8, 200, 0, 8, 0xFF, &chan, NULL, NULL) == SKRED_E_RANGE);
  CASE("ctl/range_empty_at_the_end", skred_bank_ctl_range(b, k8, 200, 0, 8, 0xFF, NULL, NULL) == SKRED_OK);
  CASE("ctl/null_bank", skred_bank_ctl_match(NULL, k8, 0, 200, 8, 0xFF, &chan, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/null_ctl", skred_bank_ctl_match(b, NULL, 0, 200, 8, 0xFF, &chan, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/null_match", skred_bank_ctl_match(b, k8, 0, 200, 8, 0xFF, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/bad_match", skred_bank_ctl_match(b, k8, 0, 200, 8, 0xFF, &off, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/mask0", skred_bank_ctl_match(b, k8, 0, 200, 8, 0, &chan, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/bad_k", skred_bank_ctl_match(b, k8, 0, 200, 5, 0x1F, &chan, NULL, NULL) == SKRED_E_RANGE);
  CASE("ctl/range_off_slot", skred_bank_ctl_match(b, k8, 8, 12, 8, 0xFF, &chan, NULL, NULL) == SKRED_E_RANGE);
  CASE("ctl/count_zero", skred_bank_ctl_match(b, k8, 8, 0, 8, 0xFF, &chan, NULL, NULL) == SKRED_E_RANGE);
  CASE("ctl/past_the_bank", skred_bank_ctl_match(b, k8, 192, 16, 8, 0xFF, &chan, NULL, NULL) == SKRED_E_RANGE);
  k8[2].set = 0;
  CASE("ctl/set0_masked", skred_bank_ctl_match(b, k8, 0, 200, 8, 0xFF, &chan, NULL, NULL) == SKRED_E_BAD_ARG);
  k8[2].set = SKRED_CTL_PAN;

  const uint32_t t4[4] = { 1, 2, 3, 0xFFFFFFFFu }, z4[4] = { 1, 0, 3, 4 }, d4[4] = { 1, 2, 1, 4 };
  skred_ctl_each_t e4[4] = { each_of(SKRED_EACH_VELOCITY, 0.5f), each_of(SKRED_EACH_INC_SCALE, 1.5f), each_of(SKRED_EACH_PAN, 0.5f), each_of(SKRED_EACH_VELOCITY, 0.25f) };
  skred_ctl_each_t a4[4] = { each_of(SKRED_EACH_AMP_SCALE, 0.5f), each_of(SKRED_EACH_AMP_SCALE, 0.5f), each_of(SKRED_EACH_AMP_SCALE, 0.5f), each_of(SKRED_EACH_AMP_SCALE, 0.5f) };
  CASE("owned/null_bank", skred_bank_ctl_owned_each(NULL, k8, e4, 8, 0xFF, list, t4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("owned/null_list", skred_bank_ctl_owned_each(b, k8, e4, 8, 0xFF, NULL, t4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("owned/null_tags", skred_bank_ctl_owned_each(b, k8, e4, 8, 0xFF, list, NULL, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("owned/null_each", skred_bank_ctl_owned_each(b, k8, NULL, 8, 0xFF, list, t4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("owned/zero_tag", skred_bank_ctl_owned_each(b, k8, e4, 8, 0xFF, list, z4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("owned/negative_n", skred_bank_ctl_owned_each(b, k8, e4, 8, 0xFF, list, t4, -1, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("owned/bad_k", skred_bank_ctl_owned_each(b, NULL, e4, 5, 0x1F, list, t4, 4, NULL, NULL, NULL) == SKRED_E_RANGE);
  CASE("owned/mask0", skred_bank_ctl_owned_each(b, k8, e4, 8, 0, list, t4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("owned/amp_scale_without_amp", skred_bank_ctl_owned_each(b, k8, a4, 8, 0xFF, list, t4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("owned/amp_scale_no_records", skred_bank_ctl_owned_each(b, NULL, a4, 8, 0xFF, list, t4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("owned/empty", skred_bank_ctl_owned_each(b, k8, e4, 8, 0xFF, list, d4, 0, NULL, NULL, NULL) == SKRED_OK);
  CASE("owned/empty_no_records", skred_bank_ctl_owned_each(b, NULL, e4, 8, 0xFF, list, t4, 0, NULL, NULL, NULL) == SKRED_OK);

  CASE("tags/null_bank", skred_bank_ctl_tags_each(NULL, k8, e4, 0, 200, 8, 0xFF, t4, 4, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("tags/null_tags", skred_bank_ctl_tags_each(b, k8, e4, 0, 200, 8, 0xFF, NULL, 4, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("tags/null_each", skred_bank_ctl_tags_each(b, k8, NULL, 0, 200, 8, 0xFF, t4, 4, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("tags/zero_tag", skred_bank_ctl_tags_each(b, k8, e4, 0, 200, 8, 0xFF, z4, 4, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("tags/dup_tag", skred_bank_ctl_tags_each(b, k8, e4, 0, 200, 8, 0xFF, d4, 4, NULL, NULL) == SKRED_E_BAD_ARG);
  uint32_t *many = (uint32_t *)malloc(1025 * sizeof(uint32_t));
  skred_ctl_each_t *many_e = (skred_ctl_each_t *)malloc(1025 * sizeof(skred_ctl_each_t));
  for (int k = 0; k < 1025; k++) { many[k] = 1u + (uint32_t)k; many_e[k] = each_of(SKRED_EACH_PAN, 0.5f); }
  CASE("tags/1025_tags", skred_bank_ctl_tags_each(b, k8, many_e, 0, 200, 8, 0xFF, many, 1025, NULL, NULL) == SKRED_E_BAD_ARG);
  free(many_e); free(many);
  CASE("tags/bad_entry", skred_bank_ctl_tags_each(b, k8, a4, 0, 200, 8, 0xFF, t4, 4, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("tags/bad_k", skred_bank_ctl_tags_each(b, NULL, e4, 0, 200, 3, 0x7, t4, 4, NULL, NULL) == SKRED_E_RANGE);
  CASE("tags/range_off_slot", skred_bank_ctl_tags_each(b, k8, e4, 4, 8, 8, 0xFF, t4, 4, NULL, NULL) == SKRED_E_RANGE);
  CASE("tags/count_zero", skred_bank_ctl_tags_each(b, k8, e4, 8, 0, 8, 0xFF, t4, 4, NULL, NULL) == SKRED_E_RANGE);
  CASE("tags/past_the_bank", skred_bank_ctl_tags_each(b, k8, e4, 0, 208, 8, 0xFF, t4, 4, NULL, NULL) == SKRED_E_RANGE);
  CASE("tags/empty", skred_bank_ctl_tags_each(b, k8, e4, 0, 200, 8, 0xFF, t4, 0, NULL, NULL) == SKRED_OK);

  CASE("bank/untouched", b->touched_total == 0 && b->control_epoch == 0 && b->upd_seq == 0 && b->upd_head == 0 && !b->d_owner && !b->d_owner_slots &&
                         !b->d_match_pair && !b->d_idle);
  free(b);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
