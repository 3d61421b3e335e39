/* The host side of the note owners without a device: skred_owner_tags_check, the sort-plus-permutation packing of the find pass
 * (sk_owner_pack) and every refusal the entry points make before anything touches the device, on a skred_bank_t that is nothing but
 * its voice count (a refused call reads no other member).  One line per case, "OK" last.  tests/test_owner_cpu.py builds and runs
 * it; built together with skred_amd/csrc/skred_bank_owner.c, the shared checks and the batch path it reaches, and -fsanitize=address,undefined
 * it is the sanitizer run of those files' host code -- from the repository root, after the library is built (the program's own copy of
 * skred_bank_owner.c, skred_bank_checks.c and skred_bank_stage.c takes the place of the library's; everything else it calls comes from the library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_owner_host.c skred_amd/csrc/skred_bank_owner.c skred_amd/csrc/skred_bank_checks.c \
 *       skred_amd/csrc/skred_bank_stage.c -o /tmp/c_owner_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_owner_host_san */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_bank_priv.h"

static int failures;
#define CASE(name, cond) do { const int ok_ = (cond); printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); failures += !ok_; } while (0)

/* n distinct non-zero tags in no order, with the top bit set on every other one; tags[0] = 0xFFFFFFFF when n > 1 */
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
  if (ok && n > 1) ok = sorted[n - 1] == 0xFFFFFFFFu && perm[n - 1] == 0;   /* the largest unsigned number sorts last */
  free(seen); free(perm); free(sorted); free(t);
  return ok;
}

int main(void) {
  CASE("const/max_tags", SKRED_OWNER_MAX_TAGS == 1024 && SK_OWNER_MAX_TAGS == 1024);
  CASE("const/flags", SKRED_OWNER_ALLOW_ZERO == 1 && SKRED_OWNER_UNIQUE == 2);
  CASE("const/lds", 2 * sizeof(uint32_t) * SKRED_OWNER_MAX_TAGS == 8192);

  const uint32_t two[2] = { 5, 0x80000000u }, zero[2] = { 5, 0 }, dup[3] = { 9, 5, 9 };
  CASE("check/plain", skred_owner_tags_check(two, 2, 0) == SKRED_OK);
  CASE("check/unique", skred_owner_tags_check(two, 2, SKRED_OWNER_UNIQUE) == SKRED_OK);
  CASE("check/null", skred_owner_tags_check(NULL, 2, 0) == SKRED_E_BAD_ARG);
  CASE("check/negative_n", skred_owner_tags_check(two, -1, 0) == SKRED_E_BAD_ARG);
  CASE("check/empty", skred_owner_tags_check(two, 0, SKRED_OWNER_UNIQUE) == SKRED_OK);
  CASE("check/unknown_flag", skred_owner_tags_check(two, 2, 4) == SKRED_E_BAD_ARG);
  CASE("check/zero", skred_owner_tags_check(zero, 2, 0) == SKRED_E_BAD_ARG);
  CASE("check/zero_allowed", skred_owner_tags_check(zero, 2, SKRED_OWNER_ALLOW_ZERO) == SKRED_OK);
  CASE("check/zero_beyond_n", skred_owner_tags_check(zero, 1, 0) == SKRED_OK);
  CASE("check/dup", skred_owner_tags_check(dup, 3, SKRED_OWNER_UNIQUE) == SKRED_E_BAD_ARG);
  CASE("check/dup_allowed", skred_owner_tags_check(dup, 3, 0) == SKRED_OK);
  CASE("check/dup_beyond_n", skred_owner_tags_check(dup, 2, SKRED_OWNER_UNIQUE) == SKRED_OK);
  uint32_t *many = make_tags(1025);
  CASE("check/1024", skred_owner_tags_check(many, 1024, SKRED_OWNER_UNIQUE) == SKRED_OK);
  CASE("check/1025", skred_owner_tags_check(many, 1025, SKRED_OWNER_UNIQUE) == SKRED_E_BAD_ARG);
  CASE("check/1025_not_unique", skred_owner_tags_check(many, 1025, 0) == SKRED_OK);
  many[1023] = many[1];
  CASE("check/1024_dup_at_the_end", skred_owner_tags_check(many, 1024, SKRED_OWNER_UNIQUE) == SKRED_E_BAD_ARG);
  free(many);

  CASE("pack/1", pack_ok(1));
  CASE("pack/2", pack_ok(2));
  CASE("pack/1023", pack_ok(1023));
  CASE("pack/1024", pack_ok(1024));
  uint32_t s3[3], p3[3];
  CASE("pack/dup_reported", sk_owner_pack(dup, 3, s3, p3) != 0);
  const uint32_t top[4] = { 0x80000000u, 1u, 0xFFFFFFFFu, 0x7FFFFFFFu };
  uint32_t s4[4], p4[4];
  CASE("pack/unsigned_order", sk_owner_pack(top, 4, s4, p4) == 0 && s4[0] == 1u && s4[1] == 0x7FFFFFFFu && s4[2] == 0x80000000u &&
                                s4[3] == 0xFFFFFFFFu && p4[0] == 1 && p4[1] == 3 && p4[2] == 0 && p4[3] == 2);

  /* the entry points: a bank that is nothing but its size */
  skred_bank_t *b = (skred_bank_t *)calloc(1, sizeof(skred_bank_t));
  b->n_voices = 200;
  int32_t list[4] = { 0, 8, 16, 24 };
  uint32_t res[3] = { 0, 0, 0 };
  const uint32_t t4[4] = { 1, 2, 3, 0xFFFFFFFFu }, z4[4] = { 1, 0, 3, 4 }, d4[4] = { 1, 2, 1, 4 };
  const uint32_t REL = SKRED_STAMP_RELEASE;

  CASE("tag/null_bank", skred_bank_tag_slots(NULL, list, t4, 4, NULL, 8, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("tag/null_list", skred_bank_tag_slots(b, NULL, t4, 4, NULL, 8, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("tag/null_tags", skred_bank_tag_slots(b, list, NULL, 4, NULL, 8, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("tag/negative_n", skred_bank_tag_slots(b, list, t4, -1, NULL, 8, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("tag/bad_k", skred_bank_tag_slots(b, list, t4, 4, NULL, 12, NULL, NULL) == SKRED_E_RANGE);
  CASE("tag/k128", skred_bank_tag_slots(b, list, t4, 4, NULL, 128, NULL, NULL) == SKRED_E_RANGE);
  CASE("tag/empty_with_zero_tags", skred_bank_tag_slots(b, list, z4, 0, NULL, 8, NULL, NULL) == SKRED_OK);

  CASE("find/null_bank", skred_bank_find_owned(NULL, 0, 200, 8, t4, 4, list, NULL) == SKRED_E_BAD_ARG);
  CASE("find/null_out", skred_bank_find_owned(b, 0, 200, 8, t4, 4, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("find/null_tags", skred_bank_find_owned(b, 0, 200, 8, NULL, 4, list, NULL) == SKRED_E_BAD_ARG);
  CASE("find/negative_n", skred_bank_find_owned(b, 0, 200, 8, t4, -1, list, NULL) == SKRED_E_BAD_ARG);
  CASE("find/zero_tag", skred_bank_find_owned(b, 0, 200, 8, z4, 4, list, NULL) == SKRED_E_BAD_ARG);
  CASE("find/dup_tag", skred_bank_find_owned(b, 0, 200, 8, d4, 4, list, NULL) == SKRED_E_BAD_ARG);
  many = make_tags(1025);
  CASE("find/1025_tags", skred_bank_find_owned(b, 0, 200, 8, many, 1025, list, NULL) == SKRED_E_BAD_ARG);
  free(many);
  CASE("find/bad_k", skred_bank_find_owned(b, 0, 200, 3, t4, 4, list, NULL) == SKRED_E_RANGE);
  CASE("find/first_off_slot", skred_bank_find_owned(b, 4, 8, 8, t4, 4, list, NULL) == SKRED_E_RANGE);
  CASE("find/count_off_slot", skred_bank_find_owned(b, 8, 12, 8, t4, 4, list, NULL) == SKRED_E_RANGE);
  CASE("find/count_zero", skred_bank_find_owned(b, 8, 0, 8, t4, 4, list, NULL) == SKRED_E_RANGE);
  CASE("find/count_negative", skred_bank_find_owned(b, 8, -8, 8, t4, 4, list, NULL) == SKRED_E_RANGE);
  CASE("find/first_negative", skred_bank_find_owned(b, -8, 8, 8, t4, 4, list, NULL) == SKRED_E_RANGE);
  CASE("find/past_the_bank", skred_bank_find_owned(b, 192, 16, 8, t4, 4, list, NULL) == SKRED_E_RANGE);
  CASE("find/huge_count", skred_bank_find_owned(b, 8, INT32_MAX - 7, 8, t4, 4, list, NULL) == SKRED_E_RANGE);
  CASE("find/empty", skred_bank_find_owned(b, 192, 8, 8, t4, 0, list, NULL) == SKRED_OK);

  CASE("stamp/null_bank", skred_bank_stamp_owned(NULL, list, t4, 4, NULL, 8, 0xFF, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/null_list", skred_bank_stamp_owned(b, NULL, t4, 4, NULL, 8, 0xFF, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/null_tags", skred_bank_stamp_owned(b, list, NULL, 4, NULL, 8, 0xFF, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/null_result", skred_bank_stamp_owned(b, list, t4, 4, NULL, 8, 0xFF, REL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/negative_n", skred_bank_stamp_owned(b, list, t4, -1, NULL, 8, 0xFF, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/zero_tag", skred_bank_stamp_owned(b, list, z4, 4, NULL, 8, 0xFF, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/no_stamp_bit", skred_bank_stamp_owned(b, list, t4, 4, NULL, 8, 0xFF, 0, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/other_bits", skred_bank_stamp_owned(b, list, t4, 4, NULL, 8, 0xFF, REL | 1, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/mask0", skred_bank_stamp_owned(b, list, t4, 4, NULL, 8, 0, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/mask_high", skred_bank_stamp_owned(b, list, t4, 4, NULL, 8, 0x100, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/bad_k", skred_bank_stamp_owned(b, list, t4, 4, NULL, 6, 0x3F, REL, res, NULL) == SKRED_E_RANGE);
  CASE("stamp/dup_tags_are_fine_but_empty", skred_bank_stamp_owned(b, list, d4, 0, NULL, 8, 0xFF, REL, res, NULL) == SKRED_OK);

  CASE("release/null_bank", skred_bank_release_tags(NULL, 0, 200, 8, 0xFF, t4, 4, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("release/null_result", skred_bank_release_tags(b, 0, 200, 8, 0xFF, t4, 4, REL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("release/null_tags", skred_bank_release_tags(b, 0, 200, 8, 0xFF, NULL, 4, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("release/zero_tag", skred_bank_release_tags(b, 0, 200, 8, 0xFF, z4, 4, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("release/dup_tag", skred_bank_release_tags(b, 0, 200, 8, 0xFF, d4, 4, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("release/bad_stamps", skred_bank_release_tags(b, 0, 200, 8, 0xFF, t4, 4, 1024, res, NULL) == SKRED_E_BAD_ARG);
  CASE("release/mask0", skred_bank_release_tags(b, 0, 200, 8, 0, t4, 4, REL, res, NULL) == SKRED_E_BAD_ARG);
  CASE("release/bad_k", skred_bank_release_tags(b, 0, 200, 0, 1, t4, 4, REL, res, NULL) == SKRED_E_RANGE);
  CASE("release/range_off_slot", skred_bank_release_tags(b, 4, 8, 8, 0xFF, t4, 4, REL, res, NULL) == SKRED_E_RANGE);
  CASE("release/past_the_bank", skred_bank_release_tags(b, 0, 208, 8, 0xFF, t4, 4, REL, res, NULL) == SKRED_E_RANGE);
  CASE("release/empty", skred_bank_release_tags(b, 0, 200, 8, 0xFF, t4, 0, REL, res, NULL) == SKRED_OK);

  skred_ctl_t k8[8];
  memset(k8, 0, sizeof(k8));
  for (int l = 0; l < 8; l++) { k8[l].set = SKRED_CTL_PAN; k8[l].pan_left = 0.25f; k8[l].pan_right = 0.75f; }
  CASE("ctl/null_bank", skred_bank_ctl_owned(NULL, k8, 8, 0xFF, list, t4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/null_list", skred_bank_ctl_owned(b, k8, 8, 0xFF, NULL, t4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/null_tags", skred_bank_ctl_owned(b, k8, 8, 0xFF, list, NULL, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/null_ctl", skred_bank_ctl_owned(b, NULL, 8, 0xFF, list, t4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/zero_tag", skred_bank_ctl_owned(b, k8, 8, 0xFF, list, z4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/negative_n", skred_bank_ctl_owned(b, k8, 8, 0xFF, list, t4, -1, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/bad_k", skred_bank_ctl_owned(b, k8, 5, 0x1F, list, t4, 4, NULL, NULL, NULL) == SKRED_E_RANGE);
  CASE("ctl/mask0", skred_bank_ctl_owned(b, k8, 8, 0, list, t4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  k8[2].set = 0;
  CASE("ctl/set0_masked", skred_bank_ctl_owned(b, k8, 8, 0xFF, list, t4, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("ctl/set0_unmasked_empty", skred_bank_ctl_owned(b, k8, 8, 0xFB, list, t4, 0, NULL, NULL, NULL) == SKRED_OK);

  /* the checks the entry points share (skred_bank_checks.c): a find refuses the empty range a controller accepts, and a call that is
   * wrong in several ways gets the code of its first check -- stamp_owned looks at the stamps before K, release_tags at K first */
  CASE("find/count_zero_at_the_end", skred_bank_find_owned(b, 200, 0, 8, t4, 4, list, NULL) == SKRED_E_RANGE);
  CASE("ctl/range_empty_at_the_end", skred_bank_ctl_range(b, k8, 200, 0, 8, 0xFB, NULL, NULL) == SKRED_OK);
  CASE("stamp/k3_mask_at_k_stamps0", skred_bank_stamp_owned(b, list, t4, 4, NULL, 3, 0x8, 0, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/k3_mask_at_k_stamps4", skred_bank_stamp_owned(b, list, t4, 4, NULL, 3, 0x8, 4, res, NULL) == SKRED_E_BAD_ARG);
  CASE("stamp/k3_mask_at_k", skred_bank_stamp_owned(b, list, t4, 4, NULL, 3, 0x8, REL, res, NULL) == SKRED_E_RANGE);
  CASE("release/k3_mask_at_k_stamps0", skred_bank_release_tags(b, 0, 200, 3, 0x8, t4, 4, 0, res, NULL) == SKRED_E_RANGE);
  CASE("release/k3_mask_at_k_stamps4", skred_bank_release_tags(b, 0, 200, 3, 0x8, t4, 4, 4, res, NULL) == SKRED_E_RANGE);
  CASE("release/mask_at_k_stamps0", skred_bank_release_tags(b, 0, 200, 4, 0x10, t4, 4, 0, res, NULL) == SKRED_E_BAD_ARG);
  CASE("release/count_zero_bad_mask", skred_bank_release_tags(b, 200, 0, 8, 0, t4, 4, REL, res, NULL) == SKRED_E_RANGE);

  CASE("clear/null_bank", skred_bank_owner_clear(NULL, 0, 8, NULL) == SKRED_E_BAD_ARG);
  CASE("clear/negative", skred_bank_owner_clear(b, 0, -1, NULL) == SKRED_E_RANGE);
  CASE("clear/past_the_bank", skred_bank_owner_clear(b, 193, 8, NULL) == SKRED_E_RANGE);
  CASE("clear/never_tagged", skred_bank_owner_clear(b, 0, 200, NULL) == SKRED_OK);
  uint32_t words[8];
  memset(words, 0xAB, sizeof(words));
  CASE("download/null", skred_bank_download_owners(NULL, words, 0, 8) == SKRED_E_BAD_ARG && skred_bank_download_owners(b, NULL, 0, 8) == SKRED_E_BAD_ARG);
  CASE("download/past_the_bank", skred_bank_download_owners(b, words, 196, 8) == SKRED_E_RANGE);
  int zeros = skred_bank_download_owners(b, words, 192, 8) == SKRED_OK;
  for (int i = 0; i < 8; i++) zeros = zeros && words[i] == 0;
  CASE("download/never_tagged_is_zeros", zeros);
  CASE("download/clocks_null", skred_bank_download_env_clocks(NULL, NULL, NULL, 0, 8) == SKRED_E_BAD_ARG);
  CASE("download/clocks_past_the_bank", skred_bank_download_env_clocks(b, NULL, NULL, 196, 8) == SKRED_E_RANGE);
  CASE("bank/untouched", b->touched_total == 0 && b->control_epoch == 0 && b->upd_seq == 0 && b->upd_head == 0 && !b->d_owner && !b->d_owner_slots);
  free(b);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
