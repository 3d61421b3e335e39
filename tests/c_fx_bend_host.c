/* The host side of the fixed-point pitch-wheel calls without a device: skred_fx_bend_check ratio by ratio, every refusal the entry
 * points make before anything touches the device, with its return code and in the documented order -- on a skred_fxbank_t that is
 * nothing but its voice count (a refused call reads no other member) --, and what travels behind skred_fxbank_bend_tags_each: the tags
 * sorted (sk_owner_pack) and the ratios permuted with them (skx_bend_pack), at n = 1, 2, 1023, 1024.  One line per case, "OK" last.
 * tests/test_fx_bend_cpu.py builds and runs it; built together with skred_amd/csrc/skred_fx_bend.c and
 * -fsanitize=address,undefined it is the sanitizer run of that file's host code -- from the repository root, after the library is
 * built (the program's own copy of skred_fx_bend.c takes the place of the library's; everything else it calls comes from the
 * library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_fx_bend_host.c skred_amd/csrc/skred_fx_bend.c -o /tmp/c_fx_bend_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_fx_bend_host_san
 * (both files are plain C host code: with hipcc the two sanitizer flags go behind -Xarch_host) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_fxbank_priv.h"

static int failures;
#define CASE(name, cond) do { const int ok_ = (cond); printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); failures += !ok_; } while (0)

#define N 600
#define BAD SKRED_E_BAD_ARG
#define RANGE SKRED_E_RANGE
#define ONE SKRED_FX_BEND_ONE

/* the sort-plus-permutation behind bend_tags_each at n tags given in descending order with a twist: entry k carries ratio 1000 + k */
static int permuted(int n) {
  uint32_t *tags = (uint32_t *)calloc((size_t)n, sizeof(uint32_t)), *sorted = (uint32_t *)calloc((size_t)n, sizeof(uint32_t));
  uint32_t *perm = (uint32_t *)calloc((size_t)n, sizeof(uint32_t)), *r = (uint32_t *)calloc((size_t)n, sizeof(uint32_t));
  uint32_t *out = (uint32_t *)calloc((size_t)n + 1, sizeof(uint32_t));
  for (int k = 0; k < n; k++) {
    tags[k] = (k & 1 ? 0x80000000u : 0u) + 5u * (uint32_t)(n - k);        /* every other one at or above 2^31: unsigned order */
    r[k] = 1000u + (uint32_t)k;
  }
  memset(out, 0xEE, ((size_t)n + 1) * sizeof(uint32_t));
  int ok = sk_owner_pack(tags, n, sorted, perm) == SKRED_OK;
  skx_bend_pack(r, n, perm, out);
  for (int j = 0; j < n && ok; j++) {
    const uint32_t k = perm[j];
    ok = k < (uint32_t)n && sorted[j] == tags[k] && (j == 0 || sorted[j - 1] < sorted[j]) && out[j] == 1000u + k;
  }
  ok = ok && out[n] == 0xEEEEEEEEu;                                       /* n words and not one more */
  free(tags); free(sorted); free(perm); free(r); free(out);
  return ok;
}

int main(void) {
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0xFFFFFFFFu, 0x80000000u }, z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u };
  const uint32_t d4[4] = { 0x03000001u, 0x03000002u, 0x03000001u, 0x03000004u };
  static uint32_t many[SKRED_OWNER_MAX_TAGS + 1], rmany[SKRED_OWNER_MAX_TAGS + 1];
  for (int k = 0; k <= SKRED_OWNER_MAX_TAGS; k++) { many[k] = 1u + (uint32_t)k; rmany[k] = ONE; }
  const uint32_t r4[4] = { 1u, ONE, ONE + 1u, 0xFFFFFFFFu }, b4[4] = { 1u, ONE, ONE + 1u, 0u };
  const skred_owner_match_t chan = { 0x03000000u, 0xFF000000u }, everyone = { 0u, 0u }, never = { 0x03000001u, 0xFF000000u };

  CASE("const/one", ONE == 1u << 24 && SKX_BEND_ONE == ONE);
  CASE("const/sizes", sizeof(skx_bend_t) == 8 && SKX_BEND_KEY == 0 && SKX_BEND_RATIO == 1);

  /* skred_fx_bend_check */
  CASE("check/plain", skred_fx_bend_check(r4, 4) == SKRED_OK);
  CASE("check/empty", skred_fx_bend_check(r4, 0) == SKRED_OK);
  CASE("check/null", skred_fx_bend_check(NULL, 0) == BAD);
  CASE("check/null_before_n", skred_fx_bend_check(NULL, -1) == BAD);
  CASE("check/negative_n", skred_fx_bend_check(r4, -1) == BAD);
  CASE("check/zero_ratio", skred_fx_bend_check(b4, 4) == BAD);
  CASE("check/zero_ratio_not_reached", skred_fx_bend_check(b4, 3) == SKRED_OK);
  CASE("check/edges", skred_fx_bend_check(r4, 1) == SKRED_OK && skred_fx_bend_check(r4 + 3, 1) == SKRED_OK);

  /* the packing: the words as they stand, in order or permuted */
  {
    uint32_t out[5];
    memset(out, 0xEE, sizeof(out));
    skx_bend_pack(r4, 4, NULL, out);
    CASE("pack/in_order", !memcmp(out, r4, sizeof(r4)) && out[4] == 0xEEEEEEEEu);
    const uint32_t perm[4] = { 3, 1, 0, 2 };
    skx_bend_pack(r4, 4, perm, out);
    CASE("pack/permuted", out[0] == r4[3] && out[1] == r4[1] && out[2] == r4[0] && out[3] == r4[2] && out[4] == 0xEEEEEEEEu);
    uint32_t sorted[4], p[4];
    CASE("pack/tags_sorted_unsigned", sk_owner_pack(t4, 4, sorted, p) == SKRED_OK && sorted[0] == 0x03000001u && sorted[2] == 0x80000000u &&
                                      sorted[3] == 0xFFFFFFFFu && p[2] == 3 && p[3] == 2);
    CASE("pack/sort_and_permute_1", permuted(1));
    CASE("pack/sort_and_permute_2", permuted(2));
    CASE("pack/sort_and_permute_1023", permuted(1023));
    CASE("pack/sort_and_permute_1024", permuted(1024));
  }

  /* the entry points: a bank that is nothing but its size */
  skred_fxbank_t *fx = (skred_fxbank_t *)calloc(1, sizeof(skred_fxbank_t));
  fx->n_voices = N;
  int32_t list[4] = { 0, 8, 16, 24 };
  uint32_t res[4] = { 7, 7, 7, 7 }, words[16];
  for (int k = 0; k < 16; k++) words[k] = 7;
  /* the channel wheel: NULL bank or match, ratio 0, the match, the range -- in that order */
  CASE("match/null_bank", skred_fxbank_bend_match(NULL, 0, N, &chan, ONE, res, NULL) == BAD);
  CASE("match/null_match", skred_fxbank_bend_match(fx, 0, N, NULL, ONE, res, NULL) == BAD);
  CASE("match/zero_ratio", skred_fxbank_bend_match(fx, 0, N, &chan, 0, res, NULL) == BAD);
  CASE("match/bad_match", skred_fxbank_bend_match(fx, 0, N, &never, ONE, res, NULL) == BAD);
  CASE("match/ratio_before_match", skred_fxbank_bend_match(fx, 0, N, &never, 0, res, NULL) == BAD &&
                                   strstr(skred_amd_last_error(), "ratio") != NULL);
  CASE("match/match_before_range", skred_fxbank_bend_match(fx, 0, N + 1, &never, ONE, res, NULL) == BAD);
  CASE("match/past_the_bank", skred_fxbank_bend_match(fx, 0, N + 1, &chan, ONE, res, NULL) == RANGE);
  CASE("match/empty_range", skred_fxbank_bend_match(fx, 0, 0, &everyone, ONE + 5u, res, NULL) == RANGE);
  CASE("match/negative_first", skred_fxbank_bend_match(fx, -1, 4, &chan, 1u, res, NULL) == RANGE);
  CASE("match/first_at_the_end", skred_fxbank_bend_match(fx, N, 1, &chan, 0xFFFFFFFFu, res, NULL) == RANGE);
  /* the per-note calls: NULL bank or list, the tags, n, the ratios -- skred_fxbank_glide_owned's order */
  CASE("owned/null_bank", skred_fxbank_bend_owned_each(NULL, r4, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_list", skred_fxbank_bend_owned_each(fx, r4, NULL, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_tags", skred_fxbank_bend_owned_each(fx, r4, list, NULL, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_ratios", skred_fxbank_bend_owned_each(fx, NULL, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/zero_tag", skred_fxbank_bend_owned_each(fx, r4, list, z4, 4, NULL, res, NULL) == BAD);
  CASE("owned/negative_n", skred_fxbank_bend_owned_each(fx, r4, list, t4, -2, NULL, res, NULL) == BAD);
  CASE("owned/zero_ratio", skred_fxbank_bend_owned_each(fx, b4, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/tags_before_ratios", skred_fxbank_bend_owned_each(fx, b4, list, z4, 4, NULL, res, NULL) == BAD &&
                                   strstr(skred_amd_last_error(), "ratio") == NULL);
  CASE("owned/repeated_tag_is_fine_but_the_ratio_is_not", skred_fxbank_bend_owned_each(fx, b4, list, d4, 4, NULL, res, NULL) == BAD &&
                                                          strstr(skred_amd_last_error(), "ratio") != NULL);
  CASE("owned/empty", skred_fxbank_bend_owned_each(fx, r4, list, t4, 0, NULL, res, NULL) == SKRED_OK);
  CASE("owned/empty_null_result", skred_fxbank_bend_owned_each(fx, r4, list, t4, 0, NULL, NULL, NULL) == SKRED_OK);
  CASE("tags/null_bank", skred_fxbank_bend_tags_each(NULL, r4, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/null_tags", skred_fxbank_bend_tags_each(fx, r4, 0, N, NULL, 4, res, NULL) == BAD);
  CASE("tags/null_ratios", skred_fxbank_bend_tags_each(fx, NULL, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/repeated_tag", skred_fxbank_bend_tags_each(fx, r4, 0, N, d4, 4, res, NULL) == BAD);
  CASE("tags/zero_tag", skred_fxbank_bend_tags_each(fx, r4, 0, N, z4, 4, res, NULL) == BAD);
  CASE("tags/too_many", skred_fxbank_bend_tags_each(fx, rmany, 0, N, many, SKRED_OWNER_MAX_TAGS + 1, res, NULL) == BAD);
  CASE("tags/zero_ratio", skred_fxbank_bend_tags_each(fx, b4, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/ratios_before_range", skred_fxbank_bend_tags_each(fx, b4, 0, N + 1, t4, 4, res, NULL) == BAD);
  CASE("tags/past_the_bank", skred_fxbank_bend_tags_each(fx, r4, 0, N + 1, t4, 4, res, NULL) == RANGE);
  CASE("tags/empty_range", skred_fxbank_bend_tags_each(fx, r4, 0, 0, t4, 4, res, NULL) == RANGE);
  CASE("tags/negative_first", skred_fxbank_bend_tags_each(fx, r4, -1, 4, t4, 4, res, NULL) == RANGE);
  CASE("tags/range_before_empty_list", skred_fxbank_bend_tags_each(fx, r4, 0, N + 1, t4, 0, res, NULL) == RANGE);
  CASE("tags/empty", skred_fxbank_bend_tags_each(fx, r4, 0, N, t4, 0, res, NULL) == SKRED_OK);
  CASE("clear/null_bank", skred_fxbank_bend_clear(NULL, 0, N, 0, NULL) == BAD);
  CASE("clear/past_the_bank", skred_fxbank_bend_clear(fx, 8, N, 1, NULL) == RANGE);
  CASE("clear/negative_count", skred_fxbank_bend_clear(fx, 0, -1, 0, NULL) == RANGE);
  CASE("clear/no_array_yet", skred_fxbank_bend_clear(fx, 0, N, 1, NULL) == SKRED_OK);
  CASE("clear/empty", skred_fxbank_bend_clear(fx, N, 0, 1, NULL) == SKRED_OK);
  CASE("download/null_bank", skred_fxbank_download_bend(NULL, words, 0, 4) == BAD);
  CASE("download/null_out", skred_fxbank_download_bend(fx, NULL, 0, 4) == BAD);
  CASE("download/negative_count", skred_fxbank_download_bend(fx, words, 0, -1) == BAD);
  CASE("download/past_the_bank", skred_fxbank_download_bend(fx, words, N - 2, 4) == RANGE);
  CASE("download/empty", skred_fxbank_download_bend(fx, words, 0, 0) == SKRED_OK && words[0] == 7);
  int zeros = skred_fxbank_download_bend(fx, words, N - 3, 3) == SKRED_OK;
  for (int k = 0; k < 6; k++) zeros = zeros && words[k] == 0;
  CASE("download/no_array_yet_gives_zeros", zeros && words[6] == 7 && words[15] == 7);

  CASE("untouched/outputs", res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && list[0] == 0 && list[3] == 24);
  CASE("untouched/bank", fx->ring_head == 0 && !fx->d_owner && !fx->d_pedal && !fx->d_glide && !fx->d_bend && !fx->d_owner_found &&
                         fx->count == 0 && !fx->ring[0].in_flight);
  free(fx);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
