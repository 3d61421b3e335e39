/* The host side of the pitch-wheel calls without a device: skred_bend_check, the packing of the ratios, the permutation that keeps
 * ratios[k] with tags[k] when the tags travel sorted (n = 1, 2, 1023, 1024) and every refusal the entry points make before anything
 * touches the device, each with its return code and in the header's order, on a skred_bank_t that is nothing but its voice count (a
 * refused call reads no other member).  One line per case, "OK" last.  tests/test_bend_cpu.py builds and runs it; built together with
 * skred_amd/csrc/skred_bank_bend.c and -fsanitize=address,undefined it is the sanitizer run of that file's host code -- from the
 * repository root, after the library is built (the program's own copy of skred_bank_bend.c takes the place of the library's;
 * everything else it calls comes from the library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_bend_host.c skred_amd/csrc/skred_bank_bend.c -o /tmp/c_bend_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_bend_host_san */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_bank_priv.h"

static int failures;
#define CASE(name, cond) do { const int ok_ = (cond); printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); failures += !ok_; } while (0)

#define N 1024
#define K 8
#define MASK 0x55ull
#define BAD SKRED_E_BAD_ARG
#define RANGE SKRED_E_RANGE

static int one(float r) { return skred_bend_check(&r, 1, K, MASK); }

/* tags in a scrambled order, ratio k marked with k: after the pack, word j must be the ratio that stood with the j-th smallest tag */
static int perm_case(int n) {
  static uint32_t tags[SKRED_OWNER_MAX_TAGS], sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS], out[SKRED_OWNER_MAX_TAGS + 1];
  static float in[SKRED_OWNER_MAX_TAGS];
  for (int k = 0; k < n; k++) {
    tags[k] = 0x80000000u ^ (uint32_t)(((uint64_t)k * 2654435761u) % 1000003u + 1u);     /* distinct: k < 1000003 and the map is a bijection mod a prime */
    in[k] = 0.5f + (float)k / 1024.0f;
  }
  out[n] = 0xA5A5A5A5u;
  if (sk_owner_pack(tags, n, sorted, perm)) return 0;
  sk_bend_pack(in, n, perm, out);
  for (int j = 0; j < n; j++) {
    if (j && sorted[j] <= sorted[j - 1]) return 0;
    if (tags[perm[j]] != sorted[j]) return 0;
    if (memcmp(&out[j], &in[perm[j]], 4)) return 0;
  }
  return out[n] == 0xA5A5A5A5u;                                                           /* nothing past word n - 1 */
}

int main(void) {
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0xFFFFFFFFu, 0x80000000u }, z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u };
  const uint32_t d4[4] = { 0x03000001u, 0x03000002u, 0x03000001u, 0x03000004u };
  static uint32_t many[SKRED_OWNER_MAX_TAGS + 1];
  static float rmany[SKRED_OWNER_MAX_TAGS + 1];
  for (int k = 0; k <= SKRED_OWNER_MAX_TAGS; k++) { many[k] = 1u + (uint32_t)k; rmany[k] = 1.5f; }
  const float r4[4] = { 1.0f, 1.0594631f, 0.5f, 2.0f }, bad4[4] = { 1.0f, 2.0f, 0.0f, 1.5f };
  const skred_owner_match_t chan = { 0x03000000u, 0xFF000000u }, wrong = { 0x03000001u, 0xFF000000u };

  CASE("const/size", sizeof(sk_bend_t) == 8 && SK_BEND_KEY == 0 && SK_BEND_RATIO == 1);

  /* skred_bend_check */
  CASE("check/plain", skred_bend_check(r4, 4, K, MASK) == SKRED_OK);
  CASE("check/empty", skred_bend_check(r4, 0, K, MASK) == SKRED_OK);
  CASE("check/null", skred_bend_check(NULL, 4, K, MASK) == BAD);
  CASE("check/null_before_k", skred_bend_check(NULL, 4, 3, MASK) == BAD);
  CASE("check/negative_n", skred_bend_check(r4, -1, K, MASK) == BAD);
  CASE("check/k3", skred_bend_check(r4, 4, 3, 1) == RANGE);
  CASE("check/k0", skred_bend_check(r4, 4, 0, 1) == RANGE);
  CASE("check/k128", skred_bend_check(r4, 4, 128, 1) == RANGE);
  CASE("check/k_before_mask", skred_bend_check(r4, 4, 3, 0) == RANGE);
  CASE("check/k_before_ratio", skred_bend_check(bad4, 4, 3, 1) == RANGE);
  CASE("check/mask0", skred_bend_check(r4, 4, K, 0) == BAD);
  CASE("check/mask_high", skred_bend_check(r4, 4, K, 0x100) == BAD);
  CASE("check/k64_full_mask", skred_bend_check(r4, 4, 64, ~0ull) == SKRED_OK);
  CASE("check/k1", skred_bend_check(r4, 4, 1, 1) == SKRED_OK);
  CASE("check/ratio_zero", one(0.0f) == BAD);
  CASE("check/ratio_negative_zero", one(-0.0f) == BAD);
  CASE("check/ratio_negative", one(-2.0f) == BAD);
  CASE("check/ratio_nan", one(NAN) == BAD);
  CASE("check/ratio_inf", one(INFINITY) == BAD);
  CASE("check/ratio_tiny", one(0x1p-149f) == SKRED_OK);
  CASE("check/ratio_huge", one(3e38f) == SKRED_OK);
  CASE("check/ratio_one", one(1.0f) == SKRED_OK);
  CASE("check/third_ratio", skred_bend_check(bad4, 4, K, MASK) == BAD);
  CASE("check/third_ratio_not_reached", skred_bend_check(bad4, 2, K, MASK) == SKRED_OK);

  /* the packing: the bits as they stand */
  { uint32_t out[4] = { 9, 9, 9, 9 };
    sk_bend_pack(r4, 4, NULL, out);
    CASE("pack/identity", !memcmp(out, r4, 16) && out[0] == 0x3f800000u);
    const uint32_t rev[4] = { 3, 2, 1, 0 };
    sk_bend_pack(r4, 4, rev, out);
    CASE("pack/reversed", !memcmp(&out[0], &r4[3], 4) && !memcmp(&out[3], &r4[0], 4) && out[3] == 0x3f800000u);
    out[2] = 7;
    sk_bend_pack(r4, 2, NULL, out);
    CASE("pack/n_words_only", out[2] == 7); }
  CASE("perm/1", perm_case(1));
  CASE("perm/2", perm_case(2));
  CASE("perm/1023", perm_case(1023));
  CASE("perm/1024", perm_case(1024));

  /* the entry points: a bank that is nothing but its size */
  skred_bank_t *b = (skred_bank_t *)calloc(1, sizeof(skred_bank_t));
  b->n_voices = N;
  int32_t list[4] = { 0, 8, 16, 24 };
  uint32_t res[4] = { 7, 7, 7, 7 }, words[16];
  for (int k = 0; k < 16; k++) words[k] = 7;
  CASE("match/null_bank", skred_bank_bend_match(NULL, 0, N, K, MASK, &chan, 1.5f, res, NULL) == BAD);
  CASE("match/null_match", skred_bank_bend_match(b, 0, N, K, MASK, NULL, 1.5f, res, NULL) == BAD);
  CASE("match/null_match_before_k", skred_bank_bend_match(b, 0, N, 3, MASK, NULL, 1.5f, res, NULL) == BAD);
  CASE("match/k12", skred_bank_bend_match(b, 0, N, 12, MASK, &chan, 1.5f, res, NULL) == RANGE);
  CASE("match/k_before_ratio", skred_bank_bend_match(b, 0, N, 12, MASK, &chan, 0.0f, res, NULL) == RANGE);
  CASE("match/mask0", skred_bank_bend_match(b, 0, N, K, 0, &chan, 1.5f, res, NULL) == BAD);
  CASE("match/mask_high", skred_bank_bend_match(b, 0, N, K, 0x1FF, &chan, 1.5f, res, NULL) == BAD);
  CASE("match/ratio_zero", skred_bank_bend_match(b, 0, N, K, MASK, &chan, 0.0f, res, NULL) == BAD);
  CASE("match/ratio_negative", skred_bank_bend_match(b, 0, N, K, MASK, &chan, -1.0f, res, NULL) == BAD);
  CASE("match/ratio_nan", skred_bank_bend_match(b, 0, N, K, MASK, &chan, NAN, res, NULL) == BAD);
  CASE("match/ratio_inf", skred_bank_bend_match(b, 0, N, K, MASK, &chan, INFINITY, res, NULL) == BAD);
  CASE("match/value_outside_mask", skred_bank_bend_match(b, 0, N, K, MASK, &wrong, 1.5f, res, NULL) == BAD);
  CASE("match/ratio_before_range", skred_bank_bend_match(b, 4, 8, K, MASK, &chan, 0.0f, res, NULL) == BAD);
  CASE("match/first_off_slot", skred_bank_bend_match(b, 4, 8, K, MASK, &chan, 1.5f, res, NULL) == RANGE);
  CASE("match/count_off_slot", skred_bank_bend_match(b, 0, 12, K, MASK, &chan, 1.5f, res, NULL) == RANGE);
  CASE("match/past_the_bank", skred_bank_bend_match(b, 0, N + K, K, MASK, &chan, 1.5f, res, NULL) == RANGE);
  CASE("match/empty_range", skred_bank_bend_match(b, 0, 0, K, MASK, &chan, 1.5f, res, NULL) == RANGE);
  CASE("owned/null_bank", skred_bank_bend_owned_each(NULL, r4, K, MASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_list", skred_bank_bend_owned_each(b, r4, K, MASK, NULL, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_tags", skred_bank_bend_owned_each(b, r4, K, MASK, list, NULL, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_ratios", skred_bank_bend_owned_each(b, NULL, K, MASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_before_k", skred_bank_bend_owned_each(b, NULL, 12, MASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/k12", skred_bank_bend_owned_each(b, r4, 12, MASK, list, t4, 4, NULL, res, NULL) == RANGE);
  CASE("owned/k_before_ratio", skred_bank_bend_owned_each(b, bad4, 12, MASK, list, z4, 4, NULL, res, NULL) == RANGE);
  CASE("owned/mask0", skred_bank_bend_owned_each(b, r4, K, 0, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/mask_high", skred_bank_bend_owned_each(b, r4, K, 0x1FF, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/bad_ratio", skred_bank_bend_owned_each(b, bad4, K, MASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/zero_tag", skred_bank_bend_owned_each(b, r4, K, MASK, list, z4, 4, NULL, res, NULL) == BAD);
  CASE("owned/negative_n", skred_bank_bend_owned_each(b, r4, K, MASK, list, t4, -2, NULL, res, NULL) == BAD);
  CASE("owned/empty", skred_bank_bend_owned_each(b, r4, K, MASK, list, t4, 0, NULL, res, NULL) == SKRED_OK);
  CASE("tags/null_bank", skred_bank_bend_tags_each(NULL, r4, 0, N, K, MASK, t4, 4, res, NULL) == BAD);
  CASE("tags/null_tags", skred_bank_bend_tags_each(b, r4, 0, N, K, MASK, NULL, 4, res, NULL) == BAD);
  CASE("tags/null_ratios", skred_bank_bend_tags_each(b, NULL, 0, N, K, MASK, t4, 4, res, NULL) == BAD);
  CASE("tags/k3", skred_bank_bend_tags_each(b, r4, 0, N, 3, 0x7, t4, 4, res, NULL) == RANGE);
  CASE("tags/mask_high", skred_bank_bend_tags_each(b, r4, 0, N, K, 0x1FF, t4, 4, res, NULL) == BAD);
  CASE("tags/bad_ratio", skred_bank_bend_tags_each(b, bad4, 0, N, K, MASK, t4, 4, res, NULL) == BAD);
  CASE("tags/zero_tag", skred_bank_bend_tags_each(b, r4, 0, N, K, MASK, z4, 4, res, NULL) == BAD);
  CASE("tags/repeated_tag", skred_bank_bend_tags_each(b, r4, 0, N, K, MASK, d4, 4, res, NULL) == BAD);
  CASE("tags/too_many", skred_bank_bend_tags_each(b, rmany, 0, N, K, MASK, many, SKRED_OWNER_MAX_TAGS + 1, res, NULL) == BAD);
  CASE("tags/negative_n", skred_bank_bend_tags_each(b, r4, 0, N, K, MASK, t4, -1, res, NULL) == BAD);
  CASE("tags/ratio_before_range", skred_bank_bend_tags_each(b, bad4, 4, 8, K, MASK, t4, 4, res, NULL) == BAD);
  CASE("tags/tag_before_range", skred_bank_bend_tags_each(b, r4, 4, 8, K, MASK, z4, 4, res, NULL) == BAD);
  CASE("tags/first_off_slot", skred_bank_bend_tags_each(b, r4, 4, 8, K, MASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/past_the_bank", skred_bank_bend_tags_each(b, r4, 0, N + K, K, MASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/empty_range", skred_bank_bend_tags_each(b, r4, 0, 0, K, MASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/empty", skred_bank_bend_tags_each(b, r4, 0, N, K, MASK, t4, 0, res, NULL) == SKRED_OK);
  CASE("clear/null_bank", skred_bank_bend_clear(NULL, 0, N, 1, NULL) == BAD);
  CASE("clear/past_the_bank", skred_bank_bend_clear(b, 8, N, 0, NULL) == RANGE);
  CASE("clear/negative_count", skred_bank_bend_clear(b, 0, -1, 0, NULL) == RANGE);
  CASE("clear/no_array_yet", skred_bank_bend_clear(b, 0, N, 1, NULL) == SKRED_OK);
  CASE("download/null_bank", skred_bank_download_bend(NULL, words, 0, 4) == BAD);
  CASE("download/null_out", skred_bank_download_bend(b, NULL, 0, 4) == BAD);
  CASE("download/past_the_bank", skred_bank_download_bend(b, words, N - 2, 4) == RANGE);
  CASE("download/empty", skred_bank_download_bend(b, words, 0, 0) == SKRED_OK && words[0] == 7);
  { int zeros = skred_bank_download_bend(b, words, N - 4, 3) == SKRED_OK;
    for (int k = 0; k < 6; k++) zeros = zeros && !words[k];
    CASE("download/no_array_yet_gives_zeros", zeros && words[6] == 7 && words[15] == 7); }

  CASE("untouched/outputs", res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && list[0] == 0 && list[3] == 24);
  CASE("untouched/bank", b->touched_total == 0 && b->control_epoch == 0 && b->upd_seq == 0 && b->upd_head == 0 && !b->d_owner && !b->d_pedal &&
                         !b->d_glide && !b->d_bend && !b->d_owner_slots);
  free(b);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
