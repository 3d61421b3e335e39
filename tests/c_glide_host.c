/* The host side of the glide calls without a device: skred_glide_check, the 32-byte packing of the entries, the permutation that keeps
 * glide[k] with tags[k] when the tags travel sorted (n = 1, 2, 1023, 1024) and every refusal the entry points make before anything
 * touches the device, on a skred_bank_t that is nothing but its voice count (a refused call reads no other member).  One line per
 * case, "OK" last.  tests/test_glide_cpu.py builds and runs it; built together with skred_amd/csrc/skred_bank_glide.c and
 * -fsanitize=address,undefined it is the sanitizer run of that file's host code -- from the repository root, after the library is
 * built (the program's own copy of skred_bank_glide.c takes the place of the library's; everything else it calls comes from the
 * library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_glide_host.c skred_amd/csrc/skred_bank_glide.c -o /tmp/c_glide_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_glide_host_san */
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
#define FROM SKRED_GLIDE_FROM_SCALE
#define TO SKRED_GLIDE_TO_SCALE

static skred_glide_t entry(uint32_t set, float up, float down, float scale) {
  skred_glide_t g;
  memset(&g, 0, sizeof(g));
  g.set = set; g.rate_up = up; g.rate_down = down; g.scale = scale;
  return g;
}

static int one(skred_glide_t g) { return skred_glide_check(&g, 1, K, MASK); }

/* tags in a scrambled order, entry k marked with k: after the pack, entry j must be the one that stood with the j-th smallest tag */
static int perm_case(int n) {
  static uint32_t tags[SKRED_OWNER_MAX_TAGS], sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  static skred_glide_t in[SKRED_OWNER_MAX_TAGS];
  static sk_glide_each_t out[SKRED_OWNER_MAX_TAGS + 1];
  for (int k = 0; k < n; k++) {
    tags[k] = 0x80000000u ^ (uint32_t)(((uint64_t)k * 2654435761u) % 1000003u + 1u);     /* distinct: k < 1000003 and the map is a bijection mod a prime */
    in[k] = entry(k & 1 ? TO : FROM, 1.0f + (float)(k + 1) / 4096.0f, 1.0f - (float)(k + 1) / 4096.0f, 0.5f + (float)k);
    in[k].reserved[0] = in[k].reserved[3] = 0;
  }
  memset(&out[n], 0xA5, sizeof(out[n]));
  if (sk_owner_pack(tags, n, sorted, perm)) return 0;
  sk_glide_pack(in, n, perm, out);
  for (int j = 0; j < n; j++) {
    if (j && sorted[j] <= sorted[j - 1]) return 0;
    if (tags[perm[j]] != sorted[j]) return 0;
    if (memcmp(out[j].w, &in[perm[j]], 16)) return 0;
    if (out[j].w[4] | out[j].w[5] | out[j].w[6] | out[j].w[7]) return 0;
  }
  for (size_t i = 0; i < sizeof(out[n]); i++)
    if (((const unsigned char *)&out[n])[i] != 0xA5) return 0;                            /* nothing past entry n - 1 */
  return 1;
}

int main(void) {
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0xFFFFFFFFu, 0x80000000u }, z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u };
  const uint32_t d4[4] = { 0x03000001u, 0x03000002u, 0x03000001u, 0x03000004u };
  static uint32_t many[SKRED_OWNER_MAX_TAGS + 1];
  static skred_glide_t gmany[SKRED_OWNER_MAX_TAGS + 1];
  for (int k = 0; k <= SKRED_OWNER_MAX_TAGS; k++) { many[k] = 1u + (uint32_t)k; gmany[k] = entry(FROM, 1.01f, 0.99f, 0.5f); }
  skred_glide_t g4[4] = { entry(FROM, 1.01f, 0.99f, 0.5f), entry(TO, 1.5f, 0.25f, 2.0f), entry(FROM, 1.0001f, 0.9999f, 1.0f),
                          entry(TO, 2.0f, 0.5f, 1e-3f) };

  CASE("const/bits", FROM == 1 && TO == 2);
  CASE("const/size", sizeof(skred_glide_t) == 32 && sizeof(sk_glide_each_t) == 32 && sizeof(sk_glide_t) == 16);

  /* skred_glide_check */
  CASE("check/plain", skred_glide_check(g4, 4, K, MASK) == SKRED_OK);
  CASE("check/empty", skred_glide_check(g4, 0, K, MASK) == SKRED_OK);
  CASE("check/null", skred_glide_check(NULL, 4, K, MASK) == BAD);
  CASE("check/null_empty", skred_glide_check(NULL, 0, K, MASK) == BAD);
  CASE("check/negative_n", skred_glide_check(g4, -1, K, MASK) == BAD);
  CASE("check/k3", skred_glide_check(g4, 4, 3, 1) == RANGE);
  CASE("check/k0", skred_glide_check(g4, 4, 0, 1) == RANGE);
  CASE("check/k128", skred_glide_check(g4, 4, 128, 1) == RANGE);
  CASE("check/k_before_mask", skred_glide_check(g4, 4, 3, 0) == RANGE);
  CASE("check/mask0", skred_glide_check(g4, 4, K, 0) == BAD);
  CASE("check/mask_high", skred_glide_check(g4, 4, K, 0x100) == BAD);
  CASE("check/k64_full_mask", skred_glide_check(g4, 4, 64, ~0ull) == SKRED_OK);
  CASE("check/k1", skred_glide_check(g4, 4, 1, 1) == SKRED_OK);
  CASE("check/set0", one(entry(0, 1.01f, 0.99f, 0.5f)) == BAD);
  CASE("check/set_both", one(entry(FROM | TO, 1.01f, 0.99f, 0.5f)) == BAD);
  CASE("check/set_unknown", one(entry(4, 1.01f, 0.99f, 0.5f)) == BAD);
  CASE("check/set_unknown_beside", one(entry(FROM | 0x80000000u, 1.01f, 0.99f, 0.5f)) == BAD);
  for (int r = 0; r < 4; r++) {
    skred_glide_t g = g4[0];
    g.reserved[r] = 1;
    char name[32];
    snprintf(name, sizeof(name), "check/reserved%d", r);
    CASE(name, one(g) == BAD);
  }
  CASE("check/up_nan", one(entry(FROM, NAN, 0.99f, 0.5f)) == BAD);
  CASE("check/up_inf", one(entry(FROM, INFINITY, 0.99f, 0.5f)) == BAD);
  CASE("check/down_nan", one(entry(FROM, 1.01f, NAN, 0.5f)) == BAD);
  CASE("check/scale_inf", one(entry(TO, 1.01f, 0.99f, INFINITY)) == BAD);
  CASE("check/scale_nan", one(entry(TO, 1.01f, 0.99f, NAN)) == BAD);
  CASE("check/up_one", one(entry(FROM, 1.0f, 0.99f, 0.5f)) == BAD);
  CASE("check/up_below_one", one(entry(FROM, 0.5f, 0.99f, 0.5f)) == BAD);
  CASE("check/up_just_above_one", one(entry(FROM, 1.0f + 0x1p-23f, 0.99f, 0.5f)) == SKRED_OK);
  CASE("check/down_one", one(entry(FROM, 1.01f, 1.0f, 0.5f)) == BAD);
  CASE("check/down_above_one", one(entry(FROM, 1.01f, 1.5f, 0.5f)) == BAD);
  CASE("check/down_zero", one(entry(FROM, 1.01f, 0.0f, 0.5f)) == BAD);
  CASE("check/down_negative", one(entry(FROM, 1.01f, -0.5f, 0.5f)) == BAD);
  CASE("check/down_just_below_one", one(entry(FROM, 1.01f, 1.0f - 0x1p-24f, 0.5f)) == SKRED_OK);
  CASE("check/scale_zero", one(entry(TO, 1.01f, 0.99f, 0.0f)) == BAD);
  CASE("check/scale_negative", one(entry(TO, 1.01f, 0.99f, -2.0f)) == BAD);
  CASE("check/scale_one", one(entry(TO, 1.01f, 0.99f, 1.0f)) == SKRED_OK);
  { skred_glide_t two[2] = { g4[0], entry(0, 1.01f, 0.99f, 0.5f) };
    CASE("check/second_entry", skred_glide_check(two, 2, K, MASK) == BAD);
    CASE("check/second_entry_not_reached", skred_glide_check(two, 1, K, MASK) == SKRED_OK); }

  /* the packing: four words as they stand, the reserved words zero whatever the caller's struct holds beyond a checked entry */
  { sk_glide_each_t out[4];
    memset(out, 0xFF, sizeof(out));
    sk_glide_pack(g4, 4, NULL, out);
    int same = 1;
    for (int k = 0; k < 4; k++) same = same && !memcmp(out[k].w, &g4[k], 16) && !(out[k].w[4] | out[k].w[5] | out[k].w[6] | out[k].w[7]);
    CASE("pack/identity", same);
    float f;
    memcpy(&f, &out[1].w[SK_GLIDE_E_SCALE], 4);
    CASE("pack/words", out[1].w[SK_GLIDE_E_SET] == TO && f == 2.0f);
    const uint32_t rev[4] = { 3, 2, 1, 0 };
    sk_glide_pack(g4, 4, rev, out);
    CASE("pack/reversed", !memcmp(out[0].w, &g4[3], 16) && !memcmp(out[3].w, &g4[0], 16)); }
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
  skred_glide_t bad4[4] = { g4[0], g4[1], entry(FROM, 1.0f, 0.99f, 0.5f), g4[3] };
  CASE("owned/null_bank", skred_bank_glide_owned(NULL, g4, K, MASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_list", skred_bank_glide_owned(b, g4, K, MASK, NULL, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_tags", skred_bank_glide_owned(b, g4, K, MASK, list, NULL, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_entries", skred_bank_glide_owned(b, NULL, K, MASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/zero_tag", skred_bank_glide_owned(b, g4, K, MASK, list, z4, 4, NULL, res, NULL) == BAD);
  CASE("owned/negative_n", skred_bank_glide_owned(b, g4, K, MASK, list, t4, -2, NULL, res, NULL) == BAD);
  CASE("owned/bad_entry", skred_bank_glide_owned(b, bad4, K, MASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/k12", skred_bank_glide_owned(b, g4, 12, MASK, list, t4, 4, NULL, res, NULL) == RANGE);
  CASE("owned/mask0", skred_bank_glide_owned(b, g4, K, 0, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/mask_high", skred_bank_glide_owned(b, g4, K, 0x1FF, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/empty", skred_bank_glide_owned(b, g4, K, MASK, list, t4, 0, NULL, res, NULL) == SKRED_OK);
  CASE("tags/null_bank", skred_bank_glide_tags(NULL, g4, 0, N, K, MASK, t4, 4, res, NULL) == BAD);
  CASE("tags/null_tags", skred_bank_glide_tags(b, g4, 0, N, K, MASK, NULL, 4, res, NULL) == BAD);
  CASE("tags/null_entries", skred_bank_glide_tags(b, NULL, 0, N, K, MASK, t4, 4, res, NULL) == BAD);
  CASE("tags/repeated_tag", skred_bank_glide_tags(b, g4, 0, N, K, MASK, d4, 4, res, NULL) == BAD);
  CASE("tags/zero_tag", skred_bank_glide_tags(b, g4, 0, N, K, MASK, z4, 4, res, NULL) == BAD);
  CASE("tags/too_many", skred_bank_glide_tags(b, gmany, 0, N, K, MASK, many, SKRED_OWNER_MAX_TAGS + 1, res, NULL) == BAD);
  CASE("tags/bad_entry", skred_bank_glide_tags(b, bad4, 0, N, K, MASK, t4, 4, res, NULL) == BAD);
  CASE("tags/first_off_slot", skred_bank_glide_tags(b, g4, 4, 8, K, MASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/past_the_bank", skred_bank_glide_tags(b, g4, 0, N + K, K, MASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/empty_range", skred_bank_glide_tags(b, g4, 0, 0, K, MASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/k3", skred_bank_glide_tags(b, g4, 0, N, 3, 0x7, t4, 4, res, NULL) == RANGE);
  CASE("tags/mask_high", skred_bank_glide_tags(b, g4, 0, N, K, 0x1FF, t4, 4, res, NULL) == BAD);
  CASE("tags/entries_before_range", skred_bank_glide_tags(b, bad4, 4, 8, K, MASK, t4, 4, res, NULL) == BAD);
  CASE("tags/empty", skred_bank_glide_tags(b, g4, 0, N, K, MASK, t4, 0, res, NULL) == SKRED_OK);
  CASE("advance/null_bank", skred_bank_glide_advance(NULL, 0, N, 64, res, NULL) == BAD);
  CASE("advance/zero_frames", skred_bank_glide_advance(b, 0, N, 0, res, NULL) == BAD);
  CASE("advance/negative_frames", skred_bank_glide_advance(b, 0, N, -64, res, NULL) == BAD);
  CASE("advance/too_many_frames", skred_bank_glide_advance(b, 0, N, 65537, res, NULL) == BAD);
  CASE("advance/frames_before_range", skred_bank_glide_advance(b, 0, N + 1, 0, res, NULL) == BAD);
  CASE("advance/empty_range", skred_bank_glide_advance(b, 0, 0, 64, res, NULL) == RANGE);
  CASE("advance/past_the_bank", skred_bank_glide_advance(b, 37, N, 64, res, NULL) == RANGE);
  CASE("advance/negative_first", skred_bank_glide_advance(b, -1, 8, 64, res, NULL) == RANGE);
  CASE("advance/no_array_no_result", skred_bank_glide_advance(b, 37, 500, 65536, NULL, NULL) == SKRED_OK);
  CASE("stop/null_bank", skred_bank_glide_stop(NULL, 0, N, 1, NULL) == BAD);
  CASE("stop/past_the_bank", skred_bank_glide_stop(b, 8, N, 0, NULL) == RANGE);
  CASE("stop/negative_count", skred_bank_glide_stop(b, 0, -1, 0, NULL) == RANGE);
  CASE("stop/no_array_yet", skred_bank_glide_stop(b, 0, N, 1, NULL) == SKRED_OK);
  CASE("download/null_bank", skred_bank_download_glide(NULL, words, 0, 4) == BAD);
  CASE("download/null_out", skred_bank_download_glide(b, NULL, 0, 4) == BAD);
  CASE("download/past_the_bank", skred_bank_download_glide(b, words, N - 2, 4) == RANGE);
  CASE("download/empty", skred_bank_download_glide(b, words, 0, 0) == SKRED_OK && words[0] == 7);
  { int zeros = skred_bank_download_glide(b, words, N - 4, 3) == SKRED_OK;
    for (int k = 0; k < 12; k++) zeros = zeros && !words[k];
    CASE("download/no_array_yet_gives_zeros", zeros && words[12] == 7 && words[15] == 7); }

  CASE("untouched/outputs", res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && list[0] == 0 && list[3] == 24);
  CASE("untouched/bank", b->touched_total == 0 && b->control_epoch == 0 && b->upd_seq == 0 && b->upd_head == 0 && !b->d_owner && !b->d_pedal &&
                         !b->d_glide && !b->d_owner_slots);
  free(b);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
