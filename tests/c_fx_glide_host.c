/* The host side of the fixed-point glide calls without a device: skred_fx_glide_check entry by entry, every refusal the entry points
 * make before anything touches the device, with its return code -- on a skred_fxbank_t that is nothing but its voice count (a refused
 * call reads no other member) --, the 32-byte packing of the entries, and what travels behind skred_fxbank_glide_tags: the tags sorted
 * (sk_owner_pack) and the entries permuted with them (skx_glide_pack), at n = 1, 2, 1023, 1024.  One line per case, "OK" last.
 * tests/test_fx_glide_cpu.py builds and runs it; built together with skred_amd/csrc/skred_fx_glide.c and
 * -fsanitize=address,undefined it is the sanitizer run of that file's host code -- from the repository root, after the library is
 * built (the program's own copy of skred_fx_glide.c takes the place of the library's; everything else it calls comes from the
 * library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_fx_glide_host.c skred_amd/csrc/skred_fx_glide.c -o /tmp/c_fx_glide_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_fx_glide_host_san
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
#define FROM SKRED_FX_GLIDE_FROM_SCALE
#define TOS SKRED_FX_GLIDE_TO_SCALE
#define TOI SKRED_FX_GLIDE_TO_INC

static skred_fx_glide_t entry(uint32_t set, uint32_t up, uint32_t down, uint32_t scale, uint32_t target) {
  skred_fx_glide_t g;
  memset(&g, 0, sizeof(g));
  g.set = set; g.up_q32 = up; g.down_q32 = down; g.scale_q16 = scale; g.target_inc = target;
  return g;
}

/* the sort-plus-permutation behind glide_tags at n tags given in descending order with a twist: entry k carries target_inc = 1000 + k */
static int permuted(int n) {
  uint32_t *tags = (uint32_t *)calloc((size_t)n, sizeof(uint32_t)), *sorted = (uint32_t *)calloc((size_t)n, sizeof(uint32_t));
  uint32_t *perm = (uint32_t *)calloc((size_t)n, sizeof(uint32_t));
  skred_fx_glide_t *g = (skred_fx_glide_t *)calloc((size_t)n, sizeof(skred_fx_glide_t));
  skx_glide_each_t *out = (skx_glide_each_t *)calloc((size_t)n, sizeof(skx_glide_each_t));
  for (int k = 0; k < n; k++) {
    tags[k] = (k & 1 ? 0x80000000u : 0u) + 5u * (uint32_t)(n - k);        /* every other one at or above 2^31: unsigned order */
    g[k] = entry(TOI, 7u + (uint32_t)k, 9u + (uint32_t)k, 0xDEADu, 1000u + (uint32_t)k);   /* (scale: not TO_INC's, travels all the same) */
  }
  memset(out, 0xEE, (size_t)n * sizeof(skx_glide_each_t));
  int ok = sk_owner_pack(tags, n, sorted, perm) == SKRED_OK;
  skx_glide_pack(g, n, perm, out);
  for (int j = 0; j < n && ok; j++) {
    const uint32_t k = perm[j];
    ok = k < (uint32_t)n && sorted[j] == tags[k] && (j == 0 || sorted[j - 1] < sorted[j]) && out[j].w[SKX_GLIDE_E_SET] == TOI &&
         out[j].w[SKX_GLIDE_E_UP] == 7u + k && out[j].w[SKX_GLIDE_E_DOWN] == 9u + k && out[j].w[SKX_GLIDE_E_SCALE] == 0xDEADu &&
         out[j].w[SKX_GLIDE_E_TARGET_INC] == 1000u + k && !out[j].w[5] && !out[j].w[6] && !out[j].w[7];
  }
  free(tags); free(sorted); free(perm); free(g); free(out);
  return ok;
}

int main(void) {
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0xFFFFFFFFu, 0x80000000u }, z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u };
  const uint32_t d4[4] = { 0x03000001u, 0x03000002u, 0x03000001u, 0x03000004u };
  static uint32_t many[SKRED_OWNER_MAX_TAGS + 1];
  static skred_fx_glide_t gmany[SKRED_OWNER_MAX_TAGS + 1];
  for (int k = 0; k <= SKRED_OWNER_MAX_TAGS; k++) { many[k] = 1u + (uint32_t)k; gmany[k] = entry(FROM, 1, 1, 65536, 0); }
  skred_fx_glide_t g4[4] = { entry(FROM, 1, 0xFFFFFFFFu, 1, 0), entry(TOS, 0xFFFFFFFFu, 1, 0xFFFFFFFFu, 0), entry(TOI, 5, 6, 0, 1),
                             entry(TOI, 5, 6, 0, 0xFFFFFFFFu) };
  skred_fx_glide_t b4[4];

  CASE("const/bits", FROM == 1 && TOS == 2 && TOI == 4);
  CASE("const/sizes", sizeof(skred_fx_glide_t) == 32 && sizeof(skx_glide_each_t) == 32 && sizeof(skx_glide_t) == 16);

  /* skred_fx_glide_check */
  CASE("check/plain", skred_fx_glide_check(g4, 4) == SKRED_OK);
  CASE("check/empty", skred_fx_glide_check(g4, 0) == SKRED_OK);
  CASE("check/null", skred_fx_glide_check(NULL, 0) == BAD);
  CASE("check/negative_n", skred_fx_glide_check(g4, -1) == BAD);
  for (uint32_t set = 0; set < 9; set++) {
    char name[32];
    snprintf(name, sizeof(name), "check/set_0x%x", set);
    memcpy(b4, g4, sizeof(g4));
    b4[3] = entry(set, 5, 6, 65536, 77);
    CASE(name, skred_fx_glide_check(b4, 4) == (set == 1 || set == 2 || set == 4 ? SKRED_OK : BAD));
  }
  memcpy(b4, g4, sizeof(g4)); b4[1].set = TOS | 0x80000000u;
  CASE("check/set_high_bit", skred_fx_glide_check(b4, 4) == BAD);
  CASE("check/bad_entry_not_reached", skred_fx_glide_check(b4, 1) == SKRED_OK);
  for (int r = 0; r < 3; r++) {
    char name[32];
    snprintf(name, sizeof(name), "check/reserved_%d", r);
    memcpy(b4, g4, sizeof(g4)); b4[2].reserved[r] = 1;
    CASE(name, skred_fx_glide_check(b4, 4) == BAD);
  }
  memcpy(b4, g4, sizeof(g4)); b4[0].up_q32 = 0;
  CASE("check/up_zero", skred_fx_glide_check(b4, 4) == BAD);
  memcpy(b4, g4, sizeof(g4)); b4[2].down_q32 = 0;
  CASE("check/down_zero", skred_fx_glide_check(b4, 4) == BAD);
  memcpy(b4, g4, sizeof(g4)); b4[0].scale_q16 = 0;
  CASE("check/from_scale_zero", skred_fx_glide_check(b4, 4) == BAD);
  memcpy(b4, g4, sizeof(g4)); b4[1].scale_q16 = 0;
  CASE("check/to_scale_zero", skred_fx_glide_check(b4, 4) == BAD);
  memcpy(b4, g4, sizeof(g4)); b4[2].target_inc = 0;
  CASE("check/to_inc_zero", skred_fx_glide_check(b4, 4) == BAD);
  memcpy(b4, g4, sizeof(g4)); b4[0].target_inc = 0; b4[2].scale_q16 = 0;
  CASE("check/unused_values_not_looked_at", skred_fx_glide_check(b4, 4) == SKRED_OK);

  /* the packing: five words as they stand, three zero words, in order or permuted */
  {
    skx_glide_each_t out[4];
    memset(out, 0xEE, sizeof(out));
    skx_glide_pack(g4, 4, NULL, out);
    int ok = 1;
    for (int k = 0; k < 4; k++)
      ok = ok && !memcmp(out[k].w, &g4[k], 20) && !out[k].w[5] && !out[k].w[6] && !out[k].w[7];
    CASE("pack/in_order", ok && out[0].w[SKX_GLIDE_E_DOWN] == 0xFFFFFFFFu && out[3].w[SKX_GLIDE_E_TARGET_INC] == 0xFFFFFFFFu);
    const uint32_t perm[4] = { 3, 1, 0, 2 };
    skx_glide_pack(g4, 4, perm, out);
    ok = 1;
    for (int j = 0; j < 4; j++) ok = ok && !memcmp(out[j].w, &g4[perm[j]], 20);
    CASE("pack/permuted", ok);
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
  memcpy(b4, g4, sizeof(g4)); b4[3].set = 3;
  CASE("owned/null_bank", skred_fxbank_glide_owned(NULL, g4, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_list", skred_fxbank_glide_owned(fx, g4, NULL, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_tags", skred_fxbank_glide_owned(fx, g4, list, NULL, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_entries", skred_fxbank_glide_owned(fx, NULL, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/zero_tag", skred_fxbank_glide_owned(fx, g4, list, z4, 4, NULL, res, NULL) == BAD);
  CASE("owned/negative_n", skred_fxbank_glide_owned(fx, g4, list, t4, -2, NULL, res, NULL) == BAD);
  CASE("owned/bad_entry", skred_fxbank_glide_owned(fx, b4, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/repeated_tag_is_fine_but_the_entry_is_not", skred_fxbank_glide_owned(fx, b4, list, d4, 4, NULL, res, NULL) == BAD);
  CASE("owned/empty", skred_fxbank_glide_owned(fx, g4, list, t4, 0, NULL, res, NULL) == SKRED_OK);
  CASE("owned/empty_null_result", skred_fxbank_glide_owned(fx, g4, list, t4, 0, NULL, NULL, NULL) == SKRED_OK);
  CASE("tags/null_bank", skred_fxbank_glide_tags(NULL, g4, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/null_tags", skred_fxbank_glide_tags(fx, g4, 0, N, NULL, 4, res, NULL) == BAD);
  CASE("tags/null_entries", skred_fxbank_glide_tags(fx, NULL, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/repeated_tag", skred_fxbank_glide_tags(fx, g4, 0, N, d4, 4, res, NULL) == BAD);
  CASE("tags/zero_tag", skred_fxbank_glide_tags(fx, g4, 0, N, z4, 4, res, NULL) == BAD);
  CASE("tags/too_many", skred_fxbank_glide_tags(fx, gmany, 0, N, many, SKRED_OWNER_MAX_TAGS + 1, res, NULL) == BAD);
  CASE("tags/bad_entry", skred_fxbank_glide_tags(fx, b4, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/entries_before_range", skred_fxbank_glide_tags(fx, b4, 0, N + 1, t4, 4, res, NULL) == BAD);
  CASE("tags/past_the_bank", skred_fxbank_glide_tags(fx, g4, 0, N + 1, t4, 4, res, NULL) == RANGE);
  CASE("tags/empty_range", skred_fxbank_glide_tags(fx, g4, 0, 0, t4, 4, res, NULL) == RANGE);
  CASE("tags/negative_first", skred_fxbank_glide_tags(fx, g4, -1, 4, t4, 4, res, NULL) == RANGE);
  CASE("tags/range_before_empty_list", skred_fxbank_glide_tags(fx, g4, 0, N + 1, t4, 0, res, NULL) == RANGE);
  CASE("tags/empty", skred_fxbank_glide_tags(fx, g4, 0, N, t4, 0, res, NULL) == SKRED_OK);
  CASE("advance/null_bank", skred_fxbank_glide_advance(NULL, 0, N, 64, res, NULL) == BAD);
  CASE("advance/zero_frames", skred_fxbank_glide_advance(fx, 0, N, 0, res, NULL) == BAD);
  CASE("advance/negative_frames", skred_fxbank_glide_advance(fx, 0, N, -64, res, NULL) == BAD);
  CASE("advance/too_many_frames", skred_fxbank_glide_advance(fx, 0, N, 65537, res, NULL) == BAD);
  CASE("advance/frames_before_range", skred_fxbank_glide_advance(fx, 0, N + 1, 0, res, NULL) == BAD);
  CASE("advance/empty_range", skred_fxbank_glide_advance(fx, 0, 0, 64, res, NULL) == RANGE);
  CASE("advance/past_the_bank", skred_fxbank_glide_advance(fx, 1, N, 64, res, NULL) == RANGE);
  CASE("advance/negative_first", skred_fxbank_glide_advance(fx, -1, 4, 64, res, NULL) == RANGE);
  CASE("advance/no_array_no_result", skred_fxbank_glide_advance(fx, 0, N, 65536, NULL, NULL) == SKRED_OK);
  CASE("stop/null_bank", skred_fxbank_glide_stop(NULL, 0, N, 0, NULL) == BAD);
  CASE("stop/past_the_bank", skred_fxbank_glide_stop(fx, 8, N, 1, NULL) == RANGE);
  CASE("stop/negative_count", skred_fxbank_glide_stop(fx, 0, -1, 0, NULL) == RANGE);
  CASE("stop/no_array_yet", skred_fxbank_glide_stop(fx, 0, N, 1, NULL) == SKRED_OK);
  CASE("stop/empty", skred_fxbank_glide_stop(fx, N, 0, 1, NULL) == SKRED_OK);
  CASE("download/null_bank", skred_fxbank_download_glide(NULL, words, 0, 4) == BAD);
  CASE("download/null_out", skred_fxbank_download_glide(fx, NULL, 0, 4) == BAD);
  CASE("download/negative_count", skred_fxbank_download_glide(fx, words, 0, -1) == BAD);
  CASE("download/past_the_bank", skred_fxbank_download_glide(fx, words, N - 2, 4) == RANGE);
  CASE("download/empty", skred_fxbank_download_glide(fx, words, 0, 0) == SKRED_OK && words[0] == 7);
  int zeros = skred_fxbank_download_glide(fx, words, N - 3, 3) == SKRED_OK;
  for (int k = 0; k < 12; k++) zeros = zeros && words[k] == 0;
  CASE("download/no_array_yet_gives_zeros", zeros && words[12] == 7 && words[15] == 7);

  CASE("untouched/outputs", res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && list[0] == 0 && list[3] == 24);
  CASE("untouched/bank", fx->ring_head == 0 && !fx->d_owner && !fx->d_pedal && !fx->d_glide && !fx->d_owner_found && fx->count == 0 &&
                         !fx->ring[0].in_flight);
  free(fx);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
