/* The host side of the fixed-point filter-envelope calls without a device: skred_fx_fenv_check refusal by refusal in the documented
 * order, every refusal the entry points make before anything touches the device, with its return code and in the documented order --
 * on a skred_fxbank_t that is nothing but its voice count (a refused call reads no other member) and on a NULL bank --, the download
 * of a bank without the array, and what travels behind skred_fxbank_fenv_tags_each: the tags sorted (sk_owner_pack) and the records
 * permuted with them (skx_fenv_pack), at n = 1, 2, 1023, 1024.  One line per case, "OK" last.
 * tests/test_fx_fenv_cpu.py builds and runs it; built together with skred_amd/csrc/skred_fx_fenv.c and -fsanitize=address,undefined
 * it is the sanitizer run of that file's host code -- from the repository root, after the library is built (the program's own copy
 * of skred_fx_fenv.c takes the place of the library's; everything else it calls comes from the library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_fx_fenv_host.c skred_amd/csrc/skred_fx_fenv.c -o /tmp/c_fx_fenv_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_fx_fenv_host_san
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
#define ABS SKRED_FX_FENV_ABS
#define REL SKRED_FX_FENV_REL
#define START SKRED_FX_FENV_START
#define WMIN SKRED_FX_CUTOFF_W_MIN
#define WMAX SKRED_FX_CUTOFF_W_MAX

static int check1(skred_fx_fenv_t r) { return skred_fx_fenv_check(&r, 1); }

/* the sort-plus-permutation behind fenv_tags_each at n tags given in descending order with a twist: record k carries peak 1000 + k */
static int permuted(int n) {
  uint32_t *tags = (uint32_t *)calloc((size_t)n, sizeof(uint32_t)), *sorted = (uint32_t *)calloc((size_t)n, sizeof(uint32_t));
  uint32_t *perm = (uint32_t *)calloc((size_t)n, sizeof(uint32_t));
  skred_fx_fenv_t *r = (skred_fx_fenv_t *)calloc((size_t)n, sizeof(skred_fx_fenv_t));
  skx_fenv_each_t *out = (skx_fenv_each_t *)calloc((size_t)n + 1, sizeof(skx_fenv_each_t));
  for (int k = 0; k < n; k++) {
    tags[k] = (k & 1 ? 0x80000000u : 0u) + 5u * (uint32_t)(n - k);        /* every other one at or above 2^31: unsigned order */
    r[k].set = REL | (k & 1 ? START : 0u);
    r[k].start = k & 1 ? 7u + (uint32_t)k : 0u;
    r[k].peak = 1000u + (uint32_t)k; r[k].sustain = 2000u + (uint32_t)k; r[k].end = 3000u + (uint32_t)k;
    r[k].rate_attack_q32 = 11u + (uint32_t)k; r[k].rate_decay_q32 = 13u + (uint32_t)k; r[k].rate_release_q32 = 17u + (uint32_t)k;
  }
  memset(out, 0xEE, ((size_t)n + 1) * sizeof(skx_fenv_each_t));
  int ok = sk_owner_pack(tags, n, sorted, perm) == SKRED_OK;
  skx_fenv_pack(r, n, perm, out);
  for (int j = 0; j < n && ok; j++) {
    const uint32_t k = perm[j], *w = out[j].w;
    ok = k < (uint32_t)n && sorted[j] == tags[k] && (j == 0 || sorted[j - 1] < sorted[j]) && w[SKX_FENV_E_SET] == r[k].set &&
         w[SKX_FENV_E_START] == r[k].start && w[SKX_FENV_E_PEAK] == 1000u + k && w[SKX_FENV_E_SUSTAIN] == 2000u + k &&
         w[SKX_FENV_E_END] == 3000u + k && w[SKX_FENV_E_RATE_ATTACK] == 11u + k && w[SKX_FENV_E_RATE_DECAY] == 13u + k &&
         w[SKX_FENV_E_RATE_RELEASE] == 17u + k;
  }
  ok = ok && out[n].w[0] == 0xEEEEEEEEu;                                  /* n records and not one more */
  free(tags); free(sorted); free(perm); free(r); free(out);
  return ok;
}

int main(void) {
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0xFFFFFFFFu, 0x80000000u }, z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u };
  const uint32_t d4[4] = { 0x03000001u, 0x03000002u, 0x03000001u, 0x03000004u };
  static uint32_t many[SKRED_OWNER_MAX_TAGS + 1];
  static skred_fx_fenv_t rmany[SKRED_OWNER_MAX_TAGS + 1];
  const skred_fx_fenv_t good = { ABS, 0, 1u << 27, 1u << 25, 1u << 22, 1u << 28, 1u << 26, 1u << 27 };
  const skred_fx_fenv_t rel = { REL | START, 1u << 15, 8u << 16, 2u << 16, 1u << 14, 1u << 28, 1u << 26, 1u << 27 };
  for (int k = 0; k <= SKRED_OWNER_MAX_TAGS; k++) { many[k] = 1u + (uint32_t)k; rmany[k] = good; }
  skred_fx_fenv_t r4[4] = { good, rel, good, rel }, b4[4] = { good, good, good, good };
  b4[3].set = ABS | REL;                                                  /* the last record is bad */
  const skred_owner_match_t chan = { 0x03000000u, 0xFF000000u }, everyone = { 0u, 0u }, never = { 0x03000001u, 0xFF000000u };

  CASE("const/sizes", sizeof(skx_fenv_t) == 32 && sizeof(skx_fenv_each_t) == 32 && sizeof(skred_fx_fenv_t) == 32 && SKX_FENV_RATE_ATTACK == 4);
  CASE("const/bits", ABS == 1 && REL == 2 && START == 4 && SKX_FENV_ALL == 7 && SKX_FENV_RELEASE == 4);

  /* skred_fx_fenv_check, in the header's order */
  {
    skred_fx_fenv_t r = good;
    CASE("check/plain", skred_fx_fenv_check(r4, 4) == SKRED_OK);
    CASE("check/empty", skred_fx_fenv_check(r4, 0) == SKRED_OK);
    CASE("check/null", skred_fx_fenv_check(NULL, 0) == BAD);
    CASE("check/null_before_n", skred_fx_fenv_check(NULL, -1) == BAD);
    CASE("check/negative_n", skred_fx_fenv_check(r4, -1) == BAD);
    CASE("check/bad_record_not_reached", skred_fx_fenv_check(b4, 3) == SKRED_OK && skred_fx_fenv_check(b4, 4) == BAD);
    r = good; r.set |= 8u; CASE("check/unknown_bits", check1(r) == BAD);
    r = good; r.set |= REL; CASE("check/abs_and_rel", check1(r) == BAD);
    r = good; r.set = START; r.start = 1u << 20; CASE("check/neither", check1(r) == BAD);
    r = good; r.start = 1u << 20; CASE("check/start_without_START", check1(r) == BAD);
    r = good; r.set |= START; r.start = 1u << 20; CASE("check/start_with_START", check1(r) == SKRED_OK);
    r = good; r.set |= START; r.start = WMIN - 1u; CASE("check/abs_start_below", check1(r) == RANGE);
    r = good; r.set |= START; r.start = 0; CASE("check/abs_start_zero_under_START", check1(r) == RANGE);
    r = good; r.peak = WMAX + 1u; CASE("check/abs_peak_above", check1(r) == RANGE);
    r = good; r.sustain = WMIN - 1u; CASE("check/abs_sustain_below", check1(r) == RANGE);
    r = good; r.end = WMAX + 1u; CASE("check/abs_end_above", check1(r) == RANGE);
    r = good; r.peak = WMAX; r.sustain = WMIN; r.end = WMIN; CASE("check/abs_edges", check1(r) == SKRED_OK);
    r = rel; r.peak = 0; CASE("check/rel_peak_zero", check1(r) == RANGE);
    r = rel; r.sustain = 0; CASE("check/rel_sustain_zero", check1(r) == RANGE);
    r = rel; r.end = 0; CASE("check/rel_end_zero", check1(r) == RANGE);
    r = rel; r.start = 0; CASE("check/rel_start_zero_under_START", check1(r) == RANGE);
    r = rel; r.set = REL; r.start = 0; CASE("check/rel_start_zero_without_START_is_not_looked_at", check1(r) == SKRED_OK);
    r = rel; r.peak = 0xFFFFFFFFu; r.end = 1u; CASE("check/rel_any_other_value", check1(r) == SKRED_OK);
    r = good; r.rate_attack_q32 = 0; CASE("check/zero_attack_rate", check1(r) == BAD);
    r = good; r.rate_decay_q32 = 0; CASE("check/zero_decay_rate", check1(r) == BAD);
    r = good; r.rate_release_q32 = 0; CASE("check/zero_release_rate", check1(r) == BAD);
    r = good; r.rate_attack_q32 = 0xFFFFFFFFu; r.rate_decay_q32 = 1u; CASE("check/any_other_rate", check1(r) == SKRED_OK);
    r = good; r.peak = 0; r.set |= 8u; CASE("check/bits_before_levels", check1(r) == BAD);
    r = good; r.peak = 0; r.set |= REL; CASE("check/abs_and_rel_before_levels", check1(r) == BAD);
    r = good; r.peak = 0; r.start = 5; CASE("check/start_before_levels", check1(r) == BAD && strstr(skred_amd_last_error(), "start") != NULL);
    r = good; r.peak = 0; r.rate_attack_q32 = 0; CASE("check/levels_before_rates", check1(r) == RANGE);
    r = rel; r.peak = 0; r.rate_attack_q32 = 0; CASE("check/rel_levels_before_rates", check1(r) == RANGE);
  }

  /* the packing: word for word, in order or permuted */
  {
    skx_fenv_each_t out[3];
    skred_fx_fenv_t two[2] = { { ABS | START, 1, 2, 3, 4, 5, 6, 7 }, { REL, 0, 22, 33, 44, 55, 66, 77 } };
    memset(out, 0xEE, sizeof(out));
    skx_fenv_pack(two, 2, NULL, out);
    CASE("pack/in_order", out[0].w[0] == (ABS | START) && out[0].w[1] == 1 && out[0].w[4] == 4 && out[0].w[7] == 7 && out[1].w[0] == REL &&
                          out[1].w[1] == 0 && out[1].w[7] == 77 && out[2].w[0] == 0xEEEEEEEEu);
    const uint32_t perm[2] = { 1, 0 };
    skx_fenv_pack(two, 2, perm, out);
    CASE("pack/permuted", out[0].w[2] == 22 && out[1].w[2] == 2 && out[2].w[0] == 0xEEEEEEEEu);
    CASE("pack/sort_and_permute_1", permuted(1));
    CASE("pack/sort_and_permute_2", permuted(2));
    CASE("pack/sort_and_permute_1023", permuted(1023));
    CASE("pack/sort_and_permute_1024", permuted(1024));
  }

  /* the entry points: a bank that is nothing but its size */
  skred_fxbank_t *fx = (skred_fxbank_t *)calloc(1, sizeof(skred_fxbank_t));
  fx->n_voices = N;
  int32_t list[4] = { 0, 8, 16, 24 };
  uint32_t res[4] = { 7, 7, 7, 7 }, words[32];
  for (int k = 0; k < 32; k++) words[k] = 7;
  /* the channel sweep: NULL bank, match or record, the record, the match, the range -- skred_fxbank_cutoff_match's order */
  CASE("match/null_bank", skred_fxbank_fenv_match(NULL, 0, N, &chan, &good, res, NULL) == BAD);
  CASE("match/null_match", skred_fxbank_fenv_match(fx, 0, N, NULL, &good, res, NULL) == BAD);
  CASE("match/null_record", skred_fxbank_fenv_match(fx, 0, N, &chan, NULL, res, NULL) == BAD);
  CASE("match/bad_record", skred_fxbank_fenv_match(fx, 0, N, &chan, &b4[3], res, NULL) == BAD);
  CASE("match/bad_match", skred_fxbank_fenv_match(fx, 0, N, &never, &good, res, NULL) == BAD);
  CASE("match/record_before_match", skred_fxbank_fenv_match(fx, 0, N, &never, &b4[3], res, NULL) == BAD && strstr(skred_amd_last_error(), "record") != NULL);
  CASE("match/match_before_range", skred_fxbank_fenv_match(fx, 0, N + 1, &never, &good, res, NULL) == BAD);
  CASE("match/past_the_bank", skred_fxbank_fenv_match(fx, 0, N + 1, &chan, &good, res, NULL) == RANGE);
  CASE("match/empty_range", skred_fxbank_fenv_match(fx, 0, 0, &everyone, &good, res, NULL) == RANGE);
  CASE("match/negative_first", skred_fxbank_fenv_match(fx, -1, 4, &chan, &good, res, NULL) == RANGE);
  CASE("match/first_at_the_end", skred_fxbank_fenv_match(fx, N, 1, &chan, &good, res, NULL) == RANGE);
  /* the per-note calls: NULL bank or list, the tags, n, the records -- skred_fxbank_cutoff_owned_each's order */
  CASE("owned/null_bank", skred_fxbank_fenv_owned_each(NULL, r4, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_list", skred_fxbank_fenv_owned_each(fx, r4, NULL, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_tags", skred_fxbank_fenv_owned_each(fx, r4, list, NULL, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_records", skred_fxbank_fenv_owned_each(fx, NULL, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/zero_tag", skred_fxbank_fenv_owned_each(fx, r4, list, z4, 4, NULL, res, NULL) == BAD);
  CASE("owned/negative_n", skred_fxbank_fenv_owned_each(fx, r4, list, t4, -2, NULL, res, NULL) == BAD);
  CASE("owned/bad_record", skred_fxbank_fenv_owned_each(fx, b4, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/tags_before_records", skred_fxbank_fenv_owned_each(fx, b4, list, z4, 4, NULL, res, NULL) == BAD &&
                                    strstr(skred_amd_last_error(), "record") == NULL);
  CASE("owned/repeated_tag_is_fine_but_the_record_is_not", skred_fxbank_fenv_owned_each(fx, b4, list, d4, 4, NULL, res, NULL) == BAD &&
                                                           strstr(skred_amd_last_error(), "record") != NULL);
  CASE("owned/empty", skred_fxbank_fenv_owned_each(fx, r4, list, t4, 0, NULL, res, NULL) == SKRED_OK);
  CASE("owned/empty_null_result", skred_fxbank_fenv_owned_each(fx, r4, list, t4, 0, NULL, NULL, NULL) == SKRED_OK);
  CASE("tags/null_bank", skred_fxbank_fenv_tags_each(NULL, r4, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/null_tags", skred_fxbank_fenv_tags_each(fx, r4, 0, N, NULL, 4, res, NULL) == BAD);
  CASE("tags/null_records", skred_fxbank_fenv_tags_each(fx, NULL, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/repeated_tag", skred_fxbank_fenv_tags_each(fx, r4, 0, N, d4, 4, res, NULL) == BAD);
  CASE("tags/zero_tag", skred_fxbank_fenv_tags_each(fx, r4, 0, N, z4, 4, res, NULL) == BAD);
  CASE("tags/too_many", skred_fxbank_fenv_tags_each(fx, rmany, 0, N, many, SKRED_OWNER_MAX_TAGS + 1, res, NULL) == BAD);
  CASE("tags/bad_record", skred_fxbank_fenv_tags_each(fx, b4, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/records_before_range", skred_fxbank_fenv_tags_each(fx, b4, 0, N + 1, t4, 4, res, NULL) == BAD);
  CASE("tags/past_the_bank", skred_fxbank_fenv_tags_each(fx, r4, 0, N + 1, t4, 4, res, NULL) == RANGE);
  CASE("tags/empty_range", skred_fxbank_fenv_tags_each(fx, r4, 0, 0, t4, 4, res, NULL) == RANGE);
  CASE("tags/negative_first", skred_fxbank_fenv_tags_each(fx, r4, -1, 4, t4, 4, res, NULL) == RANGE);
  CASE("tags/range_before_empty_list", skred_fxbank_fenv_tags_each(fx, r4, 0, N + 1, t4, 0, res, NULL) == RANGE);
  CASE("tags/empty", skred_fxbank_fenv_tags_each(fx, r4, 0, N, t4, 0, res, NULL) == SKRED_OK);
  CASE("download/null_bank", skred_fxbank_download_fenv(NULL, words, 0, 4) == BAD);
  CASE("download/null_out", skred_fxbank_download_fenv(fx, NULL, 0, 4) == BAD);
  CASE("download/negative_count", skred_fxbank_download_fenv(fx, words, 0, -1) == BAD);
  CASE("download/past_the_bank", skred_fxbank_download_fenv(fx, words, N - 2, 4) == RANGE);
  CASE("download/empty", skred_fxbank_download_fenv(fx, words, 0, 0) == SKRED_OK && words[0] == 7);
  int zeros = skred_fxbank_download_fenv(fx, words, N - 3, 3) == SKRED_OK;
  for (int k = 0; k < 24; k++) zeros = zeros && words[k] == 0;
  CASE("download/no_array_gives_zeros", zeros && words[24] == 7 && words[31] == 7);

  CASE("untouched/outputs", res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && list[0] == 0 && list[3] == 24);
  CASE("untouched/bank", fx->ring_head == 0 && !fx->d_owner && !fx->d_pedal && !fx->d_glide && !fx->d_bend && !fx->d_cut && !fx->d_fenv &&
                         !fx->d_owner_found && fx->count == 0 && !fx->ring[0].in_flight);
  free(fx);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
