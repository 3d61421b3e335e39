/* The host side of the fixed-point cutoff calls without a device: skred_fx_filter_coeffs_w at the corners of the box and its
 * refusals, skred_fx_cutoff_check refusal by refusal in the documented order, every refusal the entry points make before anything
 * touches the device, with its return code and in the documented order -- on a skred_fxbank_t that is nothing but its voice count (a
 * refused call reads no other member) --, and what travels behind skred_fxbank_cutoff_tags_each: the tags sorted (sk_owner_pack) and
 * the records permuted with them (skx_cutoff_pack), at n = 1, 2, 1023, 1024.  One line per case, "OK" last.
 * tests/test_fx_cutoff_cpu.py builds and runs it; built together with skred_amd/csrc/skred_fx_cutoff.c and
 * -fsanitize=address,undefined it is the sanitizer run of that file's host code -- from the repository root, after the library is
 * built (the program's own copy of skred_fx_cutoff.c takes the place of the library's; everything else it calls comes from the
 * library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_fx_cutoff_host.c skred_amd/csrc/skred_fx_cutoff.c -o /tmp/c_fx_cutoff_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_fx_cutoff_host_san
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
#define ABS SKRED_FX_CUTOFF_ABS
#define TRACK SKRED_FX_CUTOFF_TRACK
#define GLIDE SKRED_FX_CUTOFF_GLIDE
#define SQ SKRED_FX_CUTOFF_Q
#define SM SKRED_FX_CUTOFF_MODE
#define WMIN SKRED_FX_CUTOFF_W_MIN
#define WMAX SKRED_FX_CUTOFF_W_MAX
#define QMIN SKRED_FX_CUTOFF_Q_MIN
#define QMAX SKRED_FX_CUTOFF_Q_MAX

static int check1(skred_fx_cutoff_t r, int first_time) { return skred_fx_cutoff_check(&r, 1, first_time); }

/* the sort-plus-permutation behind cutoff_tags_each at n tags given in descending order with a twist: record k carries value 1000 + k */
static int permuted(int n) {
  uint32_t *tags = (uint32_t *)calloc((size_t)n, sizeof(uint32_t)), *sorted = (uint32_t *)calloc((size_t)n, sizeof(uint32_t));
  uint32_t *perm = (uint32_t *)calloc((size_t)n, sizeof(uint32_t));
  skred_fx_cutoff_t *r = (skred_fx_cutoff_t *)calloc((size_t)n, sizeof(skred_fx_cutoff_t));
  skx_cut_each_t *out = (skx_cut_each_t *)calloc((size_t)n + 1, sizeof(skx_cut_each_t));
  for (int k = 0; k < n; k++) {
    tags[k] = (k & 1 ? 0x80000000u : 0u) + 5u * (uint32_t)(n - k);        /* every other one at or above 2^31: unsigned order */
    r[k].set = TRACK | (k & 1 ? SQ : 0u) | (k % 3 ? 0u : GLIDE);
    r[k].value = 1000u + (uint32_t)k;
    r[k].q_q16 = 70000u + (uint32_t)k; r[k].mode = 3; r[k].up_q32 = 11u + (uint32_t)k; r[k].down_q32 = 13u + (uint32_t)k;
  }
  memset(out, 0xEE, ((size_t)n + 1) * sizeof(skx_cut_each_t));
  int ok = sk_owner_pack(tags, n, sorted, perm) == SKRED_OK;
  skx_cutoff_pack(r, n, perm, out);
  for (int j = 0; j < n && ok; j++) {
    const uint32_t k = perm[j], *w = out[j].w;
    ok = k < (uint32_t)n && sorted[j] == tags[k] && (j == 0 || sorted[j - 1] < sorted[j]) && w[SKX_CUT_E_SET] == r[k].set &&
         w[SKX_CUT_E_VALUE] == 1000u + k && w[SKX_CUT_E_Q] == (k & 1 ? 70000u + k : 0u) && w[SKX_CUT_E_MODE] == 0u &&   /* not named: zero */
         w[SKX_CUT_E_UP] == (k % 3 ? 0u : 11u + k) && w[SKX_CUT_E_DOWN] == (k % 3 ? 0u : 13u + k) && w[6] == 0u && w[7] == 0u;
  }
  ok = ok && out[n].w[0] == 0xEEEEEEEEu;                                  /* n records and not one more */
  free(tags); free(sorted); free(perm); free(r); free(out);
  return ok;
}

int main(void) {
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0xFFFFFFFFu, 0x80000000u }, z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u };
  const uint32_t d4[4] = { 0x03000001u, 0x03000002u, 0x03000001u, 0x03000004u };
  static uint32_t many[SKRED_OWNER_MAX_TAGS + 1];
  static skred_fx_cutoff_t rmany[SKRED_OWNER_MAX_TAGS + 1];
  const skred_fx_cutoff_t good = { ABS | SQ | SM, 1u << 24, 1u << 16, 1, 0, 0, { 0, 0 } };
  for (int k = 0; k <= SKRED_OWNER_MAX_TAGS; k++) { many[k] = 1u + (uint32_t)k; rmany[k] = good; }
  skred_fx_cutoff_t r4[4] = { good, good, good, good }, b4[4] = { good, good, good, good };
  b4[3].set = ABS | TRACK;                                                /* the last record is bad */
  const skred_owner_match_t chan = { 0x03000000u, 0xFF000000u }, everyone = { 0u, 0u }, never = { 0x03000001u, 0xFF000000u };

  CASE("const/sizes", sizeof(skx_cut_t) == 32 && sizeof(skx_cut_each_t) == 32 && sizeof(skred_fx_cutoff_t) == 32 && SKX_CUT_CARRY == 4);
  CASE("const/box", WMIN == 1u << 19 && WMAX == 3u << 29 && QMIN == 1u << 10 && QMAX == 1u << 26 && SKX_CUTOFF_W_MAX == WMAX);

  /* skred_fx_filter_coeffs_w: the corners, the seam, its refusals */
  {
    int32_t o[5] = { 7, 7, 7, 7, 7 };
    const uint32_t ws[6] = { WMIN, WMIN + 1u, SKRED_FX_CUTOFF_HALF_PI_Q29, SKRED_FX_CUTOFF_HALF_PI_Q29 + 1u, WMAX - 1u, WMAX };
    const uint32_t qs[4] = { QMIN, QMIN + 1u, QMAX - 1u, QMAX };
    int all = 1, stable = 1;
    for (int m = 1; m <= 5; m++)
      for (int i = 0; i < 6; i++)
        for (int j = 0; j < 4; j++) {
          all = all && skred_fx_filter_coeffs_w(m, ws[i], qs[j], o) == SKRED_OK;
          const int64_t a1 = o[3] < 0 ? -(int64_t)o[3] : o[3], a2 = o[4];
          stable = stable && a2 > -(1ll << 30) && a2 < (1ll << 30) && a1 < (1ll << 30) + a2;
          if (m == 3) stable = stable && o[1] == 0 && o[2] == -o[0];
          if (m == 5) stable = stable && o[2] == 1 << 30 && o[0] == o[4] && o[1] == o[3];
        }
    CASE("coeffs/corners", all);
    CASE("coeffs/corners_stable", stable);
    CASE("coeffs/known", skred_fx_filter_coeffs_w(1, 1u << 26, 1u << 16, o) == SKRED_OK && o[0] == 3943046 && o[1] == 7886093 && o[2] == 3943046 &&
                         o[3] == -2005698314 && o[4] == 947728676);
    o[0] = 7;
    CASE("coeffs/bypass", skred_fx_filter_coeffs_w(0, 1u << 26, 1u << 16, o) == 1 && o[0] == 7);
    CASE("coeffs/null", skred_fx_filter_coeffs_w(1, 1u << 26, 1u << 16, NULL) == BAD);
    CASE("coeffs/bad_mode", skred_fx_filter_coeffs_w(6, 1u << 26, 1u << 16, o) == BAD && skred_fx_filter_coeffs_w(-1, 1u << 26, 1u << 16, o) == BAD);
    CASE("coeffs/w_outside", skred_fx_filter_coeffs_w(1, WMIN - 1u, 1u << 16, o) == RANGE && skred_fx_filter_coeffs_w(1, WMAX + 1u, 1u << 16, o) == RANGE &&
                             skred_fx_filter_coeffs_w(1, 0u, 1u << 16, o) == RANGE);
    CASE("coeffs/q_outside", skred_fx_filter_coeffs_w(1, 1u << 26, QMIN - 1u, o) == RANGE && skred_fx_filter_coeffs_w(1, 1u << 26, QMAX + 1u, o) == RANGE);
    CASE("coeffs/refusals_write_nothing", o[0] == 7);
  }

  /* skred_fx_cutoff_check, in the header's order */
  {
    skred_fx_cutoff_t r = good;
    CASE("check/plain", skred_fx_cutoff_check(r4, 4, 0) == SKRED_OK && skred_fx_cutoff_check(r4, 4, 1) == SKRED_OK);
    CASE("check/empty", skred_fx_cutoff_check(r4, 0, 0) == SKRED_OK);
    CASE("check/null", skred_fx_cutoff_check(NULL, 0, 0) == BAD);
    CASE("check/null_before_n", skred_fx_cutoff_check(NULL, -1, 0) == BAD);
    CASE("check/negative_n", skred_fx_cutoff_check(r4, -1, 0) == BAD);
    CASE("check/bad_record_not_reached", skred_fx_cutoff_check(b4, 3, 0) == SKRED_OK && skred_fx_cutoff_check(b4, 4, 0) == BAD);
    r = good; r.set |= 32u; CASE("check/unknown_bits", check1(r, 0) == BAD);
    r = good; r.set |= TRACK; CASE("check/abs_and_track", check1(r, 0) == BAD);
    r = good; r.set &= ~(uint32_t)ABS; CASE("check/neither", check1(r, 0) == BAD);
    r = good; r.set = ABS | SQ; CASE("check/first_time_without_mode", check1(r, 1) == BAD && check1(r, 0) == SKRED_OK);
    r = good; r.set = ABS | SM; CASE("check/first_time_without_q", check1(r, 1) == BAD && check1(r, 0) == SKRED_OK);
    r = good; r.reserved[0] = 1; CASE("check/reserved_0", check1(r, 0) == BAD);
    r = good; r.reserved[1] = 1; CASE("check/reserved_1", check1(r, 0) == BAD);
    r = good; r.q_q16 = QMIN - 1u; CASE("check/q_below", check1(r, 0) == RANGE);
    r = good; r.q_q16 = QMAX + 1u; CASE("check/q_above", check1(r, 0) == RANGE);
    r = good; r.q_q16 = QMAX; CASE("check/q_edges", check1(r, 0) == SKRED_OK && (r.q_q16 = QMIN, check1(r, 0)) == SKRED_OK);
    r = good; r.set = ABS; r.q_q16 = 0; r.mode = 9; CASE("check/unnamed_q_and_mode_are_not_looked_at", check1(r, 0) == SKRED_OK);
    r = good; r.value = WMIN - 1u; CASE("check/abs_below", check1(r, 0) == RANGE);
    r = good; r.value = WMAX + 1u; CASE("check/abs_above", check1(r, 0) == RANGE);
    r = good; r.value = WMAX; CASE("check/abs_edges", check1(r, 0) == SKRED_OK && (r.value = WMIN, check1(r, 0)) == SKRED_OK);
    r = good; r.set = TRACK | SQ | SM; r.value = 0; CASE("check/track_zero", check1(r, 0) == RANGE);
    r.value = 0xFFFFFFFFu; CASE("check/track_any_other_value", check1(r, 0) == SKRED_OK && (r.value = 1u, check1(r, 0)) == SKRED_OK);
    r = good; r.mode = 0; CASE("check/mode_0", check1(r, 0) == RANGE);
    r = good; r.mode = 6; CASE("check/mode_6", check1(r, 0) == RANGE);
    r = good; r.set |= GLIDE; r.up_q32 = 0; r.down_q32 = 5; CASE("check/glide_zero_up", check1(r, 0) == BAD);
    r.up_q32 = 5; r.down_q32 = 0; CASE("check/glide_zero_down", check1(r, 0) == BAD);
    r.down_q32 = 0xFFFFFFFFu; CASE("check/glide_any_other_rate", check1(r, 0) == SKRED_OK);
    r = good; r.up_q32 = 0; r.down_q32 = 0; CASE("check/rates_without_glide_are_not_looked_at", check1(r, 0) == SKRED_OK);
    r = good; r.q_q16 = 0; r.set |= 32u; CASE("check/bits_before_q", check1(r, 0) == BAD);
    r = good; r.q_q16 = 0; r.value = 0; r.mode = 0; CASE("check/q_before_value_before_mode", check1(r, 0) == RANGE && strstr(skred_amd_last_error(), "q_q16") != NULL);
    r = good; r.mode = 0; r.set |= GLIDE; CASE("check/mode_before_rates", check1(r, 0) == RANGE);
  }

  /* the packing: named words as they stand, the others zero, in order or permuted */
  {
    skx_cut_each_t out[3];
    skred_fx_cutoff_t two[2] = { { ABS | SQ | SM | GLIDE, 111, 222, 3, 44, 55, { 0, 0 } }, { TRACK, 666, 777, 4, 88, 99, { 0, 0 } } };
    memset(out, 0xEE, sizeof(out));
    skx_cutoff_pack(two, 2, NULL, out);
    CASE("pack/in_order", out[0].w[0] == (ABS | SQ | SM | GLIDE) && out[0].w[1] == 111 && out[0].w[2] == 222 && out[0].w[3] == 3 && out[0].w[4] == 44 &&
                          out[0].w[5] == 55 && out[0].w[6] == 0 && out[0].w[7] == 0 && out[2].w[0] == 0xEEEEEEEEu);
    CASE("pack/unnamed_words_are_zero", out[1].w[0] == TRACK && out[1].w[1] == 666 && out[1].w[2] == 0 && out[1].w[3] == 0 && out[1].w[4] == 0 && out[1].w[5] == 0);
    const uint32_t perm[2] = { 1, 0 };
    skx_cutoff_pack(two, 2, perm, out);
    CASE("pack/permuted", out[0].w[1] == 666 && out[1].w[1] == 111 && out[2].w[0] == 0xEEEEEEEEu);
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
  /* the channel sweep: NULL bank, match or record, the record, the match, the range -- in that order */
  CASE("match/null_bank", skred_fxbank_cutoff_match(NULL, 0, N, &chan, &good, res, NULL) == BAD);
  CASE("match/null_match", skred_fxbank_cutoff_match(fx, 0, N, NULL, &good, res, NULL) == BAD);
  CASE("match/null_record", skred_fxbank_cutoff_match(fx, 0, N, &chan, NULL, res, NULL) == BAD);
  CASE("match/bad_record", skred_fxbank_cutoff_match(fx, 0, N, &chan, &b4[3], res, NULL) == BAD);
  CASE("match/bad_match", skred_fxbank_cutoff_match(fx, 0, N, &never, &good, res, NULL) == BAD);
  CASE("match/record_before_match", skred_fxbank_cutoff_match(fx, 0, N, &never, &b4[3], res, NULL) == BAD && strstr(skred_amd_last_error(), "record") != NULL);
  CASE("match/match_before_range", skred_fxbank_cutoff_match(fx, 0, N + 1, &never, &good, res, NULL) == BAD);
  CASE("match/past_the_bank", skred_fxbank_cutoff_match(fx, 0, N + 1, &chan, &good, res, NULL) == RANGE);
  CASE("match/empty_range", skred_fxbank_cutoff_match(fx, 0, 0, &everyone, &good, res, NULL) == RANGE);
  CASE("match/negative_first", skred_fxbank_cutoff_match(fx, -1, 4, &chan, &good, res, NULL) == RANGE);
  CASE("match/first_at_the_end", skred_fxbank_cutoff_match(fx, N, 1, &chan, &good, res, NULL) == RANGE);
  /* the per-note calls: NULL bank or list, the tags, n, the records -- skred_fxbank_bend_owned_each's order */
  CASE("owned/null_bank", skred_fxbank_cutoff_owned_each(NULL, r4, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_list", skred_fxbank_cutoff_owned_each(fx, r4, NULL, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_tags", skred_fxbank_cutoff_owned_each(fx, r4, list, NULL, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_records", skred_fxbank_cutoff_owned_each(fx, NULL, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/zero_tag", skred_fxbank_cutoff_owned_each(fx, r4, list, z4, 4, NULL, res, NULL) == BAD);
  CASE("owned/negative_n", skred_fxbank_cutoff_owned_each(fx, r4, list, t4, -2, NULL, res, NULL) == BAD);
  CASE("owned/bad_record", skred_fxbank_cutoff_owned_each(fx, b4, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/tags_before_records", skred_fxbank_cutoff_owned_each(fx, b4, list, z4, 4, NULL, res, NULL) == BAD &&
                                    strstr(skred_amd_last_error(), "record") == NULL);
  CASE("owned/repeated_tag_is_fine_but_the_record_is_not", skred_fxbank_cutoff_owned_each(fx, b4, list, d4, 4, NULL, res, NULL) == BAD &&
                                                           strstr(skred_amd_last_error(), "record") != NULL);
  CASE("owned/empty", skred_fxbank_cutoff_owned_each(fx, r4, list, t4, 0, NULL, res, NULL) == SKRED_OK);
  CASE("owned/empty_null_result", skred_fxbank_cutoff_owned_each(fx, r4, list, t4, 0, NULL, NULL, NULL) == SKRED_OK);
  CASE("tags/null_bank", skred_fxbank_cutoff_tags_each(NULL, r4, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/null_tags", skred_fxbank_cutoff_tags_each(fx, r4, 0, N, NULL, 4, res, NULL) == BAD);
  CASE("tags/null_records", skred_fxbank_cutoff_tags_each(fx, NULL, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/repeated_tag", skred_fxbank_cutoff_tags_each(fx, r4, 0, N, d4, 4, res, NULL) == BAD);
  CASE("tags/zero_tag", skred_fxbank_cutoff_tags_each(fx, r4, 0, N, z4, 4, res, NULL) == BAD);
  CASE("tags/too_many", skred_fxbank_cutoff_tags_each(fx, rmany, 0, N, many, SKRED_OWNER_MAX_TAGS + 1, res, NULL) == BAD);
  CASE("tags/bad_record", skred_fxbank_cutoff_tags_each(fx, b4, 0, N, t4, 4, res, NULL) == BAD);
  CASE("tags/records_before_range", skred_fxbank_cutoff_tags_each(fx, b4, 0, N + 1, t4, 4, res, NULL) == BAD);
  CASE("tags/past_the_bank", skred_fxbank_cutoff_tags_each(fx, r4, 0, N + 1, t4, 4, res, NULL) == RANGE);
  CASE("tags/empty_range", skred_fxbank_cutoff_tags_each(fx, r4, 0, 0, t4, 4, res, NULL) == RANGE);
  CASE("tags/negative_first", skred_fxbank_cutoff_tags_each(fx, r4, -1, 4, t4, 4, res, NULL) == RANGE);
  CASE("tags/range_before_empty_list", skred_fxbank_cutoff_tags_each(fx, r4, 0, N + 1, t4, 0, res, NULL) == RANGE);
  CASE("tags/empty", skred_fxbank_cutoff_tags_each(fx, r4, 0, N, t4, 0, res, NULL) == SKRED_OK);
  CASE("advance/null_bank", skred_fxbank_cutoff_advance(NULL, 0, N, 64, res, NULL) == BAD);
  CASE("advance/zero_frames", skred_fxbank_cutoff_advance(fx, 0, N, 0, res, NULL) == BAD);
  CASE("advance/too_many_frames", skred_fxbank_cutoff_advance(fx, 0, N, 65537, res, NULL) == BAD);
  CASE("advance/frames_before_range", skred_fxbank_cutoff_advance(fx, 0, N + 1, 0, res, NULL) == BAD);
  CASE("advance/past_the_bank", skred_fxbank_cutoff_advance(fx, 1, N, 64, res, NULL) == RANGE);
  CASE("advance/empty_range", skred_fxbank_cutoff_advance(fx, 0, 0, 64, res, NULL) == RANGE);
  CASE("advance/negative_first", skred_fxbank_cutoff_advance(fx, -1, 4, 64, res, NULL) == RANGE);
  CASE("stop/null_bank", skred_fxbank_cutoff_stop(NULL, 0, N, 0, NULL) == BAD);
  CASE("stop/past_the_bank", skred_fxbank_cutoff_stop(fx, 8, N, 1, NULL) == RANGE);
  CASE("stop/negative_count", skred_fxbank_cutoff_stop(fx, 0, -1, 0, NULL) == RANGE);
  CASE("stop/no_array_yet", skred_fxbank_cutoff_stop(fx, 0, N, 1, NULL) == SKRED_OK);
  CASE("stop/empty", skred_fxbank_cutoff_stop(fx, N, 0, 1, NULL) == SKRED_OK);
  CASE("download/null_bank", skred_fxbank_download_cutoff(NULL, words, 0, 4) == BAD);
  CASE("download/null_out", skred_fxbank_download_cutoff(fx, NULL, 0, 4) == BAD);
  CASE("download/negative_count", skred_fxbank_download_cutoff(fx, words, 0, -1) == BAD);
  CASE("download/past_the_bank", skred_fxbank_download_cutoff(fx, words, N - 2, 4) == RANGE);
  CASE("download/empty", skred_fxbank_download_cutoff(fx, words, 0, 0) == SKRED_OK && words[0] == 7);
  int zeros = skred_fxbank_download_cutoff(fx, words, N - 3, 3) == SKRED_OK;
  for (int k = 0; k < 24; k++) zeros = zeros && words[k] == 0;
  CASE("download/no_array_yet_gives_zeros", zeros && words[24] == 7 && words[31] == 7);

  CASE("untouched/outputs", res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && list[0] == 0 && list[3] == 24);
  CASE("untouched/bank", fx->ring_head == 0 && !fx->d_owner && !fx->d_pedal && !fx->d_glide && !fx->d_bend && !fx->d_cut && !fx->d_owner_found &&
                         fx->count == 0 && !fx->ring[0].in_flight);
  free(fx);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
