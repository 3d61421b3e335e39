/* The host side of the cutoff calls without a device: skred_filter_coeffs_w's refusals, skred_cutoff_check with every refusal in the
 * header's order, the 32-byte packing of the records, the permutation that keeps recs[k] with tags[k] when the tags travel sorted
 * (n = 1, 2, 1023, 1024) and every refusal the entry points make before anything touches the device, each with its return code, on a
 * skred_bank_t that is nothing but its voice count (a refused call reads no other member).  One line per case, "OK" last.
 * tests/test_cutoff_cpu.py builds and runs it; built together with skred_amd/csrc/skred_bank_cutoff.c and
 * -fsanitize=address,undefined it is the sanitizer run of that file's host code -- from the repository root, after the library is
 * built (the program's own copy of skred_bank_cutoff.c takes the place of the library's; everything else it calls comes from the
 * library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
 *       -Iskred_amd/csrc -I${ROCM_PATH:-/opt/rocm}/include tests/c_cutoff_host.c skred_amd/csrc/skred_bank_cutoff.c \
 *       -o /tmp/c_cutoff_host_san -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_cutoff_host_san */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_bank_priv.h"

static int failures;
#define CASE(name, cond) do { const int ok_ = (cond); printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); failures += !ok_; } while (0)

#define N 1024
#define K 8
#define VMASK 0x77ull
#define FMASK 0x55ull
#define BAD SKRED_E_BAD_ARG
#define RANGE SKRED_E_RANGE
#define QM (SKRED_CUTOFF_Q | SKRED_CUTOFF_MODE)

static skred_cutoff_t rec(uint32_t set, float value, float q, uint32_t mode, float up, float down) {
  skred_cutoff_t r;
  memset(&r, 0, sizeof(r));
  r.set = set; r.value = value; r.q = q; r.mode = mode; r.rate_up = up; r.rate_down = down;
  return r;
}
static int one(skred_cutoff_t r) { return skred_cutoff_check(&r, 1, K, VMASK, FMASK, 0); }

/* tags in a scrambled order, record k marked with k: after the pack, record j must be the one that stood with the j-th smallest tag */
static int perm_case(int n) {
  static uint32_t tags[SKRED_OWNER_MAX_TAGS], sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  static skred_cutoff_t in[SKRED_OWNER_MAX_TAGS];
  static sk_cut_each_t out[SKRED_OWNER_MAX_TAGS + 1];
  for (int k = 0; k < n; k++) {
    tags[k] = 0x80000000u ^ (uint32_t)(((uint64_t)k * 2654435761u) % 1000003u + 1u);     /* distinct: the map is a bijection mod a prime */
    in[k] = rec(SKRED_CUTOFF_ABS | QM, 0.5f + (float)k / 1024.0f, 0.7f, 1u + (uint32_t)k % 5u, 0.0f, 0.0f);
  }
  memset(&out[n], 0xA5, sizeof(out[n]));
  if (sk_owner_pack(tags, n, sorted, perm)) return 0;
  sk_cutoff_pack(in, n, perm, out);
  for (int j = 0; j < n; j++) {
    if (j && sorted[j] <= sorted[j - 1]) return 0;
    if (tags[perm[j]] != sorted[j]) return 0;
    if (memcmp(&out[j].w[SK_CUT_E_VALUE], &in[perm[j]].value, 4) || out[j].w[SK_CUT_E_MODE] != in[perm[j]].mode) return 0;
  }
  return out[n].w[0] == 0xA5A5A5A5u && out[n].w[7] == 0xA5A5A5A5u;                        /* nothing past record n - 1 */
}

int main(void) {
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0xFFFFFFFFu, 0x80000000u }, z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u };
  const uint32_t d4[4] = { 0x03000001u, 0x03000002u, 0x03000001u, 0x03000004u };
  static uint32_t many[SKRED_OWNER_MAX_TAGS + 1];
  static skred_cutoff_t rmany[SKRED_OWNER_MAX_TAGS + 1];
  const skred_cutoff_t good = rec(SKRED_CUTOFF_ABS | QM, 0.3f, 0.9f, 1, 0, 0);
  const skred_cutoff_t sweep = rec(SKRED_CUTOFF_TRACK | SKRED_CUTOFF_GLIDE, 0.01f, 0, 0, 1.01f, 0.99f);
  for (int k = 0; k <= SKRED_OWNER_MAX_TAGS; k++) { many[k] = 1u + (uint32_t)k; rmany[k] = good; }
  skred_cutoff_t r4[4] = { good, sweep, rec(SKRED_CUTOFF_TRACK | QM, 0.02f, 4.0f, 3, 0, 0), rec(SKRED_CUTOFF_ABS, 3.0f, 0, 0, 0, 0) };
  skred_cutoff_t bad4[4] = { good, sweep, rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_TRACK, 0.3f, 0, 0, 0, 0), good };
  const skred_owner_match_t chan = { 0x03000000u, 0xFF000000u }, wrong = { 0x03000001u, 0xFF000000u };
  float c5[5] = { 9, 9, 9, 9, 9 };

  CASE("const/sizes", sizeof(skred_cutoff_t) == 32 && sizeof(sk_cut_each_t) == 32 && sizeof(sk_cut_t) == 32 && SK_CUT_W == 0 && SK_CUT_CARRY == 4);
  CASE("const/box", SKRED_CUTOFF_W_MIN == 0x1p-10f && SKRED_CUTOFF_W_MAX == 3.0f && SKRED_CUTOFF_Q_MIN == 0x1p-6f && SKRED_CUTOFF_Q_MAX == 0x1p10f);

  /* skred_filter_coeffs_w */
  CASE("coeffs/null", skred_filter_coeffs_w(1, 0.3f, 0.9f, NULL) == BAD);
  CASE("coeffs/mode6", skred_filter_coeffs_w(6, 0.3f, 0.9f, c5) == BAD && skred_filter_coeffs_w(-1, 0.3f, 0.9f, c5) == BAD);
  CASE("coeffs/bypass", skred_filter_coeffs_w(0, 0.3f, 0.9f, c5) == 1 && c5[0] == 9 && c5[4] == 9);
  CASE("coeffs/w_low", skred_filter_coeffs_w(1, 0x1p-11f, 0.9f, c5) == RANGE && skred_filter_coeffs_w(1, 0.0f, 0.9f, c5) == RANGE);
  CASE("coeffs/w_high", skred_filter_coeffs_w(1, 3.0000002f, 0.9f, c5) == RANGE && skred_filter_coeffs_w(1, NAN, 0.9f, c5) == RANGE);
  CASE("coeffs/q_out", skred_filter_coeffs_w(1, 0.3f, 0x1p-7f, c5) == RANGE && skred_filter_coeffs_w(1, 0.3f, 1025.0f, c5) == RANGE &&
                       skred_filter_coeffs_w(1, 0.3f, INFINITY, c5) == RANGE && c5[0] == 9);
  CASE("coeffs/corners", skred_filter_coeffs_w(1, 0x1p-10f, 0x1p-6f, c5) == SKRED_OK && skred_filter_coeffs_w(5, 3.0f, 0x1p10f, c5) == SKRED_OK &&
                         isfinite(c5[0]) && c5[2] == 1.0f);
  { float a[5], b[5];
    CASE("coeffs/near_libm", skred_filter_coeffs_w(1, 0.25f, 0.9f, a) == SKRED_OK && skred_filter_coeffs(1, 0.25f, 0.9f, 6.2831855f, b) == SKRED_OK &&
                             fabsf(a[0] - b[0]) < 1e-6f && fabsf(a[3] - b[3]) < 1e-6f && fabsf(a[4] - b[4]) < 1e-6f); }

  /* skred_cutoff_check, in the header's order */
  CASE("check/plain", skred_cutoff_check(r4, 4, K, VMASK, FMASK, 0) == SKRED_OK);
  CASE("check/empty", skred_cutoff_check(r4, 0, K, VMASK, FMASK, 0) == SKRED_OK);
  CASE("check/null", skred_cutoff_check(NULL, 4, K, VMASK, FMASK, 0) == BAD);
  CASE("check/null_before_k", skred_cutoff_check(NULL, 4, 3, VMASK, FMASK, 0) == BAD);
  CASE("check/negative_n", skred_cutoff_check(r4, -1, K, VMASK, FMASK, 0) == BAD);
  CASE("check/k3", skred_cutoff_check(r4, 4, 3, 1, 1, 0) == RANGE && skred_cutoff_check(r4, 4, 0, 1, 1, 0) == RANGE && skred_cutoff_check(r4, 4, 128, 1, 1, 0) == RANGE);
  CASE("check/k_before_mask", skred_cutoff_check(r4, 4, 3, 0, 0, 0) == RANGE);
  CASE("check/k_before_record", skred_cutoff_check(bad4, 4, 3, 1, 1, 0) == RANGE);
  CASE("check/voice_mask0", skred_cutoff_check(r4, 4, K, 0, FMASK, 0) == BAD);
  CASE("check/voice_mask_high", skred_cutoff_check(r4, 4, K, 0x177, FMASK, 0) == BAD);
  CASE("check/filter_mask0", skred_cutoff_check(r4, 4, K, VMASK, 0, 0) == BAD);
  CASE("check/filter_mask_high", skred_cutoff_check(r4, 4, K, VMASK, 0x100, 0) == BAD);
  CASE("check/k64_full_masks", skred_cutoff_check(r4, 4, 64, ~0ull, ~0ull, 0) == SKRED_OK && skred_cutoff_check(r4, 4, 1, 1, 1, 0) == SKRED_OK);
  CASE("check/unknown_bit", one(rec(SKRED_CUTOFF_ABS | 32u, 0.3f, 0, 0, 0, 0)) == BAD);
  CASE("check/abs_and_track", one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_TRACK, 0.3f, 0, 0, 0, 0)) == BAD);
  CASE("check/neither", one(rec(QM, 0.3f, 0.9f, 1, 0, 0)) == BAD && one(rec(0, 0.3f, 0, 0, 0, 0)) == BAD);
  CASE("check/set_before_range", one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_TRACK, 9.0f, 0, 0, 0, 0)) == BAD);
  { skred_cutoff_t r = good; r.reserved[1] = 1;
    CASE("check/reserved", one(r) == BAD);
    r.value = 9.0f;
    CASE("check/reserved_before_box", one(r) == BAD); }
  CASE("check/value_nan", one(rec(SKRED_CUTOFF_ABS, NAN, 0, 0, 0, 0)) == BAD && one(rec(SKRED_CUTOFF_TRACK, INFINITY, 0, 0, 0, 0)) == BAD);
  CASE("check/q_nan", one(rec(SKRED_CUTOFF_ABS | QM, 0.3f, NAN, 1, 0, 0)) == BAD);
  CASE("check/q_nan_not_named", one(rec(SKRED_CUTOFF_ABS, 0.3f, NAN, 0, 0, 0)) == SKRED_OK);
  CASE("check/rate_nan", one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_GLIDE, 0.3f, 0, 0, NAN, 0.5f)) == BAD);
  CASE("check/rate_nan_not_named", one(rec(SKRED_CUTOFF_ABS, 0.3f, 0, 0, NAN, NAN)) == SKRED_OK);
  CASE("check/finite_before_box", one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_GLIDE, 9.0f, 0, 0, NAN, 0.5f)) == BAD);
  CASE("check/q_low", one(rec(SKRED_CUTOFF_ABS | QM, 0.3f, 0x1p-7f, 1, 0, 0)) == RANGE);
  CASE("check/q_high", one(rec(SKRED_CUTOFF_ABS | QM, 0.3f, 1024.5f, 1, 0, 0)) == RANGE);
  CASE("check/q_ends", one(rec(SKRED_CUTOFF_ABS | QM, 0.3f, 0x1p-6f, 1, 0, 0)) == SKRED_OK && one(rec(SKRED_CUTOFF_ABS | QM, 0.3f, 0x1p10f, 5, 0, 0)) == SKRED_OK);
  CASE("check/abs_low", one(rec(SKRED_CUTOFF_ABS, 0x1p-11f, 0, 0, 0, 0)) == RANGE);
  CASE("check/abs_high", one(rec(SKRED_CUTOFF_ABS, 3.0000002f, 0, 0, 0, 0)) == RANGE);
  CASE("check/abs_ends", one(rec(SKRED_CUTOFF_ABS, 0x1p-10f, 0, 0, 0, 0)) == SKRED_OK && one(rec(SKRED_CUTOFF_ABS, 3.0f, 0, 0, 0, 0)) == SKRED_OK);
  CASE("check/track_value", one(rec(SKRED_CUTOFF_TRACK, 0.0f, 0, 0, 0, 0)) == RANGE && one(rec(SKRED_CUTOFF_TRACK, -1.0f, 0, 0, 0, 0)) == RANGE &&
                            one(rec(SKRED_CUTOFF_TRACK, 1e30f, 0, 0, 0, 0)) == SKRED_OK);
  CASE("check/mode", one(rec(SKRED_CUTOFF_ABS | QM, 0.3f, 0.9f, 0, 0, 0)) == RANGE && one(rec(SKRED_CUTOFF_ABS | QM, 0.3f, 0.9f, 6, 0, 0)) == RANGE);
  CASE("check/rate_box", one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_GLIDE, 0.3f, 0, 0, 16.5f, 0.5f)) == RANGE &&
                         one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_GLIDE, 0.3f, 0, 0, 2.0f, 0.03f)) == RANGE);
  CASE("check/rate_up", one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_GLIDE, 0.3f, 0, 0, 1.0f, 0.5f)) == BAD && one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_GLIDE, 0.3f, 0, 0, 0.5f, 0.5f)) == BAD);
  CASE("check/rate_down", one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_GLIDE, 0.3f, 0, 0, 2.0f, 1.0f)) == BAD && one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_GLIDE, 0.3f, 0, 0, 2.0f, 2.0f)) == BAD);
  CASE("check/box_before_rates", one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_GLIDE, 9.0f, 0, 0, 1.0f, 0.5f)) == RANGE);
  CASE("check/rates_not_named", one(rec(SKRED_CUTOFF_ABS, 0.3f, 0, 0, 0.5f, 2.0f)) == SKRED_OK);
  CASE("check/smallest_rates", one(rec(SKRED_CUTOFF_ABS | SKRED_CUTOFF_GLIDE, 0.3f, 0, 0, 1.0000001f, 0.99999994f)) == SKRED_OK);
  CASE("check/filter_outside_voice", skred_cutoff_check(r4, 4, K, 0x11, FMASK, 0) == BAD);
  CASE("check/record_before_subset", skred_cutoff_check(bad4, 4, K, 0x11, FMASK, 0) == BAD && one(rec(SKRED_CUTOFF_ABS, 9.0f, 0, 0, 0, 0)) == RANGE &&
                                     skred_cutoff_check(&(skred_cutoff_t){ SKRED_CUTOFF_ABS, 9.0f }, 1, K, 0x11, FMASK, 0) == RANGE);
  CASE("check/first_time", skred_cutoff_check(r4, 1, K, VMASK, FMASK, 1) == SKRED_OK && skred_cutoff_check(r4, 2, K, VMASK, FMASK, 1) == BAD &&
                           skred_cutoff_check(&r4[3], 1, K, VMASK, FMASK, 1) == BAD && skred_cutoff_check(&r4[3], 1, K, VMASK, FMASK, 0) == SKRED_OK);
  CASE("check/third_record", skred_cutoff_check(bad4, 4, K, VMASK, FMASK, 0) == BAD && skred_cutoff_check(bad4, 2, K, VMASK, FMASK, 0) == SKRED_OK);

  /* the packing: 32 bytes, named words only */
  { sk_cut_each_t out[3];
    memset(out, 0xEE, sizeof(out));
    skred_cutoff_t in[2] = { rec(SKRED_CUTOFF_ABS, 0.3f, 7.0f, 4, 3.0f, 0.25f), rec(SKRED_CUTOFF_TRACK | SKRED_CUTOFF_GLIDE | QM, 0.01f, 0.9f, 2, 1.5f, 0.75f) };
    sk_cutoff_pack(in, 2, NULL, out);
    const float v0 = 0.3f, q1 = 0.9f, u1 = 1.5f, d1 = 0.75f;
    CASE("pack/unnamed_zeroed", out[0].w[0] == SKRED_CUTOFF_ABS && !memcmp(&out[0].w[1], &v0, 4) && !out[0].w[2] && !out[0].w[3] && !out[0].w[4] &&
                                !out[0].w[5] && !out[0].w[6] && !out[0].w[7]);
    CASE("pack/named", out[1].w[0] == (SKRED_CUTOFF_TRACK | SKRED_CUTOFF_GLIDE | QM) && !memcmp(&out[1].w[2], &q1, 4) && out[1].w[3] == 2 &&
                       !memcmp(&out[1].w[4], &u1, 4) && !memcmp(&out[1].w[5], &d1, 4) && !out[1].w[6] && !out[1].w[7]);
    CASE("pack/n_records_only", out[2].w[0] == 0xEEEEEEEEu && out[2].w[7] == 0xEEEEEEEEu);
    const uint32_t rev[2] = { 1, 0 };
    sk_cutoff_pack(in, 2, rev, out);
    CASE("pack/reversed", out[0].w[3] == 2 && out[1].w[0] == SKRED_CUTOFF_ABS); }
  CASE("perm/1", perm_case(1));
  CASE("perm/2", perm_case(2));
  CASE("perm/1023", perm_case(1023));
  CASE("perm/1024", perm_case(1024));

  /* the entry points: a bank that is nothing but its size */
  skred_bank_t *b = (skred_bank_t *)calloc(1, sizeof(skred_bank_t));
  b->n_voices = N;
  int32_t list[4] = { 0, 8, 16, 24 };
  uint32_t res[5] = { 7, 7, 7, 7, 7 }, words[32];
  for (int k = 0; k < 32; k++) words[k] = 7;
  const skred_cutoff_t far = rec(SKRED_CUTOFF_ABS, 9.0f, 0, 0, 0, 0);
  CASE("match/null_bank", skred_bank_cutoff_match(NULL, 0, N, K, FMASK, &chan, &good, res, NULL) == BAD);
  CASE("match/null_match", skred_bank_cutoff_match(b, 0, N, K, FMASK, NULL, &good, res, NULL) == BAD);
  CASE("match/null_record", skred_bank_cutoff_match(b, 0, N, K, FMASK, &chan, NULL, res, NULL) == BAD);
  CASE("match/null_before_k", skred_bank_cutoff_match(b, 0, N, 3, FMASK, &chan, NULL, res, NULL) == BAD);
  CASE("match/k12", skred_bank_cutoff_match(b, 0, N, 12, FMASK, &chan, &good, res, NULL) == RANGE);
  CASE("match/mask0", skred_bank_cutoff_match(b, 0, N, K, 0, &chan, &good, res, NULL) == BAD);
  CASE("match/mask_high", skred_bank_cutoff_match(b, 0, N, K, 0x1FF, &chan, &good, res, NULL) == BAD);
  CASE("match/mask_before_range", skred_bank_cutoff_match(b, 4, 8, K, 0, &chan, &good, res, NULL) == BAD);
  CASE("match/first_off_slot", skred_bank_cutoff_match(b, 4, 8, K, FMASK, &chan, &good, res, NULL) == RANGE);
  CASE("match/count_off_slot", skred_bank_cutoff_match(b, 0, 12, K, FMASK, &chan, &good, res, NULL) == RANGE);
  CASE("match/past_the_bank", skred_bank_cutoff_match(b, 0, N + K, K, FMASK, &chan, &good, res, NULL) == RANGE);
  CASE("match/empty_range", skred_bank_cutoff_match(b, 0, 0, K, FMASK, &chan, &good, res, NULL) == RANGE);
  CASE("match/range_before_record", skred_bank_cutoff_match(b, 4, 8, K, FMASK, &chan, &bad4[2], res, NULL) == RANGE);
  CASE("match/bad_set", skred_bank_cutoff_match(b, 0, N, K, FMASK, &chan, &bad4[2], res, NULL) == BAD);
  CASE("match/out_of_box", skred_bank_cutoff_match(b, 0, N, K, FMASK, &chan, &far, res, NULL) == RANGE);
  CASE("match/record_before_match", skred_bank_cutoff_match(b, 0, N, K, FMASK, &wrong, &far, res, NULL) == RANGE);
  CASE("match/value_outside_mask", skred_bank_cutoff_match(b, 0, N, K, FMASK, &wrong, &good, res, NULL) == BAD);
  CASE("owned/null_bank", skred_bank_cutoff_owned_each(NULL, r4, K, FMASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_list", skred_bank_cutoff_owned_each(b, r4, K, FMASK, NULL, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_tags", skred_bank_cutoff_owned_each(b, r4, K, FMASK, list, NULL, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_records", skred_bank_cutoff_owned_each(b, NULL, K, FMASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/negative_n", skred_bank_cutoff_owned_each(b, r4, K, FMASK, list, t4, -2, NULL, res, NULL) == BAD);
  CASE("owned/k12", skred_bank_cutoff_owned_each(b, r4, 12, FMASK, list, t4, 4, NULL, res, NULL) == RANGE);
  CASE("owned/mask0", skred_bank_cutoff_owned_each(b, r4, K, 0, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/mask_high", skred_bank_cutoff_owned_each(b, r4, K, 0x1FF, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/bad_record", skred_bank_cutoff_owned_each(b, bad4, K, FMASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/record_before_tag", skred_bank_cutoff_owned_each(b, bad4, K, FMASK, list, z4, 4, NULL, res, NULL) == BAD);
  CASE("owned/zero_tag", skred_bank_cutoff_owned_each(b, r4, K, FMASK, list, z4, 4, NULL, res, NULL) == BAD);
  CASE("owned/empty", skred_bank_cutoff_owned_each(b, r4, K, FMASK, list, t4, 0, NULL, res, NULL) == SKRED_OK);
  CASE("tags/null_bank", skred_bank_cutoff_tags_each(NULL, r4, 0, N, K, FMASK, t4, 4, res, NULL) == BAD);
  CASE("tags/null_tags", skred_bank_cutoff_tags_each(b, r4, 0, N, K, FMASK, NULL, 4, res, NULL) == BAD);
  CASE("tags/null_records", skred_bank_cutoff_tags_each(b, NULL, 0, N, K, FMASK, t4, 4, res, NULL) == BAD);
  CASE("tags/k3", skred_bank_cutoff_tags_each(b, r4, 0, N, 3, 0x7, t4, 4, res, NULL) == RANGE);
  CASE("tags/mask_high", skred_bank_cutoff_tags_each(b, r4, 0, N, K, 0x1FF, t4, 4, res, NULL) == BAD);
  CASE("tags/first_off_slot", skred_bank_cutoff_tags_each(b, r4, 4, 8, K, FMASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/past_the_bank", skred_bank_cutoff_tags_each(b, r4, 0, N + K, K, FMASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/empty_range", skred_bank_cutoff_tags_each(b, r4, 0, 0, K, FMASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/range_before_record", skred_bank_cutoff_tags_each(b, bad4, 4, 8, K, FMASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/bad_record", skred_bank_cutoff_tags_each(b, bad4, 0, N, K, FMASK, t4, 4, res, NULL) == BAD);
  CASE("tags/zero_tag", skred_bank_cutoff_tags_each(b, r4, 0, N, K, FMASK, z4, 4, res, NULL) == BAD);
  CASE("tags/repeated_tag", skred_bank_cutoff_tags_each(b, r4, 0, N, K, FMASK, d4, 4, res, NULL) == BAD);
  CASE("tags/too_many", skred_bank_cutoff_tags_each(b, rmany, 0, N, K, FMASK, many, SKRED_OWNER_MAX_TAGS + 1, res, NULL) == BAD);
  CASE("tags/negative_n", skred_bank_cutoff_tags_each(b, r4, 0, N, K, FMASK, t4, -1, res, NULL) == BAD);
  CASE("tags/empty", skred_bank_cutoff_tags_each(b, r4, 0, N, K, FMASK, t4, 0, res, NULL) == SKRED_OK);
  CASE("advance/null_bank", skred_bank_cutoff_advance(NULL, 0, N, 64, res, NULL) == BAD);
  CASE("advance/frames", skred_bank_cutoff_advance(b, 0, N, 0, res, NULL) == BAD && skred_bank_cutoff_advance(b, 0, N, 65537, res, NULL) == BAD);
  CASE("advance/range", skred_bank_cutoff_advance(b, 0, 0, 64, res, NULL) == RANGE && skred_bank_cutoff_advance(b, 8, N, 64, res, NULL) == RANGE);
  CASE("advance/no_array_yet", skred_bank_cutoff_advance(b, 0, N, 64, NULL, NULL) == SKRED_OK);
  CASE("stop/null_bank", skred_bank_cutoff_stop(NULL, 0, N, 1, NULL) == BAD);
  CASE("stop/past_the_bank", skred_bank_cutoff_stop(b, 8, N, 0, NULL) == RANGE);
  CASE("stop/negative_count", skred_bank_cutoff_stop(b, 0, -1, 0, NULL) == RANGE);
  CASE("stop/no_array_yet", skred_bank_cutoff_stop(b, 0, N, 1, NULL) == SKRED_OK);
  CASE("download/null_bank", skred_bank_download_cutoff(NULL, words, 0, 4) == BAD);
  CASE("download/null_out", skred_bank_download_cutoff(b, NULL, 0, 4) == BAD);
  CASE("download/past_the_bank", skred_bank_download_cutoff(b, words, N - 2, 4) == RANGE);
  CASE("download/empty", skred_bank_download_cutoff(b, words, 0, 0) == SKRED_OK && words[0] == 7);
  { int zeros = skred_bank_download_cutoff(b, words, N - 4, 3) == SKRED_OK;
    for (int k = 0; k < 24; k++) zeros = zeros && !words[k];
    CASE("download/no_array_yet_gives_zeros", zeros && words[24] == 7 && words[31] == 7); }

  CASE("untouched/outputs", res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && res[4] == 7 && list[0] == 0 && list[3] == 24);
  CASE("untouched/bank", b->touched_total == 0 && b->control_epoch == 0 && b->upd_seq == 0 && b->upd_head == 0 && !b->d_owner && !b->d_pedal &&
                         !b->d_glide && !b->d_bend && !b->d_cut && !b->d_owner_slots);
  free(b);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
