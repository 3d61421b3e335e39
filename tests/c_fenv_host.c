/* The host side of the filter-envelope calls without a device: skred_fenv_check with every refusal in the header's order, the 32-byte
 * packing of the records, the permutation that keeps recs[k] with tags[k] when the tags travel sorted (n = 1, 2, 1023, 1024) and
 * every refusal the entry points make before anything touches the device, each with its return code, on a skred_bank_t that is
 * nothing but its voice count (a refused call reads no other member).  One line per case, "OK" last.
 * tests/test_fenv_cpu.py builds and runs it; built together with skred_amd/csrc/skred_bank_fenv.c and
 * -fsanitize=address,undefined it is the sanitizer run of that file's host code -- from the repository root, after the library is
 * built (the program's own copy of skred_bank_fenv.c takes the place of the library's; everything else it calls comes from the
 * library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
 *       -Iskred_amd/csrc -I${ROCM_PATH:-/opt/rocm}/include tests/c_fenv_host.c skred_amd/csrc/skred_bank_fenv.c \
 *       -o /tmp/c_fenv_host_san -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_fenv_host_san */
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
#define A SKRED_FENV_ABS
#define R SKRED_FENV_REL
#define S SKRED_FENV_START

static skred_fenv_t rec(uint32_t set, float start, float peak, float sustain, float end, float ra, float rd, float rr) {
  skred_fenv_t r;
  memset(&r, 0, sizeof(r));
  r.set = set; r.start = start; r.peak = peak; r.sustain = sustain; r.end = end; r.rate_attack = ra; r.rate_decay = rd; r.rate_release = rr;
  return r;
}
static int one(skred_fenv_t r) { return skred_fenv_check(&r, 1, K, VMASK, FMASK); }

/* tags in a scrambled order, record k marked with k: after the pack, record j must be the one that stood with the j-th smallest tag */
static int perm_case(int n) {
  static uint32_t tags[SKRED_OWNER_MAX_TAGS], sorted[SKRED_OWNER_MAX_TAGS], perm[SKRED_OWNER_MAX_TAGS];
  static skred_fenv_t in[SKRED_OWNER_MAX_TAGS];
  static sk_fenv_each_t out[SKRED_OWNER_MAX_TAGS + 1];
  for (int k = 0; k < n; k++) {
    tags[k] = 0x80000000u ^ (uint32_t)(((uint64_t)k * 2654435761u) % 1000003u + 1u);     /* distinct: the map is a bijection mod a prime */
    in[k] = rec(A, 0, 0.5f + (float)k / 1024.0f, 0.25f, 0.125f, 1.5f, 0.75f, 0.5f + (float)k / 4096.0f);
  }
  memset(&out[n], 0xA5, sizeof(out[n]));
  if (sk_owner_pack(tags, n, sorted, perm)) return 0;
  sk_fenv_pack(in, n, perm, out);
  for (int j = 0; j < n; j++) {
    if (j && sorted[j] <= sorted[j - 1]) return 0;
    if (tags[perm[j]] != sorted[j]) return 0;
    if (memcmp(out[j].w, &in[perm[j]], sizeof(skred_fenv_t))) return 0;
  }
  return out[n].w[0] == 0xA5A5A5A5u && out[n].w[7] == 0xA5A5A5A5u;                        /* nothing past record n - 1 */
}

int main(void) {
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0xFFFFFFFFu, 0x80000000u }, z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u };
  const uint32_t d4[4] = { 0x03000001u, 0x03000002u, 0x03000001u, 0x03000004u };
  static uint32_t many[SKRED_OWNER_MAX_TAGS + 1];
  static skred_fenv_t rmany[SKRED_OWNER_MAX_TAGS + 1];
  const skred_fenv_t good = rec(A, 0, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f);
  const skred_fenv_t relative = rec(R | S, 0.5f, 8.0f, 2.0f, 1.0f, 2.0f, 0.5f, 0.25f);
  const skred_fenv_t both = rec(A | R, 0, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f);
  const skred_fenv_t far = rec(A, 0, 9.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f);
  for (int k = 0; k <= SKRED_OWNER_MAX_TAGS; k++) { many[k] = 1u + (uint32_t)k; rmany[k] = good; }
  skred_fenv_t r4[4] = { good, relative, rec(A | S, 0x1p-10f, 3.0f, 3.0f, 0x1p-10f, 16.0f, 0x1p-4f, 1.0000001f), rec(R, 0, 1e30f, 1e-30f, 1.0f, 0.5f, 2.0f, 2.0f) };
  skred_fenv_t bad4[4] = { good, relative, both, good };
  const skred_owner_match_t chan = { 0x03000000u, 0xFF000000u }, wrong = { 0x03000001u, 0xFF000000u };

  CASE("const/sizes", sizeof(skred_fenv_t) == 32 && sizeof(sk_fenv_each_t) == 32 && sizeof(sk_fenv_t) == 32 && SK_FENV_STAGE == 0 && SK_FENV_RATE_ATTACK == 4);
  CASE("const/stages", SK_FENV_OFF == 0 && SK_FENV_ATTACK == 1 && SK_FENV_DECAY == 2 && SK_FENV_SUSTAIN == 3 && SK_FENV_RELEASE == 4);

  /* skred_fenv_check, in the header's order */
  CASE("check/plain", skred_fenv_check(r4, 4, K, VMASK, FMASK) == SKRED_OK);
  CASE("check/empty", skred_fenv_check(r4, 0, K, VMASK, FMASK) == SKRED_OK);
  CASE("check/null", skred_fenv_check(NULL, 4, K, VMASK, FMASK) == BAD);
  CASE("check/null_before_k", skred_fenv_check(NULL, 4, 3, VMASK, FMASK) == BAD);
  CASE("check/negative_n", skred_fenv_check(r4, -1, K, VMASK, FMASK) == BAD);
  CASE("check/k3", skred_fenv_check(r4, 4, 3, 1, 1) == RANGE && skred_fenv_check(r4, 4, 0, 1, 1) == RANGE && skred_fenv_check(r4, 4, 128, 1, 1) == RANGE);
  CASE("check/k_before_mask", skred_fenv_check(r4, 4, 3, 0, 0) == RANGE);
  CASE("check/k_before_record", skred_fenv_check(bad4, 4, 3, 1, 1) == RANGE);
  CASE("check/voice_mask0", skred_fenv_check(r4, 4, K, 0, FMASK) == BAD);
  CASE("check/voice_mask_high", skred_fenv_check(r4, 4, K, 0x177, FMASK) == BAD);
  CASE("check/filter_mask0", skred_fenv_check(r4, 4, K, VMASK, 0) == BAD);
  CASE("check/filter_mask_high", skred_fenv_check(r4, 4, K, VMASK, 0x100) == BAD);
  CASE("check/k64_full_masks", skred_fenv_check(r4, 4, 64, ~0ull, ~0ull) == SKRED_OK && skred_fenv_check(r4, 4, 1, 1, 1) == SKRED_OK);
  CASE("check/unknown_bit", one(rec(A | 8u, 0, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f)) == BAD);
  CASE("check/abs_and_rel", one(both) == BAD);
  CASE("check/neither", one(rec(0, 0, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f)) == BAD && one(rec(S, 0.2f, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f)) == BAD);
  CASE("check/set_before_range", one(rec(A | R, 0, 9.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f)) == BAD);
  CASE("check/start_without_START", one(rec(A, 0.2f, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f)) == BAD && one(rec(R, NAN, 2.0f, 0.5f, 1.0f, 1.5f, 0.9f, 0.8f)) == BAD);
  CASE("check/start_before_box", one(rec(A, 0.2f, 9.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f)) == BAD);
  CASE("check/level_nan", one(rec(A, 0, NAN, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f)) == BAD && one(rec(A, 0, 2.0f, INFINITY, 0.1f, 1.5f, 0.9f, 0.8f)) == BAD &&
                          one(rec(R, 0, 2.0f, 0.5f, NAN, 1.5f, 0.9f, 0.8f)) == BAD && one(rec(A | S, NAN, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f)) == BAD);
  CASE("check/rate_nan", one(rec(A, 0, 2.0f, 0.5f, 0.1f, NAN, 0.9f, 0.8f)) == BAD && one(rec(A, 0, 2.0f, 0.5f, 0.1f, 1.5f, INFINITY, 0.8f)) == BAD &&
                         one(rec(A, 0, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, NAN)) == BAD);
  CASE("check/finite_before_box", one(rec(A, 0, 9.0f, 0.5f, 0.1f, NAN, 0.9f, 0.8f)) == BAD);
  CASE("check/abs_low", one(rec(A, 0, 2.0f, 0x1p-11f, 0.1f, 1.5f, 0.9f, 0.8f)) == RANGE && one(rec(A | S, 0.0f, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.8f)) == RANGE);
  CASE("check/abs_high", one(far) == RANGE && one(rec(A, 0, 2.0f, 0.5f, 3.0000002f, 1.5f, 0.9f, 0.8f)) == RANGE);
  CASE("check/abs_ends", one(r4[2]) == SKRED_OK);
  CASE("check/rel_value", one(rec(R, 0, 0.0f, 0.5f, 1.0f, 1.5f, 0.9f, 0.8f)) == RANGE && one(rec(R, 0, 2.0f, -0.5f, 1.0f, 1.5f, 0.9f, 0.8f)) == RANGE &&
                          one(rec(R | S, 0.0f, 2.0f, 0.5f, 1.0f, 1.5f, 0.9f, 0.8f)) == RANGE && one(r4[3]) == SKRED_OK);
  CASE("check/rate_box", one(rec(A, 0, 2.0f, 0.5f, 0.1f, 16.5f, 0.9f, 0.8f)) == RANGE && one(rec(A, 0, 2.0f, 0.5f, 0.1f, 1.5f, 0.03f, 0.8f)) == RANGE &&
                         one(rec(A, 0, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, 0.0f)) == RANGE && one(rec(A, 0, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, -2.0f)) == RANGE);
  CASE("check/rate_one", one(rec(A, 0, 2.0f, 0.5f, 0.1f, 1.0f, 0.9f, 0.8f)) == BAD && one(rec(A, 0, 2.0f, 0.5f, 0.1f, 1.5f, 1.0f, 0.8f)) == BAD &&
                         one(rec(A, 0, 2.0f, 0.5f, 0.1f, 1.5f, 0.9f, 1.0f)) == BAD);
  CASE("check/box_before_rate_one", one(rec(A, 0, 9.0f, 0.5f, 0.1f, 1.0f, 0.9f, 0.8f)) == RANGE && one(rec(A, 0, 2.0f, 0.5f, 0.1f, 1.0f, 0.9f, 17.0f)) == RANGE);
  CASE("check/rates_either_way", one(rec(A, 0, 2.0f, 0.5f, 0.1f, 0.5f, 2.0f, 2.0f)) == SKRED_OK && one(rec(A, 0, 2.0f, 0.5f, 0.1f, 1.0000001f, 0.99999994f, 0.5f)) == SKRED_OK);
  CASE("check/filter_outside_voice", skred_fenv_check(r4, 4, K, 0x11, FMASK) == BAD);
  CASE("check/record_before_subset", skred_fenv_check(&far, 1, K, 0x11, FMASK) == RANGE);
  CASE("check/third_record", skred_fenv_check(bad4, 4, K, VMASK, FMASK) == BAD && skred_fenv_check(bad4, 2, K, VMASK, FMASK) == SKRED_OK);

  /* the packing: 32 bytes, word for word */
  { sk_fenv_each_t out[3];
    memset(out, 0xEE, sizeof(out));
    skred_fenv_t in[2] = { good, relative };
    sk_fenv_pack(in, 2, NULL, out);
    CASE("pack/word_for_word", !memcmp(&out[0], &in[0], 32) && !memcmp(&out[1], &in[1], 32) && out[1].w[SK_FENV_E_SET] == (R | S));
    CASE("pack/n_records_only", out[2].w[0] == 0xEEEEEEEEu && out[2].w[7] == 0xEEEEEEEEu);
    const uint32_t rev[2] = { 1, 0 };
    sk_fenv_pack(in, 2, rev, out);
    CASE("pack/reversed", out[0].w[0] == (R | S) && out[1].w[0] == A); }
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
  CASE("match/null_bank", skred_bank_fenv_match(NULL, 0, N, K, FMASK, &chan, &good, res, NULL) == BAD);
  CASE("match/null_match", skred_bank_fenv_match(b, 0, N, K, FMASK, NULL, &good, res, NULL) == BAD);
  CASE("match/null_record", skred_bank_fenv_match(b, 0, N, K, FMASK, &chan, NULL, res, NULL) == BAD);
  CASE("match/null_before_k", skred_bank_fenv_match(b, 0, N, 3, FMASK, &chan, NULL, res, NULL) == BAD);
  CASE("match/k12", skred_bank_fenv_match(b, 0, N, 12, FMASK, &chan, &good, res, NULL) == RANGE);
  CASE("match/mask0", skred_bank_fenv_match(b, 0, N, K, 0, &chan, &good, res, NULL) == BAD);
  CASE("match/mask_high", skred_bank_fenv_match(b, 0, N, K, 0x1FF, &chan, &good, res, NULL) == BAD);
  CASE("match/mask_before_range", skred_bank_fenv_match(b, 4, 8, K, 0, &chan, &good, res, NULL) == BAD);
  CASE("match/first_off_slot", skred_bank_fenv_match(b, 4, 8, K, FMASK, &chan, &good, res, NULL) == RANGE);
  CASE("match/count_off_slot", skred_bank_fenv_match(b, 0, 12, K, FMASK, &chan, &good, res, NULL) == RANGE);
  CASE("match/past_the_bank", skred_bank_fenv_match(b, 0, N + K, K, FMASK, &chan, &good, res, NULL) == RANGE);
  CASE("match/empty_range", skred_bank_fenv_match(b, 0, 0, K, FMASK, &chan, &good, res, NULL) == RANGE);
  CASE("match/range_before_record", skred_bank_fenv_match(b, 4, 8, K, FMASK, &chan, &both, res, NULL) == RANGE);
  CASE("match/bad_set", skred_bank_fenv_match(b, 0, N, K, FMASK, &chan, &both, res, NULL) == BAD);
  CASE("match/out_of_box", skred_bank_fenv_match(b, 0, N, K, FMASK, &chan, &far, res, NULL) == RANGE);
  CASE("match/record_before_match", skred_bank_fenv_match(b, 0, N, K, FMASK, &wrong, &far, res, NULL) == RANGE);
  CASE("match/value_outside_mask", skred_bank_fenv_match(b, 0, N, K, FMASK, &wrong, &good, res, NULL) == BAD);
  CASE("owned/null_bank", skred_bank_fenv_owned_each(NULL, r4, K, FMASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_list", skred_bank_fenv_owned_each(b, r4, K, FMASK, NULL, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_tags", skred_bank_fenv_owned_each(b, r4, K, FMASK, list, NULL, 4, NULL, res, NULL) == BAD);
  CASE("owned/null_records", skred_bank_fenv_owned_each(b, NULL, K, FMASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/negative_n", skred_bank_fenv_owned_each(b, r4, K, FMASK, list, t4, -2, NULL, res, NULL) == BAD);
  CASE("owned/k12", skred_bank_fenv_owned_each(b, r4, 12, FMASK, list, t4, 4, NULL, res, NULL) == RANGE);
  CASE("owned/mask0", skred_bank_fenv_owned_each(b, r4, K, 0, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/mask_high", skred_bank_fenv_owned_each(b, r4, K, 0x1FF, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/bad_record", skred_bank_fenv_owned_each(b, bad4, K, FMASK, list, t4, 4, NULL, res, NULL) == BAD);
  CASE("owned/record_before_tag", skred_bank_fenv_owned_each(b, bad4, K, FMASK, list, z4, 4, NULL, res, NULL) == BAD);
  CASE("owned/zero_tag", skred_bank_fenv_owned_each(b, r4, K, FMASK, list, z4, 4, NULL, res, NULL) == BAD);
  CASE("owned/empty", skred_bank_fenv_owned_each(b, r4, K, FMASK, list, t4, 0, NULL, res, NULL) == SKRED_OK);
  CASE("tags/null_bank", skred_bank_fenv_tags_each(NULL, r4, 0, N, K, FMASK, t4, 4, res, NULL) == BAD);
  CASE("tags/null_tags", skred_bank_fenv_tags_each(b, r4, 0, N, K, FMASK, NULL, 4, res, NULL) == BAD);
  CASE("tags/null_records", skred_bank_fenv_tags_each(b, NULL, 0, N, K, FMASK, t4, 4, res, NULL) == BAD);
  CASE("tags/k3", skred_bank_fenv_tags_each(b, r4, 0, N, 3, 0x7, t4, 4, res, NULL) == RANGE);
  CASE("tags/mask_high", skred_bank_fenv_tags_each(b, r4, 0, N, K, 0x1FF, t4, 4, res, NULL) == BAD);
  CASE("tags/first_off_slot", skred_bank_fenv_tags_each(b, r4, 4, 8, K, FMASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/past_the_bank", skred_bank_fenv_tags_each(b, r4, 0, N + K, K, FMASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/empty_range", skred_bank_fenv_tags_each(b, r4, 0, 0, K, FMASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/range_before_record", skred_bank_fenv_tags_each(b, bad4, 4, 8, K, FMASK, t4, 4, res, NULL) == RANGE);
  CASE("tags/bad_record", skred_bank_fenv_tags_each(b, bad4, 0, N, K, FMASK, t4, 4, res, NULL) == BAD);
  CASE("tags/zero_tag", skred_bank_fenv_tags_each(b, r4, 0, N, K, FMASK, z4, 4, res, NULL) == BAD);
  CASE("tags/repeated_tag", skred_bank_fenv_tags_each(b, r4, 0, N, K, FMASK, d4, 4, res, NULL) == BAD);
  CASE("tags/too_many", skred_bank_fenv_tags_each(b, rmany, 0, N, K, FMASK, many, SKRED_OWNER_MAX_TAGS + 1, res, NULL) == BAD);
  CASE("tags/negative_n", skred_bank_fenv_tags_each(b, r4, 0, N, K, FMASK, t4, -1, res, NULL) == BAD);
  CASE("tags/empty", skred_bank_fenv_tags_each(b, r4, 0, N, K, FMASK, t4, 0, res, NULL) == SKRED_OK);
  CASE("download/null_bank", skred_bank_download_fenv(NULL, words, 0, 4) == BAD);
  CASE("download/null_out", skred_bank_download_fenv(b, NULL, 0, 4) == BAD);
  CASE("download/past_the_bank", skred_bank_download_fenv(b, words, N - 2, 4) == RANGE);
  CASE("download/empty", skred_bank_download_fenv(b, words, 0, 0) == SKRED_OK && words[0] == 7);
  { int zeros = skred_bank_download_fenv(b, words, N - 4, 3) == SKRED_OK;
    for (int k = 0; k < 24; k++) zeros = zeros && !words[k];
    CASE("download/no_array_yet_gives_zeros", zeros && words[24] == 7 && words[31] == 7); }

  CASE("untouched/outputs", res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && res[4] == 7 && list[0] == 0 && list[3] == 24);
  CASE("untouched/bank", b->touched_total == 0 && b->control_epoch == 0 && b->upd_seq == 0 && b->upd_head == 0 && !b->d_owner && !b->d_pedal &&
                         !b->d_glide && !b->d_bend && !b->d_cut && !b->d_fenv && !b->d_owner_slots);
  free(b);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
