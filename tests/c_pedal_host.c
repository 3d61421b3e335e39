/* The host side of the pedal calls without a device: skred_pedal_check, the packing of the pedal-up flags (every one of the sixteen
 * words over the three bits and one above them) and every refusal the entry points make before anything touches the device, on a
 * skred_bank_t that is nothing but its voice count (a refused call reads no other member).  One line per case, "OK" last.
 * tests/test_pedal_cpu.py builds and runs it; built together with skred_amd/csrc/skred_bank_pedal.c and -fsanitize=address,undefined it
 * is the sanitizer run of that file's host code -- from the repository root, after the library is built (the program's own copy of
 * skred_bank_pedal.c takes the place of the library's; everything else it calls comes from the library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_pedal_host.c skred_amd/csrc/skred_bank_pedal.c -o /tmp/c_pedal_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_pedal_host_san */
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
#define SO SKRED_PEDAL_CALL_STAMP_OWNED
#define RT SKRED_PEDAL_CALL_RELEASE_TAGS
#define LA SKRED_PEDAL_CALL_LATCH
#define UP SKRED_PEDAL_CALL_UP
#define SUS SKRED_PEDAL_LIFT_SUSTAIN
#define SOS SKRED_PEDAL_LIFT_SOSTENUTO
#define DOWN SKRED_PEDAL_SUSTAIN_DOWN

int main(void) {
  const skred_owner_match_t chan = { 0x03000000u, 0xFF000000u }, all = { 0, 0 }, off = { 0x03000001u, 0xFF000000u };
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0xFFFFFFFFu, 0x80000000u }, z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u };
  const uint32_t d4[4] = { 0x03000001u, 0x03000002u, 0x03000001u, 0x03000004u };
  static uint32_t many[SKRED_OWNER_MAX_TAGS + 1];
  for (int k = 0; k <= SKRED_OWNER_MAX_TAGS; k++) many[k] = 1u + (uint32_t)k;

  CASE("const/bits", SKRED_PEDAL_PENDING == 1 && SKRED_PEDAL_LATCHED == 2 && SUS == 1 && SOS == 2 && DOWN == 4);
  CASE("const/calls", SO == 0 && RT == 1 && LA == 2 && UP == 3);

  /* skred_pedal_check, call by call */
  CASE("check/stamp_plain", skred_pedal_check(SO, N, 0, 0, K, MASK, NULL, 0, t4, 4) == SKRED_OK);
  CASE("check/stamp_ignores_range_match_flags", skred_pedal_check(SO, N, -7, -9, K, MASK, &off, 99, t4, 4) == SKRED_OK);
  CASE("check/stamp_repeated_tag", skred_pedal_check(SO, N, 0, 0, K, MASK, NULL, 0, d4, 4) == SKRED_OK);
  CASE("check/stamp_more_than_max_tags", skred_pedal_check(SO, N, 0, 0, K, MASK, NULL, 0, many, SKRED_OWNER_MAX_TAGS + 1) == SKRED_OK);
  CASE("check/stamp_empty", skred_pedal_check(SO, N, 0, 0, K, MASK, NULL, 0, t4, 0) == SKRED_OK);
  CASE("check/stamp_null_tags", skred_pedal_check(SO, N, 0, 0, K, MASK, NULL, 0, NULL, 4) == BAD);
  CASE("check/stamp_negative_n", skred_pedal_check(SO, N, 0, 0, K, MASK, NULL, 0, t4, -1) == BAD);
  CASE("check/stamp_zero_tag", skred_pedal_check(SO, N, 0, 0, K, MASK, NULL, 0, z4, 4) == BAD);
  CASE("check/stamp_zero_tag_not_reached", skred_pedal_check(SO, N, 0, 0, K, MASK, NULL, 0, z4, 1) == SKRED_OK);
  CASE("check/stamp_k3", skred_pedal_check(SO, N, 0, 0, 3, 1, NULL, 0, t4, 4) == RANGE);
  CASE("check/stamp_k128", skred_pedal_check(SO, N, 0, 0, 128, 1, NULL, 0, t4, 4) == RANGE);
  CASE("check/stamp_mask0", skred_pedal_check(SO, N, 0, 0, K, 0, NULL, 0, t4, 4) == BAD);
  CASE("check/stamp_mask_high", skred_pedal_check(SO, N, 0, 0, K, 0x100, NULL, 0, t4, 4) == BAD);
  CASE("check/stamp_k64_full_mask", skred_pedal_check(SO, N, 0, 0, 64, ~0ull, NULL, 0, t4, 4) == SKRED_OK);
  CASE("check/release_plain", skred_pedal_check(RT, N, 0, N, K, MASK, NULL, 0, t4, 4) == SKRED_OK);
  CASE("check/release_ignores_match_flags", skred_pedal_check(RT, N, 0, N, K, MASK, &off, 99, t4, 4) == SKRED_OK);
  CASE("check/release_max_tags", skred_pedal_check(RT, N, 0, N, K, MASK, NULL, 0, many, SKRED_OWNER_MAX_TAGS) == SKRED_OK);
  CASE("check/release_too_many_tags", skred_pedal_check(RT, N, 0, N, K, MASK, NULL, 0, many, SKRED_OWNER_MAX_TAGS + 1) == BAD);
  CASE("check/release_repeated_tag", skred_pedal_check(RT, N, 0, N, K, MASK, NULL, 0, d4, 4) == BAD);
  CASE("check/release_zero_tag", skred_pedal_check(RT, N, 0, N, K, MASK, NULL, 0, z4, 4) == BAD);
  CASE("check/release_null_tags", skred_pedal_check(RT, N, 0, N, K, MASK, NULL, 0, NULL, 0) == BAD);
  CASE("check/release_first_off_slot", skred_pedal_check(RT, N, 4, 8, K, MASK, NULL, 0, t4, 4) == RANGE);
  CASE("check/release_count_off_slot", skred_pedal_check(RT, N, 0, 12, K, MASK, NULL, 0, t4, 4) == RANGE);
  CASE("check/release_empty_range", skred_pedal_check(RT, N, 8, 0, K, MASK, NULL, 0, t4, 4) == RANGE);
  CASE("check/release_past_the_bank", skred_pedal_check(RT, N, 8, N, K, MASK, NULL, 0, t4, 4) == RANGE);
  CASE("check/release_negative_first", skred_pedal_check(RT, N, -8, 16, K, MASK, NULL, 0, t4, 4) == RANGE);
  CASE("check/release_k3", skred_pedal_check(RT, N, 0, N, 3, 1, NULL, 0, t4, 4) == RANGE);
  CASE("check/release_mask0", skred_pedal_check(RT, N, 0, N, K, 0, NULL, 0, t4, 4) == BAD);
  CASE("check/release_range_before_mask", skred_pedal_check(RT, N, 4, 8, K, 0, NULL, 0, t4, 4) == RANGE);
  CASE("check/latch_plain", skred_pedal_check(LA, N, 0, N, K, MASK, &chan, 0, NULL, 0) == SKRED_OK);
  CASE("check/latch_ignores_tags_flags", skred_pedal_check(LA, N, 0, N, K, MASK, &all, 99, NULL, -4) == SKRED_OK);
  CASE("check/latch_null_match", skred_pedal_check(LA, N, 0, N, K, MASK, NULL, 0, NULL, 0) == BAD);
  CASE("check/latch_bad_match", skred_pedal_check(LA, N, 0, N, K, MASK, &off, 0, NULL, 0) == BAD);
  CASE("check/latch_mask0", skred_pedal_check(LA, N, 0, N, K, 0, &chan, 0, NULL, 0) == BAD);
  CASE("check/latch_mask_high", skred_pedal_check(LA, N, 0, N, K, 0x155, &chan, 0, NULL, 0) == BAD);
  CASE("check/latch_k0", skred_pedal_check(LA, N, 0, N, 0, 1, &chan, 0, NULL, 0) == RANGE);
  CASE("check/latch_one_slot", skred_pedal_check(LA, N, N - K, K, K, MASK, &chan, 0, NULL, 0) == SKRED_OK);
  CASE("check/latch_empty_range", skred_pedal_check(LA, N, 0, 0, K, MASK, &chan, 0, NULL, 0) == RANGE);
  CASE("check/latch_past_the_bank", skred_pedal_check(LA, N, 0, N + K, K, MASK, &chan, 0, NULL, 0) == RANGE);
  CASE("check/latch_first_off_slot", skred_pedal_check(LA, N, 4, 8, K, MASK, &chan, 0, NULL, 0) == RANGE);
  CASE("check/latch_bank_of_zero_voices", skred_pedal_check(LA, 0, 0, K, K, MASK, &chan, 0, NULL, 0) == RANGE);
  CASE("check/up_plain", skred_pedal_check(UP, N, 0, N, K, MASK, &chan, SUS, NULL, 0) == SKRED_OK);
  CASE("check/up_match_before_flags", skred_pedal_check(UP, N, 0, N, K, MASK, NULL, 0, NULL, 0) == BAD);
  CASE("check/up_flags_before_range", skred_pedal_check(UP, N, 4, 8, K, MASK, &chan, 0, NULL, 0) == BAD);
  CASE("check/up_first_off_slot", skred_pedal_check(UP, N, 4, 8, K, MASK, &chan, SOS, NULL, 0) == RANGE);
  CASE("check/up_mask0", skred_pedal_check(UP, N, 0, N, K, 0, &chan, SOS, NULL, 0) == BAD);
  CASE("check/unknown_call", skred_pedal_check(4, N, 0, N, K, MASK, &chan, SUS, t4, 4) == BAD);
  CASE("check/negative_call", skred_pedal_check(-1, N, 0, N, K, MASK, &chan, SUS, t4, 4) == BAD);

  /* the flag word: accepted exactly when it lifts a pedal, names no unknown bit and does not lift sustain while saying it stays down */
  for (uint32_t f = 0; f < 16; f++) {
    const int want = (f & ~7u) || !(f & (SUS | SOS)) || ((f & DOWN) && (f & SUS)) ? BAD : SKRED_OK;
    char name[32];
    snprintf(name, sizeof(name), "flags/0x%x", f);
    CASE(name, skred_pedal_check(UP, N, 0, N, K, MASK, &chan, f, NULL, 0) == want);
  }
  CASE("flags/accepted_set", skred_pedal_check(UP, N, 0, N, K, MASK, &chan, SUS, NULL, 0) == 0 && skred_pedal_check(UP, N, 0, N, K, MASK, &chan, SOS, NULL, 0) == 0 &&
                             skred_pedal_check(UP, N, 0, N, K, MASK, &chan, SUS | SOS, NULL, 0) == 0 &&
                             skred_pedal_check(UP, N, 0, N, K, MASK, &chan, SOS | DOWN, NULL, 0) == 0);
  CASE("flags/high_bit", skred_pedal_check(UP, N, 0, N, K, MASK, &chan, SUS | 0x80000000u, NULL, 0) == BAD);

  /* the entry points: a bank that is nothing but its size */
  skred_bank_t *b = (skred_bank_t *)calloc(1, sizeof(skred_bank_t));
  b->n_voices = N;
  int32_t list[4] = { 0, 8, 16, 24 };
  uint32_t res[4] = { 7, 7, 7, 7 }, words[4] = { 7, 7, 7, 7 };
  CASE("stamp/null_bank", skred_bank_stamp_owned_pedal(NULL, list, t4, 4, NULL, K, MASK, 1, res, NULL) == BAD);
  CASE("stamp/null_list", skred_bank_stamp_owned_pedal(b, NULL, t4, 4, NULL, K, MASK, 1, res, NULL) == BAD);
  CASE("stamp/null_result", skred_bank_stamp_owned_pedal(b, list, t4, 4, NULL, K, MASK, 1, NULL, NULL) == BAD);
  CASE("stamp/null_tags", skred_bank_stamp_owned_pedal(b, list, NULL, 4, NULL, K, MASK, 1, res, NULL) == BAD);
  CASE("stamp/zero_tag", skred_bank_stamp_owned_pedal(b, list, z4, 4, NULL, K, MASK, 0, res, NULL) == BAD);
  CASE("stamp/huge_n", skred_bank_stamp_owned_pedal(b, list, t4, -2, NULL, K, MASK, 0, res, NULL) == BAD);
  CASE("stamp/k12", skred_bank_stamp_owned_pedal(b, list, t4, 4, NULL, 12, MASK, 0, res, NULL) == RANGE);
  CASE("stamp/mask0", skred_bank_stamp_owned_pedal(b, list, t4, 4, NULL, K, 0, 0, res, NULL) == BAD);
  CASE("stamp/mask_high", skred_bank_stamp_owned_pedal(b, list, t4, 4, NULL, K, 0x1FF, 0, res, NULL) == BAD);
  CASE("stamp/empty", skred_bank_stamp_owned_pedal(b, list, t4, 0, NULL, K, MASK, 1, res, NULL) == SKRED_OK);
  CASE("release/null_bank", skred_bank_release_tags_pedal(NULL, 0, N, K, MASK, t4, 4, 1, res, NULL) == BAD);
  CASE("release/null_result", skred_bank_release_tags_pedal(b, 0, N, K, MASK, t4, 4, 1, NULL, NULL) == BAD);
  CASE("release/null_tags", skred_bank_release_tags_pedal(b, 0, N, K, MASK, NULL, 4, 1, res, NULL) == BAD);
  CASE("release/repeated_tag", skred_bank_release_tags_pedal(b, 0, N, K, MASK, d4, 4, 1, res, NULL) == BAD);
  CASE("release/zero_tag", skred_bank_release_tags_pedal(b, 0, N, K, MASK, z4, 4, 1, res, NULL) == BAD);
  CASE("release/too_many", skred_bank_release_tags_pedal(b, 0, N, K, MASK, many, SKRED_OWNER_MAX_TAGS + 1, 1, res, NULL) == BAD);
  CASE("release/first_off_slot", skred_bank_release_tags_pedal(b, 4, 8, K, MASK, t4, 4, 1, res, NULL) == RANGE);
  CASE("release/past_the_bank", skred_bank_release_tags_pedal(b, 0, N + K, K, MASK, t4, 4, 1, res, NULL) == RANGE);
  CASE("release/empty_range", skred_bank_release_tags_pedal(b, 0, 0, K, MASK, t4, 4, 1, res, NULL) == RANGE);
  CASE("release/k3", skred_bank_release_tags_pedal(b, 0, N, 3, 0x7, t4, 4, 1, res, NULL) == RANGE);
  CASE("release/mask_high", skred_bank_release_tags_pedal(b, 0, N, K, 0x1FF, t4, 4, 1, res, NULL) == BAD);
  CASE("release/empty", skred_bank_release_tags_pedal(b, 0, N, K, MASK, t4, 0, 1, res, NULL) == SKRED_OK);
  CASE("latch/null_bank", skred_bank_pedal_latch(NULL, 0, N, K, MASK, &chan, res, NULL) == BAD);
  CASE("latch/null_result", skred_bank_pedal_latch(b, 0, N, K, MASK, &chan, NULL, NULL) == BAD);
  CASE("latch/null_match", skred_bank_pedal_latch(b, 0, N, K, MASK, NULL, res, NULL) == BAD);
  CASE("latch/bad_match", skred_bank_pedal_latch(b, 0, N, K, MASK, &off, res, NULL) == BAD);
  CASE("latch/mask0", skred_bank_pedal_latch(b, 0, N, K, 0, &chan, res, NULL) == BAD);
  CASE("latch/k3", skred_bank_pedal_latch(b, 0, N, 3, 1, &chan, res, NULL) == RANGE);
  CASE("latch/first_off_slot", skred_bank_pedal_latch(b, 4, 8, K, MASK, &chan, res, NULL) == RANGE);
  CASE("latch/empty_range", skred_bank_pedal_latch(b, 0, 0, K, MASK, &chan, res, NULL) == RANGE);
  CASE("latch/past_the_bank", skred_bank_pedal_latch(b, N, K, K, MASK, &chan, res, NULL) == RANGE);
  CASE("up/null_bank", skred_bank_pedal_up(NULL, 0, N, K, MASK, &chan, SUS, res, NULL) == BAD);
  CASE("up/null_result", skred_bank_pedal_up(b, 0, N, K, MASK, &chan, SUS, NULL, NULL) == BAD);
  CASE("up/null_match", skred_bank_pedal_up(b, 0, N, K, MASK, NULL, SUS, res, NULL) == BAD);
  CASE("up/bad_match", skred_bank_pedal_up(b, 0, N, K, MASK, &off, SUS, res, NULL) == BAD);
  CASE("up/no_lift", skred_bank_pedal_up(b, 0, N, K, MASK, &chan, 0, res, NULL) == BAD);
  CASE("up/down_alone", skred_bank_pedal_up(b, 0, N, K, MASK, &chan, DOWN, res, NULL) == BAD);
  CASE("up/down_with_lift_sustain", skred_bank_pedal_up(b, 0, N, K, MASK, &chan, SUS | SOS | DOWN, res, NULL) == BAD);
  CASE("up/unknown_bit", skred_bank_pedal_up(b, 0, N, K, MASK, &chan, SUS | 8, res, NULL) == BAD);
  CASE("up/mask_high", skred_bank_pedal_up(b, 0, N, K, 0x100, &chan, SUS, res, NULL) == BAD);
  CASE("up/k128", skred_bank_pedal_up(b, 0, N, 128, 1, &chan, SUS, res, NULL) == RANGE);
  CASE("up/count_off_slot", skred_bank_pedal_up(b, 0, N - 4, K, MASK, &chan, SUS, res, NULL) == RANGE);
  CASE("up/past_the_bank", skred_bank_pedal_up(b, K, N, K, MASK, &chan, SUS, res, NULL) == RANGE);
  CASE("clear/null_bank", skred_bank_pedal_clear(NULL, 0, N, NULL) == BAD);
  CASE("clear/past_the_bank", skred_bank_pedal_clear(b, 8, N, NULL) == RANGE);
  CASE("clear/negative_count", skred_bank_pedal_clear(b, 0, -1, NULL) == RANGE);
  CASE("clear/no_array_yet", skred_bank_pedal_clear(b, 0, N, NULL) == SKRED_OK);
  CASE("download/null_bank", skred_bank_download_pedals(NULL, words, 0, 4) == BAD);
  CASE("download/null_out", skred_bank_download_pedals(b, NULL, 0, 4) == BAD);
  CASE("download/past_the_bank", skred_bank_download_pedals(b, words, N - 2, 4) == RANGE);
  CASE("download/empty", skred_bank_download_pedals(b, words, 0, 0) == SKRED_OK && words[0] == 7);
  CASE("download/no_array_yet_gives_zeros", skred_bank_download_pedals(b, words, N - 4, 3) == SKRED_OK && !words[0] && !words[1] && !words[2] && words[3] == 7);

  CASE("untouched/outputs", res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && list[0] == 0 && list[3] == 24);
  CASE("untouched/bank", b->touched_total == 0 && b->control_epoch == 0 && b->upd_seq == 0 && b->upd_head == 0 && !b->d_owner && !b->d_pedal &&
                         !b->d_owner_slots);
  free(b);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
