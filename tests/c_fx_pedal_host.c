/* The host side of the fixed-point pedal calls without a device: skred_fx_pedal_check against skred_pedal_check at one voice per slot
 * (codes and order), the pedal-up flag word, every refusal the entry points make before anything touches the device -- on a
 * skred_fxbank_t that is nothing but its voice count (a refused call reads no other member) -- and the layout the tags travel in
 * behind skred_fxbank_release_tags_pedal: sorted | permutation | the tags as given.  One line per case, "OK" last.
 * tests/test_fx_pedal_cpu.py builds and runs it; built together with skred_amd/csrc/skred_fx_pedal.c and
 * -fsanitize=address,undefined it is the sanitizer run of that file's host code -- from the repository root, after the library is
 * built (the program's own copy of skred_fx_pedal.c takes the place of the library's; everything else it calls comes from the
 * library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_fx_pedal_host.c skred_amd/csrc/skred_fx_pedal.c -o /tmp/c_fx_pedal_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_fx_pedal_host_san
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
#define SO SKRED_PEDAL_CALL_STAMP_OWNED
#define RT SKRED_PEDAL_CALL_RELEASE_TAGS
#define LA SKRED_PEDAL_CALL_LATCH
#define UP SKRED_PEDAL_CALL_UP
#define SUS SKRED_PEDAL_LIFT_SUSTAIN
#define SOS SKRED_PEDAL_LIFT_SOSTENUTO
#define DOWN SKRED_PEDAL_SUSTAIN_DOWN

/* both checks on the same arguments: the same code */
static int twin(int call, int n_voices, int first, int count, const skred_owner_match_t *m, uint32_t flags, const uint32_t *tags, int n,
                int want) {
  const int a = skred_fx_pedal_check(call, n_voices, first, count, m, flags, tags, n);
  const int b = skred_pedal_check(call, n_voices, first, count, 1, 1, m, flags, tags, n);
  return a == want && b == want;
}

int main(void) {
  const skred_owner_match_t chan = { 0x03000000u, 0xFF000000u }, all = { 0, 0 }, off = { 0x03000001u, 0xFF000000u };
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0xFFFFFFFFu, 0x80000000u }, z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u };
  const uint32_t d4[4] = { 0x03000001u, 0x03000002u, 0x03000001u, 0x03000004u };
  static uint32_t many[SKRED_OWNER_MAX_TAGS + 1];
  for (int k = 0; k <= SKRED_OWNER_MAX_TAGS; k++) many[k] = 1u + (uint32_t)k;

  CASE("const/bits", SKRED_PEDAL_PENDING == 1 && SKRED_PEDAL_LATCHED == 2 && SUS == 1 && SOS == 2 && DOWN == 4);
  CASE("const/calls", SO == 0 && RT == 1 && LA == 2 && UP == 3);

  /* skred_fx_pedal_check, call by call, each against the float bank's check at K = 1, voice_mask = 1 */
  CASE("check/stamp_plain", twin(SO, N, 0, 0, NULL, 0, t4, 4, SKRED_OK));
  CASE("check/stamp_ignores_range_match_flags", twin(SO, N, -7, -9, &off, 99, t4, 4, SKRED_OK));
  CASE("check/stamp_repeated_tag", twin(SO, N, 0, 0, NULL, 0, d4, 4, SKRED_OK));
  CASE("check/stamp_more_than_max_tags", twin(SO, N, 0, 0, NULL, 0, many, SKRED_OWNER_MAX_TAGS + 1, SKRED_OK));
  CASE("check/stamp_empty", twin(SO, N, 0, 0, NULL, 0, t4, 0, SKRED_OK));
  CASE("check/stamp_null_tags", twin(SO, N, 0, 0, NULL, 0, NULL, 4, BAD));
  CASE("check/stamp_negative_n", twin(SO, N, 0, 0, NULL, 0, t4, -1, BAD));
  CASE("check/stamp_zero_tag", twin(SO, N, 0, 0, NULL, 0, z4, 4, BAD));
  CASE("check/stamp_zero_tag_not_reached", twin(SO, N, 0, 0, NULL, 0, z4, 1, SKRED_OK));
  CASE("check/release_plain", twin(RT, N, 0, N, NULL, 0, t4, 4, SKRED_OK));
  CASE("check/release_off_the_wave_edge", twin(RT, N, 37, 500, NULL, 0, t4, 4, SKRED_OK));
  CASE("check/release_ignores_match_flags", twin(RT, N, 0, N, &off, 99, t4, 4, SKRED_OK));
  CASE("check/release_max_tags", twin(RT, N, 0, N, NULL, 0, many, SKRED_OWNER_MAX_TAGS, SKRED_OK));
  CASE("check/release_too_many_tags", twin(RT, N, 0, N, NULL, 0, many, SKRED_OWNER_MAX_TAGS + 1, BAD));
  CASE("check/release_repeated_tag", twin(RT, N, 0, N, NULL, 0, d4, 4, BAD));
  CASE("check/release_zero_tag", twin(RT, N, 0, N, NULL, 0, z4, 4, BAD));
  CASE("check/release_null_tags", twin(RT, N, 0, N, NULL, 0, NULL, 0, BAD));
  CASE("check/release_tags_before_range", twin(RT, N, 0, 0, NULL, 0, d4, 4, BAD));
  CASE("check/release_empty_range", twin(RT, N, 8, 0, NULL, 0, t4, 4, RANGE));
  CASE("check/release_negative_count", twin(RT, N, 8, -1, NULL, 0, t4, 4, RANGE));
  CASE("check/release_past_the_bank", twin(RT, N, 1, N, NULL, 0, t4, 4, RANGE));
  CASE("check/release_negative_first", twin(RT, N, -1, 16, NULL, 0, t4, 4, RANGE));
  CASE("check/latch_plain", twin(LA, N, 0, N, &chan, 0, NULL, 0, SKRED_OK));
  CASE("check/latch_ignores_tags_flags", twin(LA, N, 0, N, &all, 99, NULL, -4, SKRED_OK));
  CASE("check/latch_null_match", twin(LA, N, 0, N, NULL, 0, NULL, 0, BAD));
  CASE("check/latch_bad_match", twin(LA, N, 0, N, &off, 0, NULL, 0, BAD));
  CASE("check/latch_match_before_range", twin(LA, N, 0, 0, &off, 0, NULL, 0, BAD));
  CASE("check/latch_one_voice", twin(LA, N, N - 1, 1, &chan, 0, NULL, 0, SKRED_OK));
  CASE("check/latch_empty_range", twin(LA, N, 0, 0, &chan, 0, NULL, 0, RANGE));
  CASE("check/latch_past_the_bank", twin(LA, N, 0, N + 1, &chan, 0, NULL, 0, RANGE));
  CASE("check/latch_bank_of_zero_voices", twin(LA, 0, 0, 1, &chan, 0, NULL, 0, RANGE));
  CASE("check/up_plain", twin(UP, N, 0, N, &chan, SUS, NULL, 0, SKRED_OK));
  CASE("check/up_match_before_flags", twin(UP, N, 0, N, NULL, 0, NULL, 0, BAD));
  CASE("check/up_flags_before_range", twin(UP, N, 0, N + 1, &chan, 0, NULL, 0, BAD));
  CASE("check/up_past_the_bank", twin(UP, N, 0, N + 1, &chan, SOS, NULL, 0, RANGE));
  CASE("check/up_empty_range", twin(UP, N, 5, 0, &chan, SOS, NULL, 0, RANGE));
  CASE("check/unknown_call", twin(4, N, 0, N, &chan, SUS, t4, 4, BAD));
  CASE("check/negative_call", twin(-1, N, 0, N, &chan, SUS, t4, 4, BAD));

  /* the flag word: accepted exactly when it lifts a pedal, names no unknown bit and does not lift sustain while saying it stays down */
  for (uint32_t f = 0; f < 16; f++) {
    const int want = (f & ~7u) || !(f & (SUS | SOS)) || ((f & DOWN) && (f & SUS)) ? BAD : SKRED_OK;
    char name[32];
    snprintf(name, sizeof(name), "flags/0x%x", f);
    CASE(name, twin(UP, N, 0, N, &chan, f, NULL, 0, want));
  }
  CASE("flags/high_bit", twin(UP, N, 0, N, &chan, SUS | 0x80000000u, NULL, 0, BAD));

  /* what travels behind release_tags_pedal: sorted | perm | the tags as given (skx_owner_find_launch's slot, with_tags) */
  {
    uint32_t slot[12];
    const int rc = sk_owner_pack(t4, 4, slot, slot + 4);
    memcpy(slot + 8, t4, sizeof(t4));
    const uint32_t *sorted = slot, *perm = slot + 4, *given = slot + 8;
    int ok = rc == SKRED_OK, is_perm = 0;
    for (int j = 0; j < 4; j++) {
      ok = ok && perm[j] < 4 && sorted[j] == t4[perm[j]] && (j == 0 || sorted[j - 1] < sorted[j]) && given[j] == t4[j];
      if (perm[j] < 4) is_perm |= 1 << perm[j];
    }
    CASE("pack/sorted_unsigned_ascending", ok && sorted[0] == 0x03000001u && sorted[2] == 0x80000000u && sorted[3] == 0xFFFFFFFFu);
    CASE("pack/permutation", is_perm == 15 && perm[2] == 3 && perm[3] == 2);
    CASE("pack/tags_as_given_third", given[2] == 0xFFFFFFFFu && given[3] == 0x80000000u);
    uint32_t *big = (uint32_t *)malloc(3 * (size_t)SKRED_OWNER_MAX_TAGS * sizeof(uint32_t));
    uint32_t *rev = (uint32_t *)malloc((size_t)SKRED_OWNER_MAX_TAGS * sizeof(uint32_t));
    for (int k = 0; k < SKRED_OWNER_MAX_TAGS; k++) rev[k] = many[SKRED_OWNER_MAX_TAGS - 1 - k];
    (void)sk_owner_pack(rev, SKRED_OWNER_MAX_TAGS, big, big + SKRED_OWNER_MAX_TAGS);
    memcpy(big + 2 * SKRED_OWNER_MAX_TAGS, rev, (size_t)SKRED_OWNER_MAX_TAGS * sizeof(uint32_t));
    ok = 1;
    for (int j = 0; j < SKRED_OWNER_MAX_TAGS; j++)
      ok = ok && big[j] == 1u + (uint32_t)j && big[SKRED_OWNER_MAX_TAGS + j] == (uint32_t)(SKRED_OWNER_MAX_TAGS - 1 - j) &&
           big[2 * SKRED_OWNER_MAX_TAGS + j] == rev[j];
    CASE("pack/max_tags_reversed", ok);
    free(big);
    free(rev);
  }

  /* the entry points: a bank that is nothing but its size */
  skred_fxbank_t *fx = (skred_fxbank_t *)calloc(1, sizeof(skred_fxbank_t));
  fx->n_voices = N;
  int32_t list[4] = { 0, 8, 16, 24 };
  uint32_t res[4] = { 7, 7, 7, 7 }, words[4] = { 7, 7, 7, 7 };
  CASE("stamp/null_bank", skred_fxbank_stamp_owned_pedal(NULL, list, t4, 4, NULL, 1, res, NULL) == BAD);
  CASE("stamp/null_list", skred_fxbank_stamp_owned_pedal(fx, NULL, t4, 4, NULL, 1, res, NULL) == BAD);
  CASE("stamp/null_result", skred_fxbank_stamp_owned_pedal(fx, list, t4, 4, NULL, 1, NULL, NULL) == BAD);
  CASE("stamp/null_tags", skred_fxbank_stamp_owned_pedal(fx, list, NULL, 4, NULL, 1, res, NULL) == BAD);
  CASE("stamp/zero_tag", skred_fxbank_stamp_owned_pedal(fx, list, z4, 4, NULL, 0, res, NULL) == BAD);
  CASE("stamp/negative_n", skred_fxbank_stamp_owned_pedal(fx, list, t4, -2, NULL, 0, res, NULL) == BAD);
  CASE("stamp/empty", skred_fxbank_stamp_owned_pedal(fx, list, t4, 0, NULL, 1, res, NULL) == SKRED_OK);
  CASE("release/null_bank", skred_fxbank_release_tags_pedal(NULL, 0, N, t4, 4, 1, res, NULL) == BAD);
  CASE("release/null_result", skred_fxbank_release_tags_pedal(fx, 0, N, t4, 4, 1, NULL, NULL) == BAD);
  CASE("release/null_tags", skred_fxbank_release_tags_pedal(fx, 0, N, NULL, 4, 1, res, NULL) == BAD);
  CASE("release/repeated_tag", skred_fxbank_release_tags_pedal(fx, 0, N, d4, 4, 1, res, NULL) == BAD);
  CASE("release/zero_tag", skred_fxbank_release_tags_pedal(fx, 0, N, z4, 4, 1, res, NULL) == BAD);
  CASE("release/too_many", skred_fxbank_release_tags_pedal(fx, 0, N, many, SKRED_OWNER_MAX_TAGS + 1, 1, res, NULL) == BAD);
  CASE("release/tags_before_range", skred_fxbank_release_tags_pedal(fx, 0, N + 1, d4, 4, 1, res, NULL) == BAD);
  CASE("release/past_the_bank", skred_fxbank_release_tags_pedal(fx, 0, N + 1, t4, 4, 1, res, NULL) == RANGE);
  CASE("release/empty_range", skred_fxbank_release_tags_pedal(fx, 0, 0, t4, 4, 1, res, NULL) == RANGE);
  CASE("release/negative_first", skred_fxbank_release_tags_pedal(fx, -1, 4, t4, 4, 1, res, NULL) == RANGE);
  CASE("release/range_before_empty_list", skred_fxbank_release_tags_pedal(fx, 0, N + 1, t4, 0, 1, res, NULL) == RANGE);
  CASE("release/empty", skred_fxbank_release_tags_pedal(fx, 0, N, t4, 0, 1, res, NULL) == SKRED_OK);
  CASE("latch/null_bank", skred_fxbank_pedal_latch(NULL, 0, N, &chan, res, NULL) == BAD);
  CASE("latch/null_result", skred_fxbank_pedal_latch(fx, 0, N, &chan, NULL, NULL) == BAD);
  CASE("latch/null_match", skred_fxbank_pedal_latch(fx, 0, N, NULL, res, NULL) == BAD);
  CASE("latch/bad_match", skred_fxbank_pedal_latch(fx, 0, N, &off, res, NULL) == BAD);
  CASE("latch/match_before_range", skred_fxbank_pedal_latch(fx, 0, 0, &off, res, NULL) == BAD);
  CASE("latch/empty_range", skred_fxbank_pedal_latch(fx, 0, 0, &chan, res, NULL) == RANGE);
  CASE("latch/past_the_bank", skred_fxbank_pedal_latch(fx, N, 1, &chan, res, NULL) == RANGE);
  CASE("latch/negative_first", skred_fxbank_pedal_latch(fx, -1, 2, &chan, res, NULL) == RANGE);
  CASE("up/null_bank", skred_fxbank_pedal_up(NULL, 0, N, &chan, SUS, res, NULL) == BAD);
  CASE("up/null_result", skred_fxbank_pedal_up(fx, 0, N, &chan, SUS, NULL, NULL) == BAD);
  CASE("up/null_match", skred_fxbank_pedal_up(fx, 0, N, NULL, SUS, res, NULL) == BAD);
  CASE("up/bad_match", skred_fxbank_pedal_up(fx, 0, N, &off, SUS, res, NULL) == BAD);
  CASE("up/no_lift", skred_fxbank_pedal_up(fx, 0, N, &chan, 0, res, NULL) == BAD);
  CASE("up/down_alone", skred_fxbank_pedal_up(fx, 0, N, &chan, DOWN, res, NULL) == BAD);
  CASE("up/down_with_lift_sustain", skred_fxbank_pedal_up(fx, 0, N, &chan, SUS | SOS | DOWN, res, NULL) == BAD);
  CASE("up/unknown_bit", skred_fxbank_pedal_up(fx, 0, N, &chan, SUS | 8, res, NULL) == BAD);
  CASE("up/flags_before_range", skred_fxbank_pedal_up(fx, 0, N + 1, &chan, SUS | 8, res, NULL) == BAD);
  CASE("up/empty_range", skred_fxbank_pedal_up(fx, 0, 0, &chan, SUS, res, NULL) == RANGE);
  CASE("up/past_the_bank", skred_fxbank_pedal_up(fx, 1, N, &chan, SUS, res, NULL) == RANGE);
  CASE("clear/null_bank", skred_fxbank_pedal_clear(NULL, 0, N, NULL) == BAD);
  CASE("clear/past_the_bank", skred_fxbank_pedal_clear(fx, 8, N, NULL) == RANGE);
  CASE("clear/negative_count", skred_fxbank_pedal_clear(fx, 0, -1, NULL) == RANGE);
  CASE("clear/no_array_yet", skred_fxbank_pedal_clear(fx, 0, N, NULL) == SKRED_OK);
  CASE("download/null_bank", skred_fxbank_download_pedals(NULL, words, 0, 4) == BAD);
  CASE("download/null_out", skred_fxbank_download_pedals(fx, NULL, 0, 4) == BAD);
  CASE("download/negative_count", skred_fxbank_download_pedals(fx, words, 0, -1) == BAD);
  CASE("download/past_the_bank", skred_fxbank_download_pedals(fx, words, N - 2, 4) == RANGE);
  CASE("download/empty", skred_fxbank_download_pedals(fx, words, 0, 0) == SKRED_OK && words[0] == 7);
  CASE("download/no_array_yet_gives_zeros", skred_fxbank_download_pedals(fx, words, N - 4, 3) == SKRED_OK && !words[0] && !words[1] && !words[2] && words[3] == 7);

  CASE("untouched/outputs", res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && list[0] == 0 && list[3] == 24);
  CASE("untouched/bank", fx->ring_head == 0 && !fx->d_owner && !fx->d_pedal && !fx->d_owner_found && fx->count == 0 && !fx->ring[0].in_flight);
  free(fx);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
