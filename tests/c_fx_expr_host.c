/* The host side of channels and per-note expression on the fixed-point bank without a device: skred_fx_ctl_each_check, the
 * 32-byte packing of the entries (skx_each_pack), the sort-plus-permutation skred_fxbank_ctl_tags_each ships (sk_owner_pack with
 * skx_each_pack) and every refusal the entry points make before anything touches the device, on a skred_fxbank_t that is nothing
 * but its voice count (a refused call reads no other member).  One line per case, "OK" last.  tests/test_fx_expr_cpu.py builds and
 * runs it; built together with skred_amd/csrc/skred_fx_expr.c and the checks it shares with the float bank under
 * -fsanitize=address,undefined it is the sanitizer run of that file's host code -- from the repository root, after the library is
 * built (the program's own copy of skred_fx_expr.c and skred_bank_checks.c takes the place of the library's; everything else it
 * calls comes from the library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_fx_expr_host.c skred_amd/csrc/skred_fx_expr.c skred_amd/csrc/skred_bank_checks.c \
 *       -o /tmp/c_fx_expr_host_san -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_fx_expr_host_san */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_fxbank_priv.h"

static int failures;
#define CASE(name, cond) do { const int ok_ = (cond); printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); failures += !ok_; } while (0)
#define BAD SKRED_E_BAD_ARG
#define RNG SKRED_E_RANGE

static uint32_t *make_tags(int n) {
  uint32_t *t = (uint32_t *)malloc((size_t)(n > 0 ? n : 1) * sizeof(uint32_t));
  for (int k = 0; k < n; k++) t[k] = (1u + ((uint32_t)k * 7919u) % 1031u) | ((k & 1) ? 0x80000000u : 0u);   /* (1031 is prime: distinct for k < 1031) */
  if (n > 1) t[0] = 0xFFFFFFFFu;
  return t;
}

static skred_fx_ctl_each_t entry(uint32_t set) {
  skred_fx_ctl_each_t e;
  memset(&e, 0, sizeof(e));
  e.set = set;
  e.inc_scale_q16 = 69433; e.amp_scale_q16 = 32768; e.velocity_q15 = 65535; e.pan_left_q15 = 0; e.pan_right_q15 = 65535;
  return e;
}

/* what _ctl_tags_each ships: the tags sorted ascending as unsigned numbers, entry j = each[perm[j]] -- each[k] stays with tags[k] */
static int perm_ok(int n) {
  uint32_t *t = make_tags(n);
  uint32_t *sorted = (uint32_t *)malloc((size_t)n * sizeof(uint32_t)), *perm = (uint32_t *)malloc((size_t)n * sizeof(uint32_t));
  skred_fx_ctl_each_t *each = (skred_fx_ctl_each_t *)malloc((size_t)n * sizeof(*each));
  skx_each_t *out = (skx_each_t *)malloc((size_t)n * sizeof(*out));
  for (int k = 0; k < n; k++) { each[k] = entry(SKRED_EACH_VELOCITY | SKRED_EACH_INC_SCALE); each[k].velocity_q15 = k; each[k].inc_scale_q16 = t[k]; }
  int ok = sk_owner_pack(t, n, sorted, perm) == 0;
  skx_each_pack(each, n, perm, out);
  for (int j = 0; j < n && ok; j++)
    ok = perm[j] < (uint32_t)n && sorted[j] == t[perm[j]] && (j == 0 || sorted[j - 1] < sorted[j]) && out[j].w[SKX_EACH_W_VELOCITY] == perm[j] &&
         out[j].w[SKX_EACH_W_INC_SCALE] == sorted[j] && out[j].w[SKX_EACH_SET] == (SKRED_EACH_VELOCITY | SKRED_EACH_INC_SCALE);
  free(out); free(each); free(perm); free(sorted); free(t);
  return ok;
}

int main(void) {
  CASE("const/record", sizeof(skred_fx_ctl_each_t) == 32 && sizeof(skx_each_t) == 32 && SKX_EACH_WORDS == 8 && sizeof(skred_owner_match_t) == 8);
  CASE("const/bits", SKRED_EACH_INC_SCALE == 1 && SKRED_EACH_AMP_SCALE == 2 && SKRED_EACH_VELOCITY == 4 && SKRED_EACH_PAN == 8 && SKX_EACH_ALL == 15);
  CASE("const/offsets", offsetof(skred_fx_ctl_each_t, set) == 0 && offsetof(skred_fx_ctl_each_t, inc_scale_q16) == 4 &&
                        offsetof(skred_fx_ctl_each_t, amp_scale_q16) == 8 && offsetof(skred_fx_ctl_each_t, velocity_q15) == 12 &&
                        offsetof(skred_fx_ctl_each_t, pan_left_q15) == 16 && offsetof(skred_fx_ctl_each_t, pan_right_q15) == 20 &&
                        offsetof(skred_fx_ctl_each_t, reserved) == 24);

  /* ---- skred_fx_ctl_each_check: every refusal beside the accepted edge */
  skred_fx_ctl_t amp, pan, inc, bad;
  memset(&amp, 0, sizeof(amp)); amp.which = SKRED_CTL_AMP; amp.amp_q15 = 30000;
  memset(&pan, 0, sizeof(pan)); pan.which = SKRED_CTL_PAN; pan.pan_left_q15 = 100; pan.pan_right_q15 = 200;
  memset(&inc, 0, sizeof(inc)); inc.which = SKRED_CTL_PHASE_INC; inc.phase_inc = 1000;
  bad = pan; bad.which |= SKRED_CTL_FM_DEPTH;
  skred_fx_ctl_each_t e = entry(SKX_EACH_ALL), two[2];
  CASE("check/all_values_at_their_edges", skred_fx_ctl_each_check(&e, 1, &amp) == SKRED_OK);
  CASE("check/null_each", skred_fx_ctl_each_check(NULL, 1, &amp) == BAD && skred_fx_ctl_each_check(NULL, 0, NULL) == BAD);
  CASE("check/negative_n", skred_fx_ctl_each_check(&e, -1, &amp) == BAD);
  CASE("check/empty", skred_fx_ctl_each_check(&e, 0, NULL) == SKRED_OK);
  CASE("check/bad_ctl", skred_fx_ctl_each_check(&e, 1, &bad) == BAD && skred_fx_ctl_each_check(&e, 0, &bad) == BAD);
  e = entry(1u << 4);
  CASE("check/unknown_bit", skred_fx_ctl_each_check(&e, 1, &amp) == BAD);
  e = entry(0);
  CASE("check/set0", skred_fx_ctl_each_check(&e, 1, &amp) == BAD);
  e = entry(SKRED_EACH_PAN); e.reserved[0] = 1;
  CASE("check/reserved0", skred_fx_ctl_each_check(&e, 1, NULL) == BAD);
  e = entry(SKRED_EACH_PAN); e.reserved[1] = 1;
  CASE("check/reserved1", skred_fx_ctl_each_check(&e, 1, NULL) == BAD);
  e = entry(SKRED_EACH_VELOCITY); e.velocity_q15 = 65536;
  CASE("check/velocity_high", skred_fx_ctl_each_check(&e, 1, NULL) == BAD);
  e.velocity_q15 = -1;
  CASE("check/velocity_negative", skred_fx_ctl_each_check(&e, 1, NULL) == BAD);
  e.set = SKRED_EACH_PAN;
  CASE("check/velocity_unnamed", skred_fx_ctl_each_check(&e, 1, NULL) == SKRED_OK);
  e = entry(SKRED_EACH_VELOCITY); e.velocity_q15 = 0;
  CASE("check/velocity0", skred_fx_ctl_each_check(&e, 1, NULL) == SKRED_OK);
  e = entry(SKRED_EACH_PAN); e.pan_left_q15 = 65536;
  CASE("check/pan_left_high", skred_fx_ctl_each_check(&e, 1, NULL) == BAD);
  e = entry(SKRED_EACH_PAN); e.pan_right_q15 = -1;
  CASE("check/pan_right_negative", skred_fx_ctl_each_check(&e, 1, NULL) == BAD);
  e = entry(SKRED_EACH_AMP_SCALE); e.amp_scale_q16 = 0;
  CASE("check/amp_scale0", skred_fx_ctl_each_check(&e, 1, &amp) == BAD);
  e.set = SKRED_EACH_VELOCITY;
  CASE("check/amp_scale0_unnamed", skred_fx_ctl_each_check(&e, 1, &amp) == SKRED_OK);
  e = entry(SKRED_EACH_AMP_SCALE); e.amp_scale_q16 = 0xFFFFFFFFu;
  CASE("check/amp_scale_max", skred_fx_ctl_each_check(&e, 1, &amp) == SKRED_OK);
  CASE("check/amp_scale_without_ctl", skred_fx_ctl_each_check(&e, 1, NULL) == BAD);
  CASE("check/amp_scale_without_amp", skred_fx_ctl_each_check(&e, 1, &pan) == BAD);
  e = entry(SKRED_EACH_INC_SCALE); e.inc_scale_q16 = 0;
  CASE("check/inc_scale_any_value", skred_fx_ctl_each_check(&e, 1, &pan) == SKRED_OK && skred_fx_ctl_each_check(&e, 1, NULL) == SKRED_OK);
  CASE("check/inc_scale_with_phase_inc", skred_fx_ctl_each_check(&e, 1, &inc) == BAD);
  inc.which = SKRED_CTL_INC_SCALE; inc.inc_scale_q16 = 65536;
  CASE("check/inc_scale_with_inc_scale", skred_fx_ctl_each_check(&e, 1, &inc) == BAD);
  e.set = SKRED_EACH_PAN;
  CASE("check/pan_with_inc_scale_record", skred_fx_ctl_each_check(&e, 1, &inc) == SKRED_OK);
  two[0] = entry(SKRED_EACH_PAN); two[1] = entry(0);
  CASE("check/second_entry_bad", skred_fx_ctl_each_check(two, 2, NULL) == BAD && skred_fx_ctl_each_check(two, 1, NULL) == SKRED_OK);

  /* ---- the entries as they travel: 32 bytes, the named values word for word, the others zeroed */
  skx_each_t p[2];
  e = entry(SKX_EACH_ALL);
  memset(p, 0xAB, sizeof(p));
  skx_each_pack(&e, 1, NULL, p);
  CASE("pack/word_for_word", memcmp(&p[0], &e, 32) == 0 && p[1].w[0] == 0xABABABABu);
  e.set = SKRED_EACH_PAN; e.reserved[0] = 0;
  skx_each_pack(&e, 1, NULL, p);
  CASE("pack/unnamed_values_never_travel", p[0].w[SKX_EACH_SET] == SKRED_EACH_PAN && p[0].w[SKX_EACH_W_INC_SCALE] == 0 && p[0].w[SKX_EACH_W_AMP_SCALE] == 0 &&
                                            p[0].w[SKX_EACH_W_VELOCITY] == 0 && p[0].w[SKX_EACH_W_PAN_LEFT] == 0 && p[0].w[SKX_EACH_W_PAN_RIGHT] == 65535 &&
                                            p[0].w[6] == 0 && p[0].w[7] == 0);
  two[0] = entry(SKRED_EACH_VELOCITY); two[0].velocity_q15 = 11; two[1] = entry(SKRED_EACH_VELOCITY); two[1].velocity_q15 = 22;
  const uint32_t swap[2] = { 1, 0 };
  skx_each_pack(two, 2, swap, p);
  CASE("pack/permuted", p[0].w[SKX_EACH_W_VELOCITY] == 22 && p[1].w[SKX_EACH_W_VELOCITY] == 11);
  CASE("perm/1", perm_ok(1));
  CASE("perm/2", perm_ok(2));
  CASE("perm/3", perm_ok(3));
  CASE("perm/1023", perm_ok(1023));
  CASE("perm/1024", perm_ok(1024));

  /* ---- the entry points: a bank that is nothing but its size */
  skred_fxbank_t *fx = (skred_fxbank_t *)calloc(1, sizeof(skred_fxbank_t));
  fx->n_voices = 300;
  int32_t list[4] = { 0, 8, -1, 299 };
  uint32_t res[3] = { 0, 0, 0 };
  int total = -5;
  const uint32_t t4[4] = { 1, 2, 3, 0xFFFFFFFFu }, z4[4] = { 1, 0, 3, 4 }, d4[4] = { 1, 2, 1, 4 };
  const uint32_t REL = SKRED_STAMP_RELEASE;
  const skred_owner_match_t chan = { 0x03000000u, 0xFF000000u }, everyone = { 0, 0 }, nobody = { 0x03000001u, 0xFF000000u };
  uint32_t *many = make_tags(1025);
  skred_fx_ctl_each_t e4[4], *e1025 = (skred_fx_ctl_each_t *)malloc(1025 * sizeof(*e1025));
  for (int k = 0; k < 4; k++) e4[k] = entry(SKRED_EACH_PAN | SKRED_EACH_VELOCITY);
  for (int k = 0; k < 1025; k++) e1025[k] = entry(SKRED_EACH_PAN);

  CASE("find/null_bank", skred_fxbank_find_match(NULL, 0, 300, &chan, 4, list, res, NULL) == BAD);
  CASE("find/null_match", skred_fxbank_find_match(fx, 0, 300, NULL, 4, list, res, NULL) == BAD);
  CASE("find/value_outside_mask", skred_fxbank_find_match(fx, 0, 300, &nobody, 4, list, res, NULL) == BAD);
  CASE("find/null_count", skred_fxbank_find_match(fx, 0, 300, &chan, 4, list, NULL, NULL) == BAD);
  CASE("find/negative_max_out", skred_fxbank_find_match(fx, 0, 300, &chan, -1, list, res, NULL) == BAD);
  CASE("find/null_list", skred_fxbank_find_match(fx, 0, 300, &everyone, 4, NULL, res, NULL) == BAD);
  CASE("find/count_zero", skred_fxbank_find_match(fx, 8, 0, &chan, 4, list, res, NULL) == RNG);
  CASE("find/count_negative", skred_fxbank_find_match(fx, 8, -8, &chan, 4, list, res, NULL) == RNG);
  CASE("find/first_negative", skred_fxbank_find_match(fx, -1, 8, &chan, 4, list, res, NULL) == RNG);
  CASE("find/first_at_the_end", skred_fxbank_find_match(fx, 300, 1, &chan, 4, list, res, NULL) == RNG);
  CASE("find/past_the_bank", skred_fxbank_find_match(fx, 299, 2, &chan, 0, NULL, res, NULL) == RNG);
  CASE("find/huge_count", skred_fxbank_find_match(fx, 8, INT32_MAX, &chan, 4, list, res, NULL) == RNG);

  CASE("find_host/null_bank", skred_fxbank_find_match_host(NULL, 0, 300, &chan, 4, list, &total, NULL) == BAD);
  CASE("find_host/null_match", skred_fxbank_find_match_host(fx, 0, 300, NULL, 4, list, &total, NULL) == BAD);
  CASE("find_host/value_outside_mask", skred_fxbank_find_match_host(fx, 0, 300, &nobody, 4, list, NULL, NULL) == BAD);
  CASE("find_host/negative_max_out", skred_fxbank_find_match_host(fx, 0, 300, &chan, -1, list, &total, NULL) == BAD);
  CASE("find_host/null_list", skred_fxbank_find_match_host(fx, 0, 300, &chan, 1, NULL, &total, NULL) == BAD);
  CASE("find_host/count_zero", skred_fxbank_find_match_host(fx, 0, 0, &chan, 4, list, &total, NULL) == RNG);
  CASE("find_host/past_the_bank", skred_fxbank_find_match_host(fx, 0, 301, &chan, 0, NULL, NULL, NULL) == RNG);
  CASE("find_host/total_untouched", total == -5);

  CASE("stamp/null_bank", skred_fxbank_stamp_match(NULL, 0, 300, &chan, REL, res, NULL) == BAD);
  CASE("stamp/null_match", skred_fxbank_stamp_match(fx, 0, 300, NULL, REL, res, NULL) == BAD);
  CASE("stamp/value_outside_mask", skred_fxbank_stamp_match(fx, 0, 300, &nobody, REL, res, NULL) == BAD);
  CASE("stamp/null_result", skred_fxbank_stamp_match(fx, 0, 300, &chan, REL, NULL, NULL) == BAD);
  CASE("stamp/no_stamp_bit", skred_fxbank_stamp_match(fx, 0, 300, &chan, 0, res, NULL) == BAD);
  CASE("stamp/other_bits", skred_fxbank_stamp_match(fx, 0, 300, &chan, REL | 1, res, NULL) == BAD);
  CASE("stamp/count_zero", skred_fxbank_stamp_match(fx, 0, 0, &chan, REL, res, NULL) == RNG);
  CASE("stamp/past_the_bank", skred_fxbank_stamp_match(fx, 1, 300, &chan, REL, res, NULL) == RNG);

  CASE("ctlmatch/null_bank", skred_fxbank_ctl_match(NULL, &pan, 0, 300, &chan, res, NULL) == BAD);
  CASE("ctlmatch/null_ctl", skred_fxbank_ctl_match(fx, NULL, 0, 300, &chan, res, NULL) == BAD);
  CASE("ctlmatch/bad_ctl", skred_fxbank_ctl_match(fx, &bad, 0, 300, &chan, res, NULL) == BAD);
  CASE("ctlmatch/null_match", skred_fxbank_ctl_match(fx, &pan, 0, 300, NULL, res, NULL) == BAD);
  CASE("ctlmatch/value_outside_mask", skred_fxbank_ctl_match(fx, &pan, 0, 300, &nobody, NULL, NULL) == BAD);
  CASE("ctlmatch/count_zero", skred_fxbank_ctl_match(fx, &pan, 300, 0, &chan, NULL, NULL) == RNG);
  CASE("ctlmatch/first_negative", skred_fxbank_ctl_match(fx, &pan, -1, 2, &chan, NULL, NULL) == RNG);
  CASE("ctlmatch/past_the_bank", skred_fxbank_ctl_match(fx, &pan, 299, 2, &chan, NULL, NULL) == RNG);

  CASE("each/null_bank", skred_fxbank_ctl_owned_each(NULL, &pan, e4, list, t4, 4, NULL, NULL, NULL) == BAD);
  CASE("each/null_list", skred_fxbank_ctl_owned_each(fx, &pan, e4, NULL, t4, 4, NULL, NULL, NULL) == BAD);
  CASE("each/null_tags", skred_fxbank_ctl_owned_each(fx, &pan, e4, list, NULL, 4, NULL, NULL, NULL) == BAD);
  CASE("each/null_entries", skred_fxbank_ctl_owned_each(fx, &pan, NULL, list, t4, 4, NULL, NULL, NULL) == BAD);
  CASE("each/zero_tag", skred_fxbank_ctl_owned_each(fx, &pan, e4, list, z4, 4, NULL, NULL, NULL) == BAD);
  CASE("each/negative_n", skred_fxbank_ctl_owned_each(fx, &pan, e4, list, t4, -1, NULL, NULL, NULL) == BAD);
  CASE("each/huge_n", skred_fxbank_ctl_owned_each(fx, &pan, e4, list, t4, INT32_MAX / 64 + 1, NULL, NULL, NULL) == BAD);
  CASE("each/bad_ctl", skred_fxbank_ctl_owned_each(fx, &bad, e4, list, t4, 4, NULL, NULL, NULL) == BAD);
  e4[3].set = 0;
  CASE("each/bad_entry", skred_fxbank_ctl_owned_each(fx, &pan, e4, list, t4, 4, NULL, NULL, NULL) == BAD);
  e4[3] = entry(SKRED_EACH_AMP_SCALE);
  CASE("each/amp_scale_without_ctl", skred_fxbank_ctl_owned_each(fx, NULL, e4, list, t4, 4, NULL, NULL, NULL) == BAD);
  CASE("each/amp_scale_without_amp", skred_fxbank_ctl_owned_each(fx, &pan, e4, list, t4, 4, NULL, NULL, NULL) == BAD);
  e4[3] = entry(SKRED_EACH_INC_SCALE);
  CASE("each/inc_scale_on_an_increment", skred_fxbank_ctl_owned_each(fx, &inc, e4, list, t4, 4, NULL, NULL, NULL) == BAD);
  CASE("each/empty", skred_fxbank_ctl_owned_each(fx, NULL, e4, list, d4, 0, NULL, NULL, NULL) == SKRED_OK);

  e4[3] = entry(SKRED_EACH_PAN);
  CASE("tags/null_bank", skred_fxbank_ctl_tags_each(NULL, &pan, e4, 0, 300, t4, 4, res, NULL) == BAD);
  CASE("tags/null_tags", skred_fxbank_ctl_tags_each(fx, &pan, e4, 0, 300, NULL, 4, res, NULL) == BAD);
  CASE("tags/null_entries", skred_fxbank_ctl_tags_each(fx, &pan, NULL, 0, 300, t4, 4, res, NULL) == BAD);
  CASE("tags/zero_tag", skred_fxbank_ctl_tags_each(fx, &pan, e4, 0, 300, z4, 4, res, NULL) == BAD);
  CASE("tags/dup_tag", skred_fxbank_ctl_tags_each(fx, &pan, e4, 0, 300, d4, 4, res, NULL) == BAD);
  CASE("tags/1025_tags", skred_fxbank_ctl_tags_each(fx, NULL, e1025, 0, 300, many, 1025, res, NULL) == BAD);
  CASE("tags/negative_n", skred_fxbank_ctl_tags_each(fx, &pan, e4, 0, 300, t4, -1, res, NULL) == BAD);
  CASE("tags/bad_ctl", skred_fxbank_ctl_tags_each(fx, &bad, e4, 0, 300, t4, 4, res, NULL) == BAD);
  e4[0].reserved[1] = 7;
  CASE("tags/bad_entry", skred_fxbank_ctl_tags_each(fx, &pan, e4, 0, 300, t4, 4, res, NULL) == BAD);
  e4[0].reserved[1] = 0;
  CASE("tags/count_zero", skred_fxbank_ctl_tags_each(fx, &pan, e4, 0, 0, t4, 4, res, NULL) == RNG);
  CASE("tags/past_the_bank", skred_fxbank_ctl_tags_each(fx, &pan, e4, 0, 301, t4, 4, res, NULL) == RNG);
  CASE("tags/empty", skred_fxbank_ctl_tags_each(fx, &pan, e4, 0, 300, t4, 0, res, NULL) == SKRED_OK);

  int untouched = !fx->d_owner && !fx->d_owner_found && !fx->d_match_pair && !fx->d_idle && !fx->d_idle_out && !fx->h_idle_out &&
                  fx->ring_head == 0 && fx->count == 0 && res[0] == 0 && res[1] == 0 && res[2] == 0;
  for (int i = 0; i < SKX_RING; i++) untouched = untouched && !fx->ring[i].h && !fx->ring[i].d && !fx->ring[i].ev && !fx->ring[i].in_flight;
  CASE("bank/untouched", untouched);
  free(e1025);
  free(many);
  free(fx);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
