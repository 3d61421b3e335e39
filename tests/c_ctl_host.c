/* The host side of the patch controllers without a device: skred_ctl_check, the record packing (sk_ctl_pack) and every refusal the
 * entry points make before anything touches the device, on a skred_bank_t that is nothing but its voice count (a refused call reads
 * no other member).  One line per case, "OK" last.  tests/test_ctl_cpu.py builds and runs it; built together with
 * skred_amd/csrc/skred_bank_ctl.c, the shared checks and the batch path it reaches, and -fsanitize=address,undefined
 * it is the sanitizer run of those files' host code -- from the repository root, after the library is built (the program's own copy of
 * skred_bank_ctl.c, skred_bank_checks.c and skred_bank_stage.c takes the place of the library's; everything else it calls comes from the library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_ctl_host.c skred_amd/csrc/skred_bank_ctl.c skred_amd/csrc/skred_bank_checks.c \
 *       skred_amd/csrc/skred_bank_stage.c -o /tmp/c_ctl_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_ctl_host_san */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_bank_priv.h"

static int failures;
#define CASE(name, cond) do { const int ok_ = (cond); printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); failures += !ok_; } while (0)

static skred_ctl_t rec(uint32_t set) {
  skred_ctl_t c;
  memset(&c, 0, sizeof(c));
  c.set = set;
  c.phase_inc = 0.5f; c.inc_scale = 1.0594631f; c.amp = -0.25f; c.pan_left = 0.3f; c.pan_right = 0.7f;
  c.b0 = 0.1f; c.b1 = 0.2f; c.b2 = 0.1f; c.a1 = -1.5f; c.a2 = 0.6f;
  c.attack_time = 0.0f; c.decay_time = 0.0f; c.sustain_level = 0.5f; c.release_time = 0.0f; c.velocity = 0.9f; c.smoothing = 0.02f;
  c.fm_depth = 0.0f; c.freq_scale = 1.0f; c.am_depth = 0.0f; c.pan_depth = 0.0f; c.cz_depth = 0.0f; c.cz_dist = 0.0f;
  return c;
}

int main(void) {
  const uint32_t all_abs = (uint32_t)SK_CTL_ALL & ~(uint32_t)SKRED_CTL_INC_SCALE;
  skred_ctl_t one = rec(all_abs);
  CASE("check/all_bits_k1", skred_ctl_check(&one, 1, 1) == SKRED_OK);
  one = rec(SKRED_CTL_INC_SCALE | SKRED_CTL_AMP);
  CASE("check/scale_and_negative_amp", skred_ctl_check(&one, 1, 1) == SKRED_OK);
  CASE("check/null", skred_ctl_check(NULL, 1, 1) == SKRED_E_BAD_ARG);
  CASE("check/k0", skred_ctl_check(&one, 0, 1) == SKRED_E_RANGE);
  CASE("check/k3", skred_ctl_check(&one, 3, 1) == SKRED_E_RANGE);
  CASE("check/k128", skred_ctl_check(&one, 128, 1) == SKRED_E_RANGE);
  CASE("check/mask0", skred_ctl_check(&one, 1, 0) == SKRED_E_BAD_ARG);
  CASE("check/mask_high", skred_ctl_check(&one, 1, 2) == SKRED_E_BAD_ARG);

  /* K = 64, the single high bit: 63 records of junk nobody may look at (heap memory: a read past the array would be seen) */
  skred_ctl_t *big = (skred_ctl_t *)malloc(64 * sizeof(skred_ctl_t));
  memset(big, 0xFF, 64 * sizeof(skred_ctl_t));
  big[63] = rec(SKRED_CTL_FILTER | SKRED_CTL_PAN);
  CASE("check/k64_high_bit", skred_ctl_check(big, 64, 1ull << 63) == SKRED_OK);
  CASE("check/k64_junk_seen", skred_ctl_check(big, 64, (1ull << 63) | 1ull) == SKRED_E_BAD_ARG);
  sk_ctl_t *out = (sk_ctl_t *)malloc(64 * sizeof(sk_ctl_t));
  memset(out, 0xAB, 64 * sizeof(sk_ctl_t));
  uint64_t lists = sk_ctl_pack(big, 64, 1ull << 63, out);
  int zero = 1;
  for (int l = 0; l < 63; l++) for (int w = 0; w < SK_CTL_WORDS; w++) zero = zero && out[l].w[w] == 0;
  CASE("pack/unmasked_zeroed", zero);
  CASE("pack/masked_word_for_word", memcmp(&out[63], &big[63], sizeof(skred_ctl_t)) == 0);
  CASE("pack/filter_pan_list_nobody", lists == 0);
  big[63].set |= SKRED_CTL_VELOCITY;
  big[0] = rec(SKRED_CTL_AMP);
  big[1] = rec(SKRED_CTL_PHASE_INC);
  lists = sk_ctl_pack(big, 64, (1ull << 63) | 3ull, out);
  CASE("pack/lists", lists == ((1ull << 63) | 1ull));
  CASE("pack/first_words", out[0].w[SK_CTL_SET] == SKRED_CTL_AMP && out[1].w[SK_CTL_SET] == SKRED_CTL_PHASE_INC && out[2].w[SK_CTL_SET] == 0);
  free(out);
  free(big);

  /* the entry points: a bank that is nothing but its size */
  skred_bank_t *b = (skred_bank_t *)calloc(1, sizeof(skred_bank_t));
  b->n_voices = 200;
  skred_ctl_t k8[8];
  for (int l = 0; l < 8; l++) k8[l] = rec(SKRED_CTL_FILTER);
  int32_t dummy_list[4] = { 0, 8, 16, 24 };
  CASE("range/null_bank", skred_bank_ctl_range(NULL, k8, 0, 8, 8, 0xFF, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("range/null_ctl", skred_bank_ctl_range(b, NULL, 0, 8, 8, 0xFF, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("range/bad_k", skred_bank_ctl_range(b, k8, 0, 8, 12, 0xFF, NULL, NULL) == SKRED_E_RANGE);
  CASE("range/bad_mask", skred_bank_ctl_range(b, k8, 0, 8, 8, 0x1FF, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("range/negative_count", skred_bank_ctl_range(b, k8, 0, -8, 8, 0xFF, NULL, NULL) == SKRED_E_RANGE);
  CASE("range/negative_first", skred_bank_ctl_range(b, k8, -8, 8, 8, 0xFF, NULL, NULL) == SKRED_E_RANGE);
  CASE("range/past_the_bank", skred_bank_ctl_range(b, k8, 192, 16, 8, 0xFF, NULL, NULL) == SKRED_E_RANGE);
  CASE("range/first_past_the_bank", skred_bank_ctl_range(b, k8, 208, 0, 8, 0xFF, NULL, NULL) == SKRED_E_RANGE);
  CASE("range/huge_count", skred_bank_ctl_range(b, k8, 8, INT32_MAX - 7, 8, 0xFF, NULL, NULL) == SKRED_E_RANGE);
  CASE("range/first_off_slot", skred_bank_ctl_range(b, k8, 4, 8, 8, 0xFF, NULL, NULL) == SKRED_E_RANGE);
  CASE("range/count_off_slot", skred_bank_ctl_range(b, k8, 8, 12, 8, 0xFF, NULL, NULL) == SKRED_E_RANGE);
  CASE("range/empty", skred_bank_ctl_range(b, k8, 8, 0, 8, 0xFF, NULL, NULL) == SKRED_OK);
  CASE("range/empty_at_the_end", skred_bank_ctl_range(b, k8, 200, 0, 8, 0xFF, NULL, NULL) == SKRED_OK);
  k8[3].set = 0;
  CASE("range/set0_masked", skred_bank_ctl_range(b, k8, 0, 8, 8, 0xFF, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("range/set0_unmasked", skred_bank_ctl_range(b, k8, 8, 0, 8, 0xF7, NULL, NULL) == SKRED_OK);
  k8[3] = rec(SKRED_CTL_FILTER);
  CASE("slots/null_bank", skred_bank_ctl_slots(NULL, k8, 8, 0xFF, dummy_list, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("slots/null_list", skred_bank_ctl_slots(b, k8, 8, 0xFF, NULL, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("slots/null_ctl", skred_bank_ctl_slots(b, NULL, 8, 0xFF, dummy_list, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("slots/negative_n", skred_bank_ctl_slots(b, k8, 8, 0xFF, dummy_list, -1, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("slots/huge_n", skred_bank_ctl_slots(b, k8, 8, 0xFF, dummy_list, INT32_MAX, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("slots/bad_k", skred_bank_ctl_slots(b, k8, 5, 0xFF, dummy_list, 4, NULL, NULL, NULL) == SKRED_E_RANGE);
  CASE("slots/mask0", skred_bank_ctl_slots(b, k8, 8, 0, dummy_list, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  k8[7].b2 = NAN;
  CASE("slots/nan_coefficient", skred_bank_ctl_slots(b, k8, 8, 0xFF, dummy_list, 4, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("slots/nan_unmasked", skred_bank_ctl_slots(b, k8, 8, 0x7F, dummy_list, 0, NULL, NULL, NULL) == SKRED_OK);
  k8[7].b2 = 0.1f;
  CASE("slots/empty", skred_bank_ctl_slots(b, k8, 8, 0xFF, dummy_list, 0, NULL, NULL, NULL) == SKRED_OK);
  CASE("download/null", skred_bank_download_ctl(NULL, NULL, 0, 0, 0) == SKRED_E_BAD_ARG);
  /* the checks the entry points share (skred_bank_checks.c): an empty range at the very end is a controller's alone, and a call that
   * is wrong in several ways gets the code of its first check -- stamp_slots looks at the stamps before K and the mask */
  CASE("range/empty_at_the_end_k1", skred_bank_ctl_range(b, k8, 200, 0, 1, 1, NULL, NULL) == SKRED_OK);
  CASE("range/empty_past_the_end", skred_bank_ctl_range(b, k8, 201, 0, 1, 1, NULL, NULL) == SKRED_E_RANGE);
  CASE("slots/n_at_the_limit", skred_bank_ctl_slots(b, k8, 8, 0xFF, dummy_list, INT32_MAX / 64 + 1, NULL, NULL, NULL) == SKRED_E_BAD_ARG);
  CASE("slots/stamp_slots_k3_mask_at_k_stamps0", skred_bank_stamp_slots(b, dummy_list, 4, NULL, 3, 0x8, 0, NULL) == SKRED_E_BAD_ARG);
  CASE("slots/stamp_slots_k3_mask_at_k_stamps4", skred_bank_stamp_slots(b, dummy_list, 4, NULL, 3, 0x8, 4, NULL) == SKRED_E_BAD_ARG);
  CASE("slots/stamp_slots_k3_mask_at_k", skred_bank_stamp_slots(b, dummy_list, 4, NULL, 3, 0x8, SKRED_STAMP_RELEASE, NULL) == SKRED_E_RANGE);
  CASE("slots/stamp_slots_mask_at_k", skred_bank_stamp_slots(b, dummy_list, 4, NULL, 4, 0x10, SKRED_STAMP_RELEASE, NULL) == SKRED_E_BAD_ARG);
  CASE("bank/untouched", b->touched_total == 0 && b->control_epoch == 0 && b->upd_seq == 0 && b->upd_head == 0);
  free(b);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
