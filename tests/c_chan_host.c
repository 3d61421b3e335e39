/* The host side of channel polyphony without a device: skred_chan_check and every refusal the three entry points make before anything
 * touches the device, on a skred_bank_t that is nothing but its voice count (a refused call reads no other member), and the way the
 * burst's two queries are packed (the library's overrides: a steal query that would be refused in the fields the library overrides
 * passes, one that is wrong elsewhere does not).  One line per case, "OK" last.
 * tests/test_chan_cpu.py builds and runs it; built together with skred_amd/csrc/skred_bank_slots.c and -fsanitize=address,undefined it
 * is the sanitizer run of that file's host code -- from the repository root, after the library is built (the program's own copy of
 * skred_bank_slots.c takes the place of the library's; everything else it calls comes from the library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_chan_host.c skred_amd/csrc/skred_bank_slots.c -o /tmp/c_chan_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_chan_host_san */
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
#define WHICH (SKRED_IDLE_FINISHED | SKRED_IDLE_ENV_DONE)
#define BAD SKRED_E_BAD_ARG
#define RANGE SKRED_E_RANGE

static skred_slot_query_t idle_q(void) {
  skred_slot_query_t q;
  memset(&q, 0, sizeof(q));
  q.first = 0; q.count = N; q.slot_voices = K; q.member_mask = MASK; q.which = WHICH; q.settle_level = 1e-3f; q.from = 0; q.max_out = -5;
  return q;
}

static skred_slot_steal_query_t steal_q(void) {
  skred_slot_steal_query_t q;
  memset(&q, 0, sizeof(q));
  q.first = 0; q.count = N; q.slot_voices = K; q.policy = SKRED_STEAL_OLDEST; q.member_mask = MASK; q.max_out = 16;
  return q;
}

int main(void) {
  const skred_owner_match_t chan = { 0x03000000u, 0xFF000000u }, all = { 0, 0 }, off = { 0x03000001u, 0xFF000000u };
  const skred_owner_match_t one = { 0x03000007u, 0xFFFFFFFFu };
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0x03FFFFFFu, 0x03000001u };      /* (a tag may repeat: two notes of one id) */
  const uint32_t z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u }, w4[4] = { 0x03000001u, 0x03000002u, 0x04000003u, 0x03000004u };
  const uint32_t same[2] = { 0x03000007u, 0x03000007u };
  skred_slot_query_t iq = idle_q(), ib;
  skred_slot_steal_query_t sq = steal_q(), sb;

  CASE("const/no_cap", SKRED_CHAN_NO_CAP == 0xFFFFFFFFu && sizeof(skred_owner_match_t) == 8);
  CASE("check/plain", skred_chan_check(&iq, &sq, &chan, 8, t4, 4, N) == SKRED_OK);
  CASE("check/cap0", skred_chan_check(&iq, &sq, &chan, 0, t4, 4, N) == SKRED_OK);
  CASE("check/no_cap", skred_chan_check(&iq, &sq, &chan, SKRED_CHAN_NO_CAP, t4, 4, N) == SKRED_OK);
  CASE("check/mask0_any_tag", skred_chan_check(&iq, &sq, &all, 1, w4, 4, N) == SKRED_OK);
  CASE("check/one_note", skred_chan_check(&iq, &sq, &one, 1, same, 2, N) == SKRED_OK);
  CASE("check/empty", skred_chan_check(&iq, &sq, &chan, 1, t4, 0, N) == SKRED_OK);
  CASE("check/null_idle_q", skred_chan_check(NULL, &sq, &chan, 8, t4, 4, N) == BAD);
  CASE("check/null_steal_q", skred_chan_check(&iq, NULL, &chan, 8, t4, 4, N) == BAD);
  CASE("check/null_match", skred_chan_check(&iq, &sq, NULL, 8, t4, 4, N) == BAD);
  CASE("check/bad_match", skred_chan_check(&iq, &sq, &off, 8, t4, 4, N) == BAD);
  CASE("check/null_tags", skred_chan_check(&iq, &sq, &chan, 8, NULL, 4, N) == BAD);
  CASE("check/null_tags_empty", skred_chan_check(&iq, &sq, &chan, 8, NULL, 0, N) == BAD);
  CASE("check/negative_n", skred_chan_check(&iq, &sq, &chan, 8, t4, -1, N) == BAD);
  CASE("check/huge_n", skred_chan_check(&iq, &sq, &all, 8, t4, INT32_MAX / 64 + 1, N) == BAD);
  CASE("check/zero_tag", skred_chan_check(&iq, &sq, &chan, 8, z4, 4, N) == BAD);
  CASE("check/zero_tag_mask0", skred_chan_check(&iq, &sq, &all, 8, z4, 4, N) == BAD);
  CASE("check/zero_tag_not_reached", skred_chan_check(&iq, &sq, &chan, 8, z4, 1, N) == SKRED_OK);
  CASE("check/tag_of_another_channel", skred_chan_check(&iq, &sq, &chan, 8, w4, 4, N) == BAD);
  CASE("check/tag_of_another_channel_not_reached", skred_chan_check(&iq, &sq, &chan, 8, w4, 2, N) == SKRED_OK);
  CASE("check/tag_is_not_the_one_note", skred_chan_check(&iq, &sq, &one, 8, t4, 1, N) == BAD);
  ib = iq; ib.which = WHICH | SKRED_IDLE_AMP_ZERO;
  CASE("check/amp_zero", skred_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == BAD);
  ib = iq; ib.which = SKRED_IDLE_ENV_DONE | SKRED_IDLE_UNNAMED;
  CASE("check/idle_unnamed", skred_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == BAD);
  ib = iq; ib.which = 0;
  CASE("check/idle_no_criterion", skred_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == BAD);
  ib = iq; ib.first = 4;
  CASE("check/idle_first_off_slot", skred_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == RANGE);
  ib = iq; ib.count = N + 8;
  CASE("check/idle_past_the_bank", skred_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == RANGE);
  ib = iq; ib.from = 12;
  CASE("check/idle_from_off_slot", skred_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == RANGE);
  ib = iq; ib.settle_level = NAN;
  CASE("check/idle_settle_nan", skred_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == BAD);
  ib = iq; ib.slot_voices = 16;
  CASE("check/k_differs", skred_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == BAD);
  ib = iq; ib.member_mask = 0xFF;
  CASE("check/mask_differs", skred_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == BAD);
  sb = sq; sb.first = 8; sb.count = 64;
  CASE("check/ranges_may_differ", skred_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == SKRED_OK);
  sb = sq; sb.policy = 2;
  CASE("check/steal_policy", skred_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == BAD);
  sb = sq; sb.flags = SKRED_STEAL_UNNAMED;
  CASE("check/steal_unnamed", skred_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == BAD);
  sb = sq; sb.flags = 4;
  CASE("check/steal_flags", skred_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == BAD);
  sb = sq; sb.reserved[1] = 1;
  CASE("check/steal_reserved", skred_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == BAD);
  sb = sq; sb.member_mask = 0;
  CASE("check/steal_mask0", skred_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == BAD);
  sb = sq; sb.slot_voices = 3; sb.member_mask = 1;
  CASE("check/steal_k3", skred_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == RANGE);
  sb = sq; sb.count = 1020;
  CASE("check/steal_count_off_slot", skred_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == RANGE);
  /* the packing: exclude_idle, settle_level and max_out are the library's, whatever the caller put there */
  sb = sq; sb.exclude_idle = 8 | SKRED_IDLE_UNNAMED; sb.settle_level = -1.0f; sb.max_out = -3;
  CASE("pack/overridden_fields_are_not_looked_at", skred_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == SKRED_OK);
  sb = sq; sb.max_out = SKRED_STEAL_MAX + 1;
  CASE("pack/max_out_is_the_librarys", skred_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == SKRED_OK);
  ib = iq; ib.max_out = 7;
  CASE("pack/idle_max_out_is_the_librarys", skred_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == SKRED_OK);
  CASE("check/bank_of_zero_voices", skred_chan_check(&iq, &sq, &chan, 8, t4, 4, 0) == RANGE);

  /* the entry points: a bank that is nothing but its size */
  skred_bank_t *b = (skred_bank_t *)calloc(1, sizeof(skred_bank_t));
  b->n_voices = N;
  int32_t list[16];
  uint32_t cnt[3] = { 7, 7, 7 }, res[4] = { 7, 7, 7, 7 };
  int total = 7, sounding = 7;
  memset(list, 0xFF, sizeof(list));
  CASE("find/null_bank", skred_bank_find_steal_slots_match(NULL, &sq, &chan, list, cnt, NULL) == BAD);
  CASE("find/null_query", skred_bank_find_steal_slots_match(b, NULL, &chan, list, cnt, NULL) == BAD);
  CASE("find/null_match", skred_bank_find_steal_slots_match(b, &sq, NULL, list, cnt, NULL) == BAD);
  CASE("find/bad_match", skred_bank_find_steal_slots_match(b, &sq, &off, list, cnt, NULL) == BAD);
  CASE("find/null_count", skred_bank_find_steal_slots_match(b, &sq, &chan, list, NULL, NULL) == BAD);
  CASE("find/null_list", skred_bank_find_steal_slots_match(b, &sq, &chan, NULL, cnt, NULL) == BAD);
  sb = sq; sb.max_out = SKRED_STEAL_MAX + 1;
  CASE("find/max_out_large", skred_bank_find_steal_slots_match(b, &sb, &chan, list, cnt, NULL) == BAD);
  sb = sq; sb.exclude_idle = SKRED_IDLE_UNNAMED;
  CASE("find/exclude_unnamed", skred_bank_find_steal_slots_match(b, &sb, &chan, list, cnt, NULL) == BAD);
  sb = sq; sb.first = 4;
  CASE("find/first_off_slot", skred_bank_find_steal_slots_match(b, &sb, &chan, list, cnt, NULL) == RANGE);
  sb = sq; sb.count = N + 8;
  CASE("find/past_the_bank", skred_bank_find_steal_slots_match(b, &sb, &chan, list, cnt, NULL) == RANGE);
  CASE("find_host/null_bank", skred_bank_find_steal_slots_match_host(NULL, &sq, &chan, list, &total, &sounding, NULL) == BAD);
  CASE("find_host/null_query", skred_bank_find_steal_slots_match_host(b, NULL, &chan, list, &total, &sounding, NULL) == BAD);
  CASE("find_host/null_match", skred_bank_find_steal_slots_match_host(b, &sq, NULL, list, &total, &sounding, NULL) == BAD);
  CASE("find_host/null_list", skred_bank_find_steal_slots_match_host(b, &sq, &chan, NULL, &total, &sounding, NULL) == BAD);
  CASE("find_host/range", skred_bank_find_steal_slots_match_host(b, &sb, &chan, list, &total, &sounding, NULL) == RANGE);

  skred_note_t *notes = (skred_note_t *)calloc(4 * K, sizeof(skred_note_t));
  for (int i = 0; i < 4 * K; i++) { notes[i].phase_inc = 0.3f; notes[i].velocity = 0.5f; }
  int32_t assigned[4] = { -1, -1, -1, -1 };
#define ON(bank, i, s, m, cap, nt, tg, n, vm, r) skred_bank_note_on_channel(bank, i, s, m, cap, nt, tg, n, vm, assigned, r, NULL)
  CASE("on/null_bank", ON(NULL, &iq, &sq, &chan, 8, notes, t4, 4, MASK, res) == BAD);
  CASE("on/null_notes", ON(b, &iq, &sq, &chan, 8, NULL, t4, 4, MASK, res) == BAD);
  CASE("on/null_result", ON(b, &iq, &sq, &chan, 8, notes, t4, 4, MASK, NULL) == BAD);
  CASE("on/null_idle_q", ON(b, NULL, &sq, &chan, 8, notes, t4, 4, MASK, res) == BAD);
  CASE("on/null_steal_q", ON(b, &iq, NULL, &chan, 8, notes, t4, 4, MASK, res) == BAD);
  CASE("on/null_match", ON(b, &iq, &sq, NULL, 8, notes, t4, 4, MASK, res) == BAD);
  CASE("on/bad_match", ON(b, &iq, &sq, &off, 8, notes, t4, 4, MASK, res) == BAD);
  CASE("on/null_tags", ON(b, &iq, &sq, &chan, 8, notes, NULL, 4, MASK, res) == BAD);
  CASE("on/zero_tag", ON(b, &iq, &sq, &chan, 8, notes, z4, 4, MASK, res) == BAD);
  CASE("on/tag_of_another_channel", ON(b, &iq, &sq, &chan, 8, notes, w4, 4, MASK, res) == BAD);
  CASE("on/negative_n", ON(b, &iq, &sq, &chan, 8, notes, t4, -1, MASK, res) == BAD);
  ib = iq; ib.which = SKRED_IDLE_AMP_ZERO;
  CASE("on/amp_zero", ON(b, &ib, &sq, &chan, 8, notes, t4, 4, MASK, res) == BAD);
  ib = iq; ib.slot_voices = 4; ib.member_mask = 0x5;
  CASE("on/k_differs", ON(b, &ib, &sq, &chan, 8, notes, t4, 4, MASK, res) == BAD);
  ib = iq; ib.count = N + 8;
  CASE("on/idle_past_the_bank", ON(b, &ib, &sq, &chan, 8, notes, t4, 4, MASK, res) == RANGE);
  sb = sq; sb.first = 4;
  CASE("on/steal_first_off_slot", ON(b, &iq, &sb, &chan, 8, notes, t4, 4, MASK, res) == RANGE);
  CASE("on/voice_mask0", ON(b, &iq, &sq, &chan, 8, notes, t4, 4, 0, res) == BAD);
  CASE("on/voice_mask_high", ON(b, &iq, &sq, &chan, 8, notes, t4, 4, 0x100, res) == BAD);
  notes[K + 2].phase_inc = NAN;                              /* a masked position (bit 2) of note 1 */
  CASE("on/bad_note", ON(b, &iq, &sq, &chan, 8, notes, t4, 4, MASK, res) == BAD);
  CASE("on/bad_note_not_reached", ON(b, &iq, &sq, &chan, 8, notes, t4, 0, MASK, res) == SKRED_OK);
  notes[K + 2].phase_inc = 0.3f;
  notes[K + 1].phase_inc = NAN;                              /* outside the mask: not looked at; n == 0: nothing is done */
  CASE("on/empty", ON(b, &iq, &sq, &chan, 8, notes, t4, 0, MASK, res) == SKRED_OK);
  CASE("on/empty_null_tags", ON(b, &iq, &sq, &chan, 8, notes, NULL, 0, MASK, res) == BAD);

  CASE("untouched/outputs", cnt[0] == 7 && cnt[1] == 7 && cnt[2] == 7 && res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && total == 7 &&
                            sounding == 7 && list[0] == -1 && list[15] == -1 && assigned[0] == -1 && assigned[3] == -1);
  CASE("untouched/bank", b->touched_total == 0 && b->control_epoch == 0 && b->upd_seq == 0 && b->upd_head == 0 && !b->d_owner && !b->d_steal &&
                         !b->d_idle && !b->d_idle_out && !b->d_note_list);
  free(notes);
  free(b);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
