/* The host side of channel polyphony on the fixed-point bank without a device: skred_fx_chan_check and every refusal the three entry
 * points make before anything touches the device, on a skred_fxbank_t that is nothing but its voice count (a refused call reads no
 * other member), and the way the burst's two queries are packed (the library's overrides: a steal query that would be refused in the
 * fields the library overrides passes, one that is wrong elsewhere does not).  One line per case, "OK" last.
 * tests/test_fx_chan_cpu.py builds and runs it; built together with skred_amd/csrc/skred_fx_steal.c and -fsanitize=address,undefined it
 * is the sanitizer run of that file's host code -- from the repository root, after the library is built (the program's own copy of
 * skred_fx_steal.c takes the place of the library's; everything else it calls comes from the library):
 *   gcc -O1 -g -Wall -Werror -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iskred_amd/csrc \
 *       -I${ROCM_PATH:-/opt/rocm}/include tests/c_fx_chan_host.c skred_amd/csrc/skred_fx_steal.c -o /tmp/c_fx_chan_host_san \
 *       -Lskred_amd -lskred_amd -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lm -lpthread \
 *       -Wl,-rpath,$PWD/skred_amd -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib && /tmp/c_fx_chan_host_san */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_fxbank_priv.h"

static int failures;
#define CASE(name, cond) do { const int ok_ = (cond); printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); failures += !ok_; } while (0)

#define N 1024
#define WHICH (SKRED_IDLE_FINISHED | SKRED_IDLE_ENV_DONE)
#define BAD SKRED_E_BAD_ARG
#define RANGE SKRED_E_RANGE

static skred_fx_idle_query_t idle_q(void) {
  skred_fx_idle_query_t q;
  memset(&q, 0, sizeof(q));
  q.first = 0; q.count = N; q.which = WHICH; q.settle_q15 = 3; q.from = 0; q.max_out = -5;
  return q;
}

static skred_fx_steal_query_t steal_q(void) {
  skred_fx_steal_query_t q;
  memset(&q, 0, sizeof(q));
  q.first = 0; q.count = N; q.policy = SKRED_STEAL_OLDEST; q.max_out = 16;
  return q;
}

int main(void) {
  const skred_owner_match_t chan = { 0x03000000u, 0xFF000000u }, all = { 0, 0 }, off = { 0x03000001u, 0xFF000000u };
  const skred_owner_match_t one = { 0x03000007u, 0xFFFFFFFFu };
  const uint32_t t4[4] = { 0x03000001u, 0x03000002u, 0x03FFFFFFu, 0x03000001u };      /* (a tag may repeat: two notes of one id) */
  const uint32_t z4[4] = { 0x03000001u, 0, 0x03000003u, 0x03000004u }, w4[4] = { 0x03000001u, 0x03000002u, 0x04000003u, 0x03000004u };
  const uint32_t same[2] = { 0x03000007u, 0x03000007u };
  skred_fx_idle_query_t iq = idle_q(), ib;
  skred_fx_steal_query_t sq = steal_q(), sb;

  CASE("const/no_cap", SKRED_CHAN_NO_CAP == 0xFFFFFFFFu && sizeof(skred_owner_match_t) == 8 && sizeof(skred_fx_steal_query_t) == 40);
  CASE("check/plain", skred_fx_chan_check(&iq, &sq, &chan, 8, t4, 4, N) == SKRED_OK);
  CASE("check/cap0", skred_fx_chan_check(&iq, &sq, &chan, 0, t4, 4, N) == SKRED_OK);
  CASE("check/no_cap", skred_fx_chan_check(&iq, &sq, &chan, SKRED_CHAN_NO_CAP, t4, 4, N) == SKRED_OK);
  CASE("check/mask0_any_tag", skred_fx_chan_check(&iq, &sq, &all, 1, w4, 4, N) == SKRED_OK);
  CASE("check/one_note", skred_fx_chan_check(&iq, &sq, &one, 1, same, 2, N) == SKRED_OK);
  CASE("check/empty", skred_fx_chan_check(&iq, &sq, &chan, 1, t4, 0, N) == SKRED_OK);
  CASE("check/null_idle_q", skred_fx_chan_check(NULL, &sq, &chan, 8, t4, 4, N) == BAD);
  CASE("check/null_steal_q", skred_fx_chan_check(&iq, NULL, &chan, 8, t4, 4, N) == BAD);
  CASE("check/null_match", skred_fx_chan_check(&iq, &sq, NULL, 8, t4, 4, N) == BAD);
  CASE("check/bad_match", skred_fx_chan_check(&iq, &sq, &off, 8, t4, 4, N) == BAD);
  CASE("check/null_tags", skred_fx_chan_check(&iq, &sq, &chan, 8, NULL, 4, N) == BAD);
  CASE("check/null_tags_empty", skred_fx_chan_check(&iq, &sq, &chan, 8, NULL, 0, N) == BAD);
  CASE("check/negative_n", skred_fx_chan_check(&iq, &sq, &chan, 8, t4, -1, N) == BAD);
  CASE("check/huge_n", skred_fx_chan_check(&iq, &sq, &all, 8, t4, INT32_MAX / 64 + 1, N) == BAD);
  CASE("check/zero_tag", skred_fx_chan_check(&iq, &sq, &chan, 8, z4, 4, N) == BAD);
  CASE("check/zero_tag_mask0", skred_fx_chan_check(&iq, &sq, &all, 8, z4, 4, N) == BAD);
  CASE("check/zero_tag_not_reached", skred_fx_chan_check(&iq, &sq, &chan, 8, z4, 1, N) == SKRED_OK);
  CASE("check/tag_of_another_channel", skred_fx_chan_check(&iq, &sq, &chan, 8, w4, 4, N) == BAD);
  CASE("check/tag_of_another_channel_not_reached", skred_fx_chan_check(&iq, &sq, &chan, 8, w4, 2, N) == SKRED_OK);
  CASE("check/tag_is_not_the_one_note", skred_fx_chan_check(&iq, &sq, &one, 8, t4, 1, N) == BAD);
  ib = iq; ib.which = WHICH | SKRED_IDLE_AMP_ZERO;
  CASE("check/amp_zero", skred_fx_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == BAD);
  ib = iq; ib.which = SKRED_IDLE_ENV_DONE | SKRED_IDLE_UNNAMED;
  CASE("check/idle_unnamed", skred_fx_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == BAD);
  ib = iq; ib.which = 0;
  CASE("check/idle_no_criterion", skred_fx_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == BAD);
  ib = iq; ib.settle_q15 = -1;
  CASE("check/idle_settle_negative", skred_fx_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == BAD);
  ib = iq; ib.count = N + 1;
  CASE("check/idle_past_the_bank", skred_fx_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == RANGE);
  ib = iq; ib.count = 0;
  CASE("check/idle_empty_range", skred_fx_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == RANGE);
  ib = iq; ib.first = 8; ib.count = 64; ib.from = 7;
  CASE("check/idle_from_outside", skred_fx_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == RANGE);
  sb = sq; sb.first = 8; sb.count = 64;
  CASE("check/ranges_may_differ", skred_fx_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == SKRED_OK);
  sb = sq; sb.policy = 2;
  CASE("check/steal_policy", skred_fx_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == BAD);
  sb = sq; sb.flags = SKRED_STEAL_UNNAMED;
  CASE("check/steal_unnamed", skred_fx_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == BAD);
  sb = sq; sb.flags = 4;
  CASE("check/steal_flags", skred_fx_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == BAD);
  sb = sq; sb.reserved = 1;
  CASE("check/steal_reserved", skred_fx_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == BAD);
  sb = sq; sb.count = 0;
  CASE("check/steal_empty_range", skred_fx_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == RANGE);
  sb = sq; sb.first = -1;
  CASE("check/steal_first_negative", skred_fx_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == RANGE);
  sb = sq; sb.first = 1;
  CASE("check/steal_past_the_bank", skred_fx_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == RANGE);
  /* the packing: exclude_idle, settle_q15 and max_out are the library's, whatever the caller put there */
  sb = sq; sb.exclude_idle = 8 | SKRED_IDLE_UNNAMED; sb.settle_q15 = -1; sb.max_out = -3;
  CASE("pack/overridden_fields_are_not_looked_at", skred_fx_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == SKRED_OK);
  sb = sq; sb.max_out = SKRED_STEAL_MAX + 1;
  CASE("pack/max_out_is_the_librarys", skred_fx_chan_check(&iq, &sb, &chan, 8, t4, 4, N) == SKRED_OK);
  ib = iq; ib.max_out = 7;
  CASE("pack/idle_max_out_is_the_librarys", skred_fx_chan_check(&ib, &sq, &chan, 8, t4, 4, N) == SKRED_OK);
  CASE("check/bank_of_zero_voices", skred_fx_chan_check(&iq, &sq, &chan, 8, t4, 4, 0) != SKRED_OK);

  /* the entry points: a bank that is nothing but its size */
  skred_fxbank_t *fx = (skred_fxbank_t *)calloc(1, sizeof(skred_fxbank_t));
  fx->n_voices = N;
  int32_t list[16];
  uint32_t cnt[3] = { 7, 7, 7 }, res[4] = { 7, 7, 7, 7 };
  int total = 7, sounding = 7;
  memset(list, 0xFF, sizeof(list));
  CASE("find/null_bank", skred_fxbank_find_steal_match(NULL, &sq, &chan, list, cnt, NULL) == BAD);
  CASE("find/null_query", skred_fxbank_find_steal_match(fx, NULL, &chan, list, cnt, NULL) == BAD);
  CASE("find/null_match", skred_fxbank_find_steal_match(fx, &sq, NULL, list, cnt, NULL) == BAD);
  CASE("find/bad_match", skred_fxbank_find_steal_match(fx, &sq, &off, list, cnt, NULL) == BAD);
  CASE("find/null_count", skred_fxbank_find_steal_match(fx, &sq, &chan, list, NULL, NULL) == BAD);
  CASE("find/null_list", skred_fxbank_find_steal_match(fx, &sq, &chan, NULL, cnt, NULL) == BAD);
  sb = sq; sb.max_out = SKRED_STEAL_MAX + 1;
  CASE("find/max_out_large", skred_fxbank_find_steal_match(fx, &sb, &chan, list, cnt, NULL) == BAD);
  sb = sq; sb.exclude_idle = SKRED_IDLE_UNNAMED;
  CASE("find/exclude_unnamed", skred_fxbank_find_steal_match(fx, &sb, &chan, list, cnt, NULL) == BAD);
  sb = sq; sb.settle_q15 = -1;
  CASE("find/settle_negative", skred_fxbank_find_steal_match(fx, &sb, &chan, list, cnt, NULL) == BAD);
  sb = sq; sb.count = N + 1;
  CASE("find/past_the_bank", skred_fxbank_find_steal_match(fx, &sb, &chan, list, cnt, NULL) == RANGE);
  CASE("find_host/null_bank", skred_fxbank_find_steal_match_host(NULL, &sq, &chan, list, &total, &sounding, NULL) == BAD);
  CASE("find_host/null_query", skred_fxbank_find_steal_match_host(fx, NULL, &chan, list, &total, &sounding, NULL) == BAD);
  CASE("find_host/null_match", skred_fxbank_find_steal_match_host(fx, &sq, NULL, list, &total, &sounding, NULL) == BAD);
  CASE("find_host/null_list", skred_fxbank_find_steal_match_host(fx, &sq, &chan, NULL, &total, &sounding, NULL) == BAD);
  CASE("find_host/range", skred_fxbank_find_steal_match_host(fx, &sb, &chan, list, &total, &sounding, NULL) == RANGE);

  skred_fx_note_t *notes = (skred_fx_note_t *)calloc(4, sizeof(skred_fx_note_t));
  for (int i = 0; i < 4; i++) { notes[i].phase_inc = 3000017u; notes[i].velocity_q15 = 9000; }
  int32_t assigned[4] = { -1, -1, -1, -1 };
#define ON(bank, i, s, m, cap, nt, tg, n, r) skred_fxbank_note_on_channel(bank, i, s, m, cap, nt, tg, n, assigned, r, NULL)
  CASE("on/null_bank", ON(NULL, &iq, &sq, &chan, 8, notes, t4, 4, res) == BAD);
  CASE("on/null_notes", ON(fx, &iq, &sq, &chan, 8, NULL, t4, 4, res) == BAD);
  CASE("on/null_result", ON(fx, &iq, &sq, &chan, 8, notes, t4, 4, NULL) == BAD);
  CASE("on/null_idle_q", ON(fx, NULL, &sq, &chan, 8, notes, t4, 4, res) == BAD);
  CASE("on/null_steal_q", ON(fx, &iq, NULL, &chan, 8, notes, t4, 4, res) == BAD);
  CASE("on/null_match", ON(fx, &iq, &sq, NULL, 8, notes, t4, 4, res) == BAD);
  CASE("on/bad_match", ON(fx, &iq, &sq, &off, 8, notes, t4, 4, res) == BAD);
  CASE("on/null_tags", ON(fx, &iq, &sq, &chan, 8, notes, NULL, 4, res) == BAD);
  CASE("on/zero_tag", ON(fx, &iq, &sq, &chan, 8, notes, z4, 4, res) == BAD);
  CASE("on/tag_of_another_channel", ON(fx, &iq, &sq, &chan, 8, notes, w4, 4, res) == BAD);
  CASE("on/negative_n", ON(fx, &iq, &sq, &chan, 8, notes, t4, -1, res) == BAD);
  ib = iq; ib.which = SKRED_IDLE_AMP_ZERO;
  CASE("on/amp_zero", ON(fx, &ib, &sq, &chan, 8, notes, t4, 4, res) == BAD);
  ib = iq; ib.count = N + 1;
  CASE("on/idle_past_the_bank", ON(fx, &ib, &sq, &chan, 8, notes, t4, 4, res) == RANGE);
  sb = sq; sb.first = 1;
  CASE("on/steal_past_the_bank", ON(fx, &iq, &sb, &chan, 8, notes, t4, 4, res) == RANGE);
  sb = sq; sb.policy = 7;
  CASE("on/steal_policy", ON(fx, &iq, &sb, &chan, 8, notes, t4, 4, res) == BAD);
  notes[2].flags = 4;
  CASE("on/note_flags", ON(fx, &iq, &sq, &chan, 8, notes, t4, 4, res) == BAD);
  notes[2].flags = 0; notes[1].velocity_q15 = 65536;
  CASE("on/note_velocity", ON(fx, &iq, &sq, &chan, 8, notes, t4, 4, res) == BAD);
  notes[1].velocity_q15 = 9000; notes[3].reserved[1] = 1;
  CASE("on/note_reserved", ON(fx, &iq, &sq, &chan, 8, notes, t4, 4, res) == BAD);
  notes[3].reserved[1] = 0; notes[0].flags = SKRED_NOTE_SET_PAN; notes[0].pan_left_q15 = -1;
  CASE("on/note_pan", ON(fx, &iq, &sq, &chan, 8, notes, t4, 4, res) == BAD);
  CASE("on/empty", ON(fx, &iq, &sq, &chan, 8, notes, t4, 0, res) == SKRED_OK);
  CASE("on/empty_null_tags", ON(fx, &iq, &sq, &chan, 8, notes, NULL, 0, res) == BAD);

  CASE("untouched/outputs", cnt[0] == 7 && cnt[1] == 7 && cnt[2] == 7 && res[0] == 7 && res[1] == 7 && res[2] == 7 && res[3] == 7 && total == 7 &&
                            sounding == 7 && list[0] == -1 && list[15] == -1 && assigned[0] == -1 && assigned[3] == -1);
  CASE("untouched/bank", fx->ring_head == 0 && !fx->d_owner && !fx->d_steal && !fx->d_idle && !fx->d_steal_out && !fx->h_steal_out &&
                         !fx->d_note_list && fx->count == 0);
  free(notes);
  free(fx);
  puts(failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
