/* The bank's block planner on the CPU (skred_amd/csrc/skred_bank_plan.h, linked from libskred_amd.so): no bank, no HIP.  Every
 * expected value below was worked out by hand from the rules as they stood in render_block / classify / tape_plan before the
 * planner was split off -- never by running the planner.  One line per case ("group/name ok" or "... FAIL ..."), "OK" at the end
 * when all passed.  Run by tests/test_plan_cpu.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_amd.h"
#include "skred_bank_plan.h"

static int failures;
static const char *group_name, *case_name;
static int case_bad;

static void begin(const char *group, const char *name) { group_name = group; case_name = name; case_bad = 0; }
static void end(void) {
  if (!case_bad) printf("%s/%s ok\n", group_name, case_name);
  failures += case_bad;
}
#define EXPECT(what, want)                                                                                   \
  do {                                                                                                       \
    const long long got_ = (long long)(what), want_ = (long long)(want);                                     \
    if (got_ != want_) { printf("%s/%s FAIL %s = %lld, expected %lld\n", group_name, case_name, #what, got_, want_); case_bad = 1; } \
  } while (0)

#define CLEAN (SKM_FAST | SKM_FILTER_ALL | SKM_ENV_ALL)

/* 256 CUs, an LDS-resident pool, clean filtered bank with envelopes, truncating lookup, 512 frames, no stems / probe / taps, the
 * options a new bank has (skred_bank_create) */
static sk_plan_in_t bank_of(int n_voices) {
  sk_plan_in_t in;
  memset(&in, 0, sizeof(in));
  in.n_voices = n_voices;
  in.n_groups = (n_voices + 1023) / 1024 * 4;
  in.n_padded = in.n_groups * 256;
  in.n_cus = 256;
  in.fast_mode = CLEAN;
  in.cnt_real = n_voices;
  in.lds_table_floats = 4120;
  in.split_lds4 = 40000;
  in.num_frames = 512;
  in.interp = SKRED_INTERP_TRUNCATE;
  in.fast2_min_voices = 212992;
  in.fm2_min_voices = 1024;
  in.pack_mode = 1;
  in.fm_skew = 1;
  in.in_place_mode = 1;
  return in;
}

static sk_plan_t plan_of(const sk_plan_in_t *in, int most) {
  sk_plan_t p;
  sk_plan_family(in, &p);
  sk_plan_finish(in, most, &p);
  return p;
}

/* the issue's table, under every combination of the hints a row calls "any" */
static void family_cases(void) {
  for (int h = 0; h < 8; h++) {
    char name[64];
    sk_plan_in_t in = bank_of(4096);
    in.env_quiet = h & 1; in.list_empty = (h >> 1) & 1; in.last_family = (h & 4) ? SKRED_KERNEL_FAST2 : SKRED_KERNEL_FAST;
    snprintf(name, sizeof(name), "4096 dense, hints %d", h);
    begin("family", name);
    sk_plan_t p = plan_of(&in, 64);
    EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.n_wg, 16); EXPECT(p.pack_s, 0); EXPECT(p.one_env, 1); EXPECT(p.two_env, 0);
    EXPECT(p.interp, 0); EXPECT(p.modulated, 0); EXPECT(p.pack_shift, 6); EXPECT(p.rc, 0);
    end();

    in = bank_of(1048576);
    in.env_quiet = h & 1; in.list_empty = (h >> 1) & 1; in.last_family = (h & 4) ? SKRED_KERNEL_FAST2 : SKRED_KERNEL_FAST;
    snprintf(name, sizeof(name), "2^20 dense, hints %d", h);
    begin("family", name);
    p = plan_of(&in, 64);
    EXPECT(p.kernel, SKRED_KERNEL_FAST2); EXPECT(p.n_wg, 1024); EXPECT(p.pack_s, 0); EXPECT(p.two_env, 1); EXPECT(p.one_env, 0);
    end();

    snprintf(name, sizeof(name), "2^20 most 4 lanes, hints %d", h);
    begin("family", name);
    p = plan_of(&in, 4);
    EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.pack_s, 4); EXPECT(p.pack_shift, 2); EXPECT(p.pack_groups, 16384);
    EXPECT(p.pack_passes, 256); EXPECT(p.n_wg, 256); EXPECT(p.fast_mode & SKM_TWO_PER_LANE, 0); EXPECT(p.one_env, 1);
    end();

    snprintf(name, sizeof(name), "2^20 most 32 lanes, hints %d", h);
    begin("family", name);
    p = plan_of(&in, 32);
    EXPECT(p.kernel, SKRED_KERNEL_FAST2); EXPECT(p.pack_s, 0); EXPECT(p.pack_shift, 6); EXPECT(p.n_wg, 1024);
    end();

    in.features = SKB_ANY_MOD;
    snprintf(name, sizeof(name), "2^20 most 32 lanes modulated, hints %d", h);
    begin("family", name);
    p = plan_of(&in, 32);
    EXPECT(p.kernel, SKRED_KERNEL_MODULATED); EXPECT(p.modulated, 1); EXPECT(p.pack_s, 32); EXPECT(p.pack_shift, 5);
    EXPECT(p.pack_passes, 2048); EXPECT(p.n_wg, 2048); EXPECT(p.two_env, 0); EXPECT(p.one_env, 0);
    end();
  }
  sk_plan_in_t in = bank_of(262144);
  begin("family", "2^18 dense, envelopes moving");            /* below SK_FAST2_MOTION_MIN_VOICES */
  sk_plan_t p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.n_wg, 1024); EXPECT(p.one_env, 1);
  end();
  in.env_quiet = 1;
  begin("family", "2^18 dense, envelopes quiet");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST2); EXPECT(p.n_wg, 256); EXPECT(p.two_env, 1);
  end();

  in = bank_of(294912);                                       /* 288 passes of 1024: 256 < 288 <= 256 + 160 */
  in.last_family = SKRED_KERNEL_FAST; in.env_quiet = 1;
  begin("family", "294912 dense, quiet: second layer under five eighths");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.n_wg, 1152);
  end();
  in.env_quiet = 0;
  begin("family", "294912 dense, moving");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST2); EXPECT(p.n_wg, 288);
  end();
  in.last_family = SKRED_KERNEL_FAST2; in.list_empty = 1;     /* the two-per-lane family's own word for "quiet" */
  begin("family", "294912 dense, last block two-per-lane with an empty list");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.n_wg, 1152);
  end();

  in = bank_of(458752);                                       /* 448 passes > 416 */
  in.last_family = SKRED_KERNEL_FAST; in.env_quiet = 1;
  begin("family", "458752 dense, quiet: second layer over five eighths");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST2); EXPECT(p.n_wg, 448);
  end();
  in = bank_of(425984);                                       /* 416 passes: the last size the rule takes */
  in.last_family = SKRED_KERNEL_FAST; in.env_quiet = 1;
  begin("family", "425984 dense, quiet: exactly five eighths");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST);
  end();

  in = bank_of(212992 - 1024);
  in.env_quiet = 1;
  begin("family", "one pass below the two-per-lane crossover");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST);
  end();
  in = bank_of(212992);
  in.env_quiet = 1;
  begin("family", "at the two-per-lane crossover");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST2); EXPECT(p.n_wg, 208);
  end();
  in.force_generic = 1;
  begin("family", "force_generic");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_GENERIC); EXPECT(p.fast_mode, 0); EXPECT(p.n_wg, 832); EXPECT(p.two_env, 0); EXPECT(p.one_env, 0);
  end();
}

static void stems_cases(void) {
  sk_plan_in_t in = bank_of(1048576);
  in.stems = 1;
  begin("stems", "2^20 dense");
  sk_plan_t p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.n_wg, 2048); EXPECT(p.pack_candidate, 0);
  end();
  begin("stems", "2^20 most 4 lanes");
  p = plan_of(&in, 4);
  EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.pack_s, 0); EXPECT(p.pack_candidate, 0);
  end();
  in.fast_mode = SKM_FAST | SKM_FM;
  begin("stems", "FM bank: no skew");
  p = plan_of(&in, 64);
  EXPECT(p.fm_skew, 0);
  end();
  in.stems = 0;
  begin("stems", "FM bank without stems: skew");
  p = plan_of(&in, 64);
  EXPECT(p.fm_skew, 1); EXPECT(p.kernel, SKRED_KERNEL_FAST);
  end();
  in.features = SKB_ANY_MOD; in.stems = 1;
  begin("stems", "modulated bank: neither skew nor packing");
  p = plan_of(&in, 4);
  EXPECT(p.fm_skew, 0); EXPECT(p.pack_s, 0); EXPECT(p.kernel, SKRED_KERNEL_MODULATED);
  end();
  in = bank_of(4096);
  in.fast_mode = SKM_FAST | SKM_FM | SKM_FM_PAIR; in.stems = 1;
  begin("stems", "FM pairs stay one per lane");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.fast_mode & (SKM_FM_PAIR | SKM_TWO_PER_LANE), 0);
  end();
}

static void min_user_cases(void) {
  sk_plan_in_t in = bank_of(294912);
  in.last_family = SKRED_KERNEL_FAST; in.env_quiet = 1; in.fast2_min_user = 1; in.fast2_min_voices = 1000;
  begin("fast2_min_user", "294912 quiet: the five-eighths rule is off");
  sk_plan_t p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST2); EXPECT(p.n_wg, 288);
  end();
  in = bank_of(262144);
  in.fast2_min_user = 1; in.fast2_min_voices = 1000;
  begin("fast2_min_user", "2^18 moving: the moving-envelope rule is off");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST2);
  end();
  in = bank_of(4096);
  in.lds_table_floats = 0; in.fast2_min_user = 1; in.fast2_min_voices = 1024;
  begin("fast2_min_user", "global-table bank goes two-per-lane: 512-voice passes");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST2); EXPECT(p.n_wg, 8);
  end();
  in = bank_of(1048576);
  in.lds_table_floats = 0;
  begin("fast2_min_user", "global-table bank without it stays one per lane");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.n_wg, 2048);
  end();
  in = bank_of(4096);
  in.fast2_min_user = 1; in.fast2_min_voices = 8192;
  begin("fast2_min_user", "below the caller's threshold");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST);
  end();
}

static void fm_pair_cases(void) {
  sk_plan_in_t in = bank_of(1024);
  in.fast_mode = SKM_FAST | SKM_FM | SKM_FM_PAIR | SKM_PAIR_AP; in.features = SKB_ANY_FM; in.cnt_fm = 512;
  begin("fm_pair", "1024 voices");
  sk_plan_t p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST2); EXPECT(p.n_wg, 1); EXPECT(p.fast_mode & SKM_FM_PAIR, SKM_FM_PAIR);
  EXPECT(p.fast_mode & SKM_PAIR_AP, SKM_PAIR_AP); EXPECT(p.modulated, 0); EXPECT(p.two_env, 0); EXPECT(p.pack_candidate, 0);
  end();
  in.n_taps = 1;
  begin("fm_pair", "1024 voices with taps");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.fast_mode & (SKM_FM_PAIR | SKM_PAIR_AP | SKM_TWO_PER_LANE), 0); EXPECT(p.fm_skew, 1);
  end();
  in = bank_of(1023);
  in.fast_mode = SKM_FAST | SKM_FM | SKM_FM_PAIR; in.features = SKB_ANY_FM; in.cnt_fm = 511;
  begin("fm_pair", "1023 voices");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.fast_mode & (SKM_FM_PAIR | SKM_TWO_PER_LANE), 0);
  end();
  in = bank_of(4096);
  in.fast_mode = SKM_FAST | SKM_FM | SKM_FM_PAIR; in.features = SKB_ANY_FM; in.cnt_fm = 2048; in.lds_table_floats = 0;
  begin("fm_pair", "global-table bank");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.fm_skew, 0);
  end();
  in.lds_table_floats = 4120; in.force_generic = 1;            /* previous-frame FM off the specialised kernels: modulated */
  begin("fm_pair", "force_generic");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_MODULATED); EXPECT(p.modulated, 1);
  end();
}

static void guard_cases(void) {
  sk_plan_in_t in = bank_of(4096);
  in.interp = SKRED_INTERP_LINEAR; in.cnt_real = 100; in.cnt_guard = 100; in.guard_current = 1;
  begin("guard", "every real voice guarded, pool current");
  EXPECT(plan_of(&in, 64).interp, 2);
  end();
  in.cnt_guard = 99;
  begin("guard", "one voice without the guard");
  EXPECT(plan_of(&in, 64).interp, 1);
  end();
  in.cnt_guard = 100; in.guard_current = 0;
  begin("guard", "flags of an older pool");
  EXPECT(plan_of(&in, 64).interp, 1);
  end();
  in.guard_current = 1; in.interp = SKRED_INTERP_TRUNCATE;
  begin("guard", "truncating lookup");
  EXPECT(plan_of(&in, 64).interp, 0);
  end();
  in.interp = SKRED_INTERP_LINEAR; in.cnt_real = in.cnt_guard = 0;
  begin("guard", "no real voice");
  EXPECT(plan_of(&in, 64).interp, 1);
  end();
  in.cnt_real = in.cnt_guard = 100; in.fast_mode = SKM_FAST | SKM_FM | SKM_FM_PAIR;
  begin("guard", "two-operator FM keeps the general form");
  EXPECT(plan_of(&in, 64).interp, 1);
  end();
  in.fast_mode = CLEAN; in.features = SKB_ANY_MOD;
  begin("guard", "modulated");
  EXPECT(plan_of(&in, 64).interp, 1);
  end();
  in.features = 0; in.force_generic = 1;
  begin("guard", "generic");
  EXPECT(plan_of(&in, 64).interp, 1);
  end();
}

static void pack_mode_cases(void) {
  sk_plan_in_t in = bank_of(4096);
  in.pack_mode = 2;
  begin("pack", "mode 2, 4096 voices, most 8 lanes");
  sk_plan_t p = plan_of(&in, 8);
  EXPECT(p.pack_s, 8); EXPECT(p.pack_shift, 3); EXPECT(p.pack_groups, 64); EXPECT(p.pack_passes, 2); EXPECT(p.n_wg, 2);
  EXPECT(p.kernel, SKRED_KERNEL_FAST);
  end();
  begin("pack", "mode 2, most 5 lanes round up to 8");
  EXPECT(plan_of(&in, 5).pack_s, 8);
  end();
  begin("pack", "mode 2, 4096 voices, most 64 lanes");
  p = plan_of(&in, 64);
  EXPECT(p.pack_s, 0); EXPECT(p.pack_shift, 6); EXPECT(p.n_wg, 16);
  end();
  begin("pack", "mode 2, most 33 lanes round up to 64");
  EXPECT(plan_of(&in, 33).pack_s, 0);
  end();
  in.pack_mode = 1;
  begin("pack", "mode 1, 4096 voices, most 8 lanes: too small to pay");
  EXPECT(plan_of(&in, 8).pack_s, 0);
  end();
  in.pack_mode = 0;
  begin("pack", "mode 0");
  p = plan_of(&in, 8);
  EXPECT(p.pack_candidate, 0); EXPECT(p.pack_s, 0);
  end();
  in = bank_of(196608);                                        /* 768 groups = 3 x 256 CUs: the first size that packs by itself */
  begin("pack", "mode 1, 196608 voices, most 32 lanes");
  p = plan_of(&in, 32);
  EXPECT(p.pack_s, 32); EXPECT(p.pack_passes, 384); EXPECT(p.n_wg, 384);
  end();
  in = bank_of(196608 - 1024);
  begin("pack", "mode 1, one pass smaller");
  EXPECT(plan_of(&in, 32).pack_s, 0);
  end();
  in = bank_of(1048576);
  begin("pack", "two-per-lane bank, most 16 lanes");
  p = plan_of(&in, 16);
  EXPECT(p.pack_s, 16); EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.pack_passes, 1024);
  end();
}

static void probe_cases(void) {
  sk_plan_in_t in = bank_of(4096);
  in.n_probe = 2;
  begin("probe", "one-voice family");
  sk_plan_t p = plan_of(&in, 64);
  EXPECT(p.rc, 0); EXPECT(p.kernel, SKRED_KERNEL_FAST);
  end();
  in.force_generic = 1;
  begin("probe", "generic");
  p = plan_of(&in, 64);
  EXPECT(p.rc, SKRED_E_UNSUPPORTED); EXPECT(p.msg && strstr(p.msg, "a probe is set, but this block would run a kernel without probe instantiations") == p.msg, 1);
  end();
  in.force_generic = 0; in.features = SKB_ANY_MOD;
  begin("probe", "modulated");
  EXPECT(plan_of(&in, 64).rc, SKRED_E_UNSUPPORTED);
  end();
  in.features = 0; in.fast_mode = SKM_FAST | SKM_FM | SKM_FM_PAIR;
  begin("probe", "FM pairs");
  EXPECT(plan_of(&in, 64).rc, SKRED_E_UNSUPPORTED);
  end();
  in.fast_mode = CLEAN; in.stems = 1;
  begin("probe", "stems");
  EXPECT(plan_of(&in, 64).rc, SKRED_E_UNSUPPORTED);
  end();
  in = bank_of(1048576);
  in.n_probe = 1;
  begin("probe", "two-per-lane family");
  p = plan_of(&in, 64);
  EXPECT(p.rc, 0); EXPECT(p.kernel, SKRED_KERNEL_FAST2);
  end();
  in = bank_of(4096);
  in.n_probe = 1; in.split_mode = 2; in.env_quiet = 1;
  begin("probe", "a probe turns the split form off");
  EXPECT(plan_of(&in, 64).split, 0);
  end();
}

static void split_cases(void) {
  static const int voices[] = { 31744, 32768, 65536, 66560 }, in_window[] = { 0, 4, 4, 0 };   /* 124, 128, 256, 260 groups on 256 CUs */
  char name[64];
  for (int i = 0; i < 4; i++) {
    sk_plan_in_t in = bank_of(voices[i]);
    in.split_mode = 1; in.env_quiet = 1;
    snprintf(name, sizeof(name), "option 1, %d voices", voices[i]);
    begin("split", name);
    sk_plan_t p = plan_of(&in, 64);
    EXPECT(p.split, in_window[i]); EXPECT(p.fast_mode & SKM_SPLIT, in_window[i] ? SKM_SPLIT : 0); EXPECT(p.fast_mode & SKM_SPLIT2, 0);
    EXPECT(p.n_wg, in.n_groups);
    end();
    in.fast_mode = SKM_FAST | SKM_ENV_ALL;
    snprintf(name, sizeof(name), "option 1 without the filter, %d voices", voices[i]);
    begin("split", name);
    EXPECT(plan_of(&in, 64).split, 0);
    end();
    for (int mode = 2; mode <= 3; mode++) {
      in.split_mode = mode;
      snprintf(name, sizeof(name), "option %d, %d voices", mode, voices[i]);
      begin("split", name);
      EXPECT(plan_of(&in, 64).split, 4);
      end();
    }
  }
  for (int mode = 1; mode <= 3; mode++) {
    sk_plan_in_t in = bank_of(32768);
    in.split_mode = mode;                                      /* env_quiet 0: envelopes may move */
    snprintf(name, sizeof(name), "option %d while envelopes may move", mode);
    begin("split", name);
    EXPECT(plan_of(&in, 64).split, mode == 3 ? 4 : 0);
    end();
    in.fast_mode = SKM_FAST | SKM_FILTER_ALL;                  /* no envelope: always steady */
    snprintf(name, sizeof(name), "option %d without envelopes", mode);
    begin("split", name);
    EXPECT(plan_of(&in, 64).split, 4);
    end();
    in.n_taps = 3;
    snprintf(name, sizeof(name), "option %d with taps", mode);
    begin("split", name);
    sk_plan_t p = plan_of(&in, 64);
    EXPECT(p.split, 0); EXPECT(p.fast_mode & (SKM_SPLIT | SKM_SPLIT2), 0); EXPECT(p.kernel, SKRED_KERNEL_FAST);
    end();
    in.n_taps = 0; in.split_lds4 = 160 * 1024 + 4;
    snprintf(name, sizeof(name), "option %d, workgroup larger than a CU's LDS", mode);
    begin("split", name);
    EXPECT(plan_of(&in, 64).split, 0);
    end();
    in.split_lds4 = 160 * 1024;
    snprintf(name, sizeof(name), "option %d, workgroup exactly a CU's LDS", mode);
    begin("split", name);
    EXPECT(plan_of(&in, 64).split, 4);
    end();
  }
  static const uint32_t not_clean[] = { SKM_STOPS, SKM_FM, SKM_MIXED };
  for (int i = 0; i < 3; i++) {
    sk_plan_in_t in = bank_of(32768);
    in.split_mode = 3; in.fast_mode = SKM_FAST | SKM_FILTER_ALL | not_clean[i];
    snprintf(name, sizeof(name), "option 3, mode bit %u", not_clean[i]);
    begin("split", name);
    EXPECT(plan_of(&in, 64).split, 0);
    end();
  }
  sk_plan_in_t in = bank_of(32768);
  in.split_mode = 3; in.lds_table_floats = 0;
  begin("split", "global-table bank");
  EXPECT(plan_of(&in, 64).split, 0);
  end();
  in = bank_of(1048576);
  in.split_mode = 3;
  begin("split", "two-per-lane bank");
  EXPECT(plan_of(&in, 64).split, 0);
  end();
  begin("split", "packed bank");
  EXPECT(plan_of(&in, 4).split, 0);
  end();
  in = bank_of(4096);
  in.split_mode = 2; in.env_quiet = 1; in.split_pairs = 2;
  begin("split", "two pairs forced");
  sk_plan_t p = plan_of(&in, 64);
  EXPECT(p.split, 2); EXPECT(p.n_wg, 32); EXPECT(p.fast_mode & (SKM_SPLIT | SKM_SPLIT2), SKM_SPLIT | SKM_SPLIT2);
  end();
  in = bank_of(1025 * 256);                                     /* 1028 groups: twice that is past SK_MAX_WORKGROUPS */
  in.split_mode = 2; in.env_quiet = 1; in.split_pairs = 2; in.fast2_min_voices = 1 << 30;
  begin("split", "two pairs forced on a bank with too many half passes");
  p = plan_of(&in, 64);
  EXPECT(p.split, 4); EXPECT(p.n_wg, 1028);
  end();
}

/* a two-per-lane bank with envelopes whose list is known: last block two-per-lane, list not empty, a valid bound */
static sk_plan_in_t listed(int n_voices, uint64_t bound) {
  sk_plan_in_t in = bank_of(n_voices);
  in.env_quiet = 1;                                            /* (2^18 voices stay two-per-lane only while nothing moves) */
  in.last_family = SKRED_KERNEL_FAST2;
  in.bound_valid = 1;
  in.bound = bound;
  return in;
}

static void inplace_cases(void) {
  /* mode 1 on 256 CUs: 512 workgroup slots, passes of 1024 voices; the limit each of the rule's three branches gives:
   *   2^18: 256 passes = no full round, last round 256 (rounds == 0)          -> n / 600 = 436
   *   2^19: 512 passes = 1 round, last round empty                             -> n / 128 = 4096
   *   2^20: 1024 passes = 2 rounds, last round empty                           -> n / 256 = 4096
   *   786432: 768 passes = 1 round + 256 (256 * 20 <= 512 * 11: at most 55 %)  -> n / 600 = 1310
   *   812032: 793 passes = 1 round + 281 (5620 <= 5632: the last count inside) -> n / 600 = 1353
   *   813056: 794 passes = 1 round + 282 (5640 > 5632: fuller)                 -> 0
   *   831488: 812 passes = 1 round + 300                                       -> 0 */
  static const struct { int n; uint64_t limit; } c[] = {
    { 262144, 436 }, { 524288, 4096 }, { 1048576, 4096 }, { 786432, 1310 }, { 812032, 1353 }, { 813056, 0 }, { 831488, 0 } };
  char name[64];
  for (size_t i = 0; i < sizeof(c) / sizeof(c[0]); i++) {
    const int n = c[i].n, n_groups = (n + 1023) / 1024 * 4;
    for (int d = -1; d <= 1; d++) {
      if (d < 0 && c[i].limit == 0) continue;
      sk_plan_in_t in = listed(n, c[i].limit + (uint64_t)d);
      snprintf(name, sizeof(name), "mode 1, %d voices, bound %llu", n, (unsigned long long)in.bound);
      begin("inplace", name);
      sk_plan_t p = plan_of(&in, 64);
      EXPECT(p.kernel, SKRED_KERNEL_FAST2); EXPECT(p.two_env, 1); EXPECT(p.list_rebuild, 0);
      EXPECT(p.inplace, d <= 0);
      if (d <= 0) { EXPECT(p.own, (size_t)n_groups * 4 * 8); EXPECT(p.rows, (size_t)n_groups * 4 * 8 + (size_t)n / 64 + 64); EXPECT(p.stride, 512 + 8); }
      end();
    }
  }
  sk_plan_in_t in = listed(524288, 87000);                     /* mode 2: wherever the rows suffice: n / 6 + 64 = 87445 overflow rows */
  in.in_place_mode = 2;
  begin("inplace", "mode 2 takes a list mode 1 refuses");
  sk_plan_t p = plan_of(&in, 64);
  EXPECT(p.inplace, 1); EXPECT(p.rows, 2048 * 32 + 87381 + 64); EXPECT(p.own, 2048 * 32);
  end();
  in.bound = 87446;
  begin("inplace", "mode 2, bound past the overflow rows");
  EXPECT(plan_of(&in, 64).inplace, 0);
  end();
  in.bound = 87445; in.num_frames = 8000;                      /* 152981 rows x 8008 floats x 4 bytes > 4 GiB */
  begin("inplace", "mode 2, rows past 4 GiB");
  EXPECT(plan_of(&in, 64).inplace, 0);
  end();
  in = listed(524288, 10);
  in.in_place_mode = 0;
  begin("inplace", "mode 0");
  EXPECT(plan_of(&in, 64).inplace, 0);
  end();
  in = listed(524288, 10);
  in.list_empty = 1;
  begin("inplace", "empty list");
  EXPECT(plan_of(&in, 64).inplace, 0);
  end();
  in = listed(524288, 10);
  in.bound_valid = 0;
  begin("inplace", "no bound yet");
  EXPECT(plan_of(&in, 64).inplace, 0);
  end();
  in = listed(524288, 10);
  in.mask_dirty = 1;
  begin("inplace", "stale list: rebuilt, length unknown");
  p = plan_of(&in, 64);
  EXPECT(p.list_rebuild, 1); EXPECT(p.inplace, 0);
  end();
  in = listed(524288, 10);
  in.last_family = SKRED_KERNEL_FAST;
  begin("inplace", "another family rendered the last block");
  p = plan_of(&in, 64);
  EXPECT(p.list_rebuild, 1); EXPECT(p.inplace, 0);
  end();
  in = listed(524288, 10);
  in.lds_table_floats = 0; in.fast2_min_user = 1;
  begin("inplace", "global-table bank");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST2); EXPECT(p.inplace, 0);
  end();
  in = listed(524288, 10);
  in.fast_mode = SKM_FAST | SKM_FILTER_ALL;
  begin("inplace", "no envelopes: no list");
  p = plan_of(&in, 64);
  EXPECT(p.two_env, 0); EXPECT(p.list_rebuild, 0); EXPECT(p.inplace, 0);
  end();
}

static void class_cases(void) {
  begin("class", "no real voice");
  EXPECT(sk_plan_class_mode(0, 0, 0, 0, 0, 0, 0, 0), 0);
  end();
  begin("class", "exotic voice");
  EXPECT(sk_plan_class_mode(10, 10, 10, 1, 0, 0, 0, 0), 0);
  end();
  begin("class", "neither filter nor envelope");
  EXPECT(sk_plan_class_mode(10, 0, 0, 0, 0, 0, 0, 0), SKM_FAST);
  end();
  begin("class", "all filtered, all with envelopes");
  EXPECT(sk_plan_class_mode(10, 10, 10, 0, 0, 0, 0, 0), CLEAN);
  end();
  begin("class", "some filtered");
  EXPECT(sk_plan_class_mode(10, 4, 0, 0, 0, 0, 0, 0), SKM_FAST | SKM_FILTER_ALL | SKM_MIXED);
  end();
  begin("class", "some with envelopes");
  EXPECT(sk_plan_class_mode(10, 10, 9, 0, 0, 0, 0, 0), CLEAN | SKM_MIXED);
  end();
  begin("class", "stops");
  EXPECT(sk_plan_class_mode(10, 0, 10, 0, 2, 0, 0, 0), SKM_FAST | SKM_ENV_ALL | SKM_STOPS);
  end();
  begin("class", "FM pairs");
  EXPECT(sk_plan_class_mode(10, 0, 0, 0, 0, 5, 0, 0), SKM_FAST | SKM_FM | SKM_FM_PAIR);
  end();
  begin("class", "FM, one carrier not pair-shaped");
  EXPECT(sk_plan_class_mode(10, 0, 0, 0, 0, 5, 1, 0), SKM_FAST | SKM_FM);
  end();
  begin("class", "FM pairs with a stopping voice");
  EXPECT(sk_plan_class_mode(10, 0, 0, 0, 1, 5, 0, 0), SKM_FAST | SKM_FM | SKM_STOPS);
  end();
  begin("class", "FM pairs with amplitude or pan modulation");
  EXPECT(sk_plan_class_mode(10, 0, 0, 0, 0, 5, 0, 2), SKM_FAST | SKM_FM | SKM_FM_PAIR | SKM_PAIR_AP);
  end();
  begin("class", "PAIR_AP only together with FM_PAIR");
  EXPECT(sk_plan_class_mode(10, 0, 0, 0, 0, 5, 1, 2), SKM_FAST | SKM_FM);
  EXPECT(sk_plan_class_mode(10, 0, 0, 0, 0, 0, 0, 2), SKM_FAST);
  end();
}

/* ---- the dependency levels: two 64-voice groups, the shapes tests/mod_forms.py: levels() walks ---- */
static void level_cases(void) {
  enum { N = 128 };
  int8_t mod[4 * N];
  int level[N], want[N];
  memset(mod, -1, sizeof(mod));
  memset(want, 0, sizeof(want));
  for (int i = 0; i < N; i++) level[i] = 99;                   /* (stale values of an earlier routing) */
  mod[0 * N + 1] = 0;  want[1] = 1;                            /* fm by the voice below */
  mod[1 * N + 2] = 1;  want[2] = 2;                            /* am by a voice that is itself modulated */
  mod[2 * N + 3] = 10; want[3] = 0;                            /* a modulator ABOVE its reader (previous-frame value): no level */
  mod[3 * N + 10] = 3; want[10] = 1;
  mod[0 * N + 5] = 5;  want[5] = 0;                            /* itself */
  mod[0 * N + 64 + 4] = 2;  want[64 + 4] = 1;                  /* second group: lanes count inside the group */
  mod[0 * N + 64 + 5] = 4; mod[1 * N + 64 + 5] = 2; want[64 + 5] = 2;   /* the highest of its modulators counts */
  mod[2 * N + 64 + 63] = 5; want[64 + 63] = 3;
  begin("levels", "two groups");
  EXPECT(sk_plan_levels(mod, N, level), 3);
  for (int i = 0; i < N; i++) if (level[i] != want[i]) { printf("levels/two groups FAIL level[%d] = %d, expected %d\n", i, level[i], want[i]); case_bad = 1; }
  end();
  memset(mod, -1, sizeof(mod));
  mod[0 * N + 3] = 40; mod[1 * N + 40] = 63;
  begin("levels", "only modulators above their readers");
  EXPECT(sk_plan_levels(mod, N, level), 0);
  for (int i = 0; i < N; i++) EXPECT(level[i], 0);
  end();
}

/* ---- the tape plan ---- */
enum { TG = 20, TN = TG * 64 };
static int32_t esc[4 * TN], slot[TN], groups[TG];
static uint8_t dirty[TG];
static int level_off[SK_TAPE_MAX_LEVELS + 1], n_levels;
static char msg[256];

static int tape(void) {
  memset(dirty, 0, sizeof(dirty));
  memset(level_off, -1, sizeof(level_off));
  memset(groups, -1, sizeof(groups));
  msg[0] = 0;
  return sk_tape_plan_host(esc, TN, slot, dirty, groups, level_off, &n_levels, msg, sizeof(msg));
}
static void tape_reset(void) {
  memset(esc, -1, sizeof(esc));
  for (int v = 0; v < TN; v++) slot[v] = -1;
}
static int sources_left(void) { int n = 0; for (int v = 0; v < TN; v++) n += slot[v] != -1; return n; }

static void tape_cases(void) {
  tape_reset();
  esc[0 * TN + 0] = 70; esc[1 * TN + 1] = 70;                  /* voices 0 and 1 (group 0) read voice 70 (group 1) */
  slot[700] = 3;                                               /* a source of the previous plan */
  begin("tape", "two readers of one source");
  EXPECT(tape(), 1); EXPECT(n_levels, 1); EXPECT(level_off[0], 0); EXPECT(level_off[1], 1); EXPECT(groups[0], 1);
  EXPECT(slot[70], 0); EXPECT(slot[700], -1); EXPECT(sources_left(), 1);
  EXPECT(dirty[1], 1); EXPECT(dirty[700 / 64], 1); EXPECT(dirty[0], 0); EXPECT(dirty[2], 0);
  end();

  tape_reset();
  esc[0 * TN + 0] = 64; esc[2 * TN + 64] = 128;                /* A = voice 0 reads B = 64 reads C = 128 */
  begin("tape", "chain over three groups");
  EXPECT(tape(), 2); EXPECT(n_levels, 2);
  EXPECT(level_off[0], 0); EXPECT(level_off[1], 1); EXPECT(level_off[2], 2);
  EXPECT(groups[0], 2); EXPECT(groups[1], 1);                  /* C's group first: B's pre-pass reads C's tape row */
  EXPECT(slot[64], 0); EXPECT(slot[128], 1); EXPECT(sources_left(), 2);
  end();

  tape_reset();
  esc[0 * TN + 0] = 200; esc[1 * TN + 0] = 70;                 /* voice 0 reads voices 200 (group 3) and 70 (group 1) */
  begin("tape", "two source groups on one level, ascending");
  EXPECT(tape(), 2); EXPECT(n_levels, 1); EXPECT(level_off[0], 0); EXPECT(level_off[1], 2);
  EXPECT(groups[0], 1); EXPECT(groups[1], 3);
  EXPECT(slot[200], 0); EXPECT(slot[70], 1);                   /* slots in the order the first reader names them */
  end();

  tape_reset();
  esc[0 * TN + 300] = 5; esc[0 * TN + 301] = 900; esc[1 * TN + 5] = 901; esc[0 * TN + 130] = 5;   /* groups 4 -> 0, 14; 0 -> 14; 2 -> 0 */
  begin("tape", "a source group that reads another, readers in three groups");
  EXPECT(tape(), 3); EXPECT(n_levels, 2);
  EXPECT(level_off[0], 0); EXPECT(level_off[1], 1); EXPECT(level_off[2], 2);
  EXPECT(groups[0], 14); EXPECT(groups[1], 0);
  EXPECT(slot[901], 0); EXPECT(slot[5], 1); EXPECT(slot[900], 2);   /* first named by voice 5, by voice 130, by voice 301 */
  end();

  tape_reset();
  esc[0 * TN + 0] = 64; esc[0 * TN + 64] = 0;
  begin("tape", "two-group cycle");
  EXPECT(tape(), SKRED_E_UNSUPPORTED);
  EXPECT(strcmp(msg, "cross-group modulation: the groups of voice 64 and voice 0 read each other (a cycle between 64-voice groups: "
                     "voice 64 reads voice 0)"), 0);
  EXPECT(sources_left(), 0);
  end();

  /* group i reads group i + 1, for i = 0 .. k - 1: k source groups in a chain; group 1 sits on pre-pass level k - 1 */
  for (int k = 16; k <= 17; k++) {
    tape_reset();
    for (int i = 0; i < k; i++) esc[0 * TN + 64 * i] = 64 * (i + 1);
    begin("tape", k == 16 ? "chain 16 groups deep" : "chain 17 groups deep");
    if (k == 16) {
      EXPECT(tape(), 16); EXPECT(n_levels, 16);
      for (int l = 0; l < 16; l++) { EXPECT(level_off[l], l); EXPECT(groups[l], 16 - l); }
      EXPECT(level_off[16], 16);
    } else {
      EXPECT(tape(), SKRED_E_UNSUPPORTED);
      EXPECT(strstr(msg, "at most 16 pre-pass levels") != NULL, 1);
      EXPECT(strstr(msg, "a chain of groups 17 deep (voice 64 reads voice 128, which ...)") != NULL, 1);
      EXPECT(sources_left(), 0);
    }
    end();
  }

  tape_reset();
  slot[3] = 0; slot[640] = 1;
  begin("tape", "no cross-group edge");
  EXPECT(tape(), 0); EXPECT(n_levels, 0); EXPECT(sources_left(), 0); EXPECT(dirty[0], 1); EXPECT(dirty[10], 1); EXPECT(dirty[1], 0);
  end();
}

int main(void) {
  family_cases();
  stems_cases();
  min_user_cases();
  fm_pair_cases();
  guard_cases();
  pack_mode_cases();
  probe_cases();
  split_cases();
  inplace_cases();
  class_cases();
  level_cases();
  tape_cases();
  if (failures) { printf("%d case(s) failed\n", failures); return 1; }
  printf("OK\n");
  return 0;
}
