/* SKRED_OPT_CZ_FAST in the block planner (skred_amd/csrc/skred_bank_plan.h, linked from libskred_amd.so): no bank, no HIP.  The
 * expected values are worked out by hand from the rule in the header comment of include/skred_amd.h (SKRED_OPT_CZ_FAST) and
 * DESIGN "CZ on the one-voice kernel" -- never by running the planner.  One line per case ("cz/name ok" or "... FAIL ..."), "OK"
 * at the end when all passed.  Run by tests/test_plan_cz_cpu.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_amd.h"
#include "skred_bank_plan.h"

static int failures;
static const char *case_name;
static int case_bad;

static void begin(const char *name) { case_name = name; case_bad = 0; }
static void end(void) {
  if (!case_bad) printf("cz/%s ok\n", case_name);
  failures += case_bad;
}
#define EXPECT(what, want)                                                                                   \
  do {                                                                                                       \
    const long long got_ = (long long)(what), want_ = (long long)(want);                                     \
    if (got_ != want_) { printf("cz/%s FAIL %s = %lld, expected %lld\n", case_name, #what, got_, want_); case_bad = 1; } \
  } while (0)

/* A bank of n_voices real voices, all filtered and enveloped, n_cz of them qualifying CZ voices (n_cz_src of those with a
 * previous-frame source), n_fm plain carriers of a modulator above them that are no (even voice, next voice) pairs, no other
 * exotic voice: what skred_bank.c: sk_classify hands the planner.  256 CUs, an LDS-resident pool, 512 frames, default options. */
static sk_plan_in_t cz_bank(int n_voices, int n_cz, int n_cz_src, int n_fm) {
  sk_plan_in_t in;
  memset(&in, 0, sizeof(in));
  in.n_voices = n_voices;
  in.n_groups = (n_voices + 1023) / 1024 * 4;
  in.n_padded = in.n_groups * 256;
  in.n_cus = 256;
  /* the class as it stands today: the CZ voices are exotic */
  in.fast_mode = sk_plan_class_mode(n_voices, n_voices, n_voices, n_cz, 0, n_fm, n_fm, 0);
  /* ... and with the qualifying CZ voices taken for what the one-voice kernel can render */
  in.fast_mode_cz = n_cz ? ((sk_plan_class_mode(n_voices, n_voices, n_voices, 0, 0, n_fm + n_cz_src, n_fm + n_cz_src, 0) & ~(SKM_FM_PAIR | SKM_PAIR_AP)) | SKM_CZ) : 0u;
  in.features = (n_cz ? SKB_ANY_CZ : 0u) | (n_fm ? SKB_ANY_FM : 0u);
  in.cnt_cz = n_cz;
  in.cnt_fm = n_fm;
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

static void expect_engaged(const sk_plan_t *p) {
  EXPECT(p->kernel, SKRED_KERNEL_FAST); EXPECT(p->cz, 1); EXPECT(p->modulated, 0);
  EXPECT(p->fast_mode & SKM_FAST, SKM_FAST); EXPECT(p->fast_mode & SKM_CZ, SKM_CZ);
  EXPECT(p->fast_mode & (SKM_TWO_PER_LANE | SKM_FM_PAIR | SKM_PAIR_AP | SKM_SPLIT | SKM_SPLIT2), 0); EXPECT(p->split, 0);
  EXPECT(p->two_env, 0); EXPECT(p->rc, 0);
}

int main(void) {
  const int sizes[3] = { 256, 4096, 1048576 };
  for (int s = 0; s < 3; s++) {
    char name[96];
    const int n = sizes[s];
    sk_plan_in_t in = cz_bank(n, n, 0, 0);

    snprintf(name, sizeof(name), "%d voices, option off: the modulated kernel as before", n);
    begin(name);
    sk_plan_t p = plan_of(&in, 64);
    EXPECT(p.kernel, SKRED_KERNEL_MODULATED); EXPECT(p.modulated, 1); EXPECT(p.cz, 0); EXPECT(p.fast_mode, 0); EXPECT(p.pack_s, 0);
    EXPECT(p.n_wg, in.n_groups < 2048 ? in.n_groups : 2048);
    /* ... the very plan a bank whose CZ voices carry SKB_ANY_MOD gets (what every CZ voice did before the option existed) */
    sk_plan_in_t old = in;
    old.features = SKB_ANY_MOD; old.cnt_cz = 0; old.fast_mode_cz = 0;
    sk_plan_t q = plan_of(&old, 64);
    EXPECT(p.kernel, q.kernel); EXPECT(p.fast_mode, q.fast_mode); EXPECT(p.n_wg, q.n_wg); EXPECT(p.interp, q.interp);
    EXPECT(p.fm_skew, q.fm_skew); EXPECT(p.pack_shift, q.pack_shift); EXPECT(p.pack_candidate, q.pack_candidate);
    end();

    snprintf(name, sizeof(name), "%d voices, option on: the one-voice kernel's CZ instantiation", n);
    begin(name);
    in.cz_fast = 1;
    p = plan_of(&in, 64);
    expect_engaged(&p);
    EXPECT(p.fast_mode & SKM_FM, 0); EXPECT(p.pack_s, 0); EXPECT(p.one_env, 1);
    EXPECT(p.n_wg, in.n_groups < 2048 ? in.n_groups : 2048);
    end();

    snprintf(name, sizeof(name), "%d voices, option on, every split / two-per-lane option forced", n);
    begin(name);
    in.split_mode = 3; in.split_pairs = 4; in.fast2_min_voices = 0; in.fast2_min_user = 1; in.fm2_min_voices = 0; in.env_quiet = 1;
    p = plan_of(&in, 64);
    expect_engaged(&p);
    end();
  }

  sk_plan_in_t in = cz_bank(4096, 1024, 512, 0);
  in.cz_fast = 1;
  begin("sources above the carrier: SKM_FM, and the skew stays on at plan level");
  sk_plan_t p = plan_of(&in, 64);
  expect_engaged(&p);
  EXPECT(p.fast_mode & SKM_FM, SKM_FM); EXPECT(p.fm_skew, 1);
  end();

  in = cz_bank(4096, 64, 0, 1024);
  in.cz_fast = 1;
  begin("a bank that also has FM carriers: SKM_FM, fm_skew 1");
  p = plan_of(&in, 64);
  expect_engaged(&p);
  EXPECT(p.fast_mode & SKM_FM, SKM_FM); EXPECT(p.fm_skew, 1);
  in.fm_skew = 0;
  p = plan_of(&in, 64);
  EXPECT(p.fm_skew, 0); EXPECT(p.cz, 1);
  end();

  in = cz_bank(4096, 4096, 0, 0);
  in.cz_fast = 1; in.lds_table_floats = 0;
  begin("global-table bank: modulated");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_MODULATED); EXPECT(p.cz, 0); EXPECT(p.modulated, 1);
  end();

  in = cz_bank(4096, 4096, 0, 0);
  in.cz_fast = 1; in.features |= SKB_ANY_MOD; in.cnt_mod = 1;
  begin("SKB_ANY_MOD present: modulated");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_MODULATED); EXPECT(p.cz, 0); EXPECT(p.modulated, 1);
  end();
  in.cnt_mod = 0;                                    /* (the voice that asked for it is gone; the feature word is only ever set) */
  begin("SKB_ANY_MOD left over, no voice needs it: option on engages, option off stays modulated");
  p = plan_of(&in, 64);
  expect_engaged(&p);
  in.cz_fast = 0;
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_MODULATED); EXPECT(p.cz, 0);
  end();

  in = cz_bank(4096, 4096, 0, 0);
  in.cz_fast = 1; in.force_generic = 1;
  begin("force_generic: modulated");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_MODULATED); EXPECT(p.cz, 0); EXPECT(p.fast_mode, 0);
  end();

  in = cz_bank(4096, 100, 0, 0);
  in.cz_fast = 1;
  in.fast_mode = 0; in.fast_mode_cz = 0;            /* (another exotic voice beside the CZ voices: no class for either family) */
  begin("another exotic voice in the bank: modulated");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_MODULATED); EXPECT(p.cz, 0);
  end();

  in = cz_bank(4096, 0, 0, 0);
  in.features = SKB_ANY_CZ;                          /* (the feature word is sticky: the last CZ voice was switched off) */
  begin("no CZ voice left, option off: the sticky feature keeps the modulated kernel, as before");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_MODULATED); EXPECT(p.cz, 0);
  end();
  in.cz_fast = 1;
  begin("no CZ voice left, option on: a clean bank again");
  p = plan_of(&in, 64);
  EXPECT(p.kernel, SKRED_KERNEL_FAST); EXPECT(p.cz, 0); EXPECT(p.modulated, 0); EXPECT(p.fast_mode & SKM_CZ, 0);
  end();

  in = cz_bank(1048576, 65536, 32768, 0);           /* 4 voices of 64 in use: 16384 groups at 4 lanes -> 256 passes */
  in.cz_fast = 1;
  begin("sparse 2^20-voice bank: packed lanes as any extended-instantiation bank");
  p = plan_of(&in, 4);
  expect_engaged(&p);
  EXPECT(p.pack_s, 4); EXPECT(p.pack_shift, 2); EXPECT(p.pack_groups, 16384); EXPECT(p.pack_passes, 256); EXPECT(p.n_wg, 256);
  end();
  in = cz_bank(1024, 64, 32, 0);
  in.cz_fast = 1; in.pack_mode = 2;
  begin("sparse small bank, SKRED_OPT_PACK 2");
  p = plan_of(&in, 4);
  expect_engaged(&p);
  EXPECT(p.pack_s, 4); EXPECT(p.pack_groups, 16); EXPECT(p.pack_passes, 1); EXPECT(p.n_wg, 1);
  end();

  in = cz_bank(4096, 4096, 0, 0);
  in.cz_fast = 1; in.interp = SKRED_INTERP_LINEAR; in.cnt_guard = 4096; in.guard_current = 1;
  begin("linear lookup on guarded tables: the fold test stays (interp 1, not 2)");
  p = plan_of(&in, 64);
  expect_engaged(&p);
  EXPECT(p.interp, 1);
  end();

  in = cz_bank(4096, 4096, 0, 0);
  in.cz_fast = 1; in.stems = 1;
  begin("with the stem buffer");
  p = plan_of(&in, 64);
  expect_engaged(&p);
  EXPECT(p.pack_s, 0);
  end();

  in = cz_bank(4096, 4096, 0, 0);
  in.cz_fast = 1; in.n_taps = 16;
  begin("voice taps change neither family nor cz");
  p = plan_of(&in, 64);
  expect_engaged(&p);
  end();

  if (!failures) printf("OK\n");
  return failures ? 1 : 0;
}
