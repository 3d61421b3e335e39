/*
 * skred_bank_plan.h -- the pure half of the bank's render path: which kernel family a block runs and in what shape, the class
 * mode word, the dependency levels and the host half of the cross-group tape plan.  Integer arithmetic on facts the host
 * already holds: no HIP, no bank, nothing is mutated but the outputs named here (skred_bank_render.c: render_block and
 * skred_bank.c: sk_classify, tape_plan are the callers; tests/c_plan_cases.c runs it on the CPU).
 */
#ifndef SKRED_BANK_PLAN_H
#define SKRED_BANK_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "skred_device_layout.h"

#define SK_SPLIT_MAX_LDS (160u * 1024u)   /* LDS of a CU: sk_render_split_kernel's workgroup must fit (twice, for two workgroups per CU) */
#define SK_FM2_MIN_VOICES 1024      /* two-operator FM banks at least this large keep each (carrier, modulator) pair in one lane */
#define SK_FAST2_MOTION_MIN_VOICES 278528   /* ... while envelopes move: banks smaller than this stay on the one-voice kernel (round 3, the envelope kernel
                                               beside the steady one: 262 144 voices 184 vs 198 us per block, 294 912 voices 214 vs 202; tools/ab_env_mid.py) */
#define SK_FAST2_MIN_VOICES 212992   /* banks at least this large use two voices per lane (measured crossover, 512-frame blocks, C2 recipe: 196608 voices 86 vs 95 us, 262144 voices 108 vs 101 us; profiles/r02_v1_measure_banks.txt) */
#define SK_INPLACE_WORD_ROWS 8                   /* gain rows every 64-voice word of the list owns */
#define SK_INPLACE_DENOM 6                       /* lists up to n_voices / 6 are rendered in place (a 128-voice wave stages at most 32) */
#define SK_INPLACE_MAX_BYTES ((size_t)4 << 30)   /* ... while the gain rows stay below this */

/* everything render_block reads to decide, and nothing else */
typedef struct {
  int n_voices, n_groups, n_padded, n_cus;                 /* bank shape */
  uint32_t fast_mode, features;                            /* SKM_* of sk_plan_class_mode, SKB_* */
  int cnt_fm, cnt_real, cnt_guard;
  int guard_current;                                       /* guard_epoch == tables_epoch: the guard flags are those of the current pool */
  int32_t lds_table_floats;                                /* the padded pool's size when it is staged in LDS, else 0 */
  int num_frames, interp, stems, n_probe, n_taps;          /* the request (stems: the launch carries the full stem buffer) */
  int force_generic, fast2_min_voices, fast2_min_user, fm2_min_voices, pack_mode, fm_skew, split_mode, split_pairs, in_place_mode;
  int env_quiet, list_empty, last_family;                  /* hints: what earlier launches reported (skred_bank_priv.h) */
  int mask_dirty;                                          /* the motion list must be rebuilt before the next two-per-lane block */
  int bound_valid;
  uint64_t bound;                                          /* bound_len + touched_total - bound_touched */
  size_t split_lds4;                                       /* sk_split_lds_bytes(args, 4) */
  /* SKRED_OPT_CZ_FAST (appended: tests/c_plan_cases.c fills the fields above by name and zeroes the rest) */
  int cnt_cz;                                              /* real voices whose CZ the one-voice kernel can render (SKC_CZ) */
  int cnt_mod;                                             /* voices whose modulation only the modulated kernel serves (SKC_MOD) */
  int cz_fast;                                             /* the option */
  uint32_t fast_mode_cz;                                   /* the class mode with those voices not counted as exotic, | SKM_CZ; 0 when the
                                                              bank holds other exotic voices, or none of these */
} sk_plan_in_t;

typedef struct {
  uint32_t fast_mode;         /* final SKM_* of the launch */
  int interp;                 /* 0, 1, or 2: linear on guarded whole-table loops */
  int modulated;
  int fm_skew;
  int kernel;                 /* SKRED_KERNEL_* */
  int n_wg;
  int pack_candidate;         /* sk_plan_family: the block may pack its lanes -- the caller refreshes the lane histogram */
  int pack_s, pack_shift, pack_groups, pack_passes;   /* pack_s: lanes per 64-voice group (0: not packed) */
  int two_env, one_env;
  int split;                  /* 0, or pairs per workgroup of sk_render_split_kernel (2 / 4) */
  int list_rebuild;           /* two_env and the motion list is stale: rebuilt ahead of the block (its length is then unknown) */
  int inplace;                /* listed voices rendered in their lanes; then: */
  size_t stride, rows, own;   /* floats per gain row; rows in all; of them handed out per 64-voice word */
  int rc;                     /* != 0: the block is refused (a probe on a family without probe instantiations); msg says why */
  const char *msg;
  int cz;                     /* the block runs a CZ instantiation of the one-voice kernel (fast_mode has SKM_CZ) */
} sk_plan_t;

/* Two pure steps: sk_plan_family decides everything up to and including plan->pack_candidate; sk_plan_finish the rest, given
 * the most lanes any 64-voice group needs (the lane histogram's maximum; ignored unless pack_candidate). */
void sk_plan_family(const sk_plan_in_t *in, sk_plan_t *plan);
void sk_plan_finish(const sk_plan_in_t *in, int pack_most, sk_plan_t *plan);

/* the SKM_* class mode of a bank from its per-class voice counts */
uint32_t sk_plan_class_mode(int real, int filt, int env, int exotic, int stops, int fm, int fm_odd, int pair_ap);

/* dependency levels of a modulated bank (h_mod: [4][n_padded] modulator lane inside the 64-voice group or -1) into
 * h_level[n_padded]; returns the highest */
int sk_plan_levels(const int8_t *h_mod, int n_padded, int *h_level);

/* Host half of the cross-group tape plan over h_esc ([4][n_padded] modulator voice in another group, or -1).  Fills h_slot
 * (voice -> tape slot, -1: not a source), sets lanes_dirty[g] = 1 for every 64-voice group whose lane word changed (entries are
 * only ever set), fills groups[] (at most n_padded / 64 source groups, level by level, ascending inside a level) and level_off.
 * Returns the number of sources (0: no cross-group edge, every h_slot is -1) and *n_levels; or a negative SKRED_E_* with its text
 * in msg: SKRED_E_UNSUPPORTED for a refused routing (a cycle, too deep), SKRED_E_NO_MEM. */
int sk_tape_plan_host(const int32_t *h_esc, int n_padded, int32_t *h_slot, uint8_t *lanes_dirty, int32_t *groups,
                      int level_off[SK_TAPE_MAX_LEVELS + 1], int *n_levels, char *msg, size_t msg_size);

#endif
