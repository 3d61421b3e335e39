/*
 * skred_bank_plan.c -- the selection rules of the bank's render path as pure functions (skred_bank_plan.h).  The measured
 * figures in the comments are the project's record of why each rule stands where it does.
 */

#include <stdio.h>
#include <stdlib.h>

#include "skred_amd.h"
#include "skred_bank_plan.h"

/* Pick the kernel.  The fast kernel (skred_render_fast.hip: sk_render_fast_kernel) is valid when, over
 * all voices that can sound: none is "exotic" (stopping one-shot, reverse, sample&hold, bit-crush,
 * noise, modulated, smoother off, non-finite phase data), and the biquad / the envelope are each used
 * by all of them or by none.  Anything else runs the generic kernel; both give identical samples. */
uint32_t sk_plan_class_mode(int real, int filt, int env, int exotic, int stops, int fm, int fm_odd, int pair_ap) {
  uint32_t m = 0;
  if (real > 0 && !exotic) {
    m = SKM_FAST;
    if (filt) m |= SKM_FILTER_ALL;
    if (env) m |= SKM_ENV_ALL;
    if ((filt && filt != real) || (env && env != real)) m |= SKM_MIXED;   /* some voices only: per-lane flags */
    if (stops) m |= SKM_STOPS;
    if (fm) m |= SKM_FM;
    if (fm && !fm_odd && !stops) m |= SKM_FM_PAIR;   /* every carrier: an even voice modulated by the next one */
    if ((m & SKM_FM_PAIR) && pair_ap) m |= SKM_PAIR_AP;
  }
  return m;
}

/* dependency levels for modulated banks (skred_render_generic.hip: sk_render_mod_kernel) */
int sk_plan_levels(const int8_t *h_mod, int n_padded, int *h_level) {
  int max_level = 0;
  for (int g0 = 0; g0 < n_padded; g0 += 64) {
    for (int l = 0; l < 64; l++) {
      int lvl = 0;
      for (int k = 0; k < 4; k++) {
        const int src = h_mod[(size_t)k * n_padded + g0 + l];
        if (src >= 0 && src < l && h_level[g0 + src] + 1 > lvl) lvl = h_level[g0 + src] + 1;
      }
      h_level[g0 + l] = lvl;
      if (lvl > max_level) max_level = lvl;
    }
  }
  return max_level;
}

void sk_plan_family(const sk_plan_in_t *in, sk_plan_t *plan) {
  *plan = (sk_plan_t){ 0 };
  /* the modulated kernel serves every kind of modulation; banks whose only modulation is previous-frame FM stay on
   * the one-per-lane kernel when they are otherwise clean */
  /* SKRED_OPT_CZ_FAST: a bank whose only exotic voices are CZ voices of the fast family runs the one-voice kernel's CZ
   * instantiations -- LDS-table banks only (the table windows of the others assume an index that moves forward), and not when the
   * bank needs the modulated kernel for another reason.  The feature those voices ask for (SKB_ANY_CZ) is, like every feature
   * bit, only ever set: with the option off it stands for SKB_ANY_MOD as it always did; with the option on it counts while such
   * voices exist and this block cannot take them -- and SKB_ANY_MOD while a voice that needs the modulated kernel exists (the
   * count of them), so that `cz_on` / `cz_off` and a source moved below its carrier and back change the family block by block. */
  const int need_mod = (in->features & SKB_ANY_MOD) && !(in->cz_fast && in->cnt_mod == 0);
  const int cz = in->cz_fast && in->cnt_cz > 0 && (in->fast_mode_cz & SKM_FAST) && !in->force_generic && in->lds_table_floats > 0 && !need_mod;
  const int cz_mod = (in->features & SKB_ANY_CZ) && !(in->cz_fast && (cz || in->cnt_cz == 0));
  const uint32_t class_mode = cz ? in->fast_mode_cz : in->fast_mode;
  const int fast_ok = (class_mode & SKM_FAST) && !in->force_generic;
  const int modulated = need_mod || cz_mod || ((in->features & SKB_ANY_FM) && in->cnt_fm > 0 && !fast_ok);
  plan->cz = cz;
  plan->modulated = modulated;
  plan->n_wg = in->n_groups < SK_MAX_WORKGROUPS ? in->n_groups : SK_MAX_WORKGROUPS;   /* workgroups stride over 256-voice passes */
  plan->interp = in->interp;
  plan->fast_mode = in->force_generic ? 0u : class_mode;
  /* two voices per lane pay off for large LDS-table banks (packed fp32); banks whose tables stay in L2 / HBM do
   * better with one voice per lane at every size measured (2^16 .. 2^20: twice the waves to hide the window
   * refills behind) unless the caller set the threshold explicitly */
  if ((plan->fast_mode & SKM_FAST) && !(plan->fast_mode & (SKM_STOPS | SKM_FM | SKM_CZ)) && in->n_voices >= in->fast2_min_voices &&
      (in->lds_table_floats > 0 || in->fast2_min_user) && !in->stems)      /* (per-voice stems: the one-voice kernel writes them) */
    plan->fast_mode |= SKM_TWO_PER_LANE;        /* (voices that finish mid-launch are handled by the one-per-lane kernel only) */
  /* ... except where its 1024-voice passes fill the machine unevenly: one pass per CU up to n_cus passes, then SOME CUs with two
   * (the block takes as long as a full second layer: 262 144 voices 87 us, 294 912 voices 132 us, 524 288 voices 146 us), where
   * the one-voice kernel's finer grain wins until the second layer is about five eighths full (294 912 voices 106 us, 360 448
   * voices 121 vs 132, 393 216 voices 124 vs 133, 458 752 voices 140 vs 135; tools/measure_banks.py mid -- since the one-voice
   * kernel's LDS-table instantiations stopped reserving a table window per wave they fit four workgroups per CU) */
  if ((plan->fast_mode & SKM_TWO_PER_LANE) && !in->fast2_min_user && in->lds_table_floats > 0) {
    const int passes = in->n_groups * 2 / SK_FAST2_NW_LDS;
    /* (only while nothing moves -- with envelopes in motion the two-per-lane kernel and the envelope kernel beside it are
     * ahead at these sizes, 202 vs 214..255 us --: the family that rendered the previous block knows: an empty motion list,
     * or a one-voice launch that saw no envelope move) */
    const int quiet = !(plan->fast_mode & SKM_ENV_ALL) || (in->last_family == SKRED_KERNEL_FAST2 ? in->list_empty : in->env_quiet);
    if (quiet && passes > in->n_cus && passes <= in->n_cus + in->n_cus * 5 / 8) plan->fast_mode &= ~SKM_TWO_PER_LANE;
  }
  /* ... but while envelopes move the one-voice kernel's block form of them beats the two-per-lane kernel + envelope kernel on
   * mid-size banks (tools/ab_env_mid.py): such banks change kernels with their state (both families read and write the same
   * planes).  "Envelopes move": from a control action until a one-voice launch has reported that none did -- a speed hint. */
  if ((plan->fast_mode & SKM_TWO_PER_LANE) && (plan->fast_mode & SKM_ENV_ALL) && !(plan->fast_mode & SKM_MIXED) && !in->env_quiet &&
      !in->fast2_min_user && in->n_voices < SK_FAST2_MOTION_MIN_VOICES)
    plan->fast_mode &= ~SKM_TWO_PER_LANE;
  /* two-operator FM (every carrier an even voice, modulated by the voice after it): carrier and modulator share a lane of
   * the two-per-lane kernel, so the per-frame exchange of the one-per-lane kernel disappears.  LDS-table banks. */
  if (fast_ok && (plan->fast_mode & SKM_FM_PAIR) && in->lds_table_floats > 0 && !in->stems && in->n_voices >= in->fm2_min_voices &&
      in->n_taps == 0)                        /* (voice taps: the one-voice kernel has the tap rows; same per-voice bits) */
    plan->fast_mode |= SKM_TWO_PER_LANE;
  else
    plan->fast_mode &= ~(SKM_FM_PAIR | SKM_PAIR_AP);
  /* linear lookup on a bank whose every real voice loops over its whole table with a guard sample behind it: the specialised
   * kernels' instantiations without the fold test (two-operator FM banks keep the general form) */
  if (in->interp == SKRED_INTERP_LINEAR && (plan->fast_mode & SKM_FAST) && !(plan->fast_mode & SKM_FM_PAIR) && !modulated && in->cnt_real > 0 &&
      in->cnt_guard == in->cnt_real && in->guard_current && !cz)      /* (a warped position lands anywhere: CZ lanes keep the fold test) */
    plan->interp = 2;
  /* Sparse banks (most voices skipped by the reference's own rule, synth.c:537 -- the shipped patches use 3 to 6 voices of 64):
   * the one-voice family with the lanes PACKED -- a wave takes the voices that can sound of 64 / S aligned 64-voice groups, S = the
   * most lanes any group needs, rounded up to a power of two (skred_device_layout.h: pack_mask).  The extended instantiation
   * renders them (it holds every per-lane feature test), so the rule asks for at least half the waves to disappear; a bank the
   * two-per-lane kernel would take, for a quarter of them. */
  plan->pack_shift = 6;
  plan->fm_skew = in->fm_skew && (plan->fast_mode & SKM_FM) && in->lds_table_floats > 0 && !in->stems;   /* (the launcher drops it when the ring does not fit) */
  if (modulated) plan->fm_skew = in->fm_skew && !in->stems;        /* (the modulated kernel: its frame-lag form, same option) */
  plan->pack_candidate = in->pack_mode && (modulated || ((plan->fast_mode & SKM_FAST) && !(plan->fast_mode & SKM_FM_PAIR))) && !in->stems;   /* (the modulated kernel packs the same way) */
}

/* Sparse lists of LDS-table banks: the listed voices stay in their lanes (skred_gain_kernels.hip ahead of the steady kernel's
 * in-place instantiations, same stream) instead of going through the envelope kernel beside it -- a second kernel costs the
 * steady one a third round of workgroups however few voices it holds (DESIGN "The motion list").  The gain rows are a
 * buffer of fixed capacity, so this path is only taken under a PROVEN bound on the list's length: the length a launch
 * reported (sk_final_cols) plus every voice a control action has touched since that launch was issued -- a list is the
 * survivors of the one before plus what control actions add. */
static void plan_inplace(const sk_plan_in_t *in, sk_plan_t *plan) {
  /* (a list rebuilt ahead of this block is neither known empty nor bounded until the block reports its length) */
  const int list_empty = plan->list_rebuild ? 0 : in->list_empty, bound_valid = plan->list_rebuild ? 0 : in->bound_valid;
  if (plan->two_env && !list_empty && bound_valid && in->in_place_mode && in->lds_table_floats > 0 && !(plan->fast_mode & SKM_FM_PAIR)) {
    const uint64_t bound = in->bound;
    const size_t stride = (size_t)in->num_frames + 8;
    /* rows: SK_INPLACE_WORD_ROWS per 64-voice word of the list (handed out without an atomic), then an overflow area for words
     * that hold more -- as large as the bound must be small, so the rows cannot run out */
    const size_t own = (size_t)in->n_groups * 4 * SK_INPLACE_WORD_ROWS;
    const size_t over = (size_t)in->n_voices / (in->in_place_mode == 2 ? SK_INPLACE_DENOM : 64) + 64;   /* (mode 1 never takes lists beyond n / 128) */
    const size_t rows = own + over;
    /* ... and only where it is the faster of the two (tools/ab_inplace.py, MI355X; DESIGN "The motion list"): every wave
     * of the steady kernel that holds a listed voice runs its smoothers and reads gains (~ +30 %), so the list must be sparse;
     * and the envelope kernel beside the steady one is cheap when the steady kernel's last round of workgroups leaves slots
     * free -- it costs a whole extra round when that round is full (2^19, 2^20 voices on 256 CUs) */
    uint64_t limit = over;
    if (in->in_place_mode == 1) {
      const int slots = 2 * in->n_cus, passes = in->n_groups * 2 / SK_FAST2_NW_LDS;
      const int rounds = passes / slots, last = passes % slots;
      if (last == 0) limit = (uint64_t)in->n_voices / (128u * (unsigned)(rounds > 0 ? rounds : 1));
      else if (rounds == 0 || last * 20 <= slots * 11) limit = (uint64_t)in->n_voices / 600u;
      else limit = 0;
    }
    if (bound <= limit && bound <= over && rows * stride * sizeof(float) <= SK_INPLACE_MAX_BYTES) {
      plan->stride = stride;
      plan->rows = rows;
      plan->own = own;
      plan->inplace = 1;
    }
  }
}

void sk_plan_finish(const sk_plan_in_t *in, int pack_most, sk_plan_t *plan) {
  const int modulated = plan->modulated;
  if (plan->pack_candidate) {
    const int most = pack_most;
    int sh = 0;
    while ((1 << sh) < most) sh++;
    /* ... on a bank that fills the machine several times over: up to two 256-voice passes per CU the block's time is one pass's
     * latency whatever the waves hold, and the extended instantiation's is the longer one (131 072 voices, 5 % in use: 54 us
     * packed, 50 not; 2^20 voices: 117 against 228) */
    const int big = in->n_groups >= 3 * in->n_cus;        /* (196 608 voices: 55 us packed, 63 not; 262 144: 55 against 79) */
    if ((big && (1 << sh) <= ((!modulated && (plan->fast_mode & SKM_TWO_PER_LANE)) ? 16 : 32)) || (in->pack_mode == 2 && sh < 6)) {
      if (!modulated) plan->fast_mode &= ~SKM_TWO_PER_LANE;
      plan->pack_shift = sh;
      plan->pack_groups = in->n_padded / 64;
      const int per_pass = 4 << (6 - sh);               /* groups per 4-wave workgroup pass */
      plan->pack_passes = (plan->pack_groups + per_pass - 1) / per_pass;
      plan->pack_s = 1 << sh;
    }
  }
  plan->kernel = !(plan->fast_mode & SKM_FAST) ? SKRED_KERNEL_GENERIC
                 : (plan->fast_mode & SKM_TWO_PER_LANE) ? SKRED_KERNEL_FAST2 : SKRED_KERNEL_FAST;
  if (modulated) plan->kernel = SKRED_KERNEL_MODULATED;
  if (!modulated && (plan->fast_mode & SKM_TWO_PER_LANE)) {
    /* passes of sk_render_fast2_kernel: 1024 voices each for LDS-table banks, 512 otherwise (skred_render_fast2.hip) */
    const int passes = in->lds_table_floats > 0 ? in->n_groups * 2 / SK_FAST2_NW_LDS : in->n_groups / 2;
    plan->n_wg = passes < SK_MAX_WORKGROUPS ? passes : SK_MAX_WORKGROUPS;
  }
  if (plan->pack_s) plan->n_wg = plan->pack_passes < SK_MAX_WORKGROUPS ? plan->pack_passes : SK_MAX_WORKGROUPS;
  /* two-per-lane banks with envelopes: the voices on the motion list are rendered by sk_render_env2_kernel BESIDE the steady
   * kernel, on the bank's second stream (its own rows, its own ticket; skred_kernel_common.hpp: sk_finish_env) */
  plan->two_env = !modulated && (plan->fast_mode & SKM_TWO_PER_LANE) && (plan->fast_mode & SKM_ENV_ALL);
  /* one-per-lane banks with envelopes: a launch's report picks between the instantiation that also holds the block form of
   * envelopes in motion and the lean one (skred_render_fast.hip: RAMPK); both render everything, so a stale answer costs
   * speed, never samples */
  plan->one_env = !modulated && (plan->fast_mode & SKM_FAST) && !(plan->fast_mode & SKM_TWO_PER_LANE) && (plan->fast_mode & SKM_ENV_ALL);
  /* SKRED_OPT_SPLIT (off by default): the one-voice family on a clean LDS-table bank that is believed steady (no envelope: always;
   * envelopes: a launch has reported that none moved and no control action arrived since) with every frame split between an
   * oscillator wave and a post wave (skred_render_split.hip).  A wave whose voices are not steady after all renders itself on the
   * general path of the same kernel, so the belief decides speed only.  Built on the previous review's advice to give small and
   * mid-size banks more instruction streams per SIMD; measured (tools/ab_split.py, tools/issue_mix.hip, profiles/r04_split_*): the
   * LDS instructions of the hand-over cost a wave about what the moved arithmetic saves, and from two 64-voice groups per SIMD on
   * the SIMD's own throughput binds -- 1.4 % faster than sk_render_fast_kernel at 65 536 voices, 3 % slower at 4 096, 20 % slower at
   * 131 072 -- so the library never picks it by itself; values 1 / 2 / 3 keep it reachable (the rule of value 1: banks of 32 768 ..
   * 65 536 filtered voices on a 256-CU device).  (Decided here, ahead of the row layout: the two-pair form has twice the rows.) */
  int split = 0;
  if (!modulated && (plan->fast_mode & SKM_FAST) && !(plan->fast_mode & (SKM_TWO_PER_LANE | SKM_STOPS | SKM_FM | SKM_MIXED | SKM_CZ)) && in->lds_table_floats > 0 &&
      !in->stems && !plan->pack_s && in->split_mode && (!plan->one_env || in->env_quiet || in->split_mode == 3) && in->split_lds4 <= SK_SPLIT_MAX_LDS) {
    if (in->split_mode >= 2 || ((plan->fast_mode & SKM_FILTER_ALL) && in->n_groups * 2 >= in->n_cus && in->n_groups <= in->n_cus)) split = 4;
    if (split && in->split_pairs && (in->split_pairs == 4 || in->n_groups * 2 <= SK_MAX_WORKGROUPS)) split = in->split_pairs;   /* (tests) */
  }
  if (in->n_probe > 0) {
    /* probes are written by the probe instantiations of the specialised kernels only */
    if (modulated || !(plan->fast_mode & SKM_FAST) || (plan->fast_mode & SKM_FM_PAIR) || in->stems) {
      plan->rc = SKRED_E_UNSUPPORTED;
      plan->msg = "a probe is set, but this block would run a kernel without probe instantiations "
                  "(generic / modulated / two-operator FM pairs, or a launch with the full stem buffer)";
      return;
    }
    split = 0;
  }
  /* voice taps: every kernel family writes them -- the specialised ones through their probe instantiations, the generic,
   * modulated and tape kernels through their tap instantiations (the launchers forward on probe_out); the split form has none */
  if (in->n_taps > 0) split = 0;
  if (split) plan->fast_mode |= SKM_SPLIT | (split == 2 ? SKM_SPLIT2 : 0u);
  if (split == 2) plan->n_wg = in->n_groups * 2;
  plan->split = split;
  /* another family rendered meanwhile: it does not keep the list */
  plan->list_rebuild = plan->two_env && (in->last_family != SKRED_KERNEL_FAST2 || in->mask_dirty);
  plan_inplace(in, plan);
}

/* Cross-group modulation (SKRED_OPT_CROSS_GROUP): the plan of the tape, made again whenever a cross-group routing changed.
 * Every distinct source gets a slot (in the order its first reader comes); the groups form a graph, an edge from a reader's
 * group to its source's group; a source group's pre-pass level is 0 when it reads no tape, else 1 + the highest level it reads.
 * A cycle between groups, or a chain that needs more than SK_TAPE_MAX_LEVELS pre-pass launches, is refused (the refusal stands,
 * render after render, until the routing changes).  A refused or empty plan leaves no source. */
typedef struct { int rg, sg, reader, source; } sk_tape_edge_t;
int sk_tape_plan_host(const int32_t *h_esc, int n_padded, int32_t *h_slot, uint8_t *lanes_dirty, int32_t *groups,
                      int level_off[SK_TAPE_MAX_LEVELS + 1], int *n_levels, char *msg, size_t msg_size) {
  const int n = n_padded, G = n / 64;
  *n_levels = 0;
  /* the sources of the old plan lose their lanes (pack_refresh), those of the new one get theirs */
  for (int v = 0; v < n; v++)
    if (h_slot[v] >= 0) { h_slot[v] = -1; lanes_dirty[v >> 6] = 1; }
  size_t n_edges = 0, cap = 0;
  sk_tape_edge_t *edges = NULL;
  int *first = (int *)calloc((size_t)G + 1, sizeof(int));
  int *lvl = (int *)malloc((size_t)G * sizeof(int)), *state = (int *)calloc((size_t)G, sizeof(int));
  int *stack = (int *)malloc((size_t)G * sizeof(int)), *iter = (int *)malloc((size_t)G * sizeof(int));
  int rc = 0, n_src = 0;
  if (!first || !lvl || !state || !stack || !iter) { snprintf(msg, msg_size, "cross-group plan"); rc = SKRED_E_NO_MEM; goto out; }
  for (int g = 0; g < G; g++) {
    first[g] = (int)n_edges;
    for (int l = 0; l < 64; l++) {
      const int v = g * 64 + l;
      for (int k = 0; k < 4; k++) {
        const int md = h_esc[(size_t)k * n + v];
        if (md < 0) continue;
        if (h_slot[md] < 0) { h_slot[md] = n_src++; lanes_dirty[md >> 6] = 1; }
        int dup = 0;                                   /* (a group's readers mostly name the same few groups) */
        for (size_t e = n_edges; e > (size_t)first[g] && e + 16 > n_edges; e--) if (edges[e - 1].sg == (md >> 6)) { dup = 1; break; }
        if (dup) continue;
        if (n_edges == cap) {
          cap = cap ? 2 * cap : 1024;
          sk_tape_edge_t *ne = (sk_tape_edge_t *)realloc(edges, cap * sizeof(*edges));
          if (!ne) { snprintf(msg, msg_size, "cross-group plan"); rc = SKRED_E_NO_MEM; goto out; }
          edges = ne;
        }
        edges[n_edges++] = (sk_tape_edge_t){ g, md >> 6, v, md };
      }
    }
  }
  first[G] = (int)n_edges;
  if (n_src == 0) goto out;
  /* pre-pass levels: depth-first from every source group, iteratively (a chain may run through many groups) */
  for (int g = 0; g < G; g++) lvl[g] = 0;
  for (int s0 = 0; s0 < G && rc == 0; s0++) {
    if (state[s0] != 0) continue;
    int src_here = 0;
    for (int l = 0; l < 64 && !src_here; l++) src_here = h_slot[s0 * 64 + l] >= 0;
    if (!src_here) continue;
    int top = 0;
    stack[0] = s0; iter[0] = first[s0]; state[s0] = 1;
    while (top >= 0) {
      const int g = stack[top];
      if (iter[top] < first[g + 1]) {
        const sk_tape_edge_t *e = &edges[iter[top]++];
        const int h = e->sg;
        if (state[h] == 1) {
          snprintf(msg, msg_size, "cross-group modulation: the groups of voice %d and voice %d read each other (a cycle between "
                                  "64-voice groups: voice %d reads voice %d)", e->reader, e->source, e->reader, e->source);
          rc = SKRED_E_UNSUPPORTED;
          break;
        }
        if (state[h] == 0) { state[h] = 1; ++top; stack[top] = h; iter[top] = first[h]; }
        else if (lvl[h] + 1 > lvl[g]) lvl[g] = lvl[h] + 1;
      } else {
        state[g] = 2;
        if (lvl[g] >= SK_TAPE_MAX_LEVELS) {
          const sk_tape_edge_t *e = &edges[first[g]];
          snprintf(msg, msg_size, "cross-group modulation: a chain of groups %d deep (voice %d reads voice %d, which ...): at most %d "
                                  "pre-pass levels", lvl[g] + 1, e->reader, e->source, SK_TAPE_MAX_LEVELS);
          rc = SKRED_E_UNSUPPORTED;
          break;
        }
        if (--top >= 0 && lvl[g] + 1 > lvl[stack[top]]) lvl[stack[top]] = lvl[g] + 1;
      }
    }
  }
  if (rc) { n_src = 0; goto out; }
  {
    /* the source groups, level by level */
    int levels = 0;
    for (int g = 0; g < G; g++) {
      int src_here = 0;
      for (int l = 0; l < 64 && !src_here; l++) src_here = h_slot[g * 64 + l] >= 0;
      state[g] = src_here;
      if (src_here && lvl[g] + 1 > levels) levels = lvl[g] + 1;
    }
    int at = 0;
    for (int l = 0; l < levels; l++) {
      level_off[l] = at;
      for (int g = 0; g < G; g++) if (state[g] && lvl[g] == l) groups[at++] = g;
    }
    level_off[levels] = at;
    *n_levels = levels;
  }
out:
  if (n_src == 0) for (int v = 0; v < n; v++) h_slot[v] = -1;   /* (no plan: no source keeps a lane for the tape) */
  free(edges); free(first); free(lvl); free(state); free(stack); free(iter);
  return rc ? rc : n_src;
}
