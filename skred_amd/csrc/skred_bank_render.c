/*
 * skred_bank_render.c -- the launch half of the bank's render path behind include/skred_amd.h: one block from request to kernels.
 * What runs is decided by skred_bank_plan.c (pure: no HIP, no bank); this file validates the request, keeps the motion-list and
 * report bookkeeping, sizes the buffers and launches.  Lifecycle, tables, upload / download and options: skred_bank.c.
 */

#include <string.h>

#include "skred_bank_priv.h"

static int grow(float **buf, size_t *cap, size_t need) {
  if (*cap >= need) return SKRED_OK;
  if (*buf) { hipFree(*buf); *buf = NULL; *cap = 0; }
  HIP_TRY(hipMalloc((void **)buf, need * sizeof(float)));
  *cap = need;
  return SKRED_OK;
}

/* What earlier launches found, as far as their answers have arrived (never waits): the block's final arriver stores
 * (launch ticket << 32 | finding) into two pinned host words (skred_kernel_common.hpp: sk_final_cols). */
static void poll_reports(skred_bank_t *b) {
  if (!b->h_report) return;
  const uint64_t w0 = __atomic_load_n(&b->h_report[0], __ATOMIC_RELAXED), w1 = __atomic_load_n(&b->h_report[1], __ATOMIC_RELAXED);
  const uint32_t t0 = (uint32_t)(w0 >> 32);
  if (t0 != 0 && t0 != b->report_seen && t0 == (uint32_t)(w1 >> 32)) {     /* a new report, both words of the same launch */
    b->report_seen = t0;
    const int slot = (int)(t0 % SK_REPORT_RING);
    if (b->report_ticket[slot] == t0) {                                    /* (else: asked so long ago that its slot was re-used) */
      const int fresh = b->report_epoch[slot] == b->control_epoch;         /* no control action reached the bank since it was issued */
      const uint32_t found = (uint32_t)w0;
      if (b->report_kind[slot] == 1) {
        /* one-voice family: did an envelope move in that launch */
        if (!found && fresh) b->env_quiet = 1;
        if (found) b->env_quiet = 0;
      } else {
        /* two-per-lane family: the length of the list that block rendered.  Empty, and nothing added since: every later list is
         * empty too (a list is the survivors of the one before plus what control actions add) -- a structural fact, not an
         * inference about envelopes.  And the cross-check counter of sk_render_fast2_kernel: should it ever move, rebuild. */
        if (b->report_kind[slot] == 2 && found == 0 && fresh) b->list_empty = 1;
        if (b->report_kind[slot] == 2 && (int32_t)(t0 - b->bound_min_ticket) >= 0) {   /* (not a list from before the last rebuild) */
          b->bound_len = found;
          b->bound_touched = b->report_touched[slot];
          b->bound_valid = 1;
        }
        if ((uint32_t)w1 != b->violations_seen) {
          b->violations_seen = (uint32_t)w1;
          b->mask_dirty = 1;
          b->list_empty = 0;
          (void)fail(SKRED_E_UNSUPPORTED, "launch %u or one before it rendered a voice at a constant level whose envelope was in motion (not on the motion list): list rebuilt", t0);
        }
      }
    }
  }
}

/* this launch will report: remember what its ticket means (kind 1: one-voice "moved"; 2: list length; 3: violations only) */
static int expect_report(skred_bank_t *b, sk_render_args_t *a, int kind) {
  if (!b->h_report) {
    HIP_TRY(hipHostMalloc((void **)&b->h_report, 2 * sizeof(uint64_t), hipHostMallocCoherent));   /* (polled by the host while kernels run) */
    b->h_report[0] = b->h_report[1] = 0;
  }
  const int slot = (int)(a->launch_ticket % SK_REPORT_RING);
  b->report_ticket[slot] = a->launch_ticket;
  b->report_epoch[slot] = b->control_epoch;
  b->report_kind[slot] = (uint8_t)kind;
  b->report_touched[slot] = b->touched_total;
  a->report = (unsigned long long *)b->h_report;
  return SKRED_OK;
}

/* cross-group modulation: the tape of this block (a voice's cross-group modulators are tape codes in its SKP_MODI word from the
 * moment it was written, so such a bank never runs without the tape); ta->tape stays NULL when the block reads none */
static int block_tape(skred_bank_t *b, int num_frames, sk_tape_args_t *ta) {
  memset(ta, 0, sizeof(*ta));
  if (!(b->cross_group && b->tape_sources > 0)) return SKRED_OK;
  if (!(b->features & SKB_ANY_MOD)) return fail(SKRED_E_UNSUPPORTED, "cross-group modulation outside the modulated kernel");
  const size_t need = (size_t)b->tape_sources * ((size_t)num_frames + 1);
  if (need * sizeof(float) > SK_TAPE_MAX_BYTES)
    return fail(SKRED_E_RANGE, "cross-group modulation: %d sources x %d frames need a tape of %zu bytes (at most %zu)",
                b->tape_sources, num_frames + 1, need * sizeof(float), (size_t)SK_TAPE_MAX_BYTES);
  if (need > b->tape_cap) {
    HIP_TRY(hipDeviceSynchronize());               /* (a block on another stream may still read the old tape) */
    const int rc = grow(&b->d_tape, &b->tape_cap, need);
    if (rc) return rc;
  }
  ta->tape = b->d_tape;
  ta->slot = b->d_slot;
  return SKRED_OK;
}

/* what the planner decides on (skred_bank_plan.h), read off the bank and the request */
static void plan_input(const skred_bank_t *b, int num_frames, int interp, int stems, sk_plan_in_t *in) {
  const sk_render_args_t lds = { .lds_table_floats = b->table_floats_padded <= SK_LDS_TABLE_MAX_FLOATS ? (int32_t)b->table_floats_padded : 0 };
  memset(in, 0, sizeof(*in));
  in->n_voices = b->n_voices; in->n_groups = b->n_groups; in->n_padded = b->n_padded; in->n_cus = b->n_cus;
  in->fast_mode = b->fast_mode; in->features = b->features;
  in->cnt_fm = b->cnt_fm; in->cnt_real = b->cnt_real; in->cnt_guard = b->cnt_guard;
  in->guard_current = b->guard_epoch == b->tables_epoch;
  in->lds_table_floats = lds.lds_table_floats;
  in->num_frames = num_frames; in->interp = interp; in->stems = stems; in->n_probe = b->n_probe; in->n_taps = b->n_taps;
  in->force_generic = b->force_generic; in->fast2_min_voices = b->fast2_min_voices; in->fast2_min_user = b->fast2_min_user;
  in->fm2_min_voices = b->fm2_min_voices; in->pack_mode = b->pack_mode; in->fm_skew = b->fm_skew;
  in->split_mode = b->split_mode; in->split_pairs = b->split_pairs; in->in_place_mode = b->in_place_mode;
  in->env_quiet = b->env_quiet; in->list_empty = b->list_empty; in->last_family = b->last_family;
  in->mask_dirty = b->mask_dirty; in->bound_valid = b->bound_valid;
  in->bound = (uint64_t)b->bound_len + (b->touched_total - b->bound_touched);
  in->split_lds4 = sk_split_lds_bytes(&lds, 4);            /* (it reads the table size only) */
  in->cnt_cz = b->cnt_cz; in->cnt_mod = b->cnt_mod; in->cz_fast = b->cz_fast; in->fast_mode_cz = b->fast_mode_cz;
}

/* the render args as far as the bank, the request and the plan fix them (the rows follow: inplace_rows, partial_rows) */
static void args_from_bank(const skred_bank_t *b, const sk_plan_in_t *in, const sk_plan_t *p, float *d_stems, sk_render_args_t *a) {
  memset(a, 0, sizeof(*a));
  for (int i = 0; i < SKP_COUNT; i++) a->ro[i] = b->d_ro[i];
  for (int i = 0; i < SKS_COUNT; i++) a->rw[i] = b->d_rw[i];
  a->tables = b->d_tables;
  a->stems = d_stems;
  a->group_flag = b->d_group_flag;
  a->env_list = b->d_env_list;
  a->env_off = b->d_env_off;
  a->mask_cur = b->d_mask[b->mask_p];
  a->mask_next = b->d_mask[b->mask_p ^ 1];
  a->violations = b->d_violations;
  a->count0 = b->g.synth_sample_count;
  a->rng0 = b->g.noise_rng;
  a->n_voices = b->n_voices;
  a->n_groups = b->n_groups;
  a->num_frames = in->num_frames;
  a->table_floats = (int32_t)b->table_floats;
  a->lds_table_floats = in->lds_table_floats;
  a->interp = p->interp;
  a->features = b->features;
  a->fast_mode = p->fast_mode;
  a->pack_shift = p->pack_shift;
  a->fm_skew = p->fm_skew;
  a->form_counts = p->modulated ? b->d_form_counts : NULL;
  if (p->pack_s) {
    a->pack_groups = p->pack_groups;
    a->pack_passes = p->pack_passes;
    a->pack_mask = b->d_pack_mask;
  }
}

/* the probe's or the taps' rows of this block, cleared (a skipped / muted voice writes nothing) */
static int probe_rows(skred_bank_t *b, sk_render_args_t *a, hipStream_t s) {
  if (b->n_probe > 0) {
    a->probe_ids = b->d_probe_ids;
    a->n_probe = b->n_probe;
    a->probe_out = b->d_probe_out;
  } else if (b->n_taps > 0) {
    a->probe_ids = b->d_tap_ids;
    a->n_probe = b->n_taps;
    a->probe_out = b->d_taps_out;
  } else return SKRED_OK;
  HIP_TRY(hipMemsetAsync(a->probe_out, 0, (size_t)a->num_frames * (size_t)a->n_probe * 2 * sizeof(float), s));
  return SKRED_OK;
}

/* the motion list again from the planes (sk_plan_t: list_rebuild) */
static int rebuild_list(skred_bank_t *b, const sk_render_args_t *a, hipStream_t s) {
  b->mask_dirty = 1;
  const hipError_t ec = (hipError_t)sk_launch_classify(a, b->d_mask[b->mask_p], s);
  if (ec != hipSuccess) return fail(SKRED_E_NO_DEVICE, "classify launch -> %s", hipGetErrorString(ec));
  b->mask_dirty = 0;
  b->list_empty = 0;
  b->bound_valid = 0;                              /* the rebuilt list's length is not known until this block reports it */
  b->bound_min_ticket = b->launch_ticket + 1;
  return SKRED_OK;
}

/* listed voices rendered in place: the gain rows the plan sized */
static int inplace_rows(skred_bank_t *b, const sk_plan_t *p, sk_render_args_t *a) {
  if (p->rows * p->stride + 8 > b->env_gain_cap) {
    HIP_TRY(hipDeviceSynchronize());               /* (a block on another stream may still read the old rows) */
    const int rc = grow(&b->d_env_gain, &b->env_gain_cap, p->rows * p->stride + 8);
    if (rc) return rc;
  }
  a->env_gain = b->d_env_gain;
  a->env_gain_stride = (int32_t)p->stride;
  a->env_gain_cap = (int32_t)p->rows;
  a->env_word_rows = SK_INPLACE_WORD_ROWS;
  a->env_count = b->d_violations + 1;
  return SKRED_OK;
}

/* rows of the partial mix, the slab sums of the two-level mix-down, the per-frame master gains, and (when the envelope kernel
 * runs beside) its rows and its sum: one allocation; and where the block's mix goes */
static int partial_rows(skred_bank_t *b, int n_wg, int env_beside, float *d_sum, float *d_out, int num_channels, sk_render_args_t *a) {
  const int num_frames = a->num_frames, n_env = env_beside ? sk_env2_grid(a) : 0;
  int rc;
  const size_t row = (size_t)num_frames * 2;
  const size_t gains_at = ((size_t)n_wg + SK_FINISH_SLABS) * row;
  const size_t env_at = (gains_at + (size_t)num_frames + 3) & ~(size_t)3;          /* 16-byte aligned */
  if (env_at + ((size_t)n_env + 1) * row > b->partial_cap && b->pp_parity >= 0) HIP_TRY(hipDeviceSynchronize());   /* (a master stage of the pipelined form may still read the old rows) */
  if ((rc = grow(&b->d_partial, &b->partial_cap, env_at + ((size_t)n_env + 1) * row))) return rc;
  const int pp = b->pp_parity >= 0 && !d_out;      /* pipelined sum-only form: skred_shard_render_mix_pipelined */
  a->partial = b->d_partial;
  a->slab_rows = b->d_partial + (size_t)n_wg * row;
  a->gains = b->d_partial + gains_at;
  if (pp) {
    /* the pipelined form's master stage of block k reads its gain row on another stream while block k + 1 renders: the two rows
     * live in an allocation of their own, at offsets that depend on nothing but the parity -- not behind the rows of d_partial,
     * whose number follows the kernel family and whose length follows num_frames, both free to change from block to block */
    if ((size_t)num_frames > b->pp_gains_cap) {
      HIP_TRY(hipDeviceSynchronize());               /* (a master stage may still read the old rows) */
      if (b->d_pp_gains) { hipFree(b->d_pp_gains); b->d_pp_gains = NULL; b->pp_gains_cap = 0; }
      const size_t cap = ((size_t)num_frames + 1023) & ~(size_t)1023;
      HIP_TRY(hipMalloc((void **)&b->d_pp_gains, 2 * cap * sizeof(float)));
      b->pp_gains_cap = cap;
    }
    a->gains = b->d_pp_gains + (b->pp_parity ? b->pp_gains_cap : 0);
  }
  a->env_rows = b->d_partial + env_at;
  a->env_sum = a->env_rows + (size_t)n_env * row;
  a->env_ticket = b->d_tickets + SK_FINISH_SLABS + 1;
  a->moved = b->d_tickets + SK_FINISH_SLABS + 2;
  a->n_env_rows = n_env;
  a->env_beside = env_beside;
  b->gains_offset = gains_at;
  a->n_rows = n_wg;
  a->finish = 1;
  /* The gain workgroup walks the master gain of every frame beside the renderers.  Single-GPU form: the last arriver applies
   * it.  Sum-only form (the multi-GPU render): the gains are left for skred_bank_master(), which runs after the RCCL sum
   * and then has nothing serial left to do; the carried gain is committed there (slot 1 holds it meanwhile). */
  a->wg_shift = 1;
  a->sum_out = d_sum;
  a->mix_out = d_out;
  a->num_channels = num_channels;
  a->gain_state = b->d_gain_state;
  /* (pipelined form: the NEXT block's render starts before this block's master stage has run, so the render commits the
   * carried gain itself and the master stage, sk_bank_master_pp, only scales) */
  a->gain_commit = (d_out || pp) ? b->d_gain_state : b->d_gain_state + 1;
  b->gains_frames = (d_out || pp) ? 0 : num_frames;  /* gains for a block of this many frames are waiting for skred_bank_master */
  a->tickets = b->d_tickets;
  a->vol_target = b->g.volume_final;
  a->vol_k = b->g.volume_smoother_smoothing;
#ifdef SK_ABLATE_FINISH   /* timing experiments only (tools/ab_finish.py says how such a library is built): the block's output is then garbage */
  a->finish = 0; a->wg_shift = 0; b->gains_frames = 0;
#endif
  return SKRED_OK;
}

/* packed lanes: the words the kernel reads, and voice_sample = 0 where the reference's skip rule would have left it and no lane does */
static int pack_words(skred_bank_t *b, hipStream_t s) {
  if (b->pack_upload) {
    HIP_TRY(hipMemcpyAsync(b->d_pack_mask, b->h_pack_mask, (size_t)(b->n_padded / 64) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    b->pack_upload = 0;
  }
  if (b->pack_zero) {
    const hipError_t ez = (hipError_t)sk_launch_pack_zero(b->d_pack_mask, b->d_rw[SKS_FILT], b->n_padded, s);
    if (ez != hipSuccess) return fail(SKRED_E_NO_DEVICE, "pack_zero launch -> %s", hipGetErrorString(ez));
    b->pack_zero = 0;
  }
  return SKRED_OK;
}

/* the kernels of the block, in stream order; `ta`: its tape (ta->tape NULL: none) */
static int launch_block(skred_bank_t *b, sk_render_args_t *a, const sk_plan_t *p, const sk_tape_args_t *ta, hipStream_t s) {
  const int env_beside = a->env_beside, inplace = p->inplace;
  int rc;
  const int tslot = b->n_timed % SK_TIMING_RING;
  a->launch_ticket = ++b->launch_ticket;
  a->skip_env2 = p->two_env ? (uint32_t)b->list_empty : (uint32_t)(p->one_env && b->env_quiet);
  const int timed = b->timing_every > 0 && (b->launch_ticket % (uint32_t)b->timing_every) == 0;
  if (timed) HIP_TRY(hipEventRecord(b->ev0[tslot], s));
  hipError_t e;
  if (p->two_env && (env_beside || inplace || (a->launch_ticket & 63u) == 0)) { if ((rc = expect_report(b, a, (env_beside || inplace) ? 2 : 3))) return rc; }
  else if (p->one_env && (!a->skip_env2 || (a->launch_ticket & 15u) == 0)) { if ((rc = expect_report(b, a, 1))) return rc; }
  if (env_beside) {
    /* the list of this block, then fork: everything queued on `s` so far (updates, the classify pass, the list) is ahead of
     * the envelope kernel too; both render kernels become ready together */
    e = (hipError_t)sk_launch_collect(a, s);
    if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "collect launch -> %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(b->ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(b->side, b->ev_fork, 0));
    e = (hipError_t)sk_launch_env_fast2(a, b->side);   /* (with a probe set it forwards to the probe instantiations) */
    if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "envelope kernel launch -> %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(b->ev_join, b->side));
  }
  if (inplace) {
    e = (hipError_t)sk_launch_gain(a, s);
    if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "gain kernel launch -> %s", hipGetErrorString(e));
    b->mask_p ^= 1;                                                  /* it wrote the next block's list */
  }
  if (p->modulated && ta->tape) {
    /* the pre-pass, level by level, then the main launch: same stream, after every launch of the block that writes state */
    for (int l = 0; l < b->tape_levels; l++) {
      sk_tape_args_t tl = *ta;
      tl.groups = b->d_tape_groups + b->tape_level_off[l];
      tl.n_list = b->tape_level_off[l + 1] - b->tape_level_off[l];
      e = (hipError_t)sk_launch_tape_prepass(a, b->d_level, b->max_level, &tl, s);
      if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "tape pre-pass launch -> %s", hipGetErrorString(e));
    }
    e = (hipError_t)sk_launch_render_mod_tape(a, p->n_wg, b->d_level, b->max_level, ta, s);
  } else if (p->modulated) {
    e = (hipError_t)sk_launch_render_mod(a, p->n_wg, b->d_level, b->max_level, s);
  } else {
    e = (hipError_t)sk_launch_render(a, p->n_wg, s);
  }
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "render launch -> %s", hipGetErrorString(e));
  if (env_beside) {
    HIP_TRY(hipStreamWaitEvent(s, b->ev_join, 0));                   /* join: the block is complete on `s` */
    b->mask_p ^= 1;                                                  /* the survivors are the next block's list */
  }
  if (timed) {
    HIP_TRY(hipEventRecord(b->ev1[tslot], s));
    b->n_timed++;
  }
  return SKRED_OK;
}

/* One block: picks and launches the render kernel(s), whose last-arriving workgroups also add the per-workgroup rows
 * up (skred_kernel_common.hpp: sk_finish_block) into `d_sum` (pre-master, may be NULL) and / or, scaled by the master
 * gain of each frame, into `d_out`; advances the timeline.  What runs is decided by skred_bank_plan.c from plain facts;
 * everything here validates, sizes buffers and launches. */
static int render_block(skred_bank_t *b, int num_frames, int interp, float *d_stems, float *d_sum, float *d_out,
                        int num_channels, hipStream_t s) {
  if (interp != SKRED_INTERP_TRUNCATE && interp != SKRED_INTERP_LINEAR) return fail(SKRED_E_BAD_ARG, "render: interp %d", interp);
  if (!b->d_tables) return fail(SKRED_E_BAD_ARG, "render: no table pool set");
  if (b->n_taps > 0 && d_stems) return fail(SKRED_E_UNSUPPORTED, "render: voice taps are set and the launch carries the full stem buffer, which already holds them");
  if ((b->features & (SKB_ANY_MOD | SKB_ANY_FM)) && b->cnt_escapes > 0) {
    if (!b->cross_group)
      return fail(SKRED_E_UNSUPPORTED, "a voice is modulated by a voice outside its aligned 64-voice group: "
                                       "keep modulator and carrier in the same group (SURVEY 8e)");
    if (b->cnt_outside > 0) return fail(SKRED_E_UNSUPPORTED, "a voice is modulated by a voice outside the bank");
  }
  if (b->esc_nomem) return fail(SKRED_E_NO_MEM, "cross-group modulators: host storage");
  HIP_TRY(hipSetDevice(b->device));
  int rc = sk_classify(b);
  if (rc) return rc;
  sk_tape_args_t ta;
  if ((rc = block_tape(b, num_frames, &ta))) return rc;
  poll_reports(b);

  /* the plan; the lane histogram is refreshed (it mutates the bank) only for a block that may pack its lanes */
  sk_plan_in_t in;
  sk_plan_t p;
  plan_input(b, num_frames, interp, d_stems != NULL, &in);
  sk_plan_family(&in, &p);
  sk_plan_finish(&in, p.pack_candidate ? sk_pack_refresh(b) : 0, &p);
  b->last_kernel = p.kernel;
  if (p.rc) return fail(p.rc, "%s", p.msg);

  sk_render_args_t a;
  args_from_bank(b, &in, &p, d_stems, &a);
  if ((rc = probe_rows(b, &a, s))) return rc;
  if (p.list_rebuild && (rc = rebuild_list(b, &a, s))) return rc;
  if (p.inplace && (rc = inplace_rows(b, &p, &a))) return rc;
  if ((rc = partial_rows(b, p.n_wg, p.two_env && !b->list_empty && !p.inplace, d_sum, d_out, num_channels, &a))) return rc;
  if (p.pack_s && (rc = pack_words(b, s))) return rc;
  if ((rc = launch_block(b, &a, &p, &ta, s))) return rc;

  b->last_family = b->last_kernel;
  b->last_in_place = p.inplace;
  b->last_split = p.split;
  b->last_pack = p.pack_s;
  b->last_cz = p.cz;
  b->last_taps = b->n_taps;
  b->last_tape_sources = ta.tape ? b->tape_sources : 0;
  b->last_tape_levels = ta.tape ? b->tape_levels : 0;

  /* advance the timeline exactly as synth.c:521,525 do: one count and one LCG draw per frame */
  b->g.synth_sample_count += (uint64_t)num_frames;
  uint64_t r = b->g.noise_rng;
  for (int i = 0; i < num_frames; i++) r = r * 6364136223846793005ULL + 1442695040888963407ULL;
  b->g.noise_rng = r;
  return SKRED_OK;
}

int skred_bank_render(skred_bank_t *b, int num_frames, int interp, float *d_partial, float *d_stems, void *stream) {
  if (!b || !d_partial || num_frames <= 0) return fail(SKRED_E_BAD_ARG, "render: bad arguments");
  return render_block(b, num_frames, interp, d_stems, d_partial, NULL, 0, (hipStream_t)stream);
}

/* The two halves of a block in the PIPELINED multi-GPU form (skred_shard.c: skred_shard_render_mix_pipelined): the render of block
 * k + 1 runs while the collective and the master stage of block k are still under way on another stream, so the per-frame gains
 * live in two alternating rows (`parity`) and the carried gain is committed by the render. */
int sk_bank_render_sum_pp(skred_bank_t *b, int num_frames, int interp, float *d_sum, int parity, void *stream) {
  if (!b || !d_sum || num_frames <= 0) return fail(SKRED_E_BAD_ARG, "render_sum_pp: bad arguments");
  b->pp_parity = parity & 1;
  const int rc = render_block(b, num_frames, interp, NULL, d_sum, NULL, 0, (hipStream_t)stream);
  b->pp_parity = -1;
  return rc;
}

int sk_bank_master_pp(skred_bank_t *b, const float *d_sum, int num_frames, int num_channels, float *d_out, int parity, void *stream) {
  if (!b || !d_sum || !d_out || num_frames <= 0 || num_channels < 2 || !b->d_pp_gains || (size_t)num_frames > b->pp_gains_cap)
    return fail(SKRED_E_BAD_ARG, "master_pp: bad arguments");
  HIP_TRY(hipSetDevice(b->device));
  const float *gains = b->d_pp_gains + ((parity & 1) ? b->pp_gains_cap : 0);
  /* (nothing to commit: slots 2 and 3 of the gain state are scratch) */
  const hipError_t e = (hipError_t)sk_launch_master_apply(d_sum, gains, d_out, num_frames, num_channels, b->d_gain_state + 2, b->d_gain_state + 3, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "master launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_bank_render_mix(skred_bank_t *b, int num_frames, int interp, float *d_out, int num_channels,
                          float *d_stems, void *stream) {
  if (!b || !d_out || num_frames <= 0 || num_channels < 2) return fail(SKRED_E_BAD_ARG, "render_mix: bad arguments");
  return render_block(b, num_frames, interp, d_stems, NULL, d_out, num_channels, (hipStream_t)stream);
}

int skred_bank_master(skred_bank_t *b, const float *d_sum, int num_frames, int num_channels, float *d_out, void *stream) {
  if (!b || !d_sum || !d_out || num_frames <= 0 || num_channels < 2) return fail(SKRED_E_BAD_ARG, "master: bad arguments");
  HIP_TRY(hipSetDevice(b->device));
  hipError_t e;
  if (b->gains_frames == num_frames && b->d_partial) {
    /* the render of this block (skred_bank_render, same stream) already walked the gains: scale and commit */
    const float *gains = b->d_partial + b->gains_offset;
    e = (hipError_t)sk_launch_master_apply(d_sum, gains, d_out, num_frames, num_channels, b->d_gain_state + 1, b->d_gain_state, (hipStream_t)stream);
    b->gains_frames = 0;
  } else {
    e = (hipError_t)sk_launch_master(d_sum, d_out, num_frames, num_channels, b->g.volume_final,
                                     b->g.volume_smoother_smoothing, b->d_gain_state, (hipStream_t)stream);
  }
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "master launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_bank_render_host(skred_bank_t *b, float *buffer, int num_frames, int num_channels, int interp, float *stems) {
  if (!b || !buffer || num_frames <= 0 || num_channels < 2) return fail(SKRED_E_BAD_ARG, "render_host: bad arguments");
  HIP_TRY(hipSetDevice(b->device));
  int rc;
  if ((rc = grow(&b->d_out, &b->out_cap, (size_t)num_frames * (size_t)num_channels))) return rc;
  const size_t stem_floats = (size_t)num_frames * (size_t)b->n_voices * 2;
  if (stems && (rc = grow(&b->d_stems, &b->stems_cap, stem_floats))) return rc;
  if (num_channels > 2) HIP_TRY(hipMemsetAsync(b->d_out, 0, (size_t)num_frames * num_channels * sizeof(float), NULL));
  if ((rc = skred_bank_render_mix(b, num_frames, interp, b->d_out, num_channels, stems ? b->d_stems : NULL, NULL))) return rc;
  HIP_TRY(hipMemcpy(buffer, b->d_out, (size_t)num_frames * num_channels * sizeof(float), hipMemcpyDeviceToHost));
  if (stems) HIP_TRY(hipMemcpy(stems, b->d_stems, stem_floats * sizeof(float), hipMemcpyDeviceToHost));
  return SKRED_OK;
}

float skred_bank_last_render_ms(skred_bank_t *b) {
  if (!b || b->n_timed == 0) return -1.0f;
  const int slot = (b->n_timed - 1) % SK_TIMING_RING;
  float ms = -1.0f;
  if (hipSetDevice(b->device) != hipSuccess) return -1.0f;
  if (hipEventSynchronize(b->ev1[slot]) != hipSuccess) return -1.0f;
  if (hipEventElapsedTime(&ms, b->ev0[slot], b->ev1[slot]) != hipSuccess) return -1.0f;
  return ms;
}

void skred_bank_timing_reset(skred_bank_t *b) { if (b) b->n_timed = 0; }

int skred_bank_timing_summary(skred_bank_t *b, float *mean_ms, float *min_ms, int *count) {
  if (!b) return fail(SKRED_E_BAD_ARG, "timing_summary");
  HIP_TRY(hipSetDevice(b->device));
  const int n = b->n_timed < SK_TIMING_RING ? b->n_timed : SK_TIMING_RING;
  double sum = 0.0;
  float mn = 0.0f;
  for (int i = 0; i < n; i++) {
    float ms = 0.0f;
    HIP_TRY(hipEventSynchronize(b->ev1[i]));
    HIP_TRY(hipEventElapsedTime(&ms, b->ev0[i], b->ev1[i]));
    sum += ms;
    if (i == 0 || ms < mn) mn = ms;
  }
  if (mean_ms) *mean_ms = n ? (float)(sum / n) : -1.0f;
  if (min_ms) *min_ms = n ? mn : -1.0f;
  if (count) *count = n;
  return SKRED_OK;
}
