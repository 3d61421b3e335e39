/*
 * skred_bank.c -- C host shim behind include/skred_amd.h (bank mode).
 *
 * Plain C on purpose (the reference's host code is C, north_star: "Host code stays in C and
 * reaches the HIP kernels through a thin C-ABI shim").  It owns the HBM copy of a voice bank and
 * packs the reference-named host arrays (synth.def:12-89) into the 16-byte device planes of
 * skred_device_layout.h; skred_bank_render.c sequences the kernels of skred_render_*.hip and
 * skred_mix_kernels.hip (through skred_launch.h) as skred_bank_plan.c picks them.  There is no CPU
 * rendering here: every failure to reach the GPU is reported, never papered over.
 */

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "skred_bank_priv.h"

static __thread char g_err[512];

const char *skred_amd_last_error(void) { return g_err; }

/* every translation unit of the library reports through this (skred_bank_priv.h: fail) */
int skred_amd_set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int skred_amd_abi_version(void) { return SKRED_AMD_ABI_VERSION; }

int skred_amd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

/* ------------------------------------------------------------------ create / destroy */

/* everything after the calloc: on any failure the caller destroys the partly built bank (skred_bank_destroy
 * tolerates one), so neither the struct nor the HBM already allocated leaks */
static int bank_build(skred_bank_t *b) {
  const size_t plane_bytes = (size_t)b->n_padded * sizeof(sk_plane_t);
  /* one slab, planes back to back (read-only planes first): a window of voices across all planes is one pitched copy */
  HIP_TRY(hipMalloc((void **)&b->d_planes, (size_t)(SKP_COUNT + SKS_COUNT) * plane_bytes));
  HIP_TRY(hipMemset(b->d_planes, 0, (size_t)(SKP_COUNT + SKS_COUNT) * plane_bytes));
  for (int p = 0; p < SKP_COUNT; p++) b->d_ro[p] = b->d_planes + (size_t)p * (size_t)b->n_padded;
  for (int p = 0; p < SKS_COUNT; p++) b->d_rw[p] = b->d_planes + (size_t)(SKP_COUNT + p) * (size_t)b->n_padded;
  /* every slot starts inert (skipped by the kernel) until a voice is uploaded into it */
  sk_plane_t *inert = (sk_plane_t *)calloc((size_t)b->n_padded, sizeof(sk_plane_t));
  if (!inert) return fail(SKRED_E_NO_MEM, "calloc");
  for (int v = 0; v < b->n_padded; v++) { inert[v].w[1] = 1; inert[v].w[2] = SKF_INERT; }   /* table_size 1: fetch stays in bounds */
  hipError_t e = hipMemcpy(b->d_ro[SKP_TAB], inert, plane_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const float one = 1.0f;                          /* loop window [0,1): phase 0 + inc 0 stays in range */
    for (int v = 0; v < b->n_padded; v++) { memset(&inert[v], 0, sizeof(inert[v])); memcpy(&inert[v].w[2], &one, 4); }
    e = hipMemcpy(b->d_ro[SKP_OSC], inert, plane_bytes, hipMemcpyHostToDevice);
  }
  free(inert);
  HIP_TRY(e);
  b->h_class = (uint16_t *)calloc((size_t)b->n_padded, sizeof(uint16_t));
  b->h_mod = (int8_t *)malloc((size_t)b->n_padded * 4);
  b->h_level = (int *)calloc((size_t)b->n_padded, sizeof(int));
  if (!b->h_class || !b->h_mod || !b->h_level) return fail(SKRED_E_NO_MEM, "calloc");
  memset(b->h_mod, -1, (size_t)b->n_padded * 4);
  {
    const size_t g64 = (size_t)b->n_padded / 64;
    b->h_pack_mask = (uint64_t *)calloc(g64, sizeof(uint64_t));
    b->h_pack_dirty = (uint8_t *)calloc(g64, 1);
    if (!b->h_pack_mask || !b->h_pack_dirty) return fail(SKRED_E_NO_MEM, "calloc");
    b->pack_hist[0] = (int)g64;
    HIP_TRY(hipMalloc((void **)&b->d_pack_mask, g64 * sizeof(uint64_t)));
    HIP_TRY(hipMemset(b->d_pack_mask, 0, g64 * sizeof(uint64_t)));
  }
  HIP_TRY(hipMalloc((void **)&b->d_level, (size_t)b->n_padded * sizeof(int)));
  HIP_TRY(hipMemset(b->d_level, 0, (size_t)b->n_padded * sizeof(int)));
  /* per 128-voice wave slice of the two-per-lane kernels: listed voices; one more slot: the one-voice family's ticket */
  HIP_TRY(hipMalloc((void **)&b->d_group_flag, (size_t)(b->n_groups * 2 + 1) * sizeof(int32_t)));
  HIP_TRY(hipMemset(b->d_group_flag, 0, (size_t)(b->n_groups * 2 + 1) * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void **)&b->d_env_list, (size_t)b->n_groups * SK_GROUP * sizeof(int32_t)));
  HIP_TRY(hipMemset(b->d_env_list, 0, (size_t)b->n_groups * SK_GROUP * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void **)&b->d_env_off, (size_t)(b->n_groups * 2 + 1) * sizeof(int32_t)));
  HIP_TRY(hipMemset(b->d_env_off, 0, (size_t)(b->n_groups * 2 + 1) * sizeof(int32_t)));
  /* the motion list, double-buffered (a bit per voice), and behind it the violation counter and sk_gain_kernel's two counters
   * (skred_device_layout.h: env_count): one allocation */
  {
    const size_t words = (size_t)b->n_groups * 4;
    HIP_TRY(hipMalloc((void **)&b->d_mask[0], (2 * words + 2) * sizeof(uint64_t)));   /* + violations, env_count[0], env_count[1], pad */
    HIP_TRY(hipMemset(b->d_mask[0], 0, (2 * words + 2) * sizeof(uint64_t)));
    b->d_mask[1] = b->d_mask[0] + words;
    b->d_violations = (uint32_t *)(b->d_mask[0] + 2 * words);
    b->mask_dirty = 1;
  }
  HIP_TRY(hipStreamCreateWithPriority(&b->side, hipStreamNonBlocking, -1));   /* (the envelope kernel's few workgroups should not queue behind a full machine) */
  HIP_TRY(hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming));
  HIP_TRY(hipMalloc((void **)&b->d_gain_state, 4 * sizeof(float)));
  HIP_TRY(hipMemset(b->d_gain_state, 0, 4 * sizeof(float)));
  /* arrival tickets of the in-kernel mix-down: zero once, every last arriver re-arms its own */
  /* slabs, final, the envelope kernel's own; behind them one "an envelope moved" word per workgroup row (one-voice family) */
  HIP_TRY(hipMalloc((void **)&b->d_tickets, (SK_FINISH_SLABS + 2 + SK_MAX_WORKGROUPS) * sizeof(uint32_t)));
  HIP_TRY(hipMemset(b->d_tickets, 0, (SK_FINISH_SLABS + 2 + SK_MAX_WORKGROUPS) * sizeof(uint32_t)));
  for (int i = 0; i < SK_TIMING_RING; i++) {
    HIP_TRY(hipEventCreate(&b->ev0[i]));
    HIP_TRY(hipEventCreate(&b->ev1[i]));
  }
  return SKRED_OK;
}

int skred_bank_create(int device, int n_voices, skred_bank_t **out) {
  if (!out || n_voices <= 0) return fail(SKRED_E_BAD_ARG, "skred_bank_create: bad arguments");
  *out = NULL;
  /* voice, slice and list indices inside the kernels are 32-bit ints (scaled by up to 128 before they are widened): the
   * documented ceiling keeps every such product below 2^31 with room to spare; tests/test_gpu_parity.py renders a bank of
   * exactly this size */
  if (n_voices > SKRED_MAX_VOICES)
    return fail(SKRED_E_RANGE, "skred_bank_create: %d voices exceed SKRED_MAX_VOICES (%d)", n_voices, SKRED_MAX_VOICES);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SKRED_E_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(SKRED_E_BAD_ARG, "device %d of %d", device, ndev);
  HIP_TRY(hipSetDevice(device));
  skred_bank_t *b = (skred_bank_t *)calloc(1, sizeof(*b));
  if (!b) return fail(SKRED_E_NO_MEM, "calloc");
  b->device = device;
  if (hipDeviceGetAttribute(&b->n_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || b->n_cus <= 0) b->n_cus = 256;
  b->n_voices = n_voices;
  b->n_groups = ((n_voices + 4 * SK_GROUP - 1) / (4 * SK_GROUP)) * 4;   /* multiple of 4: the two-per-lane kernel takes up to 1024 voices per pass */
  b->fast2_min_voices = SK_FAST2_MIN_VOICES;
  b->fm2_min_voices = SK_FM2_MIN_VOICES;
  b->in_place_mode = 1;
  b->split_mode = 0;
  b->pack_mode = 1;
  b->fm_skew = 1;
  b->timing_every = 1;
  b->pp_parity = -1;
  b->n_padded = b->n_groups * SK_GROUP;
  b->class_dirty = 1;
  b->mod_dirty = 1;
  /* synth.c:85-92 defaults: volume_user 1 * AMY_FACTOR, LCG seeded with 1 (synth.c:508) */
  b->g.synth_sample_count = 0;
  b->g.noise_rng = 1;
  b->g.volume_final = 0.025f;
  b->g.volume_smoother_gain = 0.0f;
  b->g.volume_smoother_smoothing = 0.002f;
  const int rc = bank_build(b);
  if (rc) { skred_bank_destroy(b); return rc; }      /* (the error text set by the failing step survives: destroy reports nothing) */
  *out = b;
  return SKRED_OK;
}

void skred_bank_destroy(skred_bank_t *b) {
  if (!b) return;
  hipSetDevice(b->device);
  if (b->d_planes) hipFree(b->d_planes);
  if (b->d_tables) hipFree(b->d_tables);
  free(b->h_tables);
  if (b->d_partial) hipFree(b->d_partial);
  if (b->d_tickets) hipFree(b->d_tickets);
  if (b->d_gain_state) hipFree(b->d_gain_state);
  if (b->d_pp_gains) hipFree(b->d_pp_gains);
  if (b->d_probe_ids) hipFree(b->d_probe_ids);
  if (b->d_tap_ids) hipFree(b->d_tap_ids);
  if (b->d_out) hipFree(b->d_out);
  if (b->d_stems) hipFree(b->d_stems);
  free(b->h_class); free(b->h_mod); free(b->h_level);
  free(b->h_pack_mask); free(b->h_pack_dirty);
  free(b->h_esc); free(b->h_slot);
  if (b->d_slot) hipFree(b->d_slot);
  if (b->d_tape_groups) hipFree(b->d_tape_groups);
  if (b->d_tape) hipFree(b->d_tape);
  if (b->d_pack_mask) hipFree(b->d_pack_mask);
  sk_queue_free(b);
  sk_patterns_free(b);
  sk_idle_free(b);
  sk_steal_free(b);
  sk_notes_free(b);
  sk_owner_free(b);
  sk_pedal_free(b);
  sk_glide_free(b);
  sk_bend_free(b);
  sk_cutoff_free(b);
  sk_fenv_free(b);
  for (int i = 0; i < SK_UPD_RING; i++) {
    if (b->upd[i].d) hipFree(b->upd[i].d);
    if (b->upd[i].h) hipHostFree(b->upd[i].h);
  }
  if (b->h_upd_done) hipHostFree((void *)b->h_upd_done);
  if (b->d_upd_cnt) hipFree(b->d_upd_cnt);
  free(b->upd_mark);
  if (b->h_report) hipHostFree((void *)b->h_report);
  if (b->d_level) hipFree(b->d_level);
  if (b->d_group_flag) hipFree(b->d_group_flag);
  if (b->d_env_list) hipFree(b->d_env_list);
  if (b->d_env_gain) hipFree(b->d_env_gain);
  if (b->d_env_off) hipFree(b->d_env_off);
  if (b->d_mask[0]) hipFree(b->d_mask[0]);
  if (b->side) hipStreamDestroy(b->side);
  if (b->ev_fork) hipEventDestroy(b->ev_fork);
  if (b->ev_join) hipEventDestroy(b->ev_join);
  for (int i = 0; i < SK_TIMING_RING; i++) {
    if (b->ev0[i]) hipEventDestroy(b->ev0[i]);
    if (b->ev1[i]) hipEventDestroy(b->ev1[i]);
  }
  free(b);
}

int skred_bank_n_voices(const skred_bank_t *b) { return b ? b->n_voices : 0; }

/* diagnostic builds only (tools/ab_split.py --stamps; not part of the ABI): the words a -DSKS_STAMPS build of
 * sk_render_split_kernel leaves in the bank's list buffer */
int sk_debug_env_list(skred_bank_t *b, int32_t *dst, int n) {
  if (!b || !dst || n <= 0 || n > b->n_groups * SK_GROUP) return SKRED_E_BAD_ARG;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(dst, b->d_env_list, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SKRED_OK;
}

/* ------------------------------------------------------------------ tables */

int skred_bank_set_tables_f32(skred_bank_t *b, const float *pool, size_t n_floats) {
  if (!b || !pool || n_floats == 0) return fail(SKRED_E_BAD_ARG, "set_tables: bad arguments");
  if (n_floats > 0x7FFFFFF0u) return fail(SKRED_E_RANGE, "table pool too large");
  HIP_TRY(hipSetDevice(b->device));
  if (b->d_tables) { hipFree(b->d_tables); b->d_tables = NULL; }
  b->table_floats = n_floats;
  b->table_floats_padded = (n_floats + SK_TABLE_PAD + 3) & ~(size_t)3;   /* readable past the last table: see SK_TABLE_PAD */
  HIP_TRY(hipMalloc((void **)&b->d_tables, b->table_floats_padded * sizeof(float)));
  HIP_TRY(hipMemset(b->d_tables, 0, b->table_floats_padded * sizeof(float)));
  HIP_TRY(hipMemcpy(b->d_tables, pool, n_floats * sizeof(float), hipMemcpyHostToDevice));
  free(b->h_tables);
  b->h_tables = (float *)malloc(n_floats * sizeof(float));
  if (!b->h_tables) return fail(SKRED_E_NO_MEM, "set_tables: host copy of the pool");
  memcpy(b->h_tables, pool, n_floats * sizeof(float));
  b->tables_epoch++;                    /* voices packed against the old pool carry its guard flags: sk_plan_in_t guard_current */
  return SKRED_OK;
}

/* ------------------------------------------------------------------ pack / unpack */

static inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int skred_bank_upload(skred_bank_t *b, const skred_voice_bank_t *h, int src_first, int dst_first, int count) {
  if (!b || !h || count < 0) return fail(SKRED_E_BAD_ARG, "upload: bad arguments");
  if (src_first < 0 || src_first + count > h->n_voices || dst_first < 0 || dst_first + count > b->n_voices)
    return fail(SKRED_E_RANGE, "upload window [%d,+%d) -> [%d,+%d) outside bank", src_first, count, dst_first, count);
  if (count == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  /* synchronous by contract: the planes are overwritten with a blocking copy, and a render still running on a
   * non-blocking stream (the caller's, or the bank's own tail stream) is not ordered against that by itself */
  HIP_TRY(hipDeviceSynchronize());
  const int NP = SKP_COUNT + SKS_COUNT;
  sk_plane_t *st = (sk_plane_t *)calloc((size_t)NP * (size_t)count, sizeof(sk_plane_t));
  sk_voice_meta_t *meta = (sk_voice_meta_t *)malloc((size_t)count * sizeof(sk_voice_meta_t));
  if (!st || !meta) { free(st); free(meta); return fail(SKRED_E_NO_MEM, "upload staging"); }
  for (int i = 0; i < count; i++) {
    sk_plane_t ro[SKP_COUNT], rw[SKS_COUNT];
    const int rc = sk_pack_voice(b, h, src_first + i, dst_first + i, 1, ro, rw, &meta[i]);
    if (rc) { free(st); free(meta); return rc; }
    for (int p = 0; p < SKP_COUNT; p++) st[(size_t)p * count + i] = ro[p];
    for (int p = 0; p < SKS_COUNT; p++) st[(size_t)(SKP_COUNT + p) * count + i] = rw[p];
  }
  const size_t bytes = (size_t)count * sizeof(sk_plane_t);
  /* all planes of the window in one pitched copy (rows = planes) */
  const hipError_t e = hipMemcpy2D(b->d_planes + dst_first, (size_t)b->n_padded * sizeof(sk_plane_t), st, bytes, bytes, (size_t)NP,
                                   hipMemcpyHostToDevice);
  free(st);
  if (e != hipSuccess) { free(meta); HIP_TRY(e); }
  if (dst_first == 0 && count == b->n_voices) { b->features = 0; b->guard_epoch = b->tables_epoch; }   /* whole bank replaced */
  for (int i = 0; i < count; i++) sk_apply_meta(b, dst_first + i, &meta[i], 1);
  free(meta);
  sk_control_changed(b);
  b->mask_dirty = 1;                    /* the motion list is rebuilt from the planes before the next two-per-lane block */
  b->pack_zero = 1;                     /* (uploaded state may hold a voice_sample on a voice that is skipped) */
  return SKRED_OK;
}

/* Packed lanes: the words of the groups whose voices changed, and the histogram that sizes the lane slots.  A group's word
 * holds the voices that can sound (SKC_LIVE) and the voices those name as modulators (they keep a lane so that the exchange of
 * the one-voice kernel finds them; at run time they are skipped like any dead voice).  Returns the most lanes a group needs. */
int sk_pack_refresh(skred_bank_t *b) {
  if (b->pack_any_dirty) {
    const int g64 = b->n_padded / 64;
    for (int g = 0; g < g64; g++) {
      if (!b->h_pack_dirty[g]) continue;
      b->h_pack_dirty[g] = 0;
      uint64_t w = 0;
      for (int l = 0; l < 64; l++) {
        const int v = g * 64 + l;
        if (b->h_slot && b->h_slot[v] >= 0) w |= (uint64_t)1 << l;   /* a tape source keeps its lane (and its voice_sample) */
        if (!(b->h_class[v] & SKC_LIVE)) continue;
        w |= (uint64_t)1 << l;
        for (int k = 0; k < 4; k++) {
          const int m = b->h_mod[(size_t)k * b->n_padded + v];
          if (m >= 0) w |= (uint64_t)1 << m;
        }
      }
      const uint64_t old = b->h_pack_mask[g];
      if (w == old) continue;
      b->pack_hist[__builtin_popcountll(old)]--;
      b->pack_hist[__builtin_popcountll(w)]++;
      b->h_pack_mask[g] = w;
      b->pack_upload = 1;
      if (old & ~w) b->pack_zero = 1;     /* a voice lost its lane: the reference would clear its voice_sample on the next frame */
    }
    b->pack_any_dirty = 0;
  }
  int most = 64;
  while (most > 0 && b->pack_hist[most] == 0) most--;
  return most;
}

/* Cross-group modulation (SKRED_OPT_CROSS_GROUP): the plan of the tape, made again whenever a cross-group routing changed
 * (skred_bank_plan.c: sk_tape_plan_host makes it and says what it refuses), and its maps on the device.  A refusal stands, render
 * after render, until the routing changes.  A refused or empty plan leaves no source. */
static int tape_plan(skred_bank_t *b) {
  if (!b->tape_dirty) return b->tape_rc ? fail(b->tape_rc, "%s", b->tape_msg) : SKRED_OK;
  b->tape_dirty = 0;
  b->tape_rc = 0;
  b->tape_sources = b->tape_levels = 0;
  if (!b->h_esc) return SKRED_OK;
  const int n = b->n_padded;
  int rc = SKRED_OK, levels = 0;
  int32_t *groups = (int32_t *)malloc((size_t)(n / 64) * sizeof(int32_t));
  int n_src = groups ? sk_tape_plan_host(b->h_esc, n, b->h_slot, b->h_pack_dirty, groups, b->tape_level_off, &levels, b->tape_msg, sizeof(b->tape_msg))
                     : SKRED_E_NO_MEM;
  b->pack_any_dirty = 1;                                 /* (the sources of the old plan lose their lanes, those of the new one get theirs) */
  if (n_src < 0) {
    if (n_src == SKRED_E_UNSUPPORTED) rc = fail(b->tape_rc = n_src, "%s", b->tape_msg);
    else rc = fail(n_src, "cross-group plan");
    n_src = 0;
  }
  if (n_src > 0) {
    const int n_sg = b->tape_level_off[levels];
    /* (the previous block may still read the maps) */
    if (hipDeviceSynchronize() != hipSuccess) { rc = fail(SKRED_E_NO_DEVICE, "cross-group plan: synchronize"); n_src = 0; goto out; }
    if ((size_t)n_sg > b->tape_groups_cap) {
      if (b->d_tape_groups) hipFree(b->d_tape_groups);
      b->d_tape_groups = NULL; b->tape_groups_cap = 0;
      if (hipMalloc((void **)&b->d_tape_groups, (size_t)n_sg * sizeof(int32_t)) != hipSuccess) { rc = fail(SKRED_E_NO_MEM, "tape groups"); n_src = 0; goto out; }
      b->tape_groups_cap = (size_t)n_sg;
    }
    if (!b->d_slot && hipMalloc((void **)&b->d_slot, (size_t)n * sizeof(int32_t)) != hipSuccess) { b->d_slot = NULL; rc = fail(SKRED_E_NO_MEM, "tape slots"); n_src = 0; goto out; }
    if (hipMemcpy(b->d_tape_groups, groups, (size_t)n_sg * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b->d_slot, b->h_slot, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
      rc = fail(SKRED_E_NO_DEVICE, "cross-group plan: upload"); n_src = 0; goto out;
    }
    b->tape_levels = levels;
  }
out:
  if (rc && rc != SKRED_E_UNSUPPORTED) b->tape_dirty = 1;   /* (no memory / device: try again at the next render) */
  if (n_src == 0) for (int v = 0; v < n; v++) b->h_slot[v] = -1;   /* (no plan: no source keeps a lane for the tape) */
  b->tape_sources = n_src;
  free(groups);
  return rc;
}

/* The bank's class (skred_bank_plan.c: sk_plan_class_mode says which kernel families may render it) and, for modulated banks,
 * the dependency levels, each made again when the voices changed; ahead of them the tape plan. */
int sk_classify(skred_bank_t *b) {
  if (b->tape_dirty || b->tape_rc) {                         /* (the cross-group routings changed; or they were refused) */
    const int rc = tape_plan(b);
    if (rc) return rc;
  }
  if (!b->class_dirty) return SKRED_OK;
  b->fast_mode = sk_plan_class_mode(b->cnt_real, b->cnt_filter, b->cnt_env, b->cnt_exotic, b->cnt_stops, b->cnt_fm, b->cnt_fm_odd, b->cnt_pair_ap);
  /* the same class with the CZ voices of the fast family taken for what the one-voice kernel renders (SKRED_OPT_CZ_FAST; the planner
   * picks between the two words): only when they are the bank's only exotic voices.  A voice among them that reads a previous-frame
   * source makes the launch exchange voice_sample (SKM_FM); no (carrier, next voice) pairs: that is the two-per-lane kernel's shape */
  b->fast_mode_cz = 0;
  if (b->cnt_cz > 0 && b->cnt_exotic == b->cnt_cz)
    b->fast_mode_cz = (sk_plan_class_mode(b->cnt_real, b->cnt_filter, b->cnt_env, 0, b->cnt_stops, b->cnt_fm + b->cnt_cz_src, b->cnt_fm_odd + b->cnt_cz_src, b->cnt_pair_ap) &
                       ~(uint32_t)(SKM_FM_PAIR | SKM_PAIR_AP)) | SKM_CZ;
  b->class_dirty = 0;
  /* dependency levels for modulated banks (skred_render_generic.hip: sk_render_mod_kernel) */
  if (!b->mod_dirty) return SKRED_OK;
  b->mod_dirty = 0;
  b->max_level = 0;
  if (b->features & (SKB_ANY_MOD | SKB_ANY_FM | SKB_ANY_CZ)) {
    b->max_level = sk_plan_levels(b->h_mod, b->n_padded, b->h_level);
    const hipError_t e = hipMemcpy(b->d_level, b->h_level, (size_t)b->n_padded * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) { b->mod_dirty = 1; return fail(SKRED_E_NO_DEVICE, "dependency levels -> %s", hipGetErrorString(e)); }
  }
  return SKRED_OK;
}

int skred_bank_set_option(skred_bank_t *b, int option, int value) {
  if (!b) return fail(SKRED_E_BAD_ARG, "set_option");
  switch (option) {
    case SKRED_OPT_FORCE_GENERIC: b->force_generic = value != 0; return SKRED_OK;
    case SKRED_OPT_FAST2_MIN_VOICES: b->fast2_min_voices = value; b->fast2_min_user = 1; return SKRED_OK;
    case SKRED_OPT_FM2_MIN_VOICES: b->fm2_min_voices = value; return SKRED_OK;
    case SKRED_OPT_IN_PLACE: b->in_place_mode = value < 0 ? 0 : value > 2 ? 2 : value; return SKRED_OK;
    case SKRED_OPT_KERNEL_TIMING: b->timing_every = value < 0 ? 0 : value; return SKRED_OK;
    case SKRED_OPT_SPLIT_PAIRS: b->split_pairs = (value == 2 || value == 4) ? value : 0; return SKRED_OK;
    case SKRED_OPT_SPLIT: b->split_mode = value < 0 ? 0 : value > 3 ? 3 : value; return SKRED_OK;
    case SKRED_OPT_PACK: b->pack_mode = value < 0 ? 0 : value > 2 ? 2 : value; return SKRED_OK;
    case SKRED_OPT_FM_SKEW: b->fm_skew = value != 0; return SKRED_OK;
    case SKRED_OPT_CROSS_GROUP: b->cross_group = value != 0; return SKRED_OK;
    case SKRED_OPT_CZ_FAST: b->cz_fast = value != 0; return SKRED_OK;    /* (read by the next block's plan: nothing is classified again) */
    default: return fail(SKRED_E_BAD_ARG, "unknown option %d", option);
  }
}

int skred_bank_set_probe(skred_bank_t *b, const int32_t *voices, int n, float *d_probe) {
  if (!b || n < 0 || n > SK_PROBE_MAX || (n > 0 && (!voices || !d_probe))) return fail(SKRED_E_BAD_ARG, "set_probe: bad arguments");
  if (n > 0 && b->n_taps > 0) return fail(SKRED_E_BAD_ARG, "set_probe: voice taps are set (skred_bank_set_taps)");
  for (int i = 0; i < n; i++)
    if (voices[i] < 0 || voices[i] >= b->n_voices) return fail(SKRED_E_RANGE, "set_probe: voice %d outside the bank", voices[i]);
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());                   /* (a block in flight may still read the old list) */
  if (n > 0) {
    if (!b->d_probe_ids) HIP_TRY(hipMalloc((void **)&b->d_probe_ids, SK_PROBE_MAX * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(b->d_probe_ids, voices, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  b->n_probe = n;
  b->d_probe_out = n > 0 ? d_probe : NULL;
  return SKRED_OK;
}

int skred_bank_set_taps(skred_bank_t *b, const int32_t *voices, int n, float *d_taps) {
  if (!b || n < 0 || n > SK_TAPS_MAX || (n > 0 && (!voices || !d_taps))) return fail(SKRED_E_BAD_ARG, "set_taps: bad arguments");
  if (n > 0 && b->n_probe > 0) return fail(SKRED_E_BAD_ARG, "set_taps: a probe is set (skred_bank_set_probe)");
  for (int i = 0; i < n; i++)
    if (voices[i] < 0 || voices[i] >= b->n_voices) return fail(SKRED_E_RANGE, "set_taps: voice %d outside the bank", voices[i]);
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());                   /* (a block in flight may still read the old list) */
  if (n > 0) {
    if (!b->d_tap_ids) HIP_TRY(hipMalloc((void **)&b->d_tap_ids, SK_TAPS_MAX * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(b->d_tap_ids, voices, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  b->n_taps = n;
  b->d_taps_out = n > 0 ? d_taps : NULL;
  return SKRED_OK;
}

int skred_bank_set_form_counter(skred_bank_t *b, uint32_t *d_counts) {
  if (!b) return fail(SKRED_E_BAD_ARG, "set_form_counter: no bank");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());                   /* (a block in flight may still count into the old words) */
  b->d_form_counts = d_counts;
  return SKRED_OK;
}

int skred_bank_last_kernel(const skred_bank_t *b) { return b ? b->last_kernel : -1; }
int skred_bank_last_in_place(const skred_bank_t *b) { return b ? b->last_in_place : 0; }
int skred_bank_last_split(const skred_bank_t *b) { return b ? b->last_split : 0; }
int skred_bank_last_pack(const skred_bank_t *b) { return b ? b->last_pack : 0; }
int skred_bank_last_cz(const skred_bank_t *b) { return b ? b->last_cz : 0; }
int skred_bank_last_taps(const skred_bank_t *b) { return b ? b->last_taps : 0; }
int skred_bank_last_cross_group(const skred_bank_t *b, int *n_sources, int *n_levels) {
  if (!b) return fail(SKRED_E_BAD_ARG, "last_cross_group: no bank");
  if (n_sources) *n_sources = b->last_tape_sources;
  if (n_levels) *n_levels = b->last_tape_levels;
  return SKRED_OK;
}
unsigned skred_bank_list_violations(const skred_bank_t *b) { return b ? b->violations_seen : 0u; }

int skred_bank_download(skred_bank_t *b, skred_voice_bank_t *h, int src_first, int dst_first, int count) {
  if (!b || !h || count < 0) return fail(SKRED_E_BAD_ARG, "download: bad arguments");
  if (src_first < 0 || src_first + count > b->n_voices || dst_first < 0 || dst_first + count > h->n_voices)
    return fail(SKRED_E_RANGE, "download window outside bank");
  if (count == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(b->device));
  sk_plane_t *st = (sk_plane_t *)malloc((size_t)SKS_COUNT * (size_t)count * sizeof(sk_plane_t));
  if (!st) return fail(SKRED_E_NO_MEM, "download staging");
  HIP_TRY(hipDeviceSynchronize());
  const size_t bytes = (size_t)count * sizeof(sk_plane_t);
  const hipError_t e = hipMemcpy2D(st, bytes, b->d_rw[0] + src_first, (size_t)b->n_padded * sizeof(sk_plane_t), bytes, (size_t)SKS_COUNT,
                                   hipMemcpyDeviceToHost);      /* the read-write planes of the window: one pitched copy */
  if (e != hipSuccess) { free(st); HIP_TRY(e); }
  for (int i = 0; i < count; i++) {
    const int v = dst_first + i;
    const sk_plane_t *s0 = &st[(size_t)SKS_OSC * count + i];
    const sk_plane_t *s1 = &st[(size_t)SKS_FILT * count + i];
    const sk_plane_t *s2 = &st[(size_t)SKS_MISC * count + i];
    h->voice_phase[v] = u2f(s0->w[0]);
    h->voice_smoother_gain[v] = u2f(s0->w[1]);
    h->voice_filter[v].x1 = u2f(s0->w[2]); h->voice_filter[v].x2 = u2f(s0->w[3]);
    h->voice_filter[v].y1 = u2f(s1->w[0]); h->voice_filter[v].y2 = u2f(s1->w[1]);
    h->voice_sample[v] = u2f(s1->w[2]);
    h->voice_finished[v] = (s1->w[3] & SKR_FINISHED) ? 1 : 0;
    h->voice_amp_envelope[v].is_active = (s1->w[3] & SKR_ENV_ACTIVE) ? 1 : 0;
    h->voice_sample_hold[v] = u2f(s2->w[0]);
    h->voice_sample_hold_count[v] = (int32_t)s2->w[1];
    h->voice_pan_left[v] = u2f(s2->w[2]);
    h->voice_pan_right[v] = u2f(s2->w[3]);
  }
  free(st);
  return SKRED_OK;
}

/* ------------------------------------------------------------------ globals */

int skred_bank_set_globals(skred_bank_t *b, const skred_globals_t *g) {
  if (!b || !g) return fail(SKRED_E_BAD_ARG, "set_globals");
  HIP_TRY(hipSetDevice(b->device));
  /* the carried master gain lives on the device and a block's tail may still be writing it (on the caller's
   * non-blocking stream): wait for the device first */
  HIP_TRY(hipDeviceSynchronize());
  b->g = *g;
  b->gains_frames = 0;                /* gains prepared for a pending skred_bank_master no longer hold */
  HIP_TRY(hipMemcpy(b->d_gain_state, &g->volume_smoother_gain, sizeof(float), hipMemcpyHostToDevice));
  sk_control_changed(b);              /* the clock may have moved: envelope stages are a function of it */
  b->mask_dirty = 1;
  return SKRED_OK;
}

int skred_bank_get_globals(skred_bank_t *b, skred_globals_t *g) {
  if (!b || !g) return fail(SKRED_E_BAD_ARG, "get_globals");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&b->g.volume_smoother_gain, b->d_gain_state, sizeof(float), hipMemcpyDeviceToHost));
  *g = b->g;
  return SKRED_OK;
}
