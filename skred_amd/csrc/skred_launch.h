/*
 * skred_launch.h -- C-linkage launch entry points of the HIP translation units (internal to
 * libskred_amd.so; the public ABI is include/skred_amd.h).
 *
 *   skred_render_generic.hip  sk_launch_render (dispatcher), sk_launch_render_mod, sk_launch_render_mod_tape, sk_launch_tape_prepass
 *                             (with args->probe_out set they forward to the tap unit, the same source built with -DSK_PROBE_TU)
 *   skred_render_fast.hip     sk_launch_render_fast
 *   skred_render_split.hip    sk_launch_render_split, sk_split_lds_bytes
 *   skred_render_fast2.hip    sk_launch_render_fast2, sk_launch_env_fast2, sk_env2_grid, sk_launch_classify
 *   skred_gain_kernels.hip    sk_launch_gain
 *   skred_mix_kernels.hip     sk_launch_master, sk_launch_master_apply
 *   skred_update_kernels.hip  sk_launch_update, sk_launch_stamp, sk_launch_pack_zero
 *   skred_rec_kernels.hip     sk_launch_rec_minmax, sk_rec_partial_floats, sk_launch_rec_convert
 *   skred_idle_kernels.hip    sk_launch_idle, sk_idle_workgroups, sk_launch_named
 *   skred_note_kernels.hip    sk_launch_notes, sk_launch_stamp_list
 *   skred_steal_kernels.hip   sk_launch_steal, sk_launch_steal_select, sk_launch_list_append, sk_launch_chan_join
 *   skred_slot_kernels.hip    sk_launch_slots, sk_launch_slot_notes, sk_launch_slot_stamps
 *   skred_slot_steal_kernels.hip  sk_launch_slot_steal (plain and matched)
 *   skred_ctl_kernels.hip     sk_launch_ctl_range, sk_launch_ctl_slots, sk_launch_ctl_owned
 *   skred_owner_kernels.hip   sk_launch_owner_tag, sk_launch_owner_find, sk_launch_owner_stamps
 *   skred_expr_kernels.hip    sk_launch_match_find, sk_launch_match_stamps, sk_launch_ctl_match, sk_launch_ctl_owned_each_filter
 *   skred_pedal_kernels.hip   sk_launch_pedal_clear, sk_launch_pedal_stamps, sk_launch_pedal_latch, sk_launch_pedal_up
 *   skred_glide_kernels.hip   sk_launch_glide_clear, sk_launch_glide_start, sk_launch_glide_advance, sk_launch_glide_stop
 *   skred_bend_kernels.hip    sk_launch_bend_clear, sk_launch_bend_match, sk_launch_bend_each, sk_launch_bend_range_clear
 *   skred_cutoff_kernels.hip  sk_launch_cutoff_clear, sk_launch_cutoff_match, sk_launch_cutoff_each, sk_launch_cutoff_advance,
 *                             sk_launch_cutoff_stop
 *   skred_fenv_kernels.hip    sk_launch_fenv_clear, sk_launch_fenv_match, sk_launch_fenv_each (the envelope's advance is
 *                             sk_launch_cutoff_advance with the array)
 *   skred_fx_pedal_kernels.hip  skx_launch_pedal_stamps, skx_launch_pedal_latch, skx_launch_pedal_up (sk_launch_pedal_clear by
 *                             skred_fx_owner.c too)
 *   skred_fx_glide_kernels.hip  skx_launch_glide_start, skx_launch_glide_advance, skx_launch_glide_stop (prototypes in
 *                             skred_fxbank_priv.h; sk_launch_glide_clear by skred_fx_owner.c too)
 *
 * Every launcher returns the hipError_t of the launch as an int.  The render, list and master-stage launchers are called by
 * skred_bank_render.c (as skred_bank_plan.c decides), sk_launch_pack_zero too; the rest by skred_bank_update.c, skred_bank_idle.c,
 * skred_bank_steal.c, skred_bank_notes.c, skred_bank_slots.c, skred_bank_ctl.c, skred_bank_owner.c, skred_bank_expr.c, skred_bank_pedal.c, skred_bank_glide.c and
 * skred_recorder.c (sk_launch_owner_tag, sk_launch_owner_find, sk_launch_match_find, sk_launch_list_append and sk_launch_chan_join by the fixed-point
 * bank's skred_fx_owner.c, skred_fx_expr.c and skred_fx_steal.c too).  A launcher that takes `cnt, done, seq` gets them from the batch path (skred_bank_stage.c: sk_batch_send).
 */
#ifndef SKRED_LAUNCH_H
#define SKRED_LAUNCH_H

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1   /* C hosts (gcc): hipcc defines it itself */
#endif
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "skred_device_layout.h"
#include "skred_fx_layout.h"      /* skx_plane_t, for the fixed-point pedal launchers */

#ifdef __cplusplus
extern "C" {
#endif

/* picks the kernel family from args->fast_mode / args->stems and launches it on `stream` */
int sk_launch_render(const sk_render_args_t *args, int n_workgroups, hipStream_t stream);
/* banks with modulators: one aligned 64-voice group per wavefront, dependency levels in `levels` */
int sk_launch_render_mod(const sk_render_args_t *args, int n_workgroups, const int *levels, int max_level,
                         hipStream_t stream);
/* cross-group modulation (SKRED_OPT_CROSS_GROUP): the main launch, whose modulator fields below -1 are read from t->tape, and one
 * pre-pass launch that writes the tape rows of the sources in the t->n_list groups t->groups (one wavefront each); the pre-pass
 * launches of a block go level by level ahead of the main launch, all on the same stream */
int sk_launch_render_mod_tape(const sk_render_args_t *args, int n_workgroups, const int *levels, int max_level,
                              const sk_tape_args_t *t, hipStream_t stream);
int sk_launch_tape_prepass(const sk_render_args_t *args, const int *levels, int max_level, const sk_tape_args_t *t,
                           hipStream_t stream);
/* the two specialised families (called by sk_launch_render only) */
int sk_launch_render_fast(const sk_render_args_t *args, int n_workgroups, size_t lds_bytes, hipStream_t stream);
int sk_launch_render_fast2(const sk_render_args_t *args, int n_workgroups, size_t lds_bytes, hipStream_t stream);
/* args->fast_mode & SKM_SPLIT: the one-voice family with the frame split between an oscillator wave and a post wave (512-thread
 * workgroups, 256 voices per pass as sk_launch_render_fast); sk_split_lds_bytes: the LDS one of its workgroups takes */
int sk_launch_render_split(const sk_render_args_t *args, int n_workgroups, int pairs, hipStream_t stream);
size_t sk_split_lds_bytes(const sk_render_args_t *args, int pairs);
/* the two-per-lane family's motion list (skred_render_fast2.hip): the list collected from args->mask_cur and rendered by
 * sk_render_env2_kernel on `stream` -- the block's SECOND stream, beside sk_launch_render_fast2 -- with args->n_env_rows
 * workgroups (sk_env2_grid: what the device holds at once); sk_launch_classify rebuilds `mask` from the planes */
int sk_launch_collect(const sk_render_args_t *args, hipStream_t stream);      /* mask_cur -> group_flag (counts), env_off, env_list; mask_next zeroed */
int sk_launch_env_fast2(const sk_render_args_t *args, hipStream_t stream);
int sk_env2_grid(const sk_render_args_t *args);
int sk_launch_classify(const sk_render_args_t *args, uint64_t *mask, hipStream_t stream);
/* sparse lists of LDS-table banks: the listed voices stay in their lanes.  sk_launch_gain (skred_gain_kernels.hip) writes their
 * per-frame gains into args->env_gain and the next block's list into args->mask_next, then sk_launch_render_fast2 -- with
 * args->env_gain set it launches the in-place instantiations -- renders the whole bank; same stream, in this order */
int sk_launch_gain(const sk_render_args_t *args, hipStream_t stream);

int sk_launch_master(const float *sum, float *out, int num_frames, int num_channels, float target, float k,
                     float *gain_state, hipStream_t stream);
/* the same with the block's gains already walked by the render kernel (gains[num_frames], the gain to carry on in gain_pending) */
int sk_launch_master_apply(const float *sum, const float *gains, float *out, int num_frames, int num_channels,
                           const float *gain_pending, float *gain_state, hipStream_t stream);

/* scatter n voice updates into the planes; `now` = synth_sample_count for the STAMP bits; every touched voice goes on the
 * motion list (`mask`: a bit per voice, skred_device_layout.h: mask_cur) */
/* cnt / done / seq: when `done` is not NULL the workgroup that finishes last stores `seq` into *done (pinned host memory the
 * host polls before it reuses the staging buffer the batch was read from); `cnt` is that slot's arrival counter on the device */
int sk_launch_update(const sk_update_t *d_updates, int n, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT],
                     uint64_t now, uint64_t *mask, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);

/* note-on / note-off stamps only: a list of voice ids */
int sk_launch_stamp(const int32_t *d_ids, int n, uint32_t dirty, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT],
                    uint64_t now, uint64_t *mask, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);

/* packed lanes: voice_sample = 0 for every voice without a bit in d_mask (one bit per voice of the padded bank) */
int sk_launch_pack_zero(const uint64_t *d_mask, sk_plane_t *filt, int n_voices_padded, hipStream_t stream);

/* ---- the free-voice query (skred_bank_idle.c -> skred_idle_kernels.hip; include/skred_amd.h: skred_bank_find_idle) ----
 * The bits equal SKRED_IDLE_* (checked at compile time in skred_bank_idle.c). */
#define SK_IDLE_FINISHED (1u << 0)
#define SK_IDLE_ENV_DONE (1u << 1)
#define SK_IDLE_AMP_ZERO (1u << 2)
#define SK_IDLE_UNNAMED  (1u << 8)
#define SK_IDLE_SPAN 256           /* voices (and threads) per workgroup of both kernels */
/* the bank's scratch: SK_IDLE_W_COUNT words, then the workgroups' counts, then their exclusive offsets */
enum { SK_IDLE_W_TICKET = 0,      /* arrival ticket of the count kernel, re-armed by its last arriver */
       SK_IDLE_W_PART,            /* idle voices below `from` inside from's own workgroup */
       SK_IDLE_W_RANK,            /* idle voices of the range below `from` */
       SK_IDLE_W_TOTAL,           /* idle voices of the range */
       SK_IDLE_W_COUNT };
typedef struct {
  const sk_plane_t *osc_ro, *tab;  /* SKP_OSC (amp in .w), SKP_TAB (flags in .z) */
  const sk_plane_t *osc_rw, *filt; /* SKS_OSC (smoother gain in .y), SKS_FILT (rwflags in .w) */
  const uint64_t *named;           /* [n_padded / 64] or NULL without SK_IDLE_UNNAMED */
  uint32_t *words, *counts, *offsets;
  int32_t *d_voices;
  uint32_t *d_count;
  int32_t first, end, from;        /* the range [first, end), the voice the listing starts at */
  int32_t max_out;
  uint32_t which;
  float settle_level;
  int32_t base, from_wg;           /* filled by sk_launch_idle: first rounded down to 64, the workgroup that holds `from` */
} sk_idle_args_t;
int sk_idle_workgroups(int first, int count);           /* workgroups (entries of counts / offsets) a range takes */
int sk_launch_idle(const sk_idle_args_t *args, hipStream_t stream);   /* count, then (max_out > 0) scatter */
/* the named set: bit v of named[] = some voice of the bank names voice v as a modulator (cleared, then rebuilt from SKP_MODI) */
int sk_launch_named(const sk_plane_t *tab, const sk_plane_t *modi, int n_padded, int n_voices, uint64_t *named, hipStream_t stream);

/* ---- note-ons and stamps on voices named by a list in device memory (skred_bank_notes.c -> skred_note_kernels.hip;
 * include/skred_amd.h: skred_bank_notes_on_list / _stamp_list) ----
 * A note record is skred_note_t word for word (layout and flag bits checked at compile time in skred_bank_notes.c). */
enum { SK_NOTE_PHASE_INC = 0, SK_NOTE_VELOCITY, SK_NOTE_PHASE, SK_NOTE_PAN_LEFT, SK_NOTE_PAN_RIGHT, SK_NOTE_FLAGS, SK_NOTE_WORDS = 8 };
#define SK_NOTE_SET_PHASE (1u << 0)
#define SK_NOTE_SET_PAN   (1u << 1)
#define SK_NOTE_SPAN 256           /* notes (and threads) per workgroup of sk_notes_kernel */
typedef struct {
  uint32_t w[SK_NOTE_WORDS];
} sk_note_t;
/* note k -> voice d_voices[first_entry + k] while first_entry + k < d_count[0] and the entry names a voice of the bank;
 * d_assigned[n] (or NULL) and d_result[2] = placed, dropped; `now`, `mask` and cnt / done / seq as for sk_launch_update
 * (d_notes may be the pinned staging buffer).  More than SK_NOTE_SPAN notes: d_result is zeroed on `stream` ahead of the launch */
int sk_launch_notes(const sk_note_t *d_notes, int n, const int32_t *d_voices, const uint32_t *d_count, int first_entry, int n_voices,
                    sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t now, uint64_t *mask,
                    int32_t *d_assigned, uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);
/* sk_launch_stamp for the first min(n, d_count[0]) entries (d_count NULL: n) of a list in device memory; entries outside
 * [0, n_voices) are skipped */
int sk_launch_stamp_list(const int32_t *d_voices, int n, const uint32_t *d_count, int n_voices, uint32_t dirty,
                         sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t now, uint64_t *mask,
                         hipStream_t stream);

/* ---- voice stealing (skred_bank_steal.c -> skred_steal_kernels.hip; include/skred_amd.h: skred_bank_find_steal) ----
 * The k = min(max_out, candidates) smallest 64-bit keys of a range, ties by voice index: a most-significant-digit radix select
 * over SK_STEAL_DIGITS digits of SK_STEAL_BITS bits, an index-ordered count and scatter of the winners, and a sort of the at most
 * SK_STEAL_MAX winners by one workgroup.  The policy and flag bits equal SKRED_STEAL_* (checked in skred_bank_steal.c). */
#define SK_STEAL_MAX 1024
#define SK_STEAL_OLDEST 0u
#define SK_STEAL_QUIETEST 1u
#define SK_STEAL_RELEASED_FIRST (1u << 0)
#define SK_STEAL_RELEASED_ONLY  (1u << 1)
#define SK_STEAL_UNNAMED        (1u << 8)
#define SK_STEAL_BITS 11
#define SK_STEAL_BINS (1 << SK_STEAL_BITS)
#define SK_STEAL_DIGITS 6          /* 6 * 11 = 66 >= 64: the first digit holds the key's top 9 bits */
#define SK_STEAL_NOKEY (~0ull)     /* what a voice that is no candidate holds in `keys` (a key never has bit 63) */
/* the bank's scratch: SK_STEAL_W_COUNT words (zeroed once; every last arriver re-arms what it used), the digit histogram
 * (SK_STEAL_BINS words, zero between launches), four arrays of one word per workgroup (counts and exclusive offsets of the keys
 * below / equal to the threshold), the winners (SK_STEAL_MAX keys, then SK_STEAL_MAX voices), and one key per voice of the spans */
enum { SK_STEAL_W_TICKET = 0,     /* arrival ticket, shared by the launches of a query (they follow one another on the stream) */
       SK_STEAL_W_TOTAL,          /* candidates of the range */
       SK_STEAL_W_K,              /* min(max_out, total): how many the list will hold */
       SK_STEAL_W_REMAIN,         /* ... of them, how many lie in the histogram bin the digits so far select */
       SK_STEAL_W_PREFIX_LO,      /* the digits fixed so far (after the last digit pass: the threshold key) */
       SK_STEAL_W_PREFIX_HI,
       SK_CHAN_W_SOUNDING,        /* a matched key pass only (both banks): its workgroups add up the sounding slots of the match here;
                                     its last arriver stores the sum to d_count[2] and re-arms the word.  The select never touches it */
       SK_STEAL_W_COUNT = 8 };
typedef struct {
  sk_idle_args_t idle;             /* the exclusion: planes, named set, which = exclude_idle, settle_level (first / end as below) */
  const sk_plane_t *env_s;         /* SKP_ENV_S: sample_start, sample_release */
  uint32_t *words, *hist;
  uint32_t *cnt_lt, *cnt_eq, *off_lt, *off_eq;
  unsigned long long *win_keys;    /* [SK_STEAL_MAX] */
  int32_t *win_voices;             /* [SK_STEAL_MAX] */
  unsigned long long *keys;        /* [workgroups * SK_IDLE_SPAN] */
  int32_t *d_voices;
  uint32_t *d_count;
  uint64_t now, min_age;
  int32_t first, end, base;        /* the range [first, end); base: filled by sk_launch_steal (first rounded down to 64) */
  int32_t max_out;
  uint32_t policy, flags;
  int32_t digit;                   /* filled by sk_launch_steal: which digit a histogram launch counts */
} sk_steal_args_t;
/* the keys and the first digit's histogram; SK_STEAL_DIGITS - 1 further digit launches; count; scatter; sort (one workgroup, writes
 * d_voices and d_count): SK_STEAL_DIGITS + 3 launches whatever the data.  max_out == 0: the first launch alone, which writes d_count */
int sk_launch_steal(const sk_steal_args_t *args, hipStream_t stream);
/* everything behind the key pass, which reads `keys` and `words` and no plane: digits 1 .. SK_STEAL_DIGITS - 1, count, scatter,
 * sort (nothing with max_out == 0).  sk_launch_steal ends in it; the fixed-point bank's key pass (skred_fx_steal_kernels.hip)
 * enters here with `idle` and env_s left zero */
int sk_launch_steal_select(const sk_steal_args_t *args, hipStream_t stream);
/* dst[at + t] = src[t] for t < min(src_count[0], room - at), at = dst_count[0] (<= room); out_count[0] = at + copied;
 * stolen[0] = copied.  One workgroup: room - at is at most SK_STEAL_MAX entries (src holds no more) */
int sk_launch_list_append(int32_t *dst, const uint32_t *dst_count, const int32_t *src, const uint32_t *src_count, int room,
                          uint32_t *out_count, uint32_t *stolen, hipStream_t stream);
/* The join of a capped burst (channel polyphony, both banks).  One workgroup.  I = min(idle_count[0], n), S = victim_count[2],
 * V = min(victim_count[0], SK_STEAL_MAX): a = min(n, I, cap > S ? cap - S : 0), b = min(n - a, V); list[a + t] = victims[t] for
 * t < b; out_count[0] = a + b; d_result[2] = b, d_result[3] = S.  `list` has room for n entries */
int sk_launch_chan_join(int32_t *list, const uint32_t *idle_count, const int32_t *victims, const uint32_t *victim_count, int n,
                        uint32_t cap, uint32_t *out_count, uint32_t *d_result, hipStream_t stream);

/* ---- patch notes: idle slots, and notes and stamps on the voices of listed slots (skred_bank_slots.c -> skred_slot_kernels.hip;
 * include/skred_amd.h: skred_bank_find_idle_slots / _notes_on_slots / _stamp_slots) ----
 * A slot: slot_voices = K consecutive voices from a multiple of K (K a power of two <= 64), named by its first voice.  The query is
 * the free-voice query with another notion of "listed": `idle` holds the planes, the range, `from`, max_out, the criteria (never
 * SK_IDLE_UNNAMED) and the bank's idle scratch; d_voices receives first voices of slots. */
typedef struct {
  sk_idle_args_t idle;
  uint64_t member_mask;            /* bit l: voice l of a slot takes part in the idle test */
  int32_t slot_voices;
} sk_slot_args_t;
int sk_launch_slots(const sk_slot_args_t *args, hipStream_t stream);   /* count, then (max_out > 0) scatter */
/* note k (records d_notes[k * K .. k * K + K)) -> the slot d_slots[first_entry + k] while first_entry + k < d_count[0] and the entry
 * is a slot of the bank (>= 0, a multiple of K, entry + K <= n_voices); only voices with a bit in voice_mask are stored to, only
 * their records read.  d_assigned[n] (or NULL) and d_result[2] = placed, dropped notes; the rest as sk_launch_notes.  More than
 * one workgroup (n * K > SK_NOTE_SPAN): d_result is zeroed on `stream` ahead of the launch */
int sk_launch_slot_notes(const sk_note_t *d_notes, int n, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                         const uint32_t *d_count, int first_entry, int n_voices, sk_plane_t *const ro[SKP_COUNT],
                         sk_plane_t *const rw[SKS_COUNT], uint64_t now, uint64_t *mask, int32_t *d_assigned, uint32_t *d_result,
                         uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);
/* threads per workgroup of every control kernel below that takes a slot list or a range of slots: the stamps on listed slots, the
 * controllers, the owner, expression, pedal and glide kernels (skred_update_common.hpp: sk_entry_decode, sk_range_lane, sk_grid) */
#define SK_CONTROL_SPAN 256
/* sk_launch_stamp_list on the masked voices of the first min(n, d_count[0]) listed slots (d_count NULL: n); entries that are no
 * slot of the bank are skipped */
int sk_launch_slot_stamps(const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices, uint64_t voice_mask, int n_voices,
                          uint32_t dirty, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t now,
                          uint64_t *mask, hipStream_t stream);

/* ---- slot stealing (skred_bank_slots.c -> skred_slot_steal_kernels.hip; include/skred_amd.h: skred_bank_find_steal_slots) ----
 * sk_launch_steal with another key pass: one key per SLOT of slot_voices voices, stored at the slot's first voice (every other voice
 * of the spans holds SK_STEAL_NOKEY), made of the terms of the voices with a bit in member_mask; then sk_launch_steal_select as it
 * is.  `args` as for sk_launch_steal (first and end multiples of slot_voices, never SK_STEAL_UNNAMED / SK_IDLE_UNNAMED); d_voices
 * receives first voices of slots.  max_out == 0: the key pass alone, which writes d_count.
 * `owner` != NULL (one word per voice of the bank): the MATCHED query of channel polyphony (include/skred_amd.h: "channel
 * polyphony") -- a slot takes part when owner[first voice] != 0 and (owner & mask) == value, and d_count is uint32[3]: written, total
 * candidates, sounding slots of the match in the range (the key pass writes all three with max_out == 0).  NULL: value and mask are
 * not looked at, d_count is uint32[2] */
int sk_launch_slot_steal(const sk_steal_args_t *args, uint64_t member_mask, int slot_voices, const uint32_t *owner, uint32_t value,
                         uint32_t mask, hipStream_t stream);

/* ---- patch controllers (skred_bank_ctl.c -> skred_ctl_kernels.hip; include/skred_amd.h: skred_bank_ctl_range / _ctl_slots) ----
 * A controller record is skred_ctl_t word for word (layout and bits checked at compile time in skred_bank_ctl.c): word 0 names the
 * fields to store, the values follow.  The bits equal SKRED_CTL_*. */
#define SK_CTL_PHASE_INC  (1u << 0)
#define SK_CTL_INC_SCALE  (1u << 1)
#define SK_CTL_AMP        (1u << 2)
#define SK_CTL_PAN        (1u << 3)
#define SK_CTL_FILTER     (1u << 4)
#define SK_CTL_ENV_TIMES  (1u << 5)
#define SK_CTL_VELOCITY   (1u << 6)
#define SK_CTL_SMOOTHING  (1u << 7)
#define SK_CTL_FM_DEPTH   (1u << 8)
#define SK_CTL_FREQ_SCALE (1u << 9)
#define SK_CTL_AM_DEPTH   (1u << 10)
#define SK_CTL_PAN_DEPTH  (1u << 11)
#define SK_CTL_CZ_DEPTH   (1u << 12)
#define SK_CTL_CZ_DIST    (1u << 13)
#define SK_CTL_ALL        ((1u << 14) - 1u)
/* the words sk_env_motion (skred_kernel_common.hpp) reads: a voice whose record names one goes on the motion list */
#define SK_CTL_LISTS      (SK_CTL_AMP | SK_CTL_ENV_TIMES | SK_CTL_VELOCITY | SK_CTL_SMOOTHING)
enum { SK_CTL_SET = 0, SK_CTL_W_PHASE_INC, SK_CTL_W_INC_SCALE, SK_CTL_W_AMP, SK_CTL_W_PAN_LEFT, SK_CTL_W_PAN_RIGHT, SK_CTL_W_B0, SK_CTL_W_B1,
       SK_CTL_W_B2, SK_CTL_W_A1, SK_CTL_W_A2, SK_CTL_W_ATTACK, SK_CTL_W_DECAY, SK_CTL_W_SUSTAIN, SK_CTL_W_RELEASE, SK_CTL_W_VELOCITY,
       SK_CTL_W_SMOOTHING, SK_CTL_W_FM_DEPTH, SK_CTL_W_FREQ_SCALE, SK_CTL_W_AM_DEPTH, SK_CTL_W_PAN_DEPTH, SK_CTL_W_CZ_DEPTH,
       SK_CTL_W_CZ_DIST, SK_CTL_W_RESERVED, SK_CTL_WORDS };
typedef struct {
  uint32_t w[SK_CTL_WORDS];
} sk_ctl_t;
/* d_recs: slot_voices records (record l: voice l of a slot; records without a bit in voice_mask hold set == 0), possibly the pinned
 * staging buffer; cnt / done / seq and `mask` as for sk_launch_update.  d_result[2] (or NULL) is zeroed on `stream` ahead of the
 * kernel and receives voices written, stores withheld.  Range: every slot of [first, first + count), both multiples of slot_voices
 * inside the bank.  Slots: the first min(n, d_count[0]) entries (d_count NULL: n); entries that are no slot of the bank are skipped */
int sk_launch_ctl_range(const sk_ctl_t *d_recs, int slot_voices, uint64_t voice_mask, int first, int count,
                        sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t *mask, uint32_t *d_result,
                        uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);
int sk_launch_ctl_slots(const sk_ctl_t *d_recs, int slot_voices, uint64_t voice_mask, const int32_t *d_slots, int n,
                        const uint32_t *d_count, int n_voices, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT],
                        uint64_t *mask, uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);

/* ---- note owners (skred_bank_owner.c -> skred_owner_kernels.hip, the guarded controller in skred_ctl_kernels.hip;
 * include/skred_amd.h: skred_bank_tag_slots / _find_owned / _stamp_owned / _release_tags / _ctl_owned) ----
 * owner[n_voices]: one word per voice, a slot's owner at its first voice, 0 nobody.  Only these launches read or write it.
 * d_tags and the other staged arrays may be the pinned staging buffer; cnt / done / seq as for sk_launch_update. */
#define SK_OWNER_MAX_TAGS 1024
/* owner[d_slots[k]] = d_tags[k] for the first min(n, d_count[0]) entries (d_count NULL: n) that are slots of the bank; d_result[2]
 * (or NULL; zeroed on `stream` ahead of the kernel) += slots tagged, entries that are no slot */
int sk_launch_owner_tag(uint32_t *owner, const int32_t *d_slots, const uint32_t *d_tags, int n, const uint32_t *d_count, int slot_voices,
                        int n_voices, uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);
/* d_out[d_perm[j]] = min over the slots of [first, first + count) whose owner is d_sorted[j] of the slot's first voice, as an
 * unsigned minimum onto d_out[0 .. n) preset to all-ones on `stream` (-1: nobody).  d_sorted: the n tags ascending as unsigned
 * numbers, none zero, none twice; d_perm: where each stood in the caller's array.  One lane per slot */
int sk_launch_owner_find(const uint32_t *owner, int first, int count, int slot_voices, const uint32_t *d_sorted, const uint32_t *d_perm,
                         int n, int32_t *d_out, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);
/* sk_launch_slot_stamps on the entries whose owner word equals d_tags[k]; d_result[3] (zeroed on `stream` ahead of the kernel) +=
 * slots stamped, slots whose owner differs, entries that are no slot */
int sk_launch_owner_stamps(const uint32_t *owner, const int32_t *d_slots, const uint32_t *d_tags, int n, const uint32_t *d_count,
                           int slot_voices, uint64_t voice_mask, int n_voices, uint32_t dirty, sk_plane_t *const ro[SKP_COUNT],
                           sk_plane_t *const rw[SKS_COUNT], uint64_t now, uint64_t *mask, uint32_t *d_result, uint32_t *cnt,
                           uint32_t *done, uint32_t seq, hipStream_t stream);
/* sk_launch_ctl_slots on the entries whose owner word equals d_tags[k]; d_result[3] (or NULL): voices written, stores withheld,
 * slots whose owner differs */
int sk_launch_ctl_owned(const sk_ctl_t *d_recs, int slot_voices, uint64_t voice_mask, const int32_t *d_slots, const uint32_t *d_tags,
                        const uint32_t *owner, int n, const uint32_t *d_count, int n_voices, sk_plane_t *const ro[SKP_COUNT],
                        sk_plane_t *const rw[SKS_COUNT], uint64_t *mask, uint32_t *d_result, uint32_t *cnt, uint32_t *done,
                        uint32_t seq, hipStream_t stream);

/* ---- channels and per-note expression (skred_bank_expr.c -> skred_expr_kernels.hip; include/skred_amd.h: skred_bank_find_match /
 * _stamp_match / _ctl_match / _ctl_owned_each / _ctl_tags_each) ----
 * A slot matches when owner != 0 && (owner & mask) == value.  The ranges are whole slots inside the bank (checked on the host). */
/* the ordered list of the matching slots: one lane per SLOT, skred_idle_scan.hpp's count and scatter.  `idle` holds the bank's idle
 * scratch (words, counts, offsets), d_voices (the list), max_out, and d_count = two scratch words the count pass fills as it does
 * for an idle query; first / end / from / base / from_wg are set by the launcher.  d_total[0] = the total, written by the second
 * launch, which runs with max_out == 0 too */
typedef struct {
  sk_idle_args_t idle;
  const uint32_t *owner;
  uint32_t *d_total;
  uint32_t value, mask;
  int32_t first, n_slots, k_shift;
} sk_match_args_t;
int sk_launch_match_find(const sk_match_args_t *args, int first, int count, int slot_voices, hipStream_t stream);
/* sk_launch_slot_stamps on every matching slot of the range; d_result[2] (zeroed on `stream` ahead of the kernel) += slots stamped,
 * slots that did not match */
int sk_launch_match_stamps(const uint32_t *owner, uint32_t value, uint32_t mask, int first, int count, int slot_voices,
                           uint64_t voice_mask, uint32_t dirty, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT],
                           uint64_t now, uint64_t *mask_list, uint32_t *d_result, hipStream_t stream);
/* sk_launch_ctl_range on the matching slots; d_result[3] (or NULL): voices written, stores withheld, slots that did not match */
int sk_launch_ctl_match(const sk_ctl_t *d_recs, int slot_voices, uint64_t voice_mask, int first, int count, const uint32_t *owner,
                        uint32_t value, uint32_t mask, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT],
                        uint64_t *mask_list, uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);
/* A per-entry record is skred_ctl_each_t word for word (layout and bits checked at compile time in skred_bank_expr.c); the bits
 * equal SKRED_EACH_*.  Values an entry does not name arrive zeroed. */
#define SK_EACH_INC_SCALE (1u << 0)
#define SK_EACH_AMP_SCALE (1u << 1)
#define SK_EACH_VELOCITY  (1u << 2)
#define SK_EACH_PAN       (1u << 3)
#define SK_EACH_ALL       ((1u << 4) - 1u)
enum { SK_EACH_SET = 0, SK_EACH_W_INC_SCALE, SK_EACH_W_AMP_SCALE, SK_EACH_W_VELOCITY, SK_EACH_W_PAN_LEFT, SK_EACH_W_PAN_RIGHT, SK_EACH_WORDS = 8 };
typedef struct {
  uint32_t w[SK_EACH_WORDS];
} sk_each_t;
/* A per-entry filter record is skred_filter_each_t word for word (checked at compile time in skred_bank_expr.c): 32 bytes, so that
 * b0 b1 b2 a1 are one aligned 16-byte load. */
enum { SK_FILT_W_B0 = 0, SK_FILT_W_B1, SK_FILT_W_B2, SK_FILT_W_A1, SK_FILT_W_A2, SK_FILT_WORDS = 8 };
typedef struct {
  uint32_t w[SK_FILT_WORDS];
} sk_filt_each_t;
/* sk_launch_ctl_owned with entry k's record d_each[k] laid over the K records (d_recs: records without a mask bit, and all of them
 * when the caller gave none, hold set == 0); d_result[3] as there, the withheld products counted in [1].  d_filt != NULL: also entry
 * k's coefficients d_filt[k] (16-byte aligned) laid over record l, with SK_CTL_FILTER, on the voices l of filter_mask (a subset of
 * voice_mask; no masked record of it names SK_CTL_FILTER); d_each may then be NULL: the coefficients alone.  d_filt == NULL:
 * filter_mask is not looked at and d_each is required */
int sk_launch_ctl_owned_each_filter(const sk_ctl_t *d_recs, const sk_each_t *d_each, const sk_filt_each_t *d_filt, int slot_voices,
                                    uint64_t voice_mask, uint64_t filter_mask, const int32_t *d_slots, const uint32_t *d_tags,
                                    const uint32_t *owner, int n, const uint32_t *d_count, int n_voices, sk_plane_t *const ro[SKP_COUNT],
                                    sk_plane_t *const rw[SKS_COUNT], uint64_t *mask_list, uint32_t *d_result, uint32_t *cnt,
                                    uint32_t *done, uint32_t seq, hipStream_t stream);

/* ---- pedals (skred_bank_pedal.c -> skred_pedal_kernels.hip; include/skred_amd.h: skred_bank_stamp_owned_pedal /
 * _release_tags_pedal / _pedal_latch / _pedal_up) ----
 * pedal[n_voices]: one word per voice beside the owner array, a slot's word at its first voice.  Only these launches read or write
 * it.  The bits equal SKRED_PEDAL_* (checked at compile time in skred_bank_pedal.c). */
#define SK_PEDAL_PENDING        (1u << 0)
#define SK_PEDAL_LATCHED        (1u << 1)
#define SK_PEDAL_LIFT_SUSTAIN   (1u << 0)
#define SK_PEDAL_LIFT_SOSTENUTO (1u << 1)
#define SK_PEDAL_SUSTAIN_DOWN   (1u << 2)
/* pedal[d_slots[k]] = 0 under sk_launch_owner_tag's list rule: launched behind it by a bank that has a pedal array */
int sk_launch_pedal_clear(uint32_t *pedal, const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices, int n_voices,
                          hipStream_t stream);
/* sk_launch_owner_stamps with the stamp fixed to a release, except where hold_all != 0 or the slot is LATCHED: there PENDING is set
 * and nothing stamped.  d_result[4] (zeroed on `stream` ahead of the kernel) += slots stamped, slots whose owner differs, entries
 * that are no slot, slots held back */
int sk_launch_pedal_stamps(const uint32_t *owner, uint32_t *pedal, const int32_t *d_slots, const uint32_t *d_tags, int n,
                           const uint32_t *d_count, int slot_voices, uint64_t voice_mask, int n_voices, int hold_all,
                           sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint64_t now, uint64_t *mask,
                           uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);
/* LATCHED on every matching slot of the range that is not PENDING and has a held voice_mask voice (live, not released);
 * d_result[2] (zeroed on `stream` ahead of the kernel) += slots latched, slots that did not match */
int sk_launch_pedal_latch(const uint32_t *owner, uint32_t *pedal, uint32_t value, uint32_t mask, int first, int count, int slot_voices,
                          uint64_t voice_mask, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT], uint32_t *d_result,
                          hipStream_t stream);
/* flags: SK_PEDAL_LIFT_* / SK_PEDAL_SUSTAIN_DOWN.  On the matching slots: LIFT_SOSTENUTO clears LATCHED; a slot then PENDING, not
 * LATCHED and not kept by SUSTAIN_DOWN is released on its voice_mask voices and loses PENDING.  d_result[3] (zeroed on `stream`
 * ahead of the kernel) += slots released, slots still pending, slots that did not match */
int sk_launch_pedal_up(const uint32_t *owner, uint32_t *pedal, uint32_t value, uint32_t mask, int first, int count, int slot_voices,
                       uint64_t voice_mask, uint32_t flags, sk_plane_t *const ro[SKP_COUNT], sk_plane_t *const rw[SKS_COUNT],
                       uint64_t now, uint64_t *mask_list, uint32_t *d_result, hipStream_t stream);

/* ---- portamento (skred_bank_glide.c -> skred_glide_kernels.hip; include/skred_amd.h: skred_bank_glide_owned / _glide_tags /
 * _glide_advance / _glide_stop) ----
 * glide[n_voices]: four words per voice (one 16-byte load) beside the owner array.  Only these launches read or write it; the words
 * they store into the planes are voice_phase_inc's (SKP_OSC word 0), finite products or a target's bits. */
enum { SK_GLIDE_TARGET = 0, SK_GLIDE_RATE_UP, SK_GLIDE_RATE_DOWN, SK_GLIDE_CARRY, SK_GLIDE_WORDS = 4 };
typedef struct {
  uint32_t w[SK_GLIDE_WORDS];
} sk_glide_t;
/* A per-entry record is skred_glide_t word for word (layout and bits checked at compile time in skred_bank_glide.c): 32 bytes, so
 * that set, rate_up, rate_down, scale are one aligned 16-byte load.  The bits equal SKRED_GLIDE_*. */
#define SK_GLIDE_FROM_SCALE (1u << 0)
#define SK_GLIDE_TO_SCALE   (1u << 1)
enum { SK_GLIDE_E_SET = 0, SK_GLIDE_E_RATE_UP, SK_GLIDE_E_RATE_DOWN, SK_GLIDE_E_SCALE, SK_GLIDE_E_WORDS = 8 };
typedef struct {
  uint32_t w[SK_GLIDE_E_WORDS];
} sk_glide_each_t;
/* The pitch wheel's two words per voice (below): the glide launches take the array too -- NULL on a bank without one, and then, as on
 * every voice whose key word is 0, they store the bytes they always stored */
enum { SK_BEND_KEY = 0, SK_BEND_RATIO, SK_BEND_WORDS = 2 };
typedef struct {
  uint32_t w[SK_BEND_WORDS];
} sk_bend_t;
/* glide[d_slots[k] + l] = 0, l < slot_voices, under sk_launch_owner_tag's list rule: launched behind it by a bank that has a glide
 * array */
int sk_launch_glide_clear(sk_glide_t *glide, const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices, int n_voices,
                          hipStream_t stream);
/* entry k starts d_each[k]'s glide (16-byte aligned) on the voice_mask voices of d_slots[k] where that is a slot whose owner is
 * d_tags[k]; d_result[3] (may be NULL; zeroed on `stream` ahead of the kernel) += voices set gliding, starts withheld, slots whose
 * owner differs.  bend != NULL: the BEND instantiation -- on a voice with a key the glide runs on the key, and the increment is
 * stored again as key * ratio */
int sk_launch_glide_start(sk_glide_t *glide, sk_bend_t *bend, const sk_glide_each_t *d_each, int slot_voices, uint64_t voice_mask,
                          const int32_t *d_slots, const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count,
                          int n_voices, sk_plane_t *osc, uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq,
                          hipStream_t stream);
/* the advance pass by num_frames over [first, first + count) (inside the bank); d_result[2] (may be NULL; zeroed on `stream` ahead
 * of the kernel) += voices still gliding, voices that arrived; bend as above */
int sk_launch_glide_advance(sk_glide_t *glide, sk_bend_t *bend, sk_plane_t *osc, int first, int count, int num_frames,
                            uint32_t *d_result, hipStream_t stream);
/* glide[first .. first + count) = 0; snap != 0: a gliding voice's increment (bend: its key) = its target first */
int sk_launch_glide_stop(sk_glide_t *glide, sk_bend_t *bend, sk_plane_t *osc, int first, int count, int snap, hipStream_t stream);

/* ---- pitch wheel (skred_bank_bend.c -> skred_bend_kernels.hip; include/skred_amd.h: skred_bank_bend_match / _bend_owned_each /
 * _bend_tags_each / _bend_clear) ----
 * bend[n_voices]: key, ratio per voice (one 8-byte load).  Only these launches and the glide launches read or write it; the words
 * they store into the planes are voice_phase_inc's (SKP_OSC word 0): finite non-zero products or a key's bits. */
/* bend[d_slots[k] + l] = 0, l < slot_voices, under sk_launch_owner_tag's list rule: launched behind it by a bank that has a bend
 * array */
int sk_launch_bend_clear(sk_bend_t *bend, const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices, int n_voices,
                         hipStream_t stream);
/* the absolute bend to `ratio` (fp32 bits) on the voice_mask voices of the slots of [first, first + count) whose owner matches;
 * d_result[3] (may be NULL; zeroed on `stream` ahead of the kernel) += voices stored or restored, bends withheld, slots of the range
 * that did not match */
int sk_launch_bend_match(sk_bend_t *bend, uint32_t ratio, int slot_voices, uint64_t voice_mask, int first, int count,
                         const uint32_t *owner, uint32_t value, uint32_t mask, sk_plane_t *osc, uint32_t *d_result, hipStream_t stream);
/* entry k bends the voice_mask voices of d_slots[k] to d_ratios[k] (fp32 bits) where that is a slot whose owner is d_tags[k];
 * d_result[3] as above, [2]: slots whose owner differs */
int sk_launch_bend_each(sk_bend_t *bend, const uint32_t *d_ratios, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                        const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count, int n_voices, sk_plane_t *osc,
                        uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);
/* bend[first .. first + count) = 0; snap != 0: a bent voice's increment = its key first */
int sk_launch_bend_range_clear(sk_bend_t *bend, sk_plane_t *osc, int first, int count, int snap, hipStream_t stream);

/* ---- filter cutoff on the device (skred_bank_cutoff.c -> skred_cutoff_kernels.hip; include/skred_amd.h: skred_bank_cutoff_match /
 * _cutoff_owned_each / _cutoff_tags_each / _cutoff_advance / _cutoff_stop) ----
 * cut[n_voices]: eight words per voice (two 16-byte loads) beside the bend array.  Only these launches read or write it; the words
 * they store into the planes are the five biquad coefficients (SKP_GAIN words 2, 3; SKP_FILT words 0 .. 2), finite by construction.
 * The constants equal SKRED_CUTOFF_* (checked at compile time in skred_bank_cutoff.c); skred_cutoff_common.hpp has the arithmetic. */
enum { SK_CUT_W = 0, SK_CUT_TARGET, SK_CUT_RATE_UP, SK_CUT_RATE_DOWN, SK_CUT_CARRY, SK_CUT_Q, SK_CUT_MODE, SK_CUT_RESERVED, SK_CUT_WORDS = 8 };
typedef struct {
  uint32_t w[SK_CUT_WORDS];
} sk_cut_t;
/* A record is skred_cutoff_t word for word: 32 bytes, set value q mode one aligned 16-byte load, the two rates the next 8 bytes */
#define SK_CUTOFF_ABS   (1u << 0)
#define SK_CUTOFF_TRACK (1u << 1)
#define SK_CUTOFF_GLIDE (1u << 2)
#define SK_CUTOFF_Q     (1u << 3)
#define SK_CUTOFF_MODE  (1u << 4)
#define SK_CUTOFF_ALL   ((1u << 5) - 1u)
enum { SK_CUT_E_SET = 0, SK_CUT_E_VALUE, SK_CUT_E_Q, SK_CUT_E_MODE, SK_CUT_E_RATE_UP, SK_CUT_E_RATE_DOWN, SK_CUT_E_WORDS = 8 };
typedef struct {
  uint32_t w[SK_CUT_E_WORDS];
} sk_cut_each_t;
#define SK_CUTOFF_W_MIN 0x1p-10f
#define SK_CUTOFF_W_MAX 3.0f
#define SK_CUTOFF_HALF_PI 0x1.921fb6p+0f
#define SK_CUTOFF_PI_HI 0x1.921fb6p+1f
#define SK_CUTOFF_PI_LO -0x1.777a5cp-24f
#define SK_CUTOFF_S1 -0x1.555548p-3f
#define SK_CUTOFF_S2 0x1.110e6ap-7f
#define SK_CUTOFF_S3 -0x1.9f5ff4p-13f
#define SK_CUTOFF_S4 0x1.5cf92cp-19f
#define SK_CUTOFF_C1 -0x1p-1f
#define SK_CUTOFF_C2 0x1.555548p-5f
#define SK_CUTOFF_C3 -0x1.6c138p-10f
#define SK_CUTOFF_C4 0x1.9f6f7ep-16f
#define SK_CUTOFF_C5 -0x1.18003p-22f
/* the planes the cutoff launches touch: SKP_OSC (read: voice_phase_inc), SKP_GAIN and SKP_FILT (the coefficient words) */
typedef struct {
  const sk_plane_t *osc;
  sk_plane_t *gain, *filt;
} sk_cut_planes_t;
/* The filter envelope's array (declared here: the cutoff launches take it; the section below has the rest).  fenv[n_voices]: eight
 * words per voice (two 16-byte loads) beside the cutoff array; stage 0: no envelope, and then all eight words are 0 */
enum { SK_FENV_STAGE = 0, SK_FENV_W_PEAK, SK_FENV_W_SUSTAIN, SK_FENV_W_END, SK_FENV_RATE_ATTACK, SK_FENV_RATE_DECAY, SK_FENV_RATE_RELEASE,
       SK_FENV_RESERVED, SK_FENV_WORDS = 8 };
enum { SK_FENV_OFF = 0, SK_FENV_ATTACK, SK_FENV_DECAY, SK_FENV_SUSTAIN, SK_FENV_RELEASE };
typedef struct {
  uint32_t w[SK_FENV_WORDS];
} sk_fenv_t;
/* cut[d_slots[k] + l] = 0 (both halves), l < slot_voices, under sk_launch_owner_tag's list rule: launched behind it by a bank that has
 * a cutoff array */
int sk_launch_cutoff_clear(sk_cut_t *cut, const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices, int n_voices,
                           hipStream_t stream);
/* the record on the filter_mask voices of the slots of [first, first + count) whose owner matches; bend: the pitch-wheel array or
 * NULL (TRACK reads a bent voice's key); fenv: the filter-envelope array or NULL (a voice set or started loses its contour: its
 * eight fenv words = 0).  d_result[4] (may be NULL; zeroed on `stream` ahead of the kernel) += voices set or started, records
 * withheld, slots of the range that did not match, cutoffs clamped */
int sk_launch_cutoff_match(sk_cut_t *cut, const sk_bend_t *bend, sk_fenv_t *fenv, const sk_cut_each_t *rec, int slot_voices,
                           uint64_t filter_mask, int first, int count, const uint32_t *owner, uint32_t value, uint32_t mask,
                           const sk_cut_planes_t *planes, uint32_t *d_result, hipStream_t stream);
/* entry k applies d_each[k] (16-byte aligned) on the filter_mask voices of d_slots[k] where that is a slot whose owner is d_tags[k];
 * fenv as above; d_result[4] as above, [2]: slots whose owner differs */
int sk_launch_cutoff_each(sk_cut_t *cut, const sk_bend_t *bend, sk_fenv_t *fenv, const sk_cut_each_t *d_each, int slot_voices,
                          uint64_t filter_mask, const int32_t *d_slots, const uint32_t *d_tags, const uint32_t *owner, int n,
                          const uint32_t *d_count, int n_voices, const sk_cut_planes_t *planes, uint32_t *d_result, uint32_t *cnt,
                          uint32_t *done, uint32_t seq, hipStream_t stream);
/* the advance pass by num_frames over [first, first + count) (inside the bank); d_result[2] (may be NULL; zeroed on `stream` ahead of
 * the kernel) += voices still moving, voices that arrived.  fenv == NULL: the plain instantiation, the kernel of a bank without a
 * filter-envelope array (env_s is not read); else the envelope instantiation, which steps the contours and reads sample_release
 * (env_s: SKP_ENV_S) of the voices that have one */
int sk_launch_cutoff_advance(sk_cut_t *cut, sk_fenv_t *fenv, const sk_plane_t *env_s, const sk_cut_planes_t *planes, int first, int count,
                             int num_frames, uint32_t *d_result, hipStream_t stream);
/* target, rates and carry of [first, first + count) = 0; snap != 0: a moving voice's w = its target and its coefficients first; fenv
 * (or NULL): the eight fenv words of every voice of the range that has a contour = 0 */
int sk_launch_cutoff_stop(sk_cut_t *cut, sk_fenv_t *fenv, const sk_cut_planes_t *planes, int first, int count, int snap, hipStream_t stream);

/* ---- filter envelope (skred_bank_fenv.c -> skred_fenv_kernels.hip; include/skred_amd.h: skred_bank_fenv_match / _fenv_owned_each /
 * _fenv_tags_each, and skred_bank_cutoff_advance on a bank that has the array) ----
 * Only the fenv launches and the cutoff launches above read or write fenv[]; the contour moves the voice's cutoff words and through
 * them the five coefficient words, with the cutoff section's arithmetic and nothing else (skred_fenv_common.hpp: sk_fenv_enter,
 * sk_fenv_advance). */
/* A record is skred_fenv_t word for word: 32 bytes, two aligned 16-byte loads */
#define SK_FENV_ABS   (1u << 0)
#define SK_FENV_REL   (1u << 1)
#define SK_FENV_START (1u << 2)
#define SK_FENV_ALL   ((1u << 3) - 1u)
enum { SK_FENV_E_SET = 0, SK_FENV_E_START, SK_FENV_E_PEAK, SK_FENV_E_SUSTAIN, SK_FENV_E_END, SK_FENV_E_RATE_ATTACK, SK_FENV_E_RATE_DECAY,
       SK_FENV_E_RATE_RELEASE, SK_FENV_E_WORDS = 8 };
typedef struct {
  uint32_t w[SK_FENV_E_WORDS];
} sk_fenv_each_t;
/* fenv[d_slots[k] + l] = 0 (both halves), l < slot_voices, under sk_launch_owner_tag's list rule: launched behind it by a bank that has
 * a filter-envelope array */
int sk_launch_fenv_clear(sk_fenv_t *fenv, const int32_t *d_slots, int n, const uint32_t *d_count, int slot_voices, int n_voices,
                         hipStream_t stream);
/* the record on the filter_mask voices of the slots of [first, first + count) whose owner matches.  d_result[4] (may be NULL; zeroed
 * on `stream` ahead of the kernel) += voices started, records withheld, slots of the range that did not match, voices clamped */
int sk_launch_fenv_match(sk_fenv_t *fenv, sk_cut_t *cut, const sk_fenv_each_t *rec, int slot_voices, uint64_t filter_mask, int first,
                         int count, const uint32_t *owner, uint32_t value, uint32_t mask, const sk_cut_planes_t *planes, uint32_t *d_result,
                         hipStream_t stream);
/* entry k applies d_each[k] (16-byte aligned) on the filter_mask voices of d_slots[k] where that is a slot whose owner is d_tags[k];
 * d_result[4] as above, [2]: slots whose owner differs */
int sk_launch_fenv_each(sk_fenv_t *fenv, sk_cut_t *cut, const sk_fenv_each_t *d_each, int slot_voices, uint64_t filter_mask,
                        const int32_t *d_slots, const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count, int n_voices,
                        const sk_cut_planes_t *planes, uint32_t *d_result, uint32_t *cnt, uint32_t *done, uint32_t seq, hipStream_t stream);

/* ---- pedals on the fixed-point bank (skred_fx_pedal.c -> skred_fx_pedal_kernels.hip; include/skred_amd_fxpt.h:
 * skred_fxbank_stamp_owned_pedal / _release_tags_pedal / _pedal_latch / _pedal_up) ----
 * The three launchers above at one voice per slot, on the fixed-point planes (time_plane: SKX_TIME, rw0: read-write plane 0, osc:
 * SKX_OSC); the bits are SK_PEDAL_*; each d_result is zeroed on `stream` ahead of its kernel.  The clear behind a tag launch is
 * sk_launch_pedal_clear itself, at slot_voices = 1. */
/* d_result[4] += voices stamped, voices whose owner differs, entries that are no voice, voices held back */
int skx_launch_pedal_stamps(const uint32_t *owner, uint32_t *pedal, const int32_t *d_voices, const uint32_t *d_tags, int n,
                            const uint32_t *d_count, int n_voices, int hold_all, skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now,
                            uint32_t *d_result, hipStream_t stream);
/* d_result[2] += voices that satisfy the latch rule, voices of the range that did not match */
int skx_launch_pedal_latch(const uint32_t *owner, uint32_t *pedal, uint32_t value, uint32_t mask, int first, int count,
                           const skx_plane_t *osc, skx_plane_t *time_plane, skx_plane_t *rw0, uint32_t *d_result, hipStream_t stream);
/* d_result[3] += voices released, voices still pending, voices of the range that did not match */
int skx_launch_pedal_up(const uint32_t *owner, uint32_t *pedal, uint32_t value, uint32_t mask, int first, int count, uint32_t flags,
                        skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now, uint32_t *d_result, hipStream_t stream);

/* stem recorder (skred_recorder.c): min/max partials of rec[n_floats]; selected voices -> int16 pairs */
int sk_rec_partial_floats(void);
int sk_launch_rec_minmax(const float *rec, size_t n_floats, float *partial, int *n_blocks_out, hipStream_t stream);
int sk_launch_rec_convert(const float *rec, long frames, int n_voices, const int *sel, int n_sel, float scale,
                          int16_t *out, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#ifdef __HIPCC__
/* an owner word w MATCHES (value, mask): somebody owns the slot, and the masked tag is the one asked for -- both banks' masked
 * matches (channels, pedals) */
__device__ __forceinline__ bool sk_owner_matches(uint32_t w, uint32_t value, uint32_t mask) { return w != 0u && (w & mask) == value; }
#endif
#endif
