/* skred_fx_layout.h -- device layout of a fixed-point voice bank (see skred_device_layout.h for the
 * float path; same idea: 16-byte planes, one coalesced dwordx4 per lane per plane). */
#ifndef SKRED_FX_LAYOUT_H
#define SKRED_FX_LAYOUT_H
#include <stdint.h>

enum {
  SKX_OSC = 0,  /* u32 phase_inc | i32 table_offset | u32 log2_size + (flags << 8) | i32 amp_q15 */
  SKX_GAIN,     /* i32 pan_left_q15 | i32 pan_right_q15 | i32 smoother_k_q15 | i32 velocity_q15   */
  SKX_ENV,      /* u32 attack_frames | u32 decay_frames | u32 release_frames | i32 sustain_q15    */
  SKX_RECIP,    /* u32 floor(2^32/attack) | floor(2^32/decay) | floor(2^32/release) | 0           */
  SKX_TIME,     /* u32 sample_start lo,hi | u32 sample_release lo,hi                               */
  SKX_FILT,     /* i32 b0 | b1 | b2 | a1   (Q2.30)                                                 */
  SKX_FILT2,    /* i32 a2 (Q2.30) | 0 | 0 | 0                                                       */
  SKX_COUNT
};
/* read-write planes: [0] u32 phase | i32 smoother_gain_q15 | i32 voice_sample | u32 bit 0 is_active, bit 1 finished
 *                    [1] i32 x1 | x2 | y1 | y2   (biquad delay line, Q12 sample units) */
#define SKX_RW_COUNT 2

#define SKXF_USE_ENV (1u << 0)
#define SKXF_SMOOTH  (1u << 1)
#define SKXF_MUTED   (1u << 2)
#define SKXF_INERT   (1u << 3)
#define SKXF_FILTER  (1u << 4)
#define SKXF_ONE_SHOT (1u << 5)

#define SKX_GROUP 256
#define SKX_CHUNK 64
#define SKX_LDS_TABLE_MAX_BYTES 49152
#define SKX_MAX_WORKGROUPS 2048

typedef struct { uint32_t w[4]; } skx_plane_t;

typedef struct {
  const skx_plane_t *ro[SKX_COUNT];
  skx_plane_t *rw[SKX_RW_COUNT];
  const int16_t *tables;
  long long *partial;     /* [n_workgroups][num_frames][2] */
  int32_t *stems;         /* [num_frames][n_voices][2] or NULL */
  uint64_t count0;
  int32_t n_voices, n_groups, num_frames, interp;
  int32_t lds_bytes_tables;   /* bytes of the pool staged in LDS (multiple of 16), 0 = gather from L2/HBM */
  int32_t any_filter;         /* some voice of the bank runs the biquad (selects the block instantiation) */
  /* ---- the block's mix-down and master stage inside the render kernel (the float path's scheme, skred_kernel_common.hpp:
   * sk_finish_block, on int64 rows: every workgroup publishes its row write-through, the last arriver of a slab adds the slab,
   * the last slab adds the slabs -- integer sums, any order is exact -- and applies the master gain of each frame, which
   * workgroup 0 of the grid walked meanwhile) ---- */
  int32_t n_rows;             /* rendering workgroups; the grid has one more (blockIdx 0: the gain workgroup) */
  long long *slab_rows;       /* [SKX_FINISH_SLABS][num_frames][2] */
  uint32_t *tickets;          /* [SKX_FINISH_SLABS + 1], zero between launches */
  long long *sum_out;         /* [num_frames][2] pre-master sum (the operand of the multi-GPU reduce), or NULL */
  long long *mix_out;         /* [num_frames][2] post-master output, or NULL */
  int32_t *gains;             /* [num_frames] Q15 master gain per frame */
  long long *gain_state;      /* [0] Q31 gain carried between blocks (read) */
  long long *gain_commit;     /* where the gain after the last frame goes ([0] when this launch applies the stage; [1]: pending for skred_fxbank_master) */
  long long master_target_q31;
  int32_t master_k_q15;
} skx_args_t;

#define SKX_FINISH_SLABS 32
#define SKX_FINISH_FLAT_MAX 64

/* ---- live control (skred_fx_live_kernels.hip; include/skred_amd_fxpt.h: skred_fxbank_update / _find_idle / _notes_on_list) ---- */

/* bits of word 3 of read-write plane 0 */
#define SKXR_ACTIVE   1u
#define SKXR_FINISHED 2u

/* one record of an update batch: the voice as skred_fxbank_upload would pack it; `dirty` (SKRED_DIRTY_* / SKRED_STAMP_*) says
 * which of its words travel */
typedef struct __attribute__((aligned(16))) {
  int32_t voice;
  uint32_t dirty;
  uint32_t pad[2];
  skx_plane_t ro[SKX_COUNT];
  skx_plane_t rw[SKX_RW_COUNT];
} skx_update_t;                    /* 160 bytes */

/* the device's image of skred_fx_note_t, word for word */
enum { SKX_NOTE_PHASE_INC = 0, SKX_NOTE_VELOCITY, SKX_NOTE_PHASE, SKX_NOTE_PAN_LEFT, SKX_NOTE_PAN_RIGHT, SKX_NOTE_FLAGS, SKX_NOTE_WORDS = 8 };
typedef struct { uint32_t w[SKX_NOTE_WORDS]; } skx_note_t;
#define SKX_NOTE_SPAN 256          /* notes (and threads) per workgroup of sk_fx_notes_kernel */

#define SKX_IDLE_SPAN 256          /* voices (and threads) per workgroup of the two query kernels; spans are aligned to 64 voices */
/* the bank's query scratch: SKX_IDLE_W_COUNT words, then the workgroups' counts, then their exclusive offsets */
enum { SKX_IDLE_W_TICKET = 0,      /* arrival ticket of the count kernel, re-armed by its last arriver */
       SKX_IDLE_W_PART,            /* idle voices below `from` inside from's own workgroup */
       SKX_IDLE_W_RANK,            /* idle voices of the range below `from` */
       SKX_IDLE_W_TOTAL,           /* idle voices of the range */
       SKX_IDLE_W_COUNT };
typedef struct {
  const skx_plane_t *osc;          /* SKX_OSC: flags (ENV_DONE), amp_q15 (AMP_ZERO) */
  const skx_plane_t *rw0;          /* smoother gain (ENV_DONE), is_active / finished (ENV_DONE, FINISHED) */
  uint32_t *words, *counts, *offsets;
  int32_t *d_voices;
  uint32_t *d_count;
  int32_t first, end, from, max_out;
  uint32_t which;                  /* SKRED_IDLE_FINISHED | _ENV_DONE | _AMP_ZERO */
  int32_t settle_q15;
  int32_t base, from_wg;           /* filled in by the launcher: `first` rounded down to 64; the workgroup that holds `from` */
} skx_idle_args_t;

/* ---- controllers (skred_fx_ctl_kernels.hip; include/skred_amd_fxpt.h: skred_fxbank_ctl_range / _ctl_list / _ctl_owned) ----
 * the device's image of skred_fx_ctl_t, word for word; the three reserved words carry the reciprocals of the frame counts */
enum { SKX_CTL_WHICH = 0, SKX_CTL_PHASE_INC, SKX_CTL_INC_SCALE, SKX_CTL_AMP, SKX_CTL_PAN_LEFT, SKX_CTL_PAN_RIGHT,
       SKX_CTL_B0, SKX_CTL_B1, SKX_CTL_B2, SKX_CTL_A1, SKX_CTL_A2, SKX_CTL_ATTACK, SKX_CTL_DECAY, SKX_CTL_RELEASE,
       SKX_CTL_SUSTAIN, SKX_CTL_VELOCITY, SKX_CTL_SMOOTHING, SKX_CTL_RECIP_A, SKX_CTL_RECIP_D, SKX_CTL_RECIP_R, SKX_CTL_WORDS };
typedef struct { uint32_t w[SKX_CTL_WORDS]; } skx_ctl_t;     /* 80 bytes */
#define SKX_CTL_SPAN 256           /* voices or entries (and threads) per workgroup of the controller and guarded-stamp kernels */

/* ---- channels and per-note expression (skred_fx_expr_kernels.hip; include/skred_amd_fxpt.h: skred_fxbank_find_match / _stamp_match /
 * _ctl_match / _ctl_owned_each / _ctl_tags_each) ----
 * the device's image of skred_fx_ctl_each_t, word for word; the bits equal SKRED_EACH_* (checked in skred_fx_expr.c).  Values an
 * entry does not name arrive zeroed */
#define SKX_EACH_INC_SCALE (1u << 0)
#define SKX_EACH_AMP_SCALE (1u << 1)
#define SKX_EACH_VELOCITY  (1u << 2)
#define SKX_EACH_PAN       (1u << 3)
#define SKX_EACH_ALL       ((1u << 4) - 1u)
enum { SKX_EACH_SET = 0, SKX_EACH_W_INC_SCALE, SKX_EACH_W_AMP_SCALE, SKX_EACH_W_VELOCITY, SKX_EACH_W_PAN_LEFT, SKX_EACH_W_PAN_RIGHT,
       SKX_EACH_WORDS = 8 };
typedef struct { uint32_t w[SKX_EACH_WORDS]; } skx_each_t;   /* 32 bytes */
/* a per-entry filter record is skred_fx_filter_each_t word for word (checked at compile time in skred_fx_expr.c): 32 bytes, so that
 * b0 b1 b2 a1 are one aligned 16-byte load */
enum { SKX_FILT_W_B0 = 0, SKX_FILT_W_B1, SKX_FILT_W_B2, SKX_FILT_W_A1, SKX_FILT_W_A2, SKX_FILT_WORDS = 8 };
typedef struct { uint32_t w[SKX_FILT_WORDS]; } skx_filt_each_t;   /* 32 bytes */
#define SKX_EXPR_SPAN 256          /* voices or entries (and threads) per workgroup of the expression kernels */

/* ---- portamento (skred_fx_glide_kernels.hip; include/skred_amd_fxpt.h: skred_fxbank_glide_owned / _glide_tags / _glide_advance /
 * _glide_stop) ----
 * glide[n_voices]: four words per voice (one 16-byte load) beside the owner array, target == 0 "not gliding".  The float bank's
 * sk_glide_t has the same shape (checked in skred_fx_glide.c): its clear kernel serves this array too */
enum { SKX_GLIDE_TARGET = 0, SKX_GLIDE_UP, SKX_GLIDE_DOWN, SKX_GLIDE_CARRY, SKX_GLIDE_WORDS = 4 };
typedef struct { uint32_t w[SKX_GLIDE_WORDS]; } skx_glide_t;   /* 16 bytes */
/* a per-entry record is skred_fx_glide_t word for word (layout and bits checked at compile time in skred_fx_glide.c): 32 bytes, so that
 * set, up_q32, down_q32, scale_q16 are one aligned 16-byte load.  The bits equal SKRED_FX_GLIDE_* */
#define SKX_GLIDE_FROM_SCALE (1u << 0)
#define SKX_GLIDE_TO_SCALE   (1u << 1)
#define SKX_GLIDE_TO_INC     (1u << 2)
enum { SKX_GLIDE_E_SET = 0, SKX_GLIDE_E_UP, SKX_GLIDE_E_DOWN, SKX_GLIDE_E_SCALE, SKX_GLIDE_E_TARGET_INC, SKX_GLIDE_E_WORDS = 8 };
typedef struct { uint32_t w[SKX_GLIDE_E_WORDS]; } skx_glide_each_t;   /* 32 bytes */

/* ---- pitch wheel (skred_fx_bend_kernels.hip; include/skred_amd_fxpt.h: skred_fxbank_bend_match / _bend_owned_each / _bend_tags_each /
 * _bend_clear) ----
 * bend[n_voices]: two words per voice (one 8-byte load) beside the glide array: key (the unbent phase_inc; 0 "not bent") and ratio_q24.
 * The float bank's sk_bend_t has the same shape (checked in skred_fx_bend.c): its clear kernel serves this array too.  The glide
 * launches take the array as well -- NULL on a bank without one */
enum { SKX_BEND_KEY = 0, SKX_BEND_RATIO, SKX_BEND_WORDS = 2 };
typedef struct { uint32_t w[SKX_BEND_WORDS]; } skx_bend_t;     /* 8 bytes */
#define SKX_BEND_ONE (1u << 24)    /* the wheel at centre (equals SKRED_FX_BEND_ONE: checked in skred_fx_bend.c) */

/* ---- filter cutoff (skred_fx_cutoff_kernels.hip; include/skred_amd_fxpt.h: skred_fxbank_cutoff_match / _cutoff_owned_each /
 * _cutoff_tags_each / _cutoff_advance / _cutoff_stop) ----
 * cut[n_voices]: eight words per voice (two 16-byte loads) beside the bend array: w_q29 (0 "no device cutoff"), target_q29 (0 "not
 * moving"), up_q32, down_q32 | carry (0 .. 63), q_q16, mode, 0.  The float bank's sk_cut_t has the same shape (checked in
 * skred_fx_cutoff.c): its clear kernel serves this array too */
enum { SKX_CUT_W = 0, SKX_CUT_TARGET, SKX_CUT_UP, SKX_CUT_DOWN, SKX_CUT_CARRY, SKX_CUT_Q, SKX_CUT_MODE, SKX_CUT_RESERVED, SKX_CUT_WORDS = 8 };
typedef struct { uint32_t w[SKX_CUT_WORDS]; } skx_cut_t;   /* 32 bytes */
/* a record is skred_fx_cutoff_t word for word (layout and bits checked at compile time in skred_fx_cutoff.c): 32 bytes, so that set,
 * value, q_q16, mode are one aligned 16-byte load.  The bits equal SKRED_FX_CUTOFF_* */
#define SKX_CUTOFF_ABS   (1u << 0)
#define SKX_CUTOFF_TRACK (1u << 1)
#define SKX_CUTOFF_GLIDE (1u << 2)
#define SKX_CUTOFF_Q     (1u << 3)
#define SKX_CUTOFF_MODE  (1u << 4)
#define SKX_CUTOFF_ALL   ((1u << 5) - 1u)
enum { SKX_CUT_E_SET = 0, SKX_CUT_E_VALUE, SKX_CUT_E_Q, SKX_CUT_E_MODE, SKX_CUT_E_UP, SKX_CUT_E_DOWN, SKX_CUT_E_WORDS = 8 };
typedef struct { uint32_t w[SKX_CUT_E_WORDS]; } skx_cut_each_t;   /* 32 bytes */
/* THE ARITHMETIC's constants (equal to SKRED_FX_CUTOFF_*: checked in skred_fx_cutoff.c) */
#define SKX_CUTOFF_W_MIN (1u << 19)
#define SKX_CUTOFF_W_MAX (3u << 29)
#define SKX_CUTOFF_PI_Q29 1686629713u
#define SKX_CUTOFF_HALF_PI_Q29 843314857u
#define SKX_CUTOFF_S1 (-1431655761ll)
#define SKX_CUTOFF_S2 286331072ll
#define SKX_CUTOFF_S3 (-27269072ll)
#define SKX_CUTOFF_S4 1513217ll
#define SKX_CUTOFF_S5 (-52533ll)
#define SKX_CUTOFF_C2 1431655759ll
#define SKX_CUTOFF_C3 (-190887371ll)
#define SKX_CUTOFF_C4 13634516ll
#define SKX_CUTOFF_C5 (-605274ll)
#define SKX_CUTOFF_C6 17511ll

/* ---- filter envelope (skred_fx_fenv_kernels.hip, and the ENV instantiation of sk_fx_cutoff_advance_kernel; include/skred_amd_fxpt.h:
 * skred_fxbank_fenv_match / _fenv_owned_each / _fenv_tags_each / _download_fenv) ----
 * fenv[n_voices]: eight words per voice (two 16-byte loads) beside the cutoff array: stage, w_peak, w_sustain, w_end (w_q29 values in
 * the box) | rate_attack_q32, rate_decay_q32, rate_release_q32, 0.  stage 0: no contour, and all eight words are 0.  The float bank's
 * sk_fenv_t has the same shape (checked in skred_fx_fenv.c): its clear kernel serves this array too */
enum { SKX_FENV_STAGE = 0, SKX_FENV_W_PEAK, SKX_FENV_W_SUSTAIN, SKX_FENV_W_END, SKX_FENV_RATE_ATTACK, SKX_FENV_RATE_DECAY, SKX_FENV_RATE_RELEASE,
       SKX_FENV_RESERVED, SKX_FENV_WORDS = 8 };
enum { SKX_FENV_OFF = 0, SKX_FENV_ATTACK, SKX_FENV_DECAY, SKX_FENV_SUSTAIN, SKX_FENV_RELEASE };
typedef struct { uint32_t w[SKX_FENV_WORDS]; } skx_fenv_t;   /* 32 bytes */
/* a record is skred_fx_fenv_t word for word (layout and bits checked at compile time in skred_fx_fenv.c): 32 bytes, two aligned 16-byte
 * loads.  The bits equal SKRED_FX_FENV_* */
#define SKX_FENV_ABS   (1u << 0)
#define SKX_FENV_REL   (1u << 1)
#define SKX_FENV_START (1u << 2)
#define SKX_FENV_ALL   ((1u << 3) - 1u)
enum { SKX_FENV_E_SET = 0, SKX_FENV_E_START, SKX_FENV_E_PEAK, SKX_FENV_E_SUSTAIN, SKX_FENV_E_END, SKX_FENV_E_RATE_ATTACK, SKX_FENV_E_RATE_DECAY,
       SKX_FENV_E_RATE_RELEASE, SKX_FENV_E_WORDS = 8 };
typedef struct { uint32_t w[SKX_FENV_E_WORDS]; } skx_fenv_each_t;   /* 32 bytes */
#endif
