/*
 * include/skred_amd.h -- C ABI of the MI355X-native skred render path.
 *
 * One hot path is implemented: the per-voice render loop of skred's audio
 * callback, `synth()` (reference synth.c:502-630, declared synth.h:8, called
 * only from the miniaudio data_callback `synth_callback`, skred.c:107-116).
 *
 * Two boundaries are exported by libskred_amd.so:
 *
 *  (1) BANK MODE (this header): a runtime-N "voice bank" whose per-voice fields
 *      carry the reference's own names and types (synth.def:12-89; structs
 *      synth-types.h:13-38) but with N voices instead of VOICE_MAX=64
 *      (skred.h:9).  State lives in HBM between calls; every call renders
 *      `num_frames` frames for all voices with hand-written HIP kernels.
 *
 *  (2) DROP-IN MODE (include/skred_synth_abi.h): the literal synth.h surface
 *      -- `synth()`, the setters and the 75 global arrays -- backed by (1).
 *
 * Plain pointers and sizes only: no C++ or torch types cross this boundary.
 * All functions return 0 on success or a negative SKRED_E_* code; the product
 * path has NO CPU fallback: without a usable HIP device every entry point that
 * would touch the GPU fails with SKRED_E_NO_DEVICE.
 */
#ifndef SKRED_AMD_H
#define SKRED_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKRED_AMD_ABI_VERSION 1

/* ---- error codes ------------------------------------------------------- */
enum {
  SKRED_OK = 0,
  SKRED_E_NO_DEVICE = -1,   /* no HIP device / HIP call failed (see skred_amd_last_error) */
  SKRED_E_BAD_ARG = -2,
  SKRED_E_NO_MEM = -3,
  SKRED_E_RANGE = -4,       /* voice window or table offset outside the bank / pool */
  SKRED_E_UNSUPPORTED = -5, /* feature of synth() not implemented by the kernels (see flags) */
  SKRED_E_IO = -6,          /* file cannot be opened / written (skred_wav.h) */
};

/* ---- structs kept from the reference (layout-identical) ---------------- */

/* == mmf_t, synth-types.h:13-23 (48 bytes): RBJ biquad state + coefficients */
typedef struct {
  float x1, x2;             /* input delay line  */
  float y1, y2;             /* output delay line */
  float b0, b1, b2;         /* feed-forward      */
  float a1, a2;             /* feedback          */
  float last_freq, last_resonance;
  int32_t last_mode;
} skred_mmf_t;

/* == envelope_t, synth-types.h:25-38 (56 bytes): linear ADSR keyed on the global sample counter */
typedef struct {
  float a, d, s, r;         /* seconds (control path only) */
  float attack_time;        /* samples */
  float decay_time;         /* samples */
  float sustain_level;      /* 0..1    */
  float release_time;       /* samples */
  uint64_t sample_start;    /* synth_sample_count at note-on  */
  uint64_t sample_release;  /* synth_sample_count at note-off, 0 = held */
  int32_t is_active;
  float velocity;
} skred_envelope_t;

/* ---- the voice bank (host view) --------------------------------------- */

/*
 * Host-side structure-of-arrays view of N voices.  Every member is the array
 * of the same name in synth.def:12-89 with `VOICE_MAX` replaced by
 * `n_voices`; the one exception is `voice_table`, a raw `float*` in the
 * reference (synth.def:14), which becomes `voice_table_offset`: the index of
 * the table's first sample inside the table pool handed to
 * skred_bank_set_tables_f32().
 *
 * Only the fields synth() reads or writes are present.
 * A bank view may simply point at the 64-entry global arrays of the drop-in
 * facade -- that is how drop-in mode is implemented.
 */
typedef struct skred_voice_bank {
  int32_t n_voices;

  /* oscillator (osc_next, synth.c:217-275) */
  float   *voice_phase;            /* rw */
  float   *voice_phase_inc;
  int64_t *voice_table_offset;     /* replaces float *voice_table[] */
  int32_t *voice_table_size;
  int32_t *voice_one_shot;
  int32_t *voice_finished;         /* rw */
  int32_t *voice_loop_enabled;
  int32_t *voice_loop_valid;
  float   *voice_loop_start_f;
  float   *voice_loop_end_f;
  int32_t *voice_direction;
  int32_t *voice_wave_table_index; /* only compared with WAVE_TABLE_NOISE_ALT (synth.c:543) */

  /* sample chain (synth.c:560-593) */
  float   *voice_sample;           /* rw */
  float   *voice_sample_hold;      /* rw */
  int32_t *voice_sample_hold_count;/* rw */
  int32_t *voice_sample_hold_max;
  int32_t *voice_quantize;
  float   *voice_amp;
  int32_t *voice_use_amp_envelope;
  int32_t *voice_smoother_enable;
  float   *voice_smoother_gain;    /* rw */
  float   *voice_smoother_smoothing;
  int32_t *voice_filter_mode;
  skred_mmf_t      *voice_filter;        /* rw: x1 x2 y1 y2 */
  skred_envelope_t *voice_amp_envelope;  /* rw: is_active   */

  /* pan / mix (synth.c:595-612) */
  float   *voice_pan_left;         /* rw only under pan modulation */
  float   *voice_pan_right;
  int32_t *voice_disconnect;

  /* cross-voice modulation + phase distortion (synth.c:548-558,584-587,597-602,262-267) */
  int32_t *voice_freq_mod_osc;
  float   *voice_freq_mod_depth;
  float   *voice_freq_scale;
  int32_t *voice_amp_mod_osc;
  float   *voice_amp_mod_depth;
  int32_t *voice_pan_mod_osc;
  float   *voice_pan_mod_depth;
  int32_t *voice_cz_mod_osc;
  float   *voice_cz_mod_depth;
  int32_t *voice_cz_mode;
  float   *voice_cz_distortion;
} skred_voice_bank_t;

/* Scalars synth() keeps outside the per-voice arrays. */
typedef struct skred_globals {
  uint64_t synth_sample_count;       /* synth.c:85; pre-incremented per frame (synth.c:521) */
  uint64_t noise_rng;                /* synth()'s static LCG state (synth.c:504,508,525)  */
  float volume_final;                /* synth.c:90  = volume_user * AMY_FACTOR            */
  float volume_smoother_gain;        /* synth.c:91  rw                                     */
  float volume_smoother_smoothing;   /* synth.c:92                                         */
  float reserved;
} skred_globals_t;

#define SKRED_WAVE_TABLE_NOISE_ALT 6 /* skred.h:30 */

/* render flags */
enum {
  SKRED_INTERP_TRUNCATE = 0, /* table[(int)phase] -- what the reference does (synth.c:268-274) */
  SKRED_INTERP_LINEAR   = 1, /* north-star mode; defined by oracle/cpu_ref.c, not by the reference */
};

/* ---- device-side bank -------------------------------------------------- */

typedef struct skred_bank skred_bank_t; /* opaque; owns HBM state for n voices on one GPU */

int  skred_amd_abi_version(void);
int  skred_amd_device_count(void);                 /* <=0: no usable GPU */
const char *skred_amd_last_error(void);            /* thread-local text of the last failure */

/* The largest bank a GPU holds: voice and list indices inside the kernels are 32-bit (a bank of this size takes 3.2 GB of
 * HBM); skred_bank_create() refuses more with SKRED_E_RANGE before it touches the device. */
#define SKRED_MAX_VOICES (1 << 24)
int  skred_bank_create(int device, int n_voices, skred_bank_t **out);
void skred_bank_destroy(skred_bank_t *bank);
int  skred_bank_n_voices(const skred_bank_t *bank);

/* Table pool: every table a voice can name, concatenated (floats).  Replaces the
 * malloc'd wave_table_data[] tables (synth.def:1, synth.c:1224).  Tables that fit
 * are staged into LDS by the kernel; larger pools are gathered from HBM/L2. */
/* Guard samples (optional, linear interpolation only): when a table is followed in the pool by one more float equal to its
 * first sample, a voice that loops over the whole table (no loop window) finds the second tap of the linear lookup in the next
 * float at every index; a bank in which every voice does runs the lookup without the fold test at the loop end (same samples,
 * ~1.3x the throughput on LUT banks).  Pools without guards render the same, through the general form. */
int  skred_bank_set_tables_f32(skred_bank_t *bank, const float *pool, size_t n_floats);

/* Pack `count` voices starting at host index `src_first` into device slots
 * [dst_first, dst_first+count).  Host arrays stay the source of truth.
 * Synchronous: waits for all work queued on the device (renders on any stream) before the planes are overwritten;
 * so do skred_bank_set_globals, skred_bank_get_globals and skred_bank_download. */
int  skred_bank_upload(skred_bank_t *bank, const skred_voice_bank_t *host,
                       int src_first, int dst_first, int count);
/* Copy the read-write fields (marked rw above) back into the host view. */
int  skred_bank_download(skred_bank_t *bank, skred_voice_bank_t *host,
                         int src_first, int dst_first, int count);

int  skred_bank_set_globals(skred_bank_t *bank, const skred_globals_t *g);
int  skred_bank_get_globals(skred_bank_t *bank, skred_globals_t *g);

/*
 * Render `num_frames` frames of every voice (the two nested loops of
 * synth.c:520-613) and leave this GPU's PRE-master-volume stereo sum in
 * `d_partial` (device pointer, float[num_frames][2]): one kernel launch (plus,
 * while notes ramp on the two-voices-per-lane path, the envelope kernel beside it on
 * a stream of the bank's own, joined back into `stream` before the call returns).  `d_stems` (device,
 * float[num_frames][n_voices][2], the `user` buffer layout of synth.c:533-534,
 * 607-611) may be NULL.  Advances synth_sample_count and the noise LCG.
 * `stream` is a hipStream_t (NULL = default stream).  Asynchronous.
 */
int  skred_bank_render(skred_bank_t *bank, int num_frames, int interp,
                       float *d_partial, float *d_stems, void *stream);

/*
 * Master volume stage (synth.c:616-624): serial one-pole smoothing of the
 * gain, multiply, and interleave into `d_out` (device, float[num_frames]
 * [num_channels], channels 0 and 1 written).  In a multi-GPU run this is
 * called on the root after the RCCL sum of the partials.  Asynchronous.
 */
int  skred_bank_master(skred_bank_t *bank, const float *d_sum, int num_frames,
                       int num_channels, float *d_out, void *stream);

/* Single-GPU form of render + master in ONE launch: the render kernel's last-arriving workgroups add the
 * per-workgroup rows up and apply the master gain (same samples as skred_bank_render + skred_bank_master:
 * both forms add the rows in the same fixed order).  `d_out` as for skred_bank_master.  Asynchronous. */
int  skred_bank_render_mix(skred_bank_t *bank, int num_frames, int interp, float *d_out, int num_channels,
                           float *d_stems_or_null, void *stream);

/* Whole synth() contract on host buffers: render + master + D2H (+ stems). Synchronous. */
int  skred_bank_render_host(skred_bank_t *bank, float *buffer, int num_frames,
                            int num_channels, int interp, float *stems_or_null);

/* ---- block-granular updates of device-resident voices (SURVEY 8f "next" #4) -------------------------
 *
 * The reference's control path (wire.c:606-716 commands, seq.c pattern steps, deferred items) stores into the
 * per-voice arrays and the next audio block sees the change.  With the voices in HBM the host view
 * (skred_voice_bank_t, same array names) stays what control code writes to; afterwards it names the voices it
 * touched and which KIND of field, and only those travel.  Everything not named keeps the value the GPU last
 * computed -- a full skred_bank_upload() would overwrite the running phase, filter memory and smoother with
 * the host's stale copies.
 */
enum {
  SKRED_DIRTY_PARAMS        = 1u << 0, /* every parameter: phase_inc, amp, table / loop window, direction, flags, quantize,
                                          hold_max, envelope times + velocity, filter coefficients, smoother k,
                                          modulation routing and depths, cz mode -- but not the envelope clock */
  SKRED_DIRTY_PHASE         = 1u << 1, /* voice_phase, voice_finished                    (osc_trigger, synth.c:316-339) */
  SKRED_DIRTY_ENV_STATE     = 1u << 2, /* voice_amp_envelope.is_active */
  SKRED_DIRTY_PAN           = 1u << 3, /* voice_pan_left, voice_pan_right                (pan_set, synth.c:838-847) */
  SKRED_DIRTY_FILTER_STATE  = 1u << 4, /* voice_filter.x1 x2 y1 y2                       (mmf_init, synth.c:1015-1030) */
  SKRED_DIRTY_SMOOTHER      = 1u << 5, /* voice_smoother_gain */
  SKRED_DIRTY_HOLD          = 1u << 6, /* voice_sample_hold, voice_sample_hold_count */
  SKRED_DIRTY_SAMPLE        = 1u << 7, /* voice_sample */
  /* the two control actions whose stores depend on WHEN they run: the library stamps the bank's
   * synth_sample_count at application time, as the reference's functions read the global */
  SKRED_STAMP_TRIGGER       = 1u << 8, /* amp_envelope_trigger (synth.c:383-388): sample_start = now, sample_release = 0,
                                          is_active = 1; send the velocity with SKRED_DIRTY_PARAMS */
  SKRED_STAMP_RELEASE       = 1u << 9, /* amp_envelope_release (synth.c:391-395): if is_active (device state), sample_release = now */
  SKRED_DIRTY_ENV_CLOCK     = 1u << 10, /* voice_amp_envelope.sample_start / .sample_release as the host has them (kept out
                                           of PARAMS so that a later parameter change cannot undo a stamped note-on / -off) */
  SKRED_DIRTY_VALID_MASK    = 0x7FF
};
#define SKRED_QUEUE_SIZE 1024          /* skred.h:86 QUEUE_SIZE */

/* Rewrite the `dirty` parts of the listed voices (indices into both the host view and the bank) from the host
 * view, on `stream` (a hipStream_t; pass the render stream: the update is ordered before the next render on it).
 * A voice may be listed more than once; the copies are applied in order. */
int  skred_bank_update(skred_bank_t *bank, const skred_voice_bank_t *host, const int32_t *voices, int n_voices,
                       uint32_t dirty, void *stream);

/* The deferred queue: seq.c:243-257 queue_item(when, what, voice) + the first loop of seq() (seq.c:170-177).
 * The reference stores command TEXT and runs it when due; here the values are captured from the host view when
 * the item is queued (only the STAMP actions read the clock when they run).  skred_bank_run_queue() is what
 * seq() does after synth(): every item with when <= synth_sample_count + frame_count is applied, in arrival
 * order, i.e. an item takes effect at the start of the block that contains its time.  Returns the number of
 * items applied (>= 0) or a SKRED_E_* code. */
int  skred_bank_defer(skred_bank_t *bank, uint64_t when, const skred_voice_bank_t *host, const int32_t *voices,
                      int n_voices, uint32_t dirty);
int  skred_bank_run_queue(skred_bank_t *bank, int frame_count, void *stream);
int  skred_bank_queue_pending(const skred_bank_t *bank);

/* ---- the pattern step clock: the other half of seq() (seq.c:179-213) ---------------------------------------------
 *
 * skred_seq_t is the reference's sequencer state on the host, with the same arithmetic: a double clock that gains
 * (float)frame_count / (float)rate per call and fires when it reaches tempo_time_per_step (tempo_set: 1 / (bpm / 60) / 4
 * seconds, four steps per beat; 60 s until a tempo is set), one step per call at most; per RUNNING pattern the modulo
 * (default 4) divides the step rate, a muted step advances silently, the pointer wraps at the first empty step.  No
 * device is involved: tests hold it against the compiled reference call by call.
 * A bank owns one (skred_bank_seq); a step of a bank's pattern is a batch of voice updates captured when it is written,
 * and skred_bank_run_queue() -- called once per block after the render, like seq() at skred.c:119 -- applies the
 * deferred items that are due and then the steps the clock fires, in pattern order, on `stream`. */
#define SKRED_PATTERNS_MAX 16          /* skred.h:75 */
#define SKRED_SEQ_STEPS_MAX 256        /* skred.h:76 */
enum { SKRED_SEQ_STOPPED = 0, SKRED_SEQ_RUNNING = 1, SKRED_SEQ_PAUSED = 2 };   /* skred.h:80-82 */
typedef struct skred_seq skred_seq_t;
int   skred_seq_create(skred_seq_t **out);
void  skred_seq_destroy(skred_seq_t *seq);
int   skred_seq_tempo_set(skred_seq_t *seq, float bpm);                       /* tempo_set, seq.c:21-28 */
float skred_seq_time_per_step(const skred_seq_t *seq);
int   skred_seq_step_set(skred_seq_t *seq, int pattern, int step, int occupied);   /* seq_step_set: empty text = not occupied */
int   skred_seq_mute_set(skred_seq_t *seq, int pattern, int step, int mute);  /* seq_mute_set */
int   skred_seq_modulo_set(skred_seq_t *seq, int pattern, int modulo);        /* seq_modulo_set */
int   skred_seq_state_set(skred_seq_t *seq, int pattern, int state);          /* seq_state_set: 0 stop, 1 start, 2 pause, 3 resume */
int   skred_seq_pattern_reset(skred_seq_t *seq, int pattern);                 /* pattern_reset */
int   skred_seq_pointer(const skred_seq_t *seq, int pattern);
int   skred_seq_counter(const skred_seq_t *seq, int pattern);
/* one call per block: fired[] receives (pattern << 16) | step of every step whose text the reference would run */
int   skred_seq_tick(skred_seq_t *seq, int frame_count, float sample_rate, int32_t *fired, int max_fired);

skred_seq_t *skred_bank_seq(skred_bank_t *bank);                    /* the bank's own clock (tempo, mute, modulo, state through skred_seq_*) */
int  skred_bank_set_sample_rate(skred_bank_t *bank, float rate);   /* the rate the clock counts blocks in; default 44100 (MAIN_SAMPLE_RATE, skred.h:6) */
int  skred_bank_pattern_step_set(skred_bank_t *bank, int pattern, int step, const skred_voice_bank_t *host,
                                 const int32_t *voices, int n_voices, uint32_t dirty);   /* n_voices == 0: a rest */
int  skred_bank_pattern_step_clear(skred_bank_t *bank, int pattern, int step);           /* empty step: the pattern wraps here */

/* Options.  The render loop has full-featured kernels (generic; modulated for banks with cross-voice modulation) and
 * specialised ones chosen per launch from what the bank holds (one voice per lane, two per lane);
 * their per-voice results, stems included, are bit-identical.  FORCE_GENERIC pins the full-featured kernels (the parity
 * tests use it to cross-check the specialised ones). */
enum { SKRED_OPT_FORCE_GENERIC = 1, SKRED_OPT_FAST2_MIN_VOICES = 2 /* bank size from which the two-voices-per-lane kernel is used */,
       SKRED_OPT_KERNEL_TIMING = 4 /* n: an event pair brackets the render kernels of every n-th launch (default 1: every
                                      launch; 0: none).  skred_bank_last_render_ms / _timing_summary report the bracketed
                                      launches; an event pair costs ~6 us of stream time on an MI355X, hence the knob */,
       SKRED_OPT_FM2_MIN_VOICES = 5 /* bank size from which a two-operator FM bank (every carrier an even voice, frequency-
                                       modulated by the voice after it and by nothing else) keeps carrier and modulator in
                                       one lane of the two-voices-per-lane kernel */,
       SKRED_OPT_IN_PLACE = 6 /* how the motion list of a two-voices-per-lane LDS-table bank is rendered while it is short: in the
                                 steady kernel's own lanes, from per-frame gain rows written by sk_gain_kernel just ahead of it
                                 ("in place"), or by the envelope kernel beside the steady one.  1 (default): in place where that
                                 is the faster path (sparse lists; bank sizes at which a second kernel costs the steady one a
                                 whole round of workgroups); 0: never; 2: whenever the rows provably suffice (tests).  Same
                                 per-voice results either way */,
       SKRED_OPT_SPLIT = 7 /* small clean LDS-table banks, while nothing moves: the one-voice-per-lane kernel with every frame split
                              between an oscillator wave and a post wave (sk_render_split_kernel).  0 (default): never -- measured at
                              best 1.4 % faster than the unsplit kernel; 1: banks of half a 256-voice group to one
                              group per CU with filters; 2: whenever the bank qualifies; 3: even while envelopes may be moving (tests:
                              the kernel then renders the waves concerned on its general path).  Same per-voice results either way */,
       SKRED_OPT_SPLIT_PAIRS = 8 /* (tests) the split form's workgroup shape: 0 (default) four (oscillator wave, post wave)
                                    pairs per workgroup; 2 / 4: forced (two: 256-thread workgroups whose four waves land on four SIMDs) */,
       SKRED_OPT_PACK = 9 /* sparse banks -- most voices skipped by the reference's own rule, voice_amp == 0 (synth.c:537), as in every
                             shipped patch (3 to 6 voices of 64 in use): the one-voice-per-lane kernel with the lanes PACKED, a
                             wavefront holding the voices that can sound of several aligned 64-voice groups (and the modulators
                             they name) instead of all 64 voices of one.  1 (default): on banks of at least 768 voices per CU, where at least half of
                             the wavefronts disappear (three quarters for banks the two-voices-per-lane kernel would take); 0: never;
                             2: whenever any disappear (tests, small banks).  The modulated kernel packs the same way.  Launches with the full stem buffer and banks on the generic / modulated / FM-pair
                             kernels are never packed.  Per-voice state is bit-identical either way; the mix differs by
                             summation order only */,
       SKRED_OPT_FM_SKEW = 10 /* previous-frame modulation on the one-voice-per-lane kernel (`v0 ... F3,1` / `A` / `P` with the modulator
                             above its carriers, synth.c:548-555,584-587,597-602, as in 3.sk / 1.sk / 7.sk / 37.sk / 0.sk): 1 (default) a lane
                             that is read by others runs 8-frame blocks AHEAD of its readers (chains up to three levels) and hands
                             its samples over through an LDS ring, so the readers' blocks have no per-frame exchange -- wavefronts
                             whose sources are silent (`m1`) or heard with their pan at rest, each exactly one block ahead of every
                             lane that reads it, and without reverse / noise / stopping / smoother-off lanes; other wavefronts keep
                             the exchange.  0: the per-frame ds_bpermute exchange everywhere.  The same option
                             governs the modulated kernel's FRAME-LAG form (a modulator BELOW its carrier -- a same-frame dependency,
                             18.sk -- with one dependency level: the dependent lanes run one frame behind instead of every frame being
                             rendered once per level).  Same bits either way */,
       SKRED_OPT_CROSS_GROUP = 11 /* modulators outside the carrier's aligned 64-voice group (an LFO voice read by thousands of voices,
                             patches laid out back to back across group edges).  0 (default): a bank with such a routing is refused
                             (SKRED_E_UNSUPPORTED) at every render.  1: rendered through a per-block SOURCE TAPE -- the sample
                             sequences of the cross-group modulators ("sources") are rendered ahead of the block by pre-pass launches
                             of the modulated kernel, one launch per level of the graph of groups (an edge from a reader's group to
                             its source's group), and read by their readers; same bits as the reference's index-order walk.  Limits
                             (each refused with SKRED_E_UNSUPPORTED / SKRED_E_RANGE, the bank stays usable): modulators outside the
                             bank; a cycle between groups; chains that need more than 16 pre-pass launches; a tape of more than
                             256 MiB (sources x (frames + 1) x 4 bytes).  Such banks run on the modulated kernel; the specialised
                             kernels, shards and the drop-in mode do not read the tape (skred_bank_last_cross_group) */,
       SKRED_OPT_CZ_FAST = 12 /* CZ phase distortion (`c<mode>,<dist>`, cz_phasor, synth.c:149-215) on the one-voice-per-lane kernel.  0
                             (default): a bank with a CZ voice runs the modulated kernel, as it always did.  1: a bank whose CZ voices
                             ALL QUALIFY, and which holds no other voice that needs the full-featured kernels, runs the CZ
                             instantiations of the one-voice kernel (skred_bank_last_cz; skred_bank_last_kernel says
                             SKRED_KERNEL_FAST).  A voice with cz mode 1..7 qualifies when (a) its CZ source (`C`) is absent or is a
                             higher-indexed voice of the same aligned 64-voice group -- the carrier then reads the source's
                             voice_sample of the previous frame, synth.c:262-267 in index order --, and (b) its frequency / amplitude
                             / pan modulators, if any, are higher-indexed voices of that group too, or -- amplitude, pan -- the voice
                             itself.  A CZ source below the carrier (16.sk's `v2 ... C1`), the carrier as its own CZ source, a
                             source in another group, a mode outside 1..7 and non-finite phase data keep the modulated kernel; so do
                             banks whose table pool is not staged in LDS, and SKRED_OPT_FORCE_GENERIC.  May be set at any time
                             between renders; the next block follows it, in both directions, nothing is uploaded again.  A
                             wavefront that holds a CZ lane keeps the per-frame exchange (it does not take the skewed blocks of
                             SKRED_OPT_FM_SKEW; other wavefronts of the bank do).  Same per-voice bits either way; the mix differs
                             by summation order only.  Shards, the fixed-point form and the drop-in mode never set it */ };
enum { SKRED_KERNEL_GENERIC = 0, SKRED_KERNEL_FAST = 1, SKRED_KERNEL_MODULATED = 2, SKRED_KERNEL_FAST2 = 3 };
int  skred_bank_set_option(skred_bank_t *bank, int option, int value);
int  skred_bank_last_kernel(const skred_bank_t *bank);   /* SKRED_KERNEL_* of the latest render */
int  skred_bank_last_in_place(const skred_bank_t *bank);  /* 1: the latest block rendered its motion list in place (SKRED_OPT_IN_PLACE) */
int  skred_bank_last_pack(const skred_bank_t *bank);      /* lanes per 64-voice group in the latest block (SKRED_OPT_PACK), 0: not packed */
int  skred_bank_last_split(const skred_bank_t *bank);     /* 1: the latest block ran the split form of the one-voice kernel (SKRED_OPT_SPLIT) */
int  skred_bank_last_cz(const skred_bank_t *bank);        /* 1: the latest block ran a CZ instantiation of the one-voice kernel (SKRED_OPT_CZ_FAST) */
/* SKRED_OPT_CROSS_GROUP: for the latest block, the number of tape sources and of pre-pass launches (0, 0: it read no tape) */
int  skred_bank_last_cross_group(const skred_bank_t *bank, int *n_sources, int *n_levels);

/* Per-frame evidence from INSIDE the fast paths (tests).  A launch with the full stem buffer takes the kernels' frame-by-frame
 * paths, so the 8-frame block paths the benchmarks time were only ever seen through end-of-block state and the mix.  A probe names
 * up to SKRED_PROBE_MAX voices; every later block writes, for each frame, what the reference stores into its stem buffer for them
 * (synth.c:607-611: voice_sample x pan_left, x pan_right; exact zeros for a skipped or muted voice) into
 * d_probe[frame][i][2] (device memory, num_frames x n x 2 floats per block, overwritten block by block) -- from the same launch,
 * on the same kernel paths, that render the block without it (probe instantiations of the one-voice-per-lane, two-voices-per-lane,
 * in-place and envelope kernels; other kernel families return SKRED_E_UNSUPPORTED while a probe is set).  n = 0 ends it. */
#define SKRED_PROBE_MAX 64
int  skred_bank_set_probe(skred_bank_t *bank, const int32_t *voices, int n, float *d_probe);

/* VOICE TAPS: the per-frame stems of chosen voices, from every kernel family.  A launch with the full stem buffer
 * (float[frames][n_voices][2]: 8 MB per frame at 2^20 voices) is never packed, never takes the frame-lag form and renders frame by
 * frame on the one-voice kernel.  A tap names up to SKRED_TAPS_MAX voices; every later block writes into
 * d_taps[frame][k][2] (device memory, num_frames x n x 2 floats, overwritten by every block; zeroed on the render stream ahead of
 * the launch) the (left, right) the reference stores into its stem buffer for voice voices[k] at that frame (synth.c:603-611) --
 * exact zeros for a skipped, finished, muted or disconnected voice -- from the same launch and on the same kernel paths that render
 * the block without taps: packed lanes, the frame-lag form, the cross-group tape, the generic kernel and the specialised families
 * included.  The layout is what skred_recorder_append takes from a recorder created with n_voices = n: append d_taps after each
 * block on the render stream, then save.  A tap does not change what the block computes: voice state, globals and the mix are
 * bit-identical to the same block without taps, and skred_bank_last_kernel / _last_pack / _last_cross_group and the form counters
 * report the same -- with one exception: a two-operator FM bank renders on the one-voice-per-lane kernel while taps are set, as
 * it does below SKRED_OPT_FM2_MIN_VOICES (per-voice results are bit-identical across the kernel families, see the options above;
 * its mix then differs by summation order only), and the split form (SKRED_OPT_SPLIT) is not taken.
 * Refused: a voice outside the bank (SKRED_E_RANGE); n > SKRED_TAPS_MAX, or NULL pointers with n > 0 (SKRED_E_BAD_ARG); taps while
 * a probe is set and a probe while taps are set (SKRED_E_BAD_ARG for the second setter); a render with taps set and a stem buffer
 * (SKRED_E_UNSUPPORTED: the stems already contain the taps; the bank stays usable).  n = 0 ends it.  Not in the fixed-point bank,
 * shards or the drop-in mode.  The call WAITS FOR THE DEVICE (a block in flight may still read the old list): a host that must not
 * wait sets the taps once, on a buffer sized for its longest block, and queues a device-to-device copy of d_taps on the render
 * stream behind each block. */
#define SKRED_TAPS_MAX 64
int  skred_bank_set_taps(skred_bank_t *bank, const int32_t *voices, int n, float *d_taps);
int  skred_bank_last_taps(const skred_bank_t *bank);     /* taps written by the latest block, 0: none */

/* Which form the modulated kernel's wavefronts ran (tests): with `d_counts` set (device memory, two words the caller owns and
 * zeroes), every pass of every wavefront of the modulated kernel adds 1 to d_counts[0] when it runs the frame-lag form
 * (SKRED_OPT_FM_SKEW) and to d_counts[1] when it runs the level loop of a bank with same-frame dependencies.  NULL ends it;
 * unset, the kernel pays one scalar branch per pass. */
int  skred_bank_set_form_counter(skred_bank_t *bank, uint32_t *d_counts);

/* Cross-check of the motion list of the two-voices-per-lane path ("The motion list"): voices whose envelope may be
 * in motion are kept on a per-voice list ON THE DEVICE (every control action lists the voices it touches, the envelope kernel
 * keeps its voices listed until they rest) and rendered by the envelope kernel beside the steady kernel, which never has to be
 * told by the host whether anything moves.  The steady kernel still classifies every voice it renders; this is the number of
 * voices it ever found in motion without being listed, as far as reported (asynchronously).  0 by construction; should it move,
 * the list is rebuilt from the voice state by itself and skred_amd_last_error() names the launch. */
unsigned skred_bank_list_violations(const skred_bank_t *bank);

/* ---- which voices are free: an asynchronous list of idle voices, built on the device ---------------------------------
 *
 * What a note-on needs before its skred_bank_update(..., SKRED_DIRTY_PARAMS | SKRED_STAMP_TRIGGER): a voice that is not
 * sounding.  Whether a voice sounds is state only the device has (voice_finished of a one-shot that ran out mid-block,
 * is_active cleared by the kernel when a release ended, the amp smoother's running gain); skred_bank_download() returns it,
 * but waits for the whole device and copies every read-write plane of the range.  The query sweeps the words it needs where
 * they are and leaves an ordered list of voice indices in device memory, on the caller's stream.
 *
 * The predicates are stated on the reference's fields AS THE DEVICE HOLDS THEM at that point of the stream (the values
 * skred_bank_download would return there); every comparison is exact, so the list has one right answer.  A padding voice or
 * a voice without a table follows the same field rules as any other.  Routing is read as the kernels read it: frequency
 * modulation by the voice itself (ignored, synth.c:549) and a CZ source while voice_cz_mode == 0 (never read, synth.c:262)
 * name nobody; amplitude or pan modulation by the voice itself names it; a modulator index outside the bank names nobody.
 *
 * ENV_DONE carries a level for a reason: after a release has ended the smoother's target is 0, and g += k * (0 - g) in
 * float stalls on a non-zero subnormal instead of reaching 0 -- a comparison with zero would never list a smoothed voice. */
enum {                                   /* criteria: a voice is idle when ANY selected criterion holds */
  SKRED_IDLE_FINISHED = 1u << 0,         /* voice_finished != 0 (osc_next's finish rule; skipped at synth.c:531-542) */
  SKRED_IDLE_ENV_DONE = 1u << 1,         /* voice_use_amp_envelope != 0 && voice_amp_envelope.is_active == 0
                                            && (voice_smoother_enable == 0 || fabsf(voice_smoother_gain) <= settle_level) */
  SKRED_IDLE_AMP_ZERO = 1u << 2,         /* voice_amp == 0.0f (the reference's own skip rule, synth.c:537) */
  /* restrictions: a voice is listed only if ALL selected restrictions hold too */
  SKRED_IDLE_UNNAMED  = 1u << 8          /* no voice of the bank names it as FM / AM / pan / CZ modulator (voice_*_mod_osc) */
};
typedef struct skred_idle_query {
  int32_t  first, count;   /* voice range [first, first + count) inside the bank */
  uint32_t which;          /* SKRED_IDLE_* ; at least one criterion */
  float    settle_level;   /* see ENV_DONE; 0: the smoother's gain must be exactly +-0 */
  int32_t  from;           /* listing order: ascending voice index starting at `from` (first <= from < first + count),
                              wrapping to `first` -- a round-robin allocator passes last pick + 1; `first` = plain ascending */
  int32_t  max_out;        /* room in d_voices; 0: count only */
} skred_idle_query_t;

/* Asynchronous on `stream`, ordered after the renders and updates queued on it.  Writes d_voices[0 .. written) and
 * d_count[0] = written = min(total, max_out), d_count[1] = total idle voices in the range (device memory).  Entries of
 * d_voices past `written` are not touched.  Reads the bank only: state, globals, mix, reports and counters of every later
 * block are bit-identical to the same blocks without the query.  The order is by voice index, never by arrival: two queries
 * on the same state write the same bytes.  Two launches (a count whose last-arriving workgroup makes the offsets, a scatter);
 * with SKRED_IDLE_UNNAMED, after an upload or an update that changed the routing, one more that rebuilds the set of named
 * voices.  The bank owns the scratch they use: issue the queries of one bank on one stream at a time, as its renders.
 * Refused, before anything touches the device: SKRED_E_BAD_ARG -- NULL bank, query or d_count, NULL d_voices with
 * max_out > 0, no criterion bit, unknown bits, negative max_out, a settle_level that is negative or not finite;
 * SKRED_E_RANGE -- count <= 0, a range outside the bank, `from` outside the range.
 * On a shard: through skred_shard_bank(), with that rank's local indices.  Not in the fixed-point bank or the drop-in mode
 * (whose 64 voices are named by the patch). */
int  skred_bank_find_idle(skred_bank_t *bank, const skred_idle_query_t *q, int32_t *d_voices, uint32_t *d_count, void *stream);
/* The same into host memory; waits for `stream` only (not for the device, unlike skred_bank_download).
 * Returns `written` (>= 0) or a SKRED_E_* code; *total_out may be NULL. */
int  skred_bank_find_idle_host(skred_bank_t *bank, const skred_idle_query_t *q, int32_t *voices, int *total_out, void *stream);

/* ---- device-side note-ons: notes placed on a voice list the device holds, without a host wait ---------------------------
 *
 * skred_bank_find_idle leaves its list in device memory; skred_bank_update takes voice indices from the host.  These calls
 * close the gap: the notes are small records written on the host, the voices that receive them are picked ON THE DEVICE from
 * a list in device memory, at that point of the stream.  A host that paces blocks ahead of the device never waits for the list.
 *
 * A note-on is the reference's `l` command (synth.c:1153-1156): a pitch, optionally a pan, osc_trigger (synth.c:316-339) and
 * amp_envelope_trigger(voice, velocity) (synth.c:383-388).  None of these stores changes what the library's host side knows
 * about a voice -- kernel selection, packed lanes, the named set and the cross-group tape depend on voice_amp == 0, the flags,
 * the routing, the table geometry and on whether phase and increment are finite, never on the value of a finite increment,
 * the velocity, a finite phase or the pans -- which is why it can be applied to a voice whose index only
 * the device knows, provided non-finite values are refused here, on the host. */
enum { SKRED_NOTE_SET_PHASE = 1u << 0,   /* osc_trigger: voice_phase = note.phase, voice_finished = 0 */
       SKRED_NOTE_SET_PAN   = 1u << 1 }; /* pan_set: voice_pan_left / _right = note.pan_left / _right */
typedef struct skred_note {              /* 32 bytes */
  float phase_inc, velocity, phase, pan_left, pan_right;
  uint32_t flags, reserved[2];           /* reserved must be 0 */
} skred_note_t;

/* Pure host, no device: SKRED_OK, or SKRED_E_BAD_ARG for NULL notes, n < 0, unknown flag bits, non-zero reserved words, a
 * non-finite phase_inc or velocity, a non-finite phase under SET_PHASE, non-finite pans under SET_PAN (fields a note does not
 * set are not looked at).  The entry points below call it before anything touches the device. */
int  skred_notes_check(const skred_note_t *notes, int n);

/* Note k (0 <= k < n) goes to voice d_voices[first_entry + k] if first_entry + k < d_count[0] and that entry lies in
 * [0, n_voices); otherwise the note is dropped.  d_voices and d_count are device memory, read on the device at that point of
 * the stream (d_count[0] is what skred_bank_find_idle writes there; d_count and the d_count[0] entries behind d_voices must be
 * readable).  On the chosen voice the kernel stores, and nothing else: voice_phase_inc = phase_inc;
 * voice_amp_envelope.velocity = velocity; with SET_PHASE the phase and voice_finished = 0; with SET_PAN the two pan words; the
 * trigger stamp (sample_start = synth_sample_count as the bank has it at application time, sample_release = 0, is_active = 1);
 * the voice's bit on the motion list.  Filter memory, hold, smoother, sample and every other parameter keep their values.
 * d_assigned[k] (device, int32[n], may be NULL) = the voice, or -1 for a dropped note, for every k < n; d_result (device,
 * uint32[2], required): [0] notes placed, [1] n minus placed.  The results are a pure function of the inputs: two identical
 * calls on identical state write identical bytes.  The list must name distinct voices (find_idle's does); with duplicates,
 * which of the competing notes a voice ends with is unspecified, and nothing else is affected.  `first_entry` is the cursor
 * that lets several calls share one query: the second call of a block passes the number of notes sent since the query.
 * Asynchronous on `stream`, ordered like skred_bank_update (the notes are staged before the call returns: the caller's array
 * is free again).  n == 0: SKRED_OK, nothing is done, d_result is not written.
 * Refused with SKRED_E_BAD_ARG before anything touches the device: NULL bank, notes, list, count or result; n < 0;
 * first_entry < 0; whatever skred_notes_check refuses.
 * Limits.  The host view does not learn which voice got which note: read d_assigned back a block later and mirror pitch,
 * velocity (phase, pans) into it before a later SKRED_DIRTY_PARAMS update of those voices -- otherwise that update restores
 * the host's stale values.  A voice whose increment or phase was non-finite when the host last wrote it keeps its class on the
 * host: results stay correct, the bank stays on the generic kernel until the host rewrites that voice.  Not in the fixed-point
 * bank or the drop-in mode.  On a shard: through skred_shard_bank(), with that rank's local indices. */
int  skred_bank_notes_on_list(skred_bank_t *bank, const skred_note_t *notes, int n,
                              const int32_t *d_voices, const uint32_t *d_count, int first_entry,
                              int32_t *d_assigned, uint32_t *d_result, void *stream);
/* One call: the query `q` into scratch the bank owns (q->max_out is ignored: the library uses n), then the placement with
 * first_entry = 0.  Refusals of both, and SKRED_E_BAD_ARG for SKRED_IDLE_AMP_ZERO in q->which: a note-on leaves voice_amp
 * alone, so such a voice would stay silent and be listed again.  One stream at a time per bank, as for the query. */
int  skred_bank_note_on_idle(skred_bank_t *bank, const skred_idle_query_t *q, const skred_note_t *notes, int n,
                             int32_t *d_assigned, uint32_t *d_result, void *stream);
/* SKRED_STAMP_TRIGGER and / or SKRED_STAMP_RELEASE (as skred_bank_update applies them) on the first min(n, *d_count_or_null)
 * entries of a list in device memory (NULL: n entries).  Entries that are negative or >= n_voices are skipped, so a d_assigned
 * array with its -1 holes can be handed back as the note-off list.  Asynchronous on `stream`.  SKRED_E_BAD_ARG: NULL bank or
 * list, n < 0, no stamp bit or bits other than the two SKRED_STAMP_*; n == 0: SKRED_OK, nothing is done. */
int  skred_bank_stamp_list(skred_bank_t *bank, const int32_t *d_voices, int n, const uint32_t *d_count_or_null,
                           uint32_t stamps, void *stream);

/* ---- voice stealing: the sounding voices that matter least, ranked on the device ------------------------------------------
 *
 * When the idle list is shorter than a batch of notes, a polyphonic synthesizer takes the voice that matters least: the one
 * released longest ago, then the one held longest, or the quietest.  Everything such a policy reads is on the device, current at
 * every point of the stream: sample_start and sample_release (written by the stamp and note kernels), is_active (cleared by the
 * render kernels), the amp smoother's running gain, the named set.  The query ranks the candidates of a range by a 64-bit key
 * and leaves the first max_out of them in device memory, on the caller's stream, without a host wait.
 *
 * The definition, on the fields AS THE DEVICE HOLDS THEM at that point of the stream; every comparison is exact.  `now` is
 * synth_sample_count as the bank has it at application time (the value the stamps use).
 *   released  := sample_release != 0
 *   age       := sample_start > now ? 0 : now - sample_start
 *   candidate := inside the range && voice_use_amp_envelope != 0 && is_active != 0 && age >= min_age
 *                && (released, with RELEASED_ONLY) && (not in the named set, with UNNAMED)
 *                && the voice does NOT satisfy the idle predicate of (exclude_idle, settle_level) -- skred_bank_find_idle's,
 *                   criteria and SKRED_IDLE_UNNAMED restriction as there; exclude_idle == 0 excludes nobody
 *   class     := 0 when RELEASED_FIRST is set and the voice is released, else 1
 *   primary   := OLDEST: sample_release of a class-0 voice, sample_start otherwise;
 *                QUIETEST: the bits of fabsf(voice_smoother_gain) when voice_smoother_enable != 0, else 0x7fffffff
 *   key       := class << 62 | min(primary, 2^62 - 1)
 * Victim order: ascending key, ties by ascending voice index.  Padding voices and voices without a table follow the same rules. */
#define SKRED_STEAL_MAX 1024
enum { SKRED_STEAL_OLDEST = 0, SKRED_STEAL_QUIETEST = 1 };          /* policy */
enum { SKRED_STEAL_RELEASED_FIRST = 1u << 0,   /* voices in release rank ahead of held ones */
       SKRED_STEAL_RELEASED_ONLY  = 1u << 1,   /* held voices are not candidates */
       SKRED_STEAL_UNNAMED        = 1u << 8 }; /* as SKRED_IDLE_UNNAMED */
typedef struct skred_steal_query {
  int32_t  first, count;     /* voice range */
  uint32_t policy, flags;
  uint64_t min_age;          /* frames: younger notes are protected */
  uint32_t exclude_idle;     /* SKRED_IDLE_* criteria (0: none): voices these call idle are not candidates */
  float    settle_level;     /* for exclude_idle's ENV_DONE */
  int32_t  max_out;          /* 0 .. SKRED_STEAL_MAX; 0: count only */
  int32_t  reserved;         /* 0 */
} skred_steal_query_t;

/* Pure host, no device: SKRED_OK, or SKRED_E_BAD_ARG for a NULL query, an unknown policy, unknown bits in flags or exclude_idle,
 * reserved != 0, max_out outside [0, SKRED_STEAL_MAX], a settle_level that is negative or not finite; SKRED_E_RANGE for
 * count <= 0 or a range outside a bank of n_voices voices.  The entry points below call it before anything touches the device. */
int  skred_steal_check(const skred_steal_query_t *q, int n_voices);

/* Asynchronous on `stream`, ordered after the renders and updates queued on it.  Writes the first min(total, max_out) voices of
 * the victim order into d_voices, d_count[0] = written, d_count[1] = total candidates (device memory).  Entries of d_voices past
 * `written` are not touched.  Reads the bank only: state, globals, mix, reports and counters of every later block are
 * bit-identical to the same blocks without the query; the same state gives the same bytes.  A radix select over the keys: nine
 * launches whatever the data (one with max_out == 0), no workgroup ever waits for another; with UNNAMED (here or in
 * exclude_idle) one more when the routing changed.  The bank owns the scratch (8 bytes per voice, allocated by the first
 * query): issue the queries of one bank on one stream at a time, as its renders.
 * Refused before anything touches the device: what skred_steal_check refuses, and SKRED_E_BAD_ARG for a NULL bank, query or
 * d_count, or a NULL d_voices with max_out > 0.  On a shard: through skred_shard_bank(), with that rank's local indices.  Not
 * in the fixed-point bank or the drop-in mode. */
int  skred_bank_find_steal(skred_bank_t *bank, const skred_steal_query_t *q, int32_t *d_voices, uint32_t *d_count, void *stream);
/* The same into host memory; waits for `stream` only.  Returns `written` (>= 0) or a SKRED_E_* code; *total_out may be NULL. */
int  skred_bank_find_steal_host(skred_bank_t *bank, const skred_steal_query_t *q, int32_t *voices, int *total_out, void *stream);
/* A batch of notes on a bank whose polyphony may be used up, all on the device: the idle query `idle_q` into scratch the bank
 * owns (max_out = n; SKRED_IDLE_AMP_ZERO is refused as in skred_bank_note_on_idle), the steal query `steal_q` with
 * exclude_idle = idle_q->which, settle_level = idle_q->settle_level and max_out = min(n, SKRED_STEAL_MAX) (the library overrides
 * those three fields; because of the exclusion the two lists are disjoint), the victims appended behind the idle entries, and the
 * notes placed on the joined list as skred_bank_notes_on_list places them, first_entry = 0: idle voices take the first notes,
 * victims the next, in victim order; what is left is dropped.  A stolen voice gets exactly a note-on's stores: it is re-triggered
 * with the new pitch and velocity, its filter memory and smoother carry on.
 * d_result (device, uint32[3], required): [0] placed, [1] dropped, [2] how many of the placed notes went to stolen voices;
 * d_assigned as for skred_bank_notes_on_list.  The host never learns the counts.  n == 0: SKRED_OK, nothing is done.
 * Refusals: those of skred_bank_note_on_idle and of skred_bank_find_steal, before anything touches the device. */
int  skred_bank_note_on_steal(skred_bank_t *bank, const skred_idle_query_t *idle_q, const skred_steal_query_t *steal_q,
                              const skred_note_t *notes, int n, int32_t *d_assigned, uint32_t *d_result, void *stream);

/* ---- patch notes: idle SLOTS of a tiled patch, and notes and stamps on all voices of a slot ---------------------------------
 *
 * What is rendered at scale is patches: an instrument of several voices -- a carrier with its modulators, some of them enveloped
 * -- tiled over the bank, every copy an aligned run of K voices (skred_amd.banks.bank_patch).  A note on such an instrument is a
 * note on ALL voices of one copy, and a copy is free only when ALL its enveloped voices have come to rest; idle voices of
 * different copies interleave in skred_bank_find_idle's list, and a note that landed on voices of two copies would play nonsense
 * through the copies' routing.  These calls are the voice calls above, stated on slots.
 *
 * A SLOT is an aligned run of K = slot_voices voices, K in {1, 2, 4, 8, 16, 32, 64}: its first voice is a multiple of K (so it
 * never straddles an aligned 64-voice group), and the slot is named by its first voice.
 * A slot is IDLE if and only if every MEMBER voice -- voice l of the slot with bit l of member_mask set -- satisfies
 * skred_bank_find_idle's predicate for (which, settle_level), on the fields as the device holds them at that point of the stream.
 * Voices outside member_mask are never looked at: the unused voices of a patch, or an LFO without an envelope that runs forever.
 * SKRED_IDLE_UNNAMED is refused: the voices of a patch name one another by design.
 * With K = 1 and both masks 1 every call below writes the bytes of its per-voice counterpart. */
typedef struct skred_slot_query {
  int32_t  first, count;    /* voice range; first % K == 0, count % K == 0, count > 0, inside the bank */
  int32_t  slot_voices;     /* K */
  uint64_t member_mask;     /* bit l: voice l of a slot takes part in the idle test; non-zero, no bits at or above K */
  uint32_t which;           /* SKRED_IDLE_FINISHED | _ENV_DONE | _AMP_ZERO; at least one; SKRED_IDLE_UNNAMED refused */
  float    settle_level;    /* as skred_idle_query_t */
  int32_t  from;            /* a slot's first voice inside the range: listing starts there and wraps to `first` */
  int32_t  max_out;         /* room in d_slots, in slots; 0: count only */
} skred_slot_query_t;

/* Pure host, no device: SKRED_OK, or what skred_bank_find_idle_slots refuses about the query itself on a bank of n_voices voices.
 * SKRED_E_BAD_ARG: NULL query, negative max_out, SKRED_IDLE_UNNAMED or unknown bits in which, no criterion, a settle_level that is
 * negative or not finite, a member_mask that is 0 or has bits at or above K.  SKRED_E_RANGE: K not a power of two in 1 .. 64,
 * count <= 0, a range outside the bank, `from` outside the range, first, count or from not a multiple of K. */
int  skred_slot_query_check(const skred_slot_query_t *q, int n_voices);
/* Pure host, no device: skred_notes_check's rules on the n * K records of n patch notes, applied ONLY to the records of voices
 * with a bit in voice_mask (the others are not looked at), and SKRED_E_RANGE for a bad K, SKRED_E_BAD_ARG for a voice_mask that
 * is 0 or has bits at or above K. */
int  skred_slot_notes_check(const skred_note_t *notes, int n, int slot_voices, uint64_t voice_mask);

/* skred_bank_find_idle on slots.  d_slots[0 .. written) = the first voices of the idle slots of the range, ascending from `from`
 * and wrapping to `first`; d_count[0] = written = min(total, max_out), d_count[1] = total; entries past `written` are not
 * touched.  Asynchronous on `stream`, reads the bank only, the same state gives the same bytes (the order is by voice index,
 * never by arrival).  Two launches, on the scratch the voice query uses: one stream at a time per bank.  Refused before anything
 * touches the device: what skred_slot_query_check refuses, and SKRED_E_BAD_ARG for a NULL bank or d_count, or a NULL d_slots with
 * max_out > 0.  On a shard: through skred_shard_bank(), with local indices.  Not in the fixed-point bank or the drop-in mode. */
int  skred_bank_find_idle_slots(skred_bank_t *bank, const skred_slot_query_t *q, int32_t *d_slots, uint32_t *d_count, void *stream);
/* The same into host memory; waits for `stream` only.  Returns `written` (>= 0) or a SKRED_E_* code; *total_out may be NULL. */
int  skred_bank_find_idle_slots_host(skred_bank_t *bank, const skred_slot_query_t *q, int32_t *slots, int *total_out, void *stream);
/* skred_bank_notes_on_list on slots.  `notes` holds n * K records: record k * K + l is the skred_note_t for voice l of note k.
 * Note k takes the slot e = d_slots[first_entry + k] if that entry exists (first_entry + k < d_count[0]), 0 <= e, e % K == 0 and
 * e + K <= n_voices; otherwise the note is dropped whole.  On a taken slot every voice l with bit l of voice_mask set receives
 * exactly skred_bank_notes_on_list's stores for its record (increment, velocity, with SET_PHASE the phase and voice_finished = 0,
 * with SET_PAN the pans, the trigger stamp with synth_sample_count at application time, its bit on the motion list); voices without
 * a bit are not touched, their records neither read nor checked.  There is no arithmetic on the device: the pitch ratios between a
 * carrier and its modulators are the host's business and arrive as finished increments, which keeps the result bit-equal to the
 * host route.  d_assigned[k] (device, int32[n], may be NULL) = the slot's first voice or -1; d_result (device, uint32[2],
 * required) = notes placed, notes dropped -- in notes, not voices.  first_entry: the cursor of skred_bank_notes_on_list.
 * The list must name distinct slots (skred_bank_find_idle_slots' does; a hand-made list or a reused d_assigned may not): with a
 * slot named twice, which of the competing notes each of its voices ends with is unspecified -- voice by voice, so a copy may end
 * with records of both -- and nothing else is affected.
 * Asynchronous on `stream`; n == 0: SKRED_OK, nothing is done.  Refused before anything touches the device: SKRED_E_BAD_ARG for a
 * NULL bank, notes, list, count or result, n < 0, first_entry < 0, and what skred_slot_notes_check refuses. */
int  skred_bank_notes_on_slots(skred_bank_t *bank, const skred_note_t *notes, int n, int slot_voices, uint64_t voice_mask,
                               const int32_t *d_slots, const uint32_t *d_count, int first_entry,
                               int32_t *d_assigned, uint32_t *d_result, void *stream);
/* One call: the query `q` into scratch the bank owns (q->max_out is ignored: the library uses n), then the placement with
 * K = q->slot_voices and first_entry = 0.  Refusals of both, and SKRED_E_BAD_ARG for SKRED_IDLE_AMP_ZERO as in
 * skred_bank_note_on_idle. */
int  skred_bank_note_on_idle_slots(skred_bank_t *bank, const skred_slot_query_t *q, const skred_note_t *notes, int n,
                                   uint64_t voice_mask, int32_t *d_assigned, uint32_t *d_result, void *stream);
/* skred_bank_stamp_list on slots: SKRED_STAMP_TRIGGER and / or SKRED_STAMP_RELEASE on the voices with a bit in voice_mask of the
 * first min(n, *d_count_or_null) listed slots (NULL: n).  Entries that are no slot of the bank (negative, not a multiple of K,
 * past the bank) are skipped, so an earlier d_assigned with its -1 holes is the note-off list of a chord.  A slot named twice is
 * stamped twice with the same clock and the same bits, which is the same as once.  SKRED_E_BAD_ARG: NULL
 * bank or list, n < 0, no stamp bit or other bits, a bad voice_mask; SKRED_E_RANGE: a bad K; n == 0: SKRED_OK, nothing is done. */
int  skred_bank_stamp_slots(skred_bank_t *bank, const int32_t *d_slots, int n, const uint32_t *d_count_or_null,
                            int slot_voices, uint64_t voice_mask, uint32_t stamps, void *stream);

/* ---- slot stealing: the sounding copies of a tiled patch that matter least, ranked on the device ------------------------------
 *
 * skred_bank_note_on_idle_slots drops what the idle slots cannot take; a synthesizer steals.  The victims of skred_bank_find_steal
 * are single voices of many different copies and cannot serve a patch: these calls are the stealing calls above, stated on slots.
 *
 * A slot, K = slot_voices and member_mask mean what they mean for skred_slot_query_t; voice_mask what it means for
 * skred_bank_notes_on_slots.  The definition, on the fields AS THE DEVICE HOLDS THEM at that point of the stream; every comparison
 * is exact; `now` is synth_sample_count as the bank has it at application time.  For voice l of a slot:
 *   member(l)   := bit l of member_mask
 *   live(l)     := member(l) && voice_use_amp_envelope != 0 && is_active != 0
 *   released(l) := sample_release != 0
 *   age(l)      := sample_start > now ? 0 : now - sample_start
 *   idle(l)     := skred_bank_find_idle's predicate for (exclude_idle, settle_level)
 *   slot candidate := the slot inside the range
 *                  && some l is live
 *                  && every live l has age(l) >= min_age
 *                  && (with RELEASED_ONLY: every live l is released)
 *                  && NOT (exclude_idle != 0 && every member l is idle(l))
 *   class   := 0 when RELEASED_FIRST is set and every live l is released, else 1
 *   primary := OLDEST:   max over live l of (sample_release in class 0, sample_start in class 1)
 *              QUIETEST: max over live l of (the bits of fabsf(voice_smoother_gain) when voice_smoother_enable != 0, else 0x7fffffff)
 *   key     := class << 62 | min(primary, 2^62 - 1)
 * A slot is as young as its youngest live member, released as late as its last released member and as loud as its loudest live
 * member.  Victim order: ascending key, ties by ascending first voice.  Voices outside member_mask are never read; members that are
 * not live count for nothing in age, class or key.  SKRED_STEAL_UNNAMED is refused, in flags and in exclude_idle: the voices of a
 * patch name one another by design.  With K = 1 and mask 1 every line is the per-voice definition, and the calls write the bytes
 * of skred_bank_find_steal and skred_bank_note_on_steal. */
typedef struct skred_slot_steal_query {   /* 56 bytes */
  int32_t  first, count;     /* voice range; first % K == 0, count % K == 0, count > 0, inside the bank */
  int32_t  slot_voices;      /* K: a power of two, 1 .. 64 */
  uint32_t policy;           /* SKRED_STEAL_OLDEST or SKRED_STEAL_QUIETEST */
  uint64_t member_mask;      /* bit l: voice l of a slot takes part; non-zero, no bits at or above K */
  uint64_t min_age;          /* frames: a slot with a younger live member is protected */
  uint32_t flags;            /* SKRED_STEAL_RELEASED_FIRST | _RELEASED_ONLY; SKRED_STEAL_UNNAMED refused */
  uint32_t exclude_idle;     /* SKRED_IDLE_FINISHED | _ENV_DONE | _AMP_ZERO (0: none): slots these call idle are no candidates */
  float    settle_level;     /* for exclude_idle's ENV_DONE */
  int32_t  max_out;          /* 0 .. SKRED_STEAL_MAX, in slots; 0: count only */
  uint32_t reserved[2];      /* 0 */
} skred_slot_steal_query_t;

/* Pure host, no device: SKRED_OK, or SKRED_E_BAD_ARG for a NULL query, an unknown policy, unknown bits or SKRED_STEAL_UNNAMED in
 * flags, unknown bits or SKRED_IDLE_UNNAMED in exclude_idle, non-zero reserved words, max_out outside [0, SKRED_STEAL_MAX], a
 * settle_level that is negative or not finite, a member_mask that is 0 or has bits at or above K; SKRED_E_RANGE for K not a power
 * of two in 1 .. 64, count <= 0, a range outside a bank of n_voices voices, first or count not a multiple of K.  The entry points
 * below call it before anything touches the device. */
int  skred_slot_steal_check(const skred_slot_steal_query_t *q, int n_voices);

/* skred_bank_find_steal on slots, under its contract: asynchronous on `stream`; d_slots[0 .. written) = the first voices of the
 * first min(total, max_out) slots of the victim order, d_count[0] = written, d_count[1] = total candidate slots (device memory);
 * entries past `written` are not touched.  Reads the bank only; the same state gives the same bytes.  The radix select of
 * skred_bank_find_steal behind a key pass of its own (one key per slot, reduced over the members inside a wavefront): the same nine
 * launches (one with max_out == 0), the same scratch -- one stream at a time per bank --, no workgroup ever waits for another.
 * Refused before anything touches the device: what skred_slot_steal_check refuses, and SKRED_E_BAD_ARG for a NULL bank, query or
 * d_count, or a NULL d_slots with max_out > 0.  On a shard: through skred_shard_bank(), with that rank's local indices.  Not in
 * the fixed-point bank or the drop-in mode. */
int  skred_bank_find_steal_slots(skred_bank_t *bank, const skred_slot_steal_query_t *q, int32_t *d_slots, uint32_t *d_count, void *stream);
/* The same into host memory; waits for `stream` only.  Returns `written` (>= 0) or a SKRED_E_* code; *total_out may be NULL. */
int  skred_bank_find_steal_slots_host(skred_bank_t *bank, const skred_slot_steal_query_t *q, int32_t *slots, int *total_out, void *stream);
/* A burst of n patch notes (n * K records, as for skred_bank_notes_on_slots) on a tiled instrument whose polyphony may be used
 * up, all on the device: the idle-slot query `idle_q` into scratch the bank owns (max_out = n), the slot steal query `steal_q` with
 * exclude_idle = idle_q->which, settle_level = idle_q->settle_level and max_out = min(n, SKRED_STEAL_MAX) (the library overrides
 * those three fields; because of the exclusion the two lists are disjoint), the victims appended behind the idle slots, and the
 * notes placed on the joined list as skred_bank_notes_on_slots places them, first_entry = 0: idle slots take the first notes,
 * victims the next, in victim order; what is left is dropped whole.  A stolen slot gets exactly a patch note's stores on its
 * voice_mask voices: they are re-triggered, their filter memory and smoothers carry on; voices outside voice_mask are untouched.
 * d_result (device, uint32[3], required): [0] notes placed, [1] notes dropped, [2] how many of the placed notes went to stolen
 * slots; d_assigned as for skred_bank_notes_on_slots.  The host never learns the counts and waits for nothing.  n == 0: SKRED_OK,
 * nothing is done.  Refused before anything touches the device: what skred_bank_note_on_idle_slots (SKRED_IDLE_AMP_ZERO among it)
 * and skred_bank_find_steal_slots refuse, and SKRED_E_BAD_ARG when the two queries differ in slot_voices or member_mask (their
 * ranges may differ; each is made of whole slots).  On a shard: through skred_shard_bank().  Not in the fixed-point bank or the
 * drop-in mode. */
int  skred_bank_note_on_steal_slots(skred_bank_t *bank, const skred_slot_query_t *idle_q, const skred_slot_steal_query_t *steal_q,
                                    const skred_note_t *notes, int n, uint64_t voice_mask, int32_t *d_assigned, uint32_t *d_result,
                                    void *stream);

/* ---- patch controllers: a few parameter words of every copy of a tiled patch, changed on the device ----------------------------
 *
 * A performance moves controls as well as keys: a filter sweep, a volume or expression change, a pan, a modulation-depth wheel, a
 * pitch bend, a longer release -- on all copies of a patch, or on the copies of one chord.  Through skred_bank_update that is a full
 * host record per voice; the write itself is a few words.  These calls store those words with a kernel, on voices the host never
 * lists: every slot of a range, or the slots a list in device memory names (an earlier d_assigned: "this chord only").
 *
 * A slot, K = slot_voices and voice_mask mean what they mean for skred_bank_notes_on_slots.  `ctl` holds K records: record l is for
 * voice l of a slot, only voices with bit l of voice_mask set are touched, the other records are neither read nor checked.  With
 * K = 1 and mask 1 these are per-voice calls.  A record names the fields it stores in `set`; exactly those words are stored, as
 * given, and nothing else: the running phase, the filter memory, the smoother gain, the envelope clock, the flags and the routing
 * keep what the device computed.  Two stores look at the device's value first:
 *   SKRED_CTL_INC_SCALE  voice_phase_inc = voice_phase_inc * inc_scale, ONE fp32 multiply, never fused; a product that is not
 *                        finite is not stored (the voice keeps its increment).  A pitch bend of voices whose pitches the host
 *                        never learned (device-side note-ons).
 *   SKRED_CTL_AMP        stored on voices whose voice_amp != 0.0f ON THE DEVICE; a voice with amp 0 (or -0) keeps it.
 * Why those, and why the refusals below: of the words a controller stores the host-side planner reads three things -- whether
 * voice_amp == 0 (which voices can sound: the packed lanes), whether increment and phase data are finite (the voice's kernel
 * class), and the routing.  Finite values, an amp that keeps its zero-ness and no routing field leave the bank's classes, counters,
 * lane words, named set and tape plan right without the host knowing which voice holds what -- the argument skred_bank_notes_on_list
 * makes for notes.
 * Voices whose record names AMP, ENV_TIMES, VELOCITY or SMOOTHING go on the motion list (those are the words that can set an envelope
 * or a smoother moving); the other controllers do not, so a bank-wide filter sweep costs the next block nothing.
 * LIMIT, as for notes: the host view goes stale.  Before a later skred_bank_update with SKRED_DIRTY_PARAMS (or SKRED_DIRTY_PAN) of
 * such a voice, mirror the values into the host view; skred_bank_download_ctl reads them back where the host cannot know them (a
 * scaled increment, a withheld amp).  On a shard: through skred_shard_bank(), with that rank's local indices.  The fixed-point bank
 * has per-voice controllers of its own (include/skred_amd_fxpt.h: skred_fxbank_ctl_range / _ctl_list / _ctl_owned, without slots and
 * without the depth, scale and CZ fields).  Not in the drop-in mode; deferred items and pattern steps carry host records only. */
enum { SKRED_CTL_PHASE_INC = 1u<<0,  /* voice_phase_inc = phase_inc */
       SKRED_CTL_INC_SCALE = 1u<<1,  /* voice_phase_inc = voice_phase_inc * inc_scale: ONE float multiply, unfused; a product that is
                                        not finite is not stored (the voice keeps its increment; counted in d_result[1]) */
       SKRED_CTL_AMP       = 1u<<2,  /* voice_amp = amp on voices whose voice_amp != 0.0f ON THE DEVICE; others keep 0 (counted) */
       SKRED_CTL_PAN       = 1u<<3,  /* voice_pan_left / _right */
       SKRED_CTL_FILTER    = 1u<<4,  /* voice_filter.b0 b1 b2 a1 a2 (coefficients as mmf_set_params made them; memory untouched) */
       SKRED_CTL_ENV_TIMES = 1u<<5,  /* attack_time, decay_time, sustain_level, release_time */
       SKRED_CTL_VELOCITY  = 1u<<6,
       SKRED_CTL_SMOOTHING = 1u<<7,  /* voice_smoother_smoothing */
       SKRED_CTL_FM_DEPTH  = 1u<<8, SKRED_CTL_FREQ_SCALE = 1u<<9, SKRED_CTL_AM_DEPTH = 1u<<10, SKRED_CTL_PAN_DEPTH = 1u<<11,
       SKRED_CTL_CZ_DEPTH  = 1u<<12, SKRED_CTL_CZ_DIST = 1u<<13 };
typedef struct skred_ctl { uint32_t set; float phase_inc, inc_scale, amp, pan_left, pan_right, b0, b1, b2, a1, a2,
                           attack_time, decay_time, sustain_level, release_time, velocity, smoothing,
                           fm_depth, freq_scale, am_depth, pan_depth, cz_depth, cz_dist; uint32_t reserved; } skred_ctl_t;  /* 96 bytes */

/* Pure host, no device: SKRED_OK, or what the two entry points refuse about the controller itself.  SKRED_E_RANGE: K not a power of
 * two in 1 .. 64.  SKRED_E_BAD_ARG: NULL ctl; a voice_mask that is 0 or has bits at or above K; and, in a record whose mask bit is
 * set: unknown bits in set, set == 0, reserved != 0, both PHASE_INC and INC_SCALE, a named value that is not finite, amp == 0 under
 * SKRED_CTL_AMP (a controller never silences a voice for good: the planner would not know).  Values a field does not name are not
 * looked at.  Negative amp, zero depths and zero times are accepted. */
int  skred_ctl_check(const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask);
/* The controller on every slot of [first, first + count): first and count multiples of K, inside the bank.  Asynchronous on `stream`:
 * the K records travel through the staging ring of skred_bank_update (`ctl` is free again on return), one kernel stores them,
 * nothing waits for the device.  d_result (device memory, uint32[2], may be NULL) is cleared on the stream ahead of the kernel:
 * [0] = voices written (masked voices of the range), [1] = stores withheld by the two guards above (AMP on a zero-amp voice, a
 * scaled increment that is not finite); both are sums, the same whatever the order of arrival.
 * Refused before anything touches the device: what skred_ctl_check refuses; SKRED_E_BAD_ARG for a NULL bank; SKRED_E_RANGE for
 * count < 0, a range outside the bank, first or count not a multiple of K.  count == 0: SKRED_OK, nothing is done. */
int  skred_bank_ctl_range(skred_bank_t *bank, const skred_ctl_t *ctl, int first, int count, int slot_voices, uint64_t voice_mask,
                          uint32_t *d_result, void *stream);
/* The controller on the first min(n, *d_count_or_null) slots of a list in device memory (NULL: n).  Entries that are no slot of the
 * bank -- negative, not a multiple of K, past the bank -- are skipped: skred_bank_stamp_slots' rules, so the d_assigned of a
 * skred_bank_note_on_idle_slots serves, -1 holes and all, as the list for "this chord only".  A slot named twice gets the same
 * absolute stores twice, which is the same as once and is counted twice in d_result; with SKRED_CTL_INC_SCALE its increment is
 * UNSPECIFIED (scaled once or twice), nothing else is affected.  d_result and the rest as for skred_bank_ctl_range.
 * Refused before anything touches the device: what skred_ctl_check refuses; SKRED_E_BAD_ARG for a NULL bank or list, n < 0 or
 * n > INT32_MAX / 64.  n == 0: SKRED_OK, nothing is done. */
int  skred_bank_ctl_slots(skred_bank_t *bank, const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask,
                          const int32_t *d_slots, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
/* The words a controller can store, as the device holds them, into the host view -- what skred_bank_download leaves out:
 * voice_phase_inc, voice_amp, the envelope's four times and velocity, voice_smoother_smoothing, the filter's five coefficients, the
 * four modulation depths / scale, voice_cz_mod_depth, voice_cz_distortion (and the pans, which skred_bank_download returns too).
 * Waits for the device, like skred_bank_download; windows as there. */
int  skred_bank_download_ctl(skred_bank_t *bank, skred_voice_bank_t *host, int src_first, int dst_first, int count);

/* ---- note owners: note-offs and controllers that cannot hit a stolen slot --------------------------------------------------
 *
 * A note-off is skred_bank_stamp_slots on an earlier d_assigned, "this chord only" is skred_bank_ctl_slots on one: both act on a
 * slot INDEX, and since the stealing calls exist that index may hold somebody else's note by the time the call arrives (chord A is
 * placed, the bank fills up, chord B steals A's slots, A's key is lifted: B is released).  A host that kept its own key -> slot map
 * would have to read every d_assigned back, one stream wait per burst.  These calls keep the answer on the device instead.
 *
 * owner[n_voices] is a uint32 array in device memory that only the calls of this section read or write.  The OWNER of a slot is the
 * word at the slot's FIRST voice (K = 1: the voice's own word; ranges of different K can live in one bank); 0 means "nobody".  The
 * bank allocates the array (4 bytes per voice) on the first call of this section other than _owner_clear and _download_owners and
 * zero-fills it; that first call waits for the device once, like the first query.  skred_bank_upload, _update, the renders, notes,
 * stamps, steals and controllers above never touch it, and no render kernel, probe, tap or report reads it: state, mix, reports
 * and form counters of every block are bit-identical to the same blocks without owner calls.
 *
 * The sequence of a MIDI-style host: draw a non-zero tag per note, place the burst with any of the six note-on calls, then
 * skred_bank_tag_slots(d_assigned, tags) on the same stream -- a thief's tags overwrite its victims'.  Note-off by id:
 * skred_bank_release_tags(tags); note-off or "this chord only" on a kept d_assigned: skred_bank_stamp_owned / _ctl_owned with the
 * tags the entries are expected to carry.  Tagged and untagged note-ons should not share a range: an untagged note that steals a
 * tagged slot leaves the victim's tag in place, and the victim's note-off would release it.
 * All calls are asynchronous on `stream` and ordered like skred_bank_update; host arrays travel through its staging ring, so the
 * caller's array is free on return and nothing waits for the device.  A slot, K = slot_voices and voice_mask mean what they mean for
 * skred_bank_notes_on_slots.  n == 0: SKRED_OK, nothing is done.  On a shard: through skred_shard_bank(), with that rank's local
 * indices.  The fixed-point bank has the same calls per voice (include/skred_amd_fxpt.h: skred_fxbank_tag_list / _find_owned /
 * _stamp_owned / _release_tags / _ctl_owned / _owner_clear / _download_owners), which share skred_owner_tags_check and the tag and
 * find kernels with these.  Not in the drop-in mode; deferred items and pattern steps carry no tags. */
#define SKRED_OWNER_MAX_TAGS 1024
enum { SKRED_OWNER_ALLOW_ZERO = 1u << 0,   /* tag 0 is accepted (skred_bank_tag_slots: it clears the owner) */
       SKRED_OWNER_UNIQUE     = 1u << 1 }; /* no tag twice and n <= SKRED_OWNER_MAX_TAGS (skred_bank_find_owned, _release_tags) */
/* Pure host, no device: SKRED_OK, or SKRED_E_BAD_ARG for NULL tags, n < 0, unknown flags, a zero tag without ALLOW_ZERO, and with
 * UNIQUE a tag that appears twice or n > SKRED_OWNER_MAX_TAGS.  Every entry point below calls it before anything touches the device. */
int  skred_owner_tags_check(const uint32_t *tags, int n, uint32_t flags);
/* owner[d_slots[k]] = tags[k] (host uint32[n]; 0 clears) for the first min(n, *d_count_or_null) entries (NULL: n) that are slots of
 * the bank -- skred_bank_stamp_slots' rule, so a d_assigned with its -1 holes is the natural argument right after a note-on call.
 * A slot named twice with different tags ends up with one of them, unspecified which.  d_result (device, uint32[2], may be NULL) is
 * cleared on the stream ahead of the kernel: [0] slots tagged, [1] entries of those first min(n, count) that are no slot.
 * SKRED_E_BAD_ARG: NULL bank, list or tags, n < 0 or n > INT32_MAX / 64; SKRED_E_RANGE: a bad K. */
int  skred_bank_tag_slots(skred_bank_t *bank, const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                          int slot_voices, uint32_t *d_result, void *stream);
/* d_slots_out[k] (device, int32[n]) = the LOWEST first voice of a slot of [first, first + count) whose owner equals tags[k], or -1.
 * tags: host uint32[n], 1 <= n <= SKRED_OWNER_MAX_TAGS, none zero, none twice.  The same state gives the same bytes, whatever order
 * the workgroups arrive in (an unsigned minimum); no workgroup waits for another.  SKRED_E_BAD_ARG: NULL bank, tags or d_slots_out,
 * what skred_owner_tags_check(UNIQUE) refuses; SKRED_E_RANGE: a bad K, first or count not a multiple of K, count <= 0, a range
 * outside the bank. */
int  skred_bank_find_owned(skred_bank_t *bank, int first, int count, int slot_voices, const uint32_t *tags, int n,
                           int32_t *d_slots_out, void *stream);
/* skred_bank_stamp_slots with a guard: entry k (of the first min(n, *d_count_or_null)) is stamped only if it is a slot of the bank
 * AND owner[slot] == tags[k]; tags are non-zero, so an untagged slot never matches.  The stores are skred_bank_stamp_slots'.
 * d_result (device, uint32[3], required) is cleared on the stream ahead of the kernel: [0] slots stamped, [1] slots whose owner
 * differs (the note was stolen or re-tagged), [2] entries that are no slot; sums, the same whatever the order of arrival.
 * SKRED_E_BAD_ARG: NULL bank, list, tags or result, n < 0 or n > INT32_MAX / 64, a zero tag, bad stamp bits, a bad voice_mask;
 * SKRED_E_RANGE: a bad K. */
int  skred_bank_stamp_owned(skred_bank_t *bank, const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                            int slot_voices, uint64_t voice_mask, uint32_t stamps, uint32_t *d_result, void *stream);
/* Note-off by note id: skred_bank_find_owned into scratch the bank owns, then skred_bank_stamp_owned on that list with the same
 * tags.  Each tag stamps at most ONE slot, the lowest that carries it, so the call lists at most n * popcount(voice_mask) voices
 * whatever the caller tagged.  d_result as for skred_bank_stamp_owned; [2] counts the tags nobody in the range carries, [1] is 0.
 * One stream at a time per bank, as for the queries.  Refusals of both calls. */
int  skred_bank_release_tags(skred_bank_t *bank, int first, int count, int slot_voices, uint64_t voice_mask, const uint32_t *tags,
                             int n, uint32_t stamps, uint32_t *d_result, void *stream);
/* skred_bank_ctl_slots under the same guard: the same stores, the same two withheld-store rules, the same motion-list rule, and a
 * controller that lists nobody leaves the planner's reports alone.  d_result (device, uint32[3], may be NULL): [0] voices written,
 * [1] stores withheld, [2] slots whose owner differs.  Refused: what skred_bank_ctl_slots refuses, NULL tags, a zero tag. */
int  skred_bank_ctl_owned(skred_bank_t *bank, const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                          const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
/* owner[first .. first + count) = 0 on `stream` (nothing to do on a bank that was never tagged).  SKRED_E_RANGE: count < 0 or a
 * range outside the bank. */
int  skred_bank_owner_clear(skred_bank_t *bank, int first, int count, void *stream);
/* The owner words of [first, first + count) into host_u32; waits for the device, like skred_bank_download; zeros on a bank that
 * was never tagged. */
int  skred_bank_download_owners(skred_bank_t *bank, uint32_t *host_u32, int first, int count);
/* The envelope clocks of [first, first + count) as the device holds them -- what skred_bank_download leaves out, and what a stamp
 * stores: sample_start and sample_release (either may be NULL).  Waits for the device, like skred_bank_download. */
int  skred_bank_download_env_clocks(skred_bank_t *bank, uint64_t *sample_start, uint64_t *sample_release, int first, int count);

/* ---- channels and per-note expression: masked owner matches, per-entry controller values -----------------------------------
 *
 * The owner word is 32 bits the host draws freely, so a part of it can name a CHANNEL: tag = channel << 24 | note id.  Parts that
 * share one stolen-from range then still have "all notes off on channel 3", "mod wheel on channel 3" and "how many notes does
 * channel 3 hold" -- without a list of every live tag on the host, which stealing would make wrong.  And a host that plays MPE,
 * polyphonic aftertouch or per-note bend gives n sounding notes n DIFFERENT values in one call instead of n calls.
 *
 * A slot, K = slot_voices and voice_mask mean what they mean for skred_bank_notes_on_slots; the owner array is the one of the
 * section above, allocated by the first call that needs it exactly as there.  All device calls are asynchronous on `stream` and
 * ordered like skred_bank_update; host arrays travel through its staging ring, so the caller's memory is free on return and nothing
 * waits for the device (skred_bank_find_match_host waits for its stream, and says so).  Results are pure functions of the state:
 * the same state gives the same bytes whatever order the workgroups arrive in.  One stream at a time per bank, as for the queries.
 * No render kernel, probe, tap or report reads anything these calls add; what the writing calls tell the planner is what their
 * unguarded twins tell it (below).
 * The fixed-point bank has the same calls per voice (include/skred_amd_fxpt.h: skred_fxbank_find_match / _stamp_match / _ctl_match /
 * _ctl_owned_each / _ctl_tags_each, with this section's skred_owner_match_t and SKRED_EACH_* bits).
 * Out of scope: the drop-in mode, deferred items and pattern steps (they carry no tags).  On a shard: through skred_shard_bank(), with that rank's local indices, and nothing beyond that.
 *
 * A. Masked owner matches.  A slot MATCHES m when owner != 0 && (owner & m->mask) == m->value: mask 0 with value 0 is every tagged
 * slot, mask 0xFF000000 a channel byte, mask 0xFFFFFFFF one note.  An untagged slot matches nothing. */
typedef struct { uint32_t value, mask; } skred_owner_match_t;
/* Pure host: SKRED_OK, or SKRED_E_BAD_ARG for NULL and for value & ~mask != 0 (a value no owner word can give). */
int  skred_owner_match_check(const skred_owner_match_t *m);
/* The first voices of the matching slots of [first, first + count), ascending, into d_slots[0 .. min(total, max_out)) (device,
 * int32); d_count[0] (device, uint32[1]) = the TOTAL number of matching slots, whether or not the list was cut short -- the count
 * word a later skred_bank_ctl_slots / _stamp_slots with n = max_out takes as it is.  max_out == 0: the count alone (d_slots may
 * be NULL).  Entries past min(total, max_out) are not written.  The compaction is the idle queries' (ordered by index, no
 * workgroup waits for another) and uses the same scratch.
 * SKRED_E_BAD_ARG: NULL bank, match or d_count, what skred_owner_match_check refuses, max_out < 0, NULL d_slots with max_out > 0;
 * SKRED_E_RANGE: a bad K, first or count not a multiple of K, count <= 0, a range outside the bank. */
int  skred_bank_find_match(skred_bank_t *bank, int first, int count, int slot_voices, const skred_owner_match_t *m, int max_out,
                           int32_t *d_slots, uint32_t *d_count, void *stream);
/* The same into host memory, waiting for `stream` ONLY (as skred_bank_find_idle_slots_host): returns the number of slots written
 * to slots[0 .. max_out) or a negative error; *total_out (may be NULL) = the total. */
int  skred_bank_find_match_host(skred_bank_t *bank, int first, int count, int slot_voices, const skred_owner_match_t *m, int max_out,
                                int32_t *slots, int *total_out, void *stream);
/* skred_bank_stamp_slots' stores on the voice_mask voices of EVERY matching slot of the range -- all notes off on a channel -- in one
 * pass over the range, with no list in between.  d_result (device, uint32[2], required) is cleared on the stream ahead of the
 * kernel: [0] slots stamped, [1] slots of the range that did not match.  The planner is told what skred_bank_stamp_slots on every
 * slot of the range would tell it: (count / K) * popcount(voice_mask) more voices may be on the motion list (the host cannot know
 * how many slots match; the bound only has to hold).
 * Refusals of skred_bank_find_match about bank, match and range; SKRED_E_BAD_ARG for a NULL d_result, bad stamp bits, a bad
 * voice_mask. */
int  skred_bank_stamp_match(skred_bank_t *bank, int first, int count, int slot_voices, uint64_t voice_mask, const skred_owner_match_t *m,
                            uint32_t stamps, uint32_t *d_result, void *stream);
/* skred_bank_ctl_range under the match guard: the same stores, the same two withheld-store rules, the same rule for which words put
 * a voice on the motion list -- on the matching slots only.  d_result (device, uint32[3], may be NULL): [0] voices written,
 * [1] stores withheld, [2] slots of the range that did not match.  The motion-list bound grows as for skred_bank_ctl_range on the
 * same range, and only when a record names AMP, ENV_TIMES, VELOCITY or SMOOTHING: a filter or pan sweep of a channel leaves the
 * planner's reports alone, and the block behind it stays the steady block.
 * Refused: what skred_ctl_check and skred_owner_match_check refuse, a NULL bank; SKRED_E_RANGE as for skred_bank_find_match. */
int  skred_bank_ctl_match(skred_bank_t *bank, const skred_ctl_t *ctl, int first, int count, int slot_voices, uint64_t voice_mask,
                          const skred_owner_match_t *m, uint32_t *d_result, void *stream);

/* B. Per-entry controller values.  skred_bank_ctl_owned stores ONE set of K records on all n listed notes; here entry k of the list
 * brings a small record of its own, whose named values replace or scale the records' for that entry alone:
 *   SKRED_EACH_INC_SCALE  voice_phase_inc = voice_phase_inc * inc_scale on every masked voice of the slot: the device's value, ONE
 *                         fp32 multiply, never fused; a product that is not finite is withheld and counted (SKRED_CTL_INC_SCALE's
 *                         rule).  Per-note pitch bend.
 *   SKRED_EACH_AMP_SCALE  needs record l of `ctl` to name SKRED_CTL_AMP: the amp stored on voice l is ctl[l].amp * amp_scale, ONE
 *                         fp32 multiply, never fused, under SKRED_CTL_AMP's device-side guard (a voice with amp 0 keeps it).  A
 *                         product that is zero or not finite is withheld and counted, and the voice's amp is left alone.
 *                         Polyphonic aftertouch on a patch whose voices differ in level.
 *   SKRED_EACH_VELOCITY   the entry's velocity replaces record l's, or supplies it where the record does not name the field.
 *   SKRED_EACH_PAN        the same for the pan pair.
 * Everything else a record names is stored as skred_bank_ctl_owned stores it.  `ctl` may be NULL: no base records, the entries
 * supply everything (AMP_SCALE is then refused). */
enum { SKRED_EACH_INC_SCALE = 1u << 0, SKRED_EACH_AMP_SCALE = 1u << 1, SKRED_EACH_VELOCITY = 1u << 2, SKRED_EACH_PAN = 1u << 3 };
typedef struct skred_ctl_each { uint32_t set; float inc_scale, amp_scale, velocity, pan_left, pan_right;
                                uint32_t reserved[2]; } skred_ctl_each_t;   /* 32 bytes */
/* Pure host: SKRED_OK, or what the two entry points refuse about the entries.  SKRED_E_RANGE: a bad K.  SKRED_E_BAD_ARG: NULL each,
 * n < 0, a bad voice_mask; with ctl != NULL what skred_ctl_check refuses; in an entry: unknown bits in set, set == 0, a reserved word
 * that is not 0, a named value that is not finite, amp_scale == 0 under AMP_SCALE; AMP_SCALE where ctl is NULL or a masked record
 * lacks SKRED_CTL_AMP; INC_SCALE where a masked record names SKRED_CTL_PHASE_INC or SKRED_CTL_INC_SCALE.  Values an entry does not
 * name are not looked at (and never shipped). */
int  skred_ctl_each_check(const skred_ctl_each_t *each, int n, const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask);
/* Entry k (of the first min(n, *d_count_or_null)) acts on d_slots[k] only if that is a slot of the bank AND owner[slot] == tags[k]
 * (non-zero); on that slot it performs skred_bank_ctl_owned's stores with each[k]'s replacements.  d_result (device, uint32[3], may
 * be NULL): [0] voices written, [1] stores withheld (the two guards and the products above), [2] slots whose owner differs.  A slot
 * named twice behaves as skred_bank_ctl_slots documents: absolute stores twice, a scaled increment UNSPECIFIED.  When an entry or a
 * record names a listing word (AMP_SCALE, VELOCITY; AMP, ENV_TIMES, VELOCITY, SMOOTHING) the motion-list bound grows by
 * n * popcount(voice_mask); otherwise the planner's reports are left alone.
 * Refused: what skred_ctl_each_check refuses, NULL bank, list or tags, a zero tag, n > INT32_MAX / 64.  n == 0: SKRED_OK. */
int  skred_bank_ctl_owned_each(skred_bank_t *bank, const skred_ctl_t *ctl, const skred_ctl_each_t *each, int slot_voices,
                               uint64_t voice_mask, const int32_t *d_slots, const uint32_t *tags, int n,
                               const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
/* Expression by note id: skred_bank_find_owned of the tags over [first, first + count) into scratch the bank owns, then the call
 * above on that list -- built as skred_bank_release_tags is.  each[k] goes with tags[k]: the tags travel sorted, and the entries
 * are permuted with them on the host.  Tags unique, none zero, n <= SKRED_OWNER_MAX_TAGS; each tag reaches at most ONE slot, the
 * lowest that carries it.  d_result as above; [2] is 0 (a tag nobody carries is a -1 entry and is not counted).
 * Refusals of both calls. */
int  skred_bank_ctl_tags_each(skred_bank_t *bank, const skred_ctl_t *ctl, const skred_ctl_each_t *each, int first, int count,
                              int slot_voices, uint64_t voice_mask, const uint32_t *tags, int n, uint32_t *d_result, void *stream);

/* C. Per-note timbre: per-entry filter coefficients.  The two calls of B with one more array: entry k also brings ONE set of biquad
 * coefficients, stored on every voice l of its slot that has bit l of filter_mask set -- key tracking, velocity-to-cutoff, MPE
 * timbre (CC 74) on a patch whose voices are filtered, n notes with n cutoffs in one call.  The words are SKRED_CTL_FILTER's:
 * voice_filter.b0 b1 b2 a1 a2 = filt[k]; the filter memory (x1 x2 y1 y2) is untouched, and a voice whose filter is bypassed keeps
 * the words without reading them.  Entry k acts exactly as it does in B (a valid slot whose owner is tags[k]); the records of `ctl`
 * and the values of each[k] are stored as there, under the same two withheld-store rules and the same listing rule.  `each` may be
 * NULL here: the coefficients only; `ctl` may be NULL as in B.  d_result keeps its three words; a voice written only through
 * filter_mask counts in [0] once, like any written voice (filter_mask is a subset of voice_mask, and [0] counts the voices of
 * voice_mask).  FILTER is not a listing word: a call whose records and entries name none leaves the planner's reports alone, and
 * the block behind it is the steady block.  One set per entry: voices of one slot that need different coefficients take a record
 * of `ctl` each (SKRED_CTL_FILTER) on the lanes outside filter_mask.
 * Out of scope: the drop-in mode, deferred items and pattern steps.  Coefficients computed on the device: the section "filter cutoff
 * on the device" below.  On a shard: through
 * skred_shard_bank(), with that rank's local indices.  The fixed-point bank has the twin (include/skred_amd_fxpt.h:
 * skred_fxbank_ctl_owned_each_filter / _ctl_tags_each_filter). */
typedef struct skred_filter_each { float b0, b1, b2, a1, a2; uint32_t reserved[3]; } skred_filter_each_t;   /* 32 bytes, reserved 0 */
/* Pure host: SKRED_OK, or what the two entry points refuse about the coefficients.  SKRED_E_RANGE: a bad K.  SKRED_E_BAD_ARG: NULL
 * filt, n < 0, a bad voice_mask, filter_mask == 0 or with a bit outside voice_mask; with ctl != NULL what skred_ctl_check refuses,
 * and a record l with bit l in filter_mask that itself names SKRED_CTL_FILTER (two sets of coefficients for one voice: ambiguous,
 * as INC_SCALE against PHASE_INC is); in an entry: a reserved word that is not 0, a coefficient that is not finite. */
int  skred_filter_each_check(const skred_filter_each_t *filt, int n, const skred_ctl_t *ctl_or_null, int slot_voices,
                             uint64_t voice_mask, uint64_t filter_mask);
/* skred_bank_ctl_owned_each with filt[k] beside each[k].  The three arrays and the tags travel through the staging ring in one
 * batch; one kernel reads them.  Refused: what skred_bank_ctl_owned_each refuses (a NULL `each` excepted) and what
 * skred_filter_each_check refuses.  n == 0: SKRED_OK. */
int  skred_bank_ctl_owned_each_filter(skred_bank_t *bank, const skred_ctl_t *ctl_or_null, const skred_ctl_each_t *each_or_null,
                                      const skred_filter_each_t *filt, int slot_voices, uint64_t voice_mask, uint64_t filter_mask,
                                      const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                                      uint32_t *d_result, void *stream);
/* skred_bank_ctl_tags_each with filt[k] beside tags[k]: the tags travel sorted, and filt is permuted on the host with each by the
 * same permutation.  Refusals of skred_bank_ctl_tags_each (a NULL `each` excepted) and of skred_filter_each_check. */
int  skred_bank_ctl_tags_each_filter(skred_bank_t *bank, const skred_ctl_t *ctl_or_null, const skred_ctl_each_t *each_or_null,
                                     const skred_filter_each_t *filt, int first, int count, int slot_voices, uint64_t voice_mask,
                                     uint64_t filter_mask, const uint32_t *tags, int n, uint32_t *d_result, void *stream);
/* The coefficients of one filter setting, pure host: the arithmetic of the drop-in mode's mmf_set_params (RBJ cookbook, fp32, the
 * operations in its order; skred_synth_dropin.c calls this function) with the sample rate as an argument, so that a host computes
 * key-tracked coefficients without a voice array.  mode: 1 low-pass, 2 high-pass, 3 band-pass, 4 notch, 5 all-pass; any other
 * non-zero mode is low-pass, as there.  out5 = b0 b1 b2 a1 a2.  Returns SKRED_OK; 1 for mode 0 (bypass: nothing is computed and out5
 * is left as it is, as mmf_set_params leaves the voice's words); SKRED_E_BAD_ARG for a NULL out5.  The arguments are not judged: a
 * resonance of 0 gives coefficients that are not finite, which skred_filter_each_check refuses. */
int  skred_filter_coeffs(int mode, float freq, float resonance, float sample_rate, float out5[5]);

/* ---- channel polyphony: stealing inside one channel, note-ons under a cap ---------------------------------------------------
 *
 * A channel can be swept, bent and silenced (the section above); these calls let it ALLOCATE.  skred_bank_find_steal_slots ranks
 * every sounding slot of a range, whoever owns it -- a burst on the pad channel takes the bass line's notes -- and nothing limits
 * how many slots a channel holds.  The host cannot enforce a limit: the number of sounding slots of a channel is device state.
 *
 * Slots, K, member_mask, live, released, age, idle, class, primary and key mean what skred_slot_steal_query_t defines;
 * match(o) := o != 0 && (o & m.mask) == m.value is skred_owner_match_t's rule; a slot's owner is the word at its first voice.  On
 * the fields AS THE DEVICE HOLDS THEM at that point of the stream, every comparison exact:
 *   sounding(slot)  := slot inside the range && match(owner[slot]) && some member is live
 *                      && NOT (exclude_idle != 0 && every member is idle)
 *   candidate(slot) := sounding(slot) && every live member has age >= min_age
 *                      && (with RELEASED_ONLY: every live member is released)
 * Victim order as before: ascending key, ties by ascending first voice.  An untagged slot (owner 0) is never sounding in this sense:
 * it is neither counted nor stolen.  A slot that does not match costs one owner word and no plane read.
 *
 * skred_bank_find_steal_slots under its contract (asynchronous, reads the bank and the owner array only, the same state gives the
 * same bytes, the bank's steal scratch -- one stream at a time --, no workgroup ever waits for another), restricted to the match:
 * d_slots[0 .. written) = the first min(total, max_out) victims, d_count (device, uint32[3]): [0] written, [1] total candidates,
 * [2] the sounding slots of the match in the range -- the channel's current polyphony.  max_out == 0: a census of the channel in
 * one launch.  With mask == 0 and every sounding slot tagged the list and d_count[0..1] are skred_bank_find_steal_slots' bytes.
 * Refused before anything touches the device: what skred_slot_steal_check and skred_owner_match_check refuse, and SKRED_E_BAD_ARG
 * for a NULL bank, query or d_count, or a NULL d_slots with max_out > 0. */
int  skred_bank_find_steal_slots_match(skred_bank_t *bank, const skred_slot_steal_query_t *q, const skred_owner_match_t *m,
                                       int32_t *d_slots, uint32_t *d_count, void *stream);
/* The same into host memory; waits for `stream` only.  Returns `written` (>= 0) or a SKRED_E_* code; *total_out and *sounding_out
 * may be NULL. */
int  skred_bank_find_steal_slots_match_host(skred_bank_t *bank, const skred_slot_steal_query_t *q, const skred_owner_match_t *m,
                                            int32_t *slots, int *total_out, int *sounding_out, void *stream);
/* A burst of n patch notes of ONE channel under a polyphony cap: skred_bank_note_on_steal_slots with three differences, all decided
 * on the device.  With I = idle slots listed by idle_q (at most n), S = the channel's sounding count (d_count[2] of the matched
 * query above, run with steal_q and m) and V = the victims that query wrote:
 *   a = min(n, I, cap > S ? cap - S : 0)   notes take the first a idle slots            (idle slots are limited by the cap),
 *   b = min(n - a, V)                      notes take the channel's victims, in victim order (stealing stays inside the channel),
 *   the remaining n - a - b notes are dropped whole,
 * and note k's slot gets owner = tags[k], as skred_bank_tag_slots on d_assigned would write it (every placed note is tagged; a
 * thief's tag overwrites its victim's).  d_result (device, uint32[4], required): [0] placed, [1] dropped, [2] stolen (b), [3] S as
 * seen before the burst.  d_assigned as for skred_bank_notes_on_slots.
 * Consequences: a channel at or below its cap never exceeds it; a channel above a lowered cap does not grow (a = 0: every note
 * steals one of its own); a burst cannot steal from itself (both lists are made before a note is placed, and they are disjoint);
 * cap = 1 with min_age = 0 is mono mode -- the new note takes the old one's slot; SKRED_CHAN_NO_CAP never limits.  Victims come from
 * the channel only: there is no bank-wide fallback here -- a host that wants one calls skred_bank_note_on_steal_slots.
 * The library overrides steal_q's exclude_idle, settle_level and max_out as skred_bank_note_on_steal_slots does.  Five steps on
 * `stream`: the idle query, the matched key pass and its select, one one-workgroup join kernel, the slot-note launch, the owner-tag
 * launch.  The motion-list bound grows by n * popcount(voice_mask); the host never learns the counts and waits for nothing.
 * skred_chan_check is the pure-host statement of what is refused before anything touches the device: what
 * skred_slot_query_check (with max_out = n), skred_slot_steal_check (with the overrides) and skred_owner_match_check refuse;
 * SKRED_E_BAD_ARG for a NULL query, n < 0, SKRED_IDLE_AMP_ZERO in idle_q->which, queries that differ in slot_voices or
 * member_mask, NULL tags, n > INT32_MAX / 64, a tag that is 0 or does not satisfy m (such a note would not count towards its own
 * channel).  Every cap is accepted.  The entry point also refuses a NULL bank, notes or d_result and what skred_slot_notes_check
 * refuses.  n == 0: SKRED_OK, nothing is done.  On a shard: through skred_shard_bank(), with that rank's local indices.
 * The fixed-point bank has the same calls per voice (include/skred_amd_fxpt.h: skred_fxbank_find_steal_match / _find_steal_match_host /
 * _note_on_channel, skred_fx_chan_check).  Not built here (out of scope): shards beyond skred_shard_bank(), the drop-in mode, deferred
 * items and pattern steps. */
#define SKRED_CHAN_NO_CAP 0xFFFFFFFFu
int  skred_chan_check(const skred_slot_query_t *idle_q, const skred_slot_steal_query_t *steal_q, const skred_owner_match_t *m,
                      uint32_t cap, const uint32_t *tags, int n, int n_voices);
int  skred_bank_note_on_channel(skred_bank_t *bank, const skred_slot_query_t *idle_q, const skred_slot_steal_query_t *steal_q,
                                const skred_owner_match_t *m, uint32_t cap, const skred_note_t *notes, const uint32_t *tags, int n,
                                uint64_t voice_mask, int32_t *d_assigned, uint32_t *d_result, void *stream);

/* ---- pedals: sustain and sostenuto hold note-offs back on the device --------------------------------------------------------
 *
 * Under a sustain pedal (MIDI CC 64) a note-off is remembered per sounding note and executed when the pedal goes up; the sostenuto
 * pedal (CC 66) does the same for the notes that were held down when IT went down.  Which slot holds a note is device state (notes
 * land on idle slots and steal slots there), so a host that kept its own list of pending note-offs would release the wrong note
 * after a theft, and would need a read-back behind a stream wait on every pedal-up.  These calls keep the pedal state beside the
 * owner word instead.
 *
 * pedal[n_voices] is a uint32 array in device memory that only the calls of this section read or write; a slot's word is the word at
 * its FIRST voice.  SKRED_PEDAL_PENDING: a note-off arrived and was held back.  SKRED_PEDAL_LATCHED: sostenuto caught this note.
 * The bank allocates the array (4 bytes per voice) behind the owner array on the first call of this section other than _pedal_clear
 * and _download_pedals and zero-fills it; that call waits for the device once, as the first owner call does.  No render kernel, probe,
 * tap, report or planner rule reads the word: blocks rendered with and without pedal calls that hold nothing are bit-identical.
 *
 * A NEW NOTE CLEARS THE WORD.  The natural tag is channel << 24 | key, and keys are struck again: once the array exists, every tag
 * launch of the bank (skred_bank_tag_slots, the tags of skred_bank_note_on_channel) is followed on its stream by a launch that stores
 * 0 into the pedal word of every slot it tagged -- the same list, the same min(n, *d_count) rule, the same "is a slot" rule.  So a
 * thief's tag call clears its victim's bits, and a key struck again under the pedal (the same slot in the same block in mono mode)
 * starts clean: the pedal-up releases the old note-off's slot only if the old note is still the one that sounds there.  A bank that
 * never made a pedal call launches nothing more.
 *
 * All calls are asynchronous on `stream` and ordered like skred_bank_update; host arrays travel through its staging ring; nothing
 * waits for the device; results are pure functions of the state, whatever the order of arrival; one stream at a time per bank.  A
 * slot, K = slot_voices, voice_mask, tags and matches mean what they mean in the three sections above.
 *
 * Stated behaviour: a pending note ranks in the steal queries as the held note it is (its envelope has no release clock).
 * skred_bank_stamp_match / _release_tags / _stamp_owned on a pending slot stamp at once and LEAVE the bit: a later pedal_up stamps
 * again, as a second amp_envelope_release of the reference would -- "all notes off" under a pedal is therefore skred_bank_pedal_up or
 * _pedal_clear first.  Tagged and untagged note-ons still must not share a range.
 * The fixed-point bank's twin of these calls is include/skred_amd_fxpt.h's section of the same name (skred_fxbank_stamp_owned_pedal ..
 * skred_fxbank_download_pedals), on these constants.  Not built here: the drop-in mode, deferred items and pattern steps, shards
 * beyond skred_shard_bank(). */
enum { SKRED_PEDAL_PENDING = 1u << 0, SKRED_PEDAL_LATCHED = 1u << 1 };
enum { SKRED_PEDAL_LIFT_SUSTAIN = 1u << 0,     /* the sustain pedal goes up */
       SKRED_PEDAL_LIFT_SOSTENUTO = 1u << 1,   /* the sostenuto pedal goes up */
       SKRED_PEDAL_SUSTAIN_DOWN = 1u << 2 };   /* sostenuto lifts while sustain stays down: pending notes stay pending */
enum { SKRED_PEDAL_CALL_STAMP_OWNED = 0, SKRED_PEDAL_CALL_RELEASE_TAGS, SKRED_PEDAL_CALL_LATCH, SKRED_PEDAL_CALL_UP };
/* Pure host, no device: what the entry point named by `call` refuses about everything but its pointers to the bank, the list and the
 * result, in the order it checks.  Arguments a call does not take are not looked at (STAMP_OWNED: first, count, m, flags;
 * RELEASE_TAGS: m, flags; LATCH: tags, n, flags; UP: tags, n).
 *   STAMP_OWNED   SKRED_E_BAD_ARG: NULL tags, n < 0, a zero tag, n > INT32_MAX / 64, a bad voice_mask; SKRED_E_RANGE: a bad K.
 *   RELEASE_TAGS  SKRED_E_BAD_ARG: what skred_owner_tags_check(UNIQUE) refuses, a zero tag, a bad voice_mask; SKRED_E_RANGE: a bad K,
 *                 first or count not a multiple of K, count <= 0, a range outside the bank of n_voices voices.
 *   LATCH         SKRED_E_BAD_ARG: what skred_owner_match_check refuses, a bad voice_mask; SKRED_E_RANGE as above.
 *   UP            the same, and SKRED_E_BAD_ARG for flags with unknown bits, without a LIFT bit, or with SUSTAIN_DOWN and LIFT_SUSTAIN.
 * An unknown `call`: SKRED_E_BAD_ARG.  Every entry point below calls it before anything touches the device; a refused call writes
 * nothing. */
int  skred_pedal_check(int call, int n_voices, int first, int count, int slot_voices, uint64_t voice_mask, const skred_owner_match_t *m,
                       uint32_t flags, const uint32_t *tags, int n);
/* skred_bank_stamp_owned with the stamp fixed to SKRED_STAMP_RELEASE and one more decision per entry whose owner equals its tag:
 * hold_all != 0 (the host knows the channel's sustain pedal is down) or a LATCHED slot -> pedal[slot] |= PENDING and nothing is
 * stamped; otherwise the slot is stamped exactly as skred_bank_stamp_owned stamps it.  d_result (device, uint32[4], required) is
 * cleared on the stream ahead of the kernel: [0] slots stamped, [1] slots whose owner differs, [2] entries that are no slot,
 * [3] slots held back.  A slot named twice ends with the same word and the same clocks as named once; it is counted twice.  With
 * hold_all == 0 on a bank where nothing is latched, the bank's bytes and words 0..2 are skred_bank_stamp_owned's.  The motion-list
 * bound grows by n * popcount(voice_mask).  n == 0: SKRED_OK, nothing is done.
 * Refused: NULL bank, list or result, what skred_pedal_check(STAMP_OWNED) refuses. */
int  skred_bank_stamp_owned_pedal(skred_bank_t *bank, const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                                  int slot_voices, uint64_t voice_mask, int hold_all, uint32_t *d_result, void *stream);
/* Note-off by note id under the pedals: skred_bank_release_tags' find pass into the same scratch -- each tag reaches at most ONE
 * slot, the lowest of [first, first + count) that carries it -- then the call above on that list.  d_result as above; [2] counts the
 * tags nobody in the range carries, [1] is 0.  Refused: NULL bank or result, what skred_pedal_check(RELEASE_TAGS) refuses. */
int  skred_bank_release_tags_pedal(skred_bank_t *bank, int first, int count, int slot_voices, uint64_t voice_mask, const uint32_t *tags,
                                   int n, int hold_all, uint32_t *d_result, void *stream);
/* Sostenuto down, in one pass over the range, no list: a slot that matches m gets LATCHED when its PENDING bit is clear AND at least
 * one voice_mask voice is HELD -- voice_use_amp_envelope != 0 && is_active != 0 && sample_release == 0, the terms live and released of
 * skred_slot_steal_query_t, on the fields as the device holds them at that point of the stream.  Notes struck later are not caught
 * (their tag launch clears the word), nor notes whose note-off is already pending.  d_result (device, uint32[2], required) is
 * cleared on the stream ahead of the kernel: [0] slots that satisfy the rule (latched now or before), [1] slots of the range that
 * did not match.  Reads the planes and writes the pedal array only: the planner is told nothing.
 * Refused: NULL bank or result, what skred_pedal_check(LATCH) refuses. */
int  skred_bank_pedal_latch(skred_bank_t *bank, int first, int count, int slot_voices, uint64_t voice_mask, const skred_owner_match_t *m,
                            uint32_t *d_result, void *stream);
/* A pedal goes up, in one pass over the matching slots of the range.  flags: at least one of LIFT_SUSTAIN and LIFT_SOSTENUTO;
 * SUSTAIN_DOWN (the host says sustain stays down while sostenuto lifts) is refused together with LIFT_SUSTAIN.  With LIFT_SOSTENUTO
 * the slot's LATCHED bit is cleared.  A slot that is then PENDING, not LATCHED and not kept by SUSTAIN_DOWN gets skred_bank_stamp_slots'
 * SKRED_STAMP_RELEASE on its voice_mask voices, and its PENDING bit is cleared: the release clock is this call's, not the note-off's.
 * d_result (device, uint32[3], required) is cleared on the stream ahead of the kernel: [0] slots released, [1] slots still pending
 * after the call, [2] slots of the range that did not match.  The planner is told what skred_bank_stamp_match on the same range
 * tells it: (count / K) * popcount(voice_mask) more voices may be on the motion list.
 * Refused: NULL bank or result, what skred_pedal_check(UP) refuses. */
int  skred_bank_pedal_up(skred_bank_t *bank, int first, int count, int slot_voices, uint64_t voice_mask, const skred_owner_match_t *m,
                         uint32_t flags, uint32_t *d_result, void *stream);
/* pedal[first .. first + count) = 0 on `stream` (nothing to do on a bank without a pedal array).  SKRED_E_RANGE: count < 0 or a
 * range outside the bank. */
int  skred_bank_pedal_clear(skred_bank_t *bank, int first, int count, void *stream);
/* The pedal words of [first, first + count) into host_u32; waits for the device, like skred_bank_download; zeros on a bank without
 * a pedal array. */
int  skred_bank_download_pedals(skred_bank_t *bank, uint32_t *host_u32, int first, int count);

/* ---- portamento: pitch glides that advance and land on the device ---------------------------------------------------------
 *
 * A glide moves a voice's voice_phase_inc towards a TARGET increment by one fp32 multiply per 64 frames and stores the target's bits
 * when it gets there: portamento between two keys of a mono lead (MIDI CC 5 / 65 / 84), a slide into a chord.  The reference stores
 * voice_glissando_enable / _speed / _target and never reads them, so the behaviour is defined here.  The host-driven route -- one
 * skred_bank_ctl_tags_each(SKRED_EACH_INC_SCALE) per block -- needs a host that counts blocks per note, and never lands: repeated
 * multiplies do not arrive at the note-on's increment bit for bit.  For device-placed notes the host does not know the increment at
 * all; the glide's state lies where the increment lives.
 *
 * glide[n_voices] is an array of four words PER VOICE (one uint4: target, rate_up, rate_down as fp32 bit patterns, carry as an
 * integer) in device memory that only the calls of this section read or write.  target == 0 (all bits) means "not gliding".  The bank
 * allocates the array (16 bytes per voice) behind the owner array on the first skred_bank_glide_owned / _glide_tags call and
 * zero-fills it; that call waits for the device once, as the first owner call does.  No render kernel, report, probe, tap or planner
 * rule reads the array, and a glide stores nothing but finite increments, which is all the planner looks at (SKRED_CTL_INC_SCALE's
 * argument): blocks rendered with and without glide calls that move nothing are bit-identical, and a glide call leaves the planner's
 * reports alone.  A bank that never starts a glide launches nothing more and allocates nothing.
 *
 * ADVANCE BY F FRAMES (skred_bank_glide_advance), for every gliding voice of a range, with inc = voice_phase_inc as the device holds
 * it:
 *   0. inc zero, not finite, or of the other sign than the target: the voice ARRIVES at once (a glide cannot cross zero).
 *   1. c = carry + F, m = c >> 6, carry = c & 63.
 *   2. m times, stopping at arrival:  |inc| < |target|: inc = inc * rate_up (ONE fp32 multiply, round to nearest, never fused); the
 *      voice arrives if the product is not finite or |inc| >= |target|.  |inc| > |target|: inc = inc * rate_down; it arrives if the
 *      product is not finite or |inc| <= |target|.  |inc| == |target|: it arrives.
 *   3. on arrival inc = target (the bits) and the voice's four words are cleared.
 * So the pass stores only finite products or the target; the rates are per 64 frames, and the increments at every multiple of 64
 * frames do not depend on how the host cuts its blocks; the loop runs at most F / 64 + 1 times.  The glide moves ONCE PER BLOCK, as
 * every control of the reference does: steps of 11.6 ms at 512 frames, 1.5 ms at 64.  Per-frame glides are not part of this.
 *
 * A NEW NOTE CLEARS THE WORDS.  Once the array exists, every tag launch of the bank (skred_bank_tag_slots, the tags of
 * skred_bank_note_on_channel) is followed on its stream by a launch that zeroes the glide words of all K voices of every slot it
 * tagged (the pedal word's rule): a thief or a key struck again does not inherit its victim's glide.  The order for mono legato is
 * therefore skred_bank_note_on_channel, then skred_bank_glide_tags(SKRED_GLIDE_FROM_SCALE).  On a bank that has a pedal array too
 * the tag kernel, the pedal clear and the glide clear run in that order inside one staged batch; each clear reads the list and the
 * count word only, so neither depends on the other.
 *
 * A RELEASE LEAVES THE WORDS ALONE.  A note-off (by list, by note id, by match) and a pedal-up stamp the envelope and touch nothing
 * else: a released note and a note whose note-off is pending glide on, through the tail, until the glide arrives, a tag launch takes
 * the slot or skred_bank_glide_stop ends it.  skred_bank_pedal_latch reads HELD from the envelope alone: a gliding note is latched
 * like any other.  The steal queries rank a gliding slot by its envelope clocks, as they rank a pending one.
 *
 * All calls are asynchronous on `stream` and ordered like skred_bank_update; host arrays travel through its staging ring, so the
 * caller's memory is free on return; nothing waits for the device but the download and the first allocation; one stream at a time per
 * bank.  A slot, K = slot_voices, voice_mask and tags mean what they mean in the sections above.
 *
 * Limits: glides belong with tagged notes.  A SKRED_CTL_PHASE_INC / _INC_SCALE bend of a gliding voice is undone on arrival (the
 * target's bits are stored): bend the target with SKRED_GLIDE_TO_SCALE, or bend with the calls of the pitch-wheel section below, which
 * a glide carries to its target.  The host view of voice_phase_inc goes stale, as for
 * SKRED_CTL_INC_SCALE; skred_bank_download_ctl reads it back.  On a shard: through skred_shard_bank(), with that rank's local indices.
 * This section is the float bank's alone: a fixed-point twin of these calls is a follow-up.  Also out of scope: the drop-in mode (it
 * keeps voice_glissando_* as dead data), deferred items and pattern steps. */
enum { SKRED_GLIDE_FROM_SCALE = 1u << 0,   /* target = inc (the pitch a note-on just stored), then inc = inc * scale: slide INTO the note
                                              from the previous key; the host needs the ratio of two keys, never an increment */
       SKRED_GLIDE_TO_SCALE = 1u << 1 };   /* target = (gliding ? the old target : inc) * scale, inc stays: legato onto a new key without
                                              a retrigger; a chain of them composes on the intended notes */
typedef struct skred_glide { uint32_t set; float rate_up, rate_down, scale; uint32_t reserved[4]; } skred_glide_t;   /* 32 bytes */
/* Pure host: SKRED_OK, or what the two starting calls refuse about the entries, in this order.  SKRED_E_BAD_ARG: a NULL array, n < 0;
 * SKRED_E_RANGE: a bad K (not a power of two in 1 .. 64); SKRED_E_BAD_ARG: a voice_mask that is 0 or has bits at or above K; in an
 * entry: set that is not exactly one of the two bits, a reserved word that is not 0, a value that is not finite, rate_up <= 1,
 * rate_down >= 1 or <= 0, scale <= 0. */
int  skred_glide_check(const skred_glide_t *glide, int n, int slot_voices, uint64_t voice_mask);
/* Entry k (of the first min(n, *d_count_or_null)) acts on d_slots[k] only if that is a slot of the bank AND owner[slot] == tags[k]
 * (non-zero): it starts glide[k]'s glide on every voice_mask voice of the slot -- the words above, carry = 0.  Either product is ONE
 * unfused fp32 multiply; where the product or inc is zero or not finite the start is withheld and counted, and the voice (its
 * increment and its glide words) is left exactly as it was.  d_result (device, uint32[3], may be NULL; cleared on the stream ahead of
 * the kernel): [0] voices set gliding, [1] starts withheld, [2] slots whose owner differs.  A slot named twice: UNSPECIFIED.  The
 * planner is told nothing.
 * Refused: NULL bank, list or tags, a zero tag, n > INT32_MAX / 64, what skred_glide_check refuses.  n == 0: SKRED_OK. */
int  skred_bank_glide_owned(skred_bank_t *bank, const skred_glide_t *glide, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                            const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
/* Glides by note id: skred_bank_find_owned of the tags over [first, first + count) into scratch the bank owns, then the call above
 * on that list -- built as skred_bank_ctl_tags_each is.  glide[k] goes with tags[k]: the tags travel sorted, the entries are permuted
 * with them on the host.  Tags unique, none zero, n <= SKRED_OWNER_MAX_TAGS; each tag reaches at most ONE slot, the lowest that
 * carries it.  d_result as above; [2] is 0.  Refusals of both calls; SKRED_E_RANGE: first or count not a multiple of K, count <= 0,
 * a range outside the bank. */
int  skred_bank_glide_tags(skred_bank_t *bank, const skred_glide_t *glide, int first, int count, int slot_voices, uint64_t voice_mask,
                           const uint32_t *tags, int n, uint32_t *d_result, void *stream);
/* The advance pass above over the voices [first, first + count): purely per voice, no K.  d_result (device, uint32[2], may be NULL;
 * cleared on the stream ahead of the kernel): [0] voices still gliding after the pass, [1] voices that arrived in it.  The host calls
 * it ahead of each render on the ranges of the channels that have portamento on; a lazily read [0] == 0 tells it to stop.  A voice
 * that does not glide costs one 16-byte load.  On a bank without a glide array: SKRED_OK, d_result (if given) is cleared on the
 * stream, nothing is launched.
 * SKRED_E_BAD_ARG: NULL bank, num_frames outside 1 .. 65536; SKRED_E_RANGE: count <= 0 or a range outside the bank. */
int  skred_bank_glide_advance(skred_bank_t *bank, int first, int count, int num_frames, uint32_t *d_result, void *stream);
/* The glide words of [first, first + count) are cleared on `stream`; with snap != 0 a gliding voice's increment is set to its target
 * first.  Nothing to do on a bank without a glide array.  SKRED_E_RANGE: count < 0 or a range outside the bank. */
int  skred_bank_glide_stop(skred_bank_t *bank, int first, int count, int snap, void *stream);
/* The glide words of [first, first + count) into host_u32x4 (4 * count words: target, rate_up, rate_down, carry per voice); waits
 * for the device, like skred_bank_download_owners; zeros on a bank that never started a glide. */
int  skred_bank_download_glide(skred_bank_t *bank, uint32_t *host_u32x4, int first, int count);

/* ---- pitch wheel: bends that return to the key's bits and compose with glides -----------------------------------------------
 *
 * SKRED_CTL_INC_SCALE / SKRED_EACH_INC_SCALE multiply the increment the device holds, and that is all a host can do to a note it did
 * not place itself.  As a pitch wheel the route has three defects.  A bend never comes back: up by r and back by 1 / r leaves
 * fl(fl(inc * r) * fl(1 / r)), which is not inc for most values, and after a few hundred wheel messages every note of the channel is
 * detuned against a freshly struck note on the same key.  Bends are relative: the host has to remember the last wheel position per
 * channel and send ratios of ratios, and a note stolen and struck again between two messages gets the wrong one.  And a bend of a
 * gliding voice is undone on arrival (the portamento section's limits).  The calls of this section keep the KEY's increment beside
 * the one the oscillator reads and derive the sounding increment as key * ratio with one multiply, every time.
 *
 * bend[n_voices] is an array of two words PER VOICE (one uint2: key, ratio -- fp32 bit patterns) in device memory that only the calls
 * of this section and the glide kernels read or write.  key == 0 (all bits) means "not bent".  The bank allocates the array (8 bytes
 * per voice, behind the glide array in the bank's record; the owner array first, when no owner call came before) on the first
 * skred_bank_bend_match / _bend_owned_each / _bend_tags_each call and zero-fills it; that call waits for the device once, as the
 * first owner, pedal and glide calls do.  No render kernel, report, probe, tap or planner rule reads the array, and a bend stores
 * nothing but finite non-zero increments (SKRED_CTL_INC_SCALE's argument): blocks rendered with and without bend calls that move
 * nothing are bit-identical, and a bend call leaves the planner's reports alone.  A bank that never bends launches nothing more and
 * allocates nothing.
 *
 * ABSOLUTE BEND of voice v to ratio r, with inc = voice_phase_inc as the device holds it:
 *   1. k = key[v] ? key[v] : inc -- the first bend captures the key.
 *   2. r's bits are those of 1.0f: inc = k is stored, but only if key[v] != 0, and both words are cleared.  The wheel at centre
 *      restores the key's bits and leaves no state.
 *   3. otherwise p = k * r, ONE fp32 multiply, round to nearest, never fused.  k zero or not finite, or p zero or not finite: the
 *      bend is WITHHELD and counted, and the voice and its words stay exactly as they were.  Else inc = p, key[v] = k, ratio[v] = r.
 * The ratio is absolute: the host sends the wheel's position, never a ratio of positions, and the same message twice is the same
 * bits twice.  A voice counts as stored or restored when step 3 stored it or step 2 found key[v] != 0.
 *
 * A NEW NOTE CLEARS THE WORDS.  Once the array exists, every tag launch of the bank (skred_bank_tag_slots, the tags of
 * skred_bank_note_on_channel) is followed on its stream by a launch that zeroes the bend words of all K voices of every slot it
 * tagged -- the pedal and glide rule, beside their two clears in one staged batch; each clear reads the list and the count word
 * only.  Without it a thief's first bend would restore its victim's key.  A note struck under a deflected wheel is therefore
 * skred_bank_note_on_channel, then skred_bank_bend_tags_each with the channel's current ratio, then -- optionally, last --
 * skred_bank_glide_tags(SKRED_GLIDE_FROM_SCALE).
 *
 * GLIDES UNDER A BEND.  On a bank with a bend array the glide calls read it: on a voice with key != 0 every place the portamento
 * section says inc reads and writes KEY instead -- skred_bank_glide_owned / _tags with FROM_SCALE: target = key, key = key * scale;
 * with TO_SCALE: target = (gliding ? the old target : key) * scale, key stays; skred_bank_glide_advance: the step loop runs on key,
 * and on arrival key = the target's bits; skred_bank_glide_stop with snap: key = target.  After a start that was not withheld, after
 * every advance of a gliding voice and after a snap of one, the sounding increment is stored again as key * ratio: one multiply,
 * and that one store is withheld (uncounted; key and the glide words stand) where the product is zero or not finite.  So a glide
 * under a bend lands on target * ratio, and the wheel back at centre then gives the target's bits exactly.  On voices with key == 0,
 * and on a bank without a bend array, the glide calls store the bytes they always stored.
 *
 * All calls are asynchronous on `stream` and ordered like skred_bank_update; host arrays travel through its staging ring, so the
 * caller's memory is free on return; nothing waits for the device but the download and the first allocation; one stream at a time
 * per bank.  A slot, K = slot_voices, voice_mask, tags and matches mean what they mean in the sections above.  Every d_result
 * (device, uint32[3], may be NULL) is cleared on the stream ahead of the kernel: [0] voices stored or restored, [1] bends withheld,
 * [2] slots not owned (the _each calls) or slots of the range that did not match (skred_bank_bend_match).
 *
 * Limits: a SKRED_CTL_PHASE_INC / _INC_SCALE store on a bent voice is overwritten by the next bend (which multiplies the key it
 * captured): bend with these calls instead.  A release leaves the words alone, as for glides: a released note follows the wheel
 * through its tail.  Bends belong with tagged notes.  The host view of voice_phase_inc goes stale; skred_bank_download_ctl reads it
 * back.  On a shard: through skred_shard_bank(), with that rank's local indices.  The fixed-point twin is
 * include/skred_amd_fxpt.h's section "pitch wheel" (skred_fxbank_bend_*: Q24 ratios, integer products); the drop-in mode, deferred
 * items and pattern steps are follow-ups. */
/* Pure host: SKRED_OK, or what the bending calls refuse about K, the mask and the ratios, in this order.  SKRED_E_BAD_ARG: a NULL
 * array; SKRED_E_RANGE: a bad K (not a power of two in 1 .. 64); SKRED_E_BAD_ARG: a voice_mask that is 0 or has bits at or above K, a
 * ratio that is not finite or <= 0, n < 0. */
int  skred_bend_check(const float *ratios, int n, int slot_voices, uint64_t voice_mask);
/* The channel wheel: the rule above, to `ratio`, on every voice_mask voice of every slot of [first, first + count) whose owner
 * matches m.  Geometry, guard and counting are skred_bank_ctl_match's; d_result[2] counts the slots that did not match.  The planner
 * is told nothing.
 * Refused, in this order: SKRED_E_BAD_ARG: NULL bank or match; SKRED_E_RANGE: a bad K; SKRED_E_BAD_ARG: a bad voice_mask, a ratio
 * that is not finite or <= 0, what skred_owner_match_check refuses; SKRED_E_RANGE: first or count not a multiple of K, count <= 0, a
 * range outside the bank. */
int  skred_bank_bend_match(skred_bank_t *bank, int first, int count, int slot_voices, uint64_t voice_mask, const skred_owner_match_t *m,
                           float ratio, uint32_t *d_result, void *stream);
/* Per-note bend (MPE): entry k (of the first min(n, *d_count_or_null)) acts on d_slots[k] only if that is a slot of the bank AND
 * owner[slot] == tags[k] (non-zero); it applies the rule, to ratios[k], on every voice_mask voice of the slot.  d_result[2] counts
 * the slots whose owner differs.  A slot named twice: UNSPECIFIED.  The planner is told nothing.
 * Refused, in this order: SKRED_E_BAD_ARG: NULL bank, ratios, list or tags; SKRED_E_RANGE: a bad K; SKRED_E_BAD_ARG: a bad
 * voice_mask, a ratio that is not finite or <= 0, a zero tag, n < 0 or n > INT32_MAX / 64.  n == 0: SKRED_OK. */
int  skred_bank_bend_owned_each(skred_bank_t *bank, const float *ratios, int slot_voices, uint64_t voice_mask, const int32_t *d_slots,
                                const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
/* Per-note bend by note id: skred_bank_find_owned of the tags over [first, first + count) into scratch the bank owns, then the call
 * above on that list -- built as skred_bank_glide_tags is.  ratios[k] goes with tags[k]: the tags travel sorted, the ratios are
 * permuted with them on the host.  Tags unique, none zero, n <= SKRED_OWNER_MAX_TAGS; each tag reaches at most ONE slot, the lowest
 * that carries it.  d_result[2] is 0.
 * Refused: as above, then SKRED_E_BAD_ARG: n > SKRED_OWNER_MAX_TAGS, a tag that appears twice; then SKRED_E_RANGE: first or count
 * not a multiple of K, count <= 0, a range outside the bank. */
int  skred_bank_bend_tags_each(skred_bank_t *bank, const float *ratios, int first, int count, int slot_voices, uint64_t voice_mask,
                               const uint32_t *tags, int n, uint32_t *d_result, void *stream);
/* The bend words of [first, first + count) are cleared on `stream`; with snap != 0 a bent voice's increment is set to its key first
 * (the wheel at centre, without the guard).  Nothing to do on a bank without a bend array.  SKRED_E_BAD_ARG: NULL bank;
 * SKRED_E_RANGE: count < 0 or a range outside the bank. */
int  skred_bank_bend_clear(skred_bank_t *bank, int first, int count, int snap, void *stream);
/* The bend words of [first, first + count) into host_u32x2 (2 * count words: key, ratio per voice); waits for the device, like
 * skred_bank_download_owners; zeros on a bank that never bent. */
int  skred_bank_download_bend(skred_bank_t *bank, uint32_t *host_u32x2, int first, int count);

/* ---- filter cutoff on the device: key-tracked cutoffs that glide and land ------------------------------------------------------
 *
 * SKRED_CTL_FILTER and skred_filter_each_t bring five finished coefficients, which the host computes with skred_filter_coeffs (libm's
 * sinf / cosf).  A cutoff that follows each note's own pitch therefore needs the increment the device holds (a download after a
 * glide or a bend), a cutoff that moves needs one per-note upload per block, and a host-driven ramp of libm results lands on no
 * particular bits.  The calls of this section keep the CUTOFF beside the voice -- the normalised angular cutoff w = 2 pi f / rate in
 * radians per frame, the resonance q and the mode -- and compute the coefficients on the device with arithmetic that is defined here
 * operation by operation, so that the device, skred_filter_coeffs_w and tests/cutoff_model.py give the same bits.
 *
 * THE ARITHMETIC (skred_filter_coeffs_w(mode, w, q)).  Every multiply, add, subtract and divide is ONE correctly rounded fp32
 * operation (round to nearest even, never fused); a negation flips the sign bit.
 *   1. range reduction to [0, pi / 2]:  if w > SKRED_CUTOFF_HALF_PI: r = (SKRED_CUTOFF_PI_HI - w) + SKRED_CUTOFF_PI_LO (the difference
 *      first: it is exact for w in [pi / 2, 3]) and the cosine below changes its sign; else r = w.
 *   2. z = r * r.
 *   3. sine, Horner in z:  p = S4;  p = p * z + S3;  p = p * z + S2;  p = p * z + S1;  sn = r + (r * z) * p.
 *   4. cosine, Horner in z:  c = C5;  c = c * z + C4;  c = c * z + C3;  c = c * z + C2;  c = c * z + C1;  c = 1 + z * c;
 *      cs = c, or -c behind the reduction of step 1.
 *   5. skred_filter_coeffs' sequence, unchanged:  alpha = sn / (2 * q);  a0 = 1 + alpha;
 *        mode 1 (low-pass):  d = 1 - cs;  b0 = d / 2;  b1 = d;  b2 = b0        mode 2 (high-pass):  s = 1 + cs;  b0 = s / 2;  b1 = -s;  b2 = b0
 *        mode 3 (band-pass): b0 = alpha;  b1 = 0;  b2 = -alpha                  mode 4 (notch):      b0 = 1;  b1 = -2 * cs;  b2 = 1
 *        mode 5 (all-pass):  b0 = 1 - alpha;  b1 = -2 * cs;  b2 = 1 + alpha
 *      out5 = b0 / a0,  b1 / a0,  b2 / a0,  (-2 * cs) / a0,  (1 - alpha) / a0.
 * The constants are the literals below.  THE BOX: w in [SKRED_CUTOFF_W_MIN, SKRED_CUTOFF_W_MAX], q in [SKRED_CUTOFF_Q_MIN,
 * SKRED_CUTOFF_Q_MAX].  Inside it no intermediate is denormal, no divisor is zero (alpha lies in about [4.8e-7, 32]) and every
 * coefficient is finite, which is all the planner asks of the words.
 *
 * ACCURACY, measured by tests/test_cutoff_cpu.py on a grid of 201 values of w (both ends, 72 values spread geometrically over the box,
 * SKRED_CUTOFF_HALF_PI and the 64 fp32 values on either side of that seam) x 17 values of q (both ends, geometric) x 5 modes, against
 * an fp64 evaluation of the same formulas on the same fp32 (w, q): the largest absolute error of each coefficient, of this function
 * and of skred_filter_coeffs(mode, w, q, 2 pi) (libm).  The test holds every entry of the first table to at most 4 x the second's.
 *                     skred_filter_coeffs_w                              skred_filter_coeffs (the yardstick)
 *   mode    b0       b1       b2       a1       a2           b0       b1       b2       a1       a2
 *   1    8.2e-08  1.6e-07  8.2e-08  2.7e-07  8.7e-08      9.3e-08  1.9e-07  9.3e-08  2.4e-07  9.0e-08
 *   2    1.2e-07  2.4e-07  1.2e-07  2.7e-07  8.7e-08      1.2e-07  2.4e-07  1.2e-07  2.4e-07  9.0e-08
 *   3    7.7e-08  0        7.7e-08  2.7e-07  8.7e-08      7.7e-08  0        7.7e-08  2.4e-07  9.0e-08
 *   4    8.3e-08  2.7e-07  8.3e-08  2.7e-07  8.7e-08      8.3e-08  2.4e-07  8.3e-08  2.4e-07  9.0e-08
 *   5    8.7e-08  2.7e-07  0        2.7e-07  8.7e-08      9.0e-08  2.4e-07  0        2.4e-07  9.0e-08
 * The largest ratio is 1.12 (a1, and b1 where it is -2 cs / a0): the factor of 4 is met with a degree-9 sine and a degree-10 cosine.
 * Stability (|a2| < 1 and |a1| < 1 + a2) holds on the whole grid for modes 1 .. 5.
 *
 * cut[n_voices] is an array of eight words PER VOICE (two uint4: w, target, rate_up, rate_down as fp32 bit patterns; carry 0 .. 63, q,
 * mode, a reserved 0) in device memory that only the calls of this section read or write.  w == 0 (all bits) means "no device cutoff",
 * target == 0 "not moving".  The bank allocates the array (32 bytes per voice; the owner array first, when no owner call came before)
 * on the first skred_bank_cutoff_match / _cutoff_owned_each / _cutoff_tags_each call and zero-fills it; that call waits for the device
 * once.  No render kernel, report, probe, tap or planner rule reads the array, the calls store nothing but finite coefficient words,
 * and FILTER is not a listing word: a cutoff call leaves the planner's reports alone, and the block behind it is the steady block.
 * The filter memory (x1 x2 y1 y2) is untouched; velocity, smoothing and cz_distortion, the neighbours of the five words, keep their
 * bits; a voice whose filter is bypassed keeps the words without reading them.  A bank that never calls these allocates and launches
 * nothing more.
 *
 * A RECORD ON VOICE v (skred_cutoff_t; the voices are those of filter_mask in a slot the guard lets through):
 *   1. v has no cutoff word (w == 0) and the record does not name BOTH SKRED_CUTOFF_Q and SKRED_CUTOFF_MODE: WITHHELD and counted.
 *   2. q = the record's with SKRED_CUTOFF_Q, else the voice's; mode likewise with SKRED_CUTOFF_MODE.
 *   3. SKRED_CUTOFF_ABS: wn = value.  SKRED_CUTOFF_TRACK: k = the key word of a bent voice (the pitch-wheel section), else
 *      voice_phase_inc -- the word a glide runs on.  k zero or not finite: WITHHELD and counted.  wn = |k| * value, ONE multiply; a
 *      product outside the box (an infinite one too) is CLAMPED to the nearer end and counted.  The host supplies value = harmonic *
 *      2 pi / table_size of the patch voice -- a ratio, never an increment -- and full keyboard tracking survives glides and stealing
 *      without a read-back.
 *   4. SKRED_CUTOFF_GLIDE on a voice that has a cutoff word: target = wn, rate_up, rate_down = the record's, carry = 0; w and the
 *      coefficients stand until the next advance.  Otherwise (no GLIDE, or the voice's first cutoff): w = wn, target = rate_up =
 *      rate_down = carry = 0 -- any movement stops -- and the five coefficient words = THE ARITHMETIC(mode, wn, q).
 * A withheld record leaves the voice and its eight words exactly as they were.
 *
 * ADVANCE BY F FRAMES (skred_bank_cutoff_advance), for every moving voice of a range: c = carry + F, m = c >> 6.  m times, stopping at
 * arrival: w < target: w = w * rate_up, arrived if w >= target; w > target: w = w * rate_down, arrived if w <= target; w == target:
 * arrived.  On arrival w = THE TARGET'S BITS and target, rates and carry are cleared; else carry = c & 63.  Then the coefficients are
 * computed ONCE from that final w (also when m == 0).  The rates are per 64 frames, and w at every multiple of 64 frames does not
 * depend on how the host cuts its blocks; a voice that has landed holds the bits of a voice set with SKRED_CUTOFF_ABS at the target.
 * A voice that does not move costs one 16-byte load.  The cutoff moves once per block, as every control here does.
 *
 * A NEW NOTE CLEARS THE WORDS.  Once the array exists, every tag launch of the bank is followed on its stream by a launch that zeroes
 * all eight words of all K voices of every slot it tagged (the pedal, glide and bend rule, beside their clears): a thief or a key
 * struck again does not inherit a moving cutoff.  The coefficients stay what they were, as today.  The order for a tracked note is
 * skred_bank_note_on_channel, then skred_bank_bend_tags_each / skred_bank_glide_tags, then skred_bank_cutoff_tags_each.
 *
 * All calls are asynchronous on `stream` and ordered like skred_bank_update; host arrays travel through its staging ring; nothing
 * waits for the device but the download and the first allocation; one stream at a time per bank; the same state gives the same bytes.
 * d_result of the three record calls (device, uint32[4], may be NULL; cleared on the stream ahead of the kernel): [0] voices set or
 * started, [1] records withheld, [2] slots not owned (the _each calls) or slots of the range that did not match, [3] cutoffs clamped.
 *
 * Limits: a tracked cutoff is computed when the call runs and does not follow later bends or glides: send it again.  A
 * SKRED_CTL_FILTER store (or per-entry coefficients) on a voice with a cutoff word is overwritten by that voice's next moving
 * advance, and otherwise leaves w stale.  A release leaves the words alone -- unless the voice has a filter envelope (the next
 * section), whose release stage the advance pass starts from the voice's release clock.  The fixed-point bank has its own integer twin
 * (include/skred_amd_fxpt.h, section "filter cutoff").  Not built: the drop-in mode, deferred items and pattern steps.  On a
 * shard: through skred_shard_bank(), with that rank's local indices. */
#define SKRED_CUTOFF_W_MIN 0x1p-10f
#define SKRED_CUTOFF_W_MAX 3.0f
#define SKRED_CUTOFF_Q_MIN 0x1p-6f
#define SKRED_CUTOFF_Q_MAX 0x1p10f
#define SKRED_CUTOFF_RATE_MIN 0x1p-4f      /* the box of rate_down and rate_up: a factor of 16 per 64 frames either way */
#define SKRED_CUTOFF_RATE_MAX 0x1p4f
#define SKRED_CUTOFF_HALF_PI 0x1.921fb6p+0f
#define SKRED_CUTOFF_PI_HI 0x1.921fb6p+1f
#define SKRED_CUTOFF_PI_LO -0x1.777a5cp-24f
#define SKRED_CUTOFF_S1 -0x1.555548p-3f
#define SKRED_CUTOFF_S2 0x1.110e6ap-7f
#define SKRED_CUTOFF_S3 -0x1.9f5ff4p-13f
#define SKRED_CUTOFF_S4 0x1.5cf92cp-19f
#define SKRED_CUTOFF_C1 -0x1p-1f
#define SKRED_CUTOFF_C2 0x1.555548p-5f
#define SKRED_CUTOFF_C3 -0x1.6c138p-10f
#define SKRED_CUTOFF_C4 0x1.9f6f7ep-16f
#define SKRED_CUTOFF_C5 -0x1.18003p-22f
/* Pure host, THE ARITHMETIC above.  out5 = b0 b1 b2 a1 a2.  Returns SKRED_OK; 1 for mode 0 (bypass: out5 is left as it is, as
 * skred_filter_coeffs leaves it); SKRED_E_BAD_ARG for a NULL out5 or a mode outside 0 .. 5; SKRED_E_RANGE for a w or q that is not
 * finite or lies outside the box.  skred_filter_coeffs and the drop-in mode stay as they are. */
int  skred_filter_coeffs_w(int mode, float w, float q, float out5[5]);
enum { SKRED_CUTOFF_ABS = 1u << 0,     /* w = value */
       SKRED_CUTOFF_TRACK = 1u << 1,   /* w = |k| * value, k the voice's key increment: exactly one of ABS and TRACK */
       SKRED_CUTOFF_GLIDE = 1u << 2,   /* the computed w is the TARGET, reached at rate_up / rate_down per 64 frames */
       SKRED_CUTOFF_Q = 1u << 3,       /* the record names q */
       SKRED_CUTOFF_MODE = 1u << 4 };  /* the record names mode (1 .. 5) */
typedef struct skred_cutoff { uint32_t set; float value, q; uint32_t mode; float rate_up, rate_down; uint32_t reserved[2]; } skred_cutoff_t;   /* 32 bytes */
/* Pure host: SKRED_OK, or what the record calls refuse about K, the masks and the n records, in this order.  SKRED_E_BAD_ARG: a NULL
 * array, n < 0; SKRED_E_RANGE: a bad K (not a power of two in 1 .. 64); SKRED_E_BAD_ARG: a voice_mask or a filter_mask that is 0 or
 * has bits at or above K; in a record: unknown bits in set, SKRED_CUTOFF_ABS with SKRED_CUTOFF_TRACK or neither, first_time != 0 and
 * not both SKRED_CUTOFF_Q and SKRED_CUTOFF_MODE; a reserved word that is not 0; a named value that is not finite (value always; q
 * with Q; the rates with GLIDE); SKRED_E_RANGE: a named q outside the box, an ABS value outside the box, a TRACK value <= 0, a mode
 * outside 1 .. 5, a rate under GLIDE outside [SKRED_CUTOFF_RATE_MIN, SKRED_CUTOFF_RATE_MAX]; SKRED_E_BAD_ARG: rate_up <= 1 or
 * rate_down >= 1 under GLIDE; last, a filter_mask with a bit outside voice_mask.  voice_mask: the voices of a slot the patch plays
 * (the note-on's mask); the entry points themselves take filter_mask alone and check it against all K lanes.  first_time: the
 * caller states that the voices have no cutoff word yet -- the entry points cannot know (they pass 0), and there the kernel
 * withholds and counts instead. */
int  skred_cutoff_check(const skred_cutoff_t *rec, int n, int slot_voices, uint64_t voice_mask, uint64_t filter_mask, int first_time);
/* The channel sweep: the record on every filter_mask voice of every slot of [first, first + count) whose owner matches m.  Geometry,
 * guard and counting are skred_bank_ctl_match's; the record is a kernel argument.  The planner is told nothing.
 * Refused, in this order: SKRED_E_BAD_ARG: NULL bank, match or record; SKRED_E_RANGE: a bad K; SKRED_E_BAD_ARG: a bad filter_mask;
 * SKRED_E_RANGE: first or count not a multiple of K, count <= 0, a range outside the bank; then what skred_cutoff_check refuses about
 * the record; then what skred_owner_match_check refuses. */
int  skred_bank_cutoff_match(skred_bank_t *bank, int first, int count, int slot_voices, uint64_t filter_mask, const skred_owner_match_t *m,
                             const skred_cutoff_t *rec, uint32_t *d_result, void *stream);
/* One record per entry: entry k (of the first min(n, *d_count_or_null)) acts on d_slots[k] only if that is a slot of the bank AND
 * owner[slot] == tags[k] (non-zero).  A slot named twice: UNSPECIFIED.
 * Refused, in this order: SKRED_E_BAD_ARG: NULL bank, records, list or tags, n < 0; SKRED_E_RANGE: a bad K; SKRED_E_BAD_ARG: a bad
 * filter_mask; what skred_cutoff_check refuses about the records; a zero tag, n > INT32_MAX / 64.  n == 0: SKRED_OK. */
int  skred_bank_cutoff_owned_each(skred_bank_t *bank, const skred_cutoff_t *recs, int slot_voices, uint64_t filter_mask,
                                  const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result,
                                  void *stream);
/* By note id: skred_bank_find_owned of the tags over [first, first + count) into scratch the bank owns, then the call above on that
 * list.  recs[k] goes with tags[k]: the tags travel sorted, the records are permuted with them on the host.  1 ..
 * SKRED_OWNER_MAX_TAGS tags, unique, none zero; d_result[2] is 0.  Refused: as above with the range behind the masks, then a repeated
 * tag or n > SKRED_OWNER_MAX_TAGS. */
int  skred_bank_cutoff_tags_each(skred_bank_t *bank, const skred_cutoff_t *recs, int first, int count, int slot_voices, uint64_t filter_mask,
                                 const uint32_t *tags, int n, uint32_t *d_result, void *stream);
/* The advance pass above over the voices [first, first + count): purely per voice, no K.  d_result (device, uint32[2], may be NULL;
 * cleared on the stream ahead of the kernel): [0] voices still moving after the pass, [1] voices that arrived in it.  The host calls
 * it once per block.  On a bank without a cutoff array: SKRED_OK, d_result (if given) is cleared on the stream, nothing is launched.
 * SKRED_E_BAD_ARG: NULL bank, num_frames outside 1 .. 65536; SKRED_E_RANGE: count <= 0 or a range outside the bank. */
int  skred_bank_cutoff_advance(skred_bank_t *bank, int first, int count, int num_frames, uint32_t *d_result, void *stream);
/* Every movement of [first, first + count) ends on `stream`: target, rates and carry are cleared, w, q and mode stay; with snap != 0 a
 * moving voice's w is set to its target and its coefficients computed first.  Nothing to do on a bank without a cutoff array.
 * SKRED_E_BAD_ARG: NULL bank; SKRED_E_RANGE: count < 0 or a range outside the bank. */
int  skred_bank_cutoff_stop(skred_bank_t *bank, int first, int count, int snap, void *stream);
/* The cutoff words of [first, first + count) into host_u32x8 (8 * count words); waits for the device, like
 * skred_bank_download_owners; zeros on a bank that never set a cutoff. */
int  skred_bank_download_cutoff(skred_bank_t *bank, uint32_t *host_u32x8, int first, int count);

/* ---- filter envelope: per-note cutoff contours that follow the gate ---------------------------------------------------------------
 *
 * The cutoff section above sets a cutoff, tracks the key and glides to ONE target.  A subtractive voice wants a contour per note: the
 * cutoff opens from a floor to a peak at the note-on, falls to a sustain level while the key is held, and closes after the note-off.
 * With the cutoff calls alone the host sends one SKRED_CUTOFF_GLIDE per stage and has to time them -- and the last one it cannot time:
 * under a sustain or sostenuto pedal, after skred_bank_stamp_match, skred_bank_release_tags or a steal the host does not know when, or
 * whether, a slot's release clock was stamped.  The device knows: sample_release lies beside every voice, and every note-off path of
 * the control plane ends in a stamp of that word.  So the contour is a small program kept beside the voice; the per-block pass the
 * cutoff already has (skred_bank_cutoff_advance) steps it, and the release stage starts from the voice's own release clock.
 *
 * fenv[n_voices] is an array of eight words PER VOICE (two uint4: stage, w_peak, w_sustain, w_end -- the levels as fp32 bit patterns
 * inside the cutoff box; rate_attack, rate_decay, rate_release, a reserved 0) in device memory that only the calls of this section and
 * the cutoff calls read or write.  stage: 0 no envelope (all eight words are 0 then), 1 attack, 2 decay, 3 sustain, 4 release.  The
 * bank allocates the array (32 bytes per voice; the cutoff and owner arrays first, when they do not exist yet) on the first
 * skred_bank_fenv_match / _fenv_owned_each / _fenv_tags_each call and zero-fills it; that call may wait for the device once.  The
 * envelope MOVES THE VOICE'S CUTOFF WORDS (w, target, the two rates, carry) and through them the five coefficient words; it has no
 * arithmetic of its own: a step is the cutoff advance's one multiply, a coefficient store is THE ARITHMETIC(mode, w, q) of the cutoff
 * section.  No render kernel, report, probe, tap or planner rule reads the array, and what the cutoff section says about the
 * planner, the filter memory and the neighbouring words holds here.  A bank that never calls these allocates and launches nothing
 * more, and every entry point behaves on it as it did.
 *
 * ENTERING A STAGE with level T and rate r (per 64 frames), from the voice's w:
 *   the stage LANDS AT ONCE -- w = T's bits, and the next stage is entered by this rule -- if w == T, or r > 1 and w > T, or r < 1 and
 *   w < T (the rate points away from the level).  Otherwise target = T and rate_up = rate_down = r.
 *     attack (1):  T = w_peak,    r = rate_attack;   next: decay
 *     decay (2):   T = w_sustain, r = rate_decay;    next: sustain
 *     sustain (3): target = rate_up = rate_down = 0: the voice rests, not moving, and the stage word stays 3
 *     release (4): T = w_end,     r = rate_release;  next: none -- when the release lands ALL EIGHT fenv words are cleared, target,
 *                  rates and carry are 0, and w keeps w_end's bits: the voice is a voice set with SKRED_CUTOFF_ABS at w_end.
 *   carry is kept across stage changes: the note keeps its 64-frame grid from the record to the end of the release.
 *
 * A RECORD ON VOICE v (skred_fenv_t; the voices are those of filter_mask in a slot the guard lets through):
 *   1. v has no cutoff word (w == 0): WITHHELD and counted; both arrays of the voice stay as they were.  The base cutoff, q and mode
 *      come from skred_bank_cutoff_* first.
 *   2. w_now = the voice's w when the kernel runs.  SKRED_FENV_ABS: the four levels start, peak, sustain, end are w values.
 *      SKRED_FENV_REL: each level = w_now * value, ONE multiply each; a product outside the box is CLAMPED to the nearer end, and the
 *      VOICE is counted once however many of its levels were clamped.  A tracked base therefore gives a tracked contour.  Exactly one
 *      of ABS and REL is named.  Without SKRED_FENV_START the start level is neither computed nor clamped.
 *   3. SKRED_FENV_START: w = the start level at once.  Otherwise the contour starts from w_now (and `start` must be 0).
 *   4. Any movement the voice had ends: carry = 0, the fenv words = 1, the three levels, the three rates, 0, and the attack is ENTERED
 *      by the rule above.  Stages that land at once chain, as far as sustain (the release is entered by the advance pass only).
 *   5. If w changed, the five coefficient words = THE ARITHMETIC(mode, w, q), once, from the final w.
 *
 * ADVANCE BY F FRAMES.  skred_bank_cutoff_advance is the one per-block pass.  On a bank with an fenv array, for every voice of the
 * range with stage != 0:
 *   1. stage is 1 .. 3 and the voice's sample_release != 0: the release is ENTERED first (it may land at once, which ends the contour).
 *   2. c = carry + F, m = c >> 6.  m times, while the voice has a target: w = w * rate, ONE multiply; arrived at the target if w >=
 *      target going up, w <= target going down; on arrival w = THE TARGET'S BITS and the next stage is ENTERED; the remaining steps
 *      continue in it.  (Sustain has no target: the remaining steps do nothing.)
 *   3. carry = c & 63 -- through sustain too, which is what keeps the grid -- or 0 when the contour ended.
 *   4. If the voice was moving when the pass began or step 1 entered the release, the coefficients are computed ONCE from the final w.
 *      A voice resting in sustain stores no coefficient.
 * A voice with stage == 0 is advanced by the cutoff section's rule.  d_result keeps its meaning: [0] voices moving after the pass
 * (a target != 0: a voice resting in sustain is not moving), [1] voices that arrived at any stage's level in the pass, stepped or at
 * once; a voice that arrives at several levels in one pass counts once.
 * THE STATED PROPERTY: for a fixed sequence of control calls at fixed frame positions and a block cut at every call, w at every
 * multiple of 64 frames from the record on does not depend on where else the host cuts its blocks.
 * Cost: a voice with stage == 0 costs its one 16-byte cutoff load and one 4-byte fenv load; one with a contour two more 16-byte
 * loads of fenv, the second half of its cutoff words and the 8 bytes of its release clock.
 * A trigger stamp alone does not restart a contour (a releasing contour goes on releasing); a new record does.
 *
 * WHO ENDS AN ENVELOPE.  Once the array exists, every tag launch of the bank is followed on its stream by a launch that zeroes all
 * eight fenv words of all K voices of every slot it tagged -- the sixth clear, beside the owner, pedal, glide, bend and cutoff ones: a
 * thief or a key struck again inherits no contour.  skred_bank_cutoff_match / _cutoff_owned_each / _cutoff_tags_each zero the fenv
 * words of the voices they set or start (a withheld record leaves them), skred_bank_cutoff_stop those of every voice of its range:
 * a cutoff call on an enveloped voice ends the contour and then does what it always did.  The order for a note is
 * skred_bank_note_on_channel, then skred_bank_bend_tags_each / skred_bank_glide_tags, then skred_bank_cutoff_tags_each, then
 * skred_bank_fenv_tags_each.
 *
 * All calls are asynchronous on `stream` and ordered like skred_bank_update; host arrays travel through its staging ring; nothing
 * waits for the device but the download and the first allocation; one stream at a time per bank; the same state gives the same bytes.
 * d_result of the three record calls (device, uint32[4], may be NULL; cleared on the stream ahead of the kernel): [0] voices started,
 * [1] records withheld, [2] slots not owned (the _each calls) or slots of the range that did not match, [3] voices clamped.
 *
 * Limits: REL levels are computed when the record runs and do not follow later bends or glides: send the record again.  A
 * SKRED_CTL_FILTER store on a voice with a moving contour is overwritten by the next advance.  Not built: the
 * drop-in mode, deferred items and pattern steps.  On a shard: through skred_shard_bank(), with that rank's local indices. */
enum { SKRED_FENV_ABS = 1u << 0,      /* the four levels are w values inside the box */
       SKRED_FENV_REL = 1u << 1,      /* each level = w_now * value: exactly one of ABS and REL */
       SKRED_FENV_START = 1u << 2 };  /* w = the start level at once; without it `start` must be 0 */
typedef struct skred_fenv { uint32_t set; float start, peak, sustain, end, rate_attack, rate_decay, rate_release; } skred_fenv_t;   /* 32 bytes */
/* Pure host: SKRED_OK, or what the record calls refuse about K, the masks and the n records, in this order.  SKRED_E_BAD_ARG: a NULL
 * array, n < 0; SKRED_E_RANGE: a bad K (not a power of two in 1 .. 64); SKRED_E_BAD_ARG: a voice_mask or a filter_mask that is 0 or
 * has bits at or above K; in a record: unknown bits in set, SKRED_FENV_ABS with SKRED_FENV_REL or neither; start != 0 without
 * SKRED_FENV_START; a value that is not finite (the levels named, the three rates); SKRED_E_RANGE: an ABS level outside the box, a REL
 * value <= 0, a rate outside [SKRED_CUTOFF_RATE_MIN, SKRED_CUTOFF_RATE_MAX]; SKRED_E_BAD_ARG: a rate equal to 1; last, a filter_mask
 * with a bit outside voice_mask.  voice_mask: the voices of a slot the patch plays (the note-on's mask); the entry points themselves
 * take filter_mask alone and check it against all K lanes. */
int  skred_fenv_check(const skred_fenv_t *recs, int n, int slot_voices, uint64_t voice_mask, uint64_t filter_mask);
/* The channel sweep: the record on every filter_mask voice of every slot of [first, first + count) whose owner matches m.  Geometry,
 * guard and counting are skred_bank_cutoff_match's; the record is a kernel argument.  The planner is told nothing.
 * Refused, in this order: SKRED_E_BAD_ARG: NULL bank, match or record; SKRED_E_RANGE: a bad K; SKRED_E_BAD_ARG: a bad filter_mask;
 * SKRED_E_RANGE: first or count not a multiple of K, count <= 0, a range outside the bank; then what skred_fenv_check refuses about
 * the record; then what skred_owner_match_check refuses. */
int  skred_bank_fenv_match(skred_bank_t *bank, int first, int count, int slot_voices, uint64_t filter_mask, const skred_owner_match_t *m,
                           const skred_fenv_t *rec, uint32_t *d_result, void *stream);
/* One record per entry: entry k (of the first min(n, *d_count_or_null)) acts on d_slots[k] only if that is a slot of the bank AND
 * owner[slot] == tags[k] (non-zero).  A slot named twice: UNSPECIFIED.
 * Refused, in this order: SKRED_E_BAD_ARG: NULL bank, records, list or tags, n < 0; SKRED_E_RANGE: a bad K; SKRED_E_BAD_ARG: a bad
 * filter_mask; what skred_fenv_check refuses about the records; a zero tag, n > INT32_MAX / 64.  n == 0: SKRED_OK. */
int  skred_bank_fenv_owned_each(skred_bank_t *bank, const skred_fenv_t *recs, int slot_voices, uint64_t filter_mask, const int32_t *d_slots,
                                const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
/* By note id: skred_bank_find_owned of the tags over [first, first + count) into scratch the bank owns, then the call above on that
 * list.  recs[k] goes with tags[k]: the tags travel sorted, the records are permuted with them on the host.  1 ..
 * SKRED_OWNER_MAX_TAGS tags, unique, none zero; d_result[2] is 0.  Refused: as above with the range behind the masks, then a repeated
 * tag or n > SKRED_OWNER_MAX_TAGS. */
int  skred_bank_fenv_tags_each(skred_bank_t *bank, const skred_fenv_t *recs, int first, int count, int slot_voices, uint64_t filter_mask,
                               const uint32_t *tags, int n, uint32_t *d_result, void *stream);
/* The fenv words of [first, first + count) into host_u32x8 (8 * count words); waits for the device, like
 * skred_bank_download_cutoff; zeros on a bank without the array. */
int  skred_bank_download_fenv(skred_bank_t *bank, uint32_t *host_u32x8, int first, int count);

/* ---- voices sharded over the GPUs of one node (BASELINE config 3) -----------------------------------
 *
 * One process per GPU.  Rank r of `world` owns the contiguous block [lo, hi) of the bank's voices and renders its
 * PRE-master partial mix float[F][2]; the one exchange step of the path is the sum of those partials on `root` (one
 * RCCL reduce of 8*F bytes per block, over xGMI), after which the root applies the master volume stage once.  This is
 * the host side of BASELINE config 3 in C: what the reference's audio callback (skred.c:107-116: synth() then the
 * output) becomes when the voices of one bank live on several GPUs.  A cut is only legal where no voice is modulated
 * across it (skred_shard_cut_ok; skred_shard_upload refuses otherwise).
 *
 * The three steps of a block are function pointers so that the same sequencing runs elsewhere: skred_shard_create()
 * wires them to the bank-mode entry points and to ncclReduce (after skred_shard_init_rccl); a program with its own
 * communicator replaces `reduce`; the CPU tests (tests/test_sharded_gloo.py) supply all three. */
typedef struct skred_shard skred_shard_t;
typedef struct skred_shard_ops {
  void *ctx;            /* passed to render and master */
  int (*render)(void *ctx, int num_frames, int interp, float *partial, void *stream);   /* this rank's pre-master sum -> partial[F][2] */
  int (*master)(void *ctx, const float *sum, int num_frames, int num_channels, float *out, void *stream);   /* root only: synth.c:616-624 */
  void *reduce_ctx;     /* passed to reduce */
  int (*reduce)(void *reduce_ctx, float *partial, size_t n_floats, int root, void *stream);   /* sum over ranks, in place on the root */
} skred_shard_ops_t;

int  skred_shard_partition(int total_voices, int world, int rank, int *lo, int *hi);   /* blocks differ by at most one voice */
int  skred_shard_cut_ok(const skred_voice_bank_t *whole_bank, int lo, int hi);         /* 1: no modulation crosses the cut */
int  skred_shard_create(int device, int rank, int world, int root, int total_voices, skred_shard_t **out);   /* + this rank's bank on `device` */
int  skred_shard_create_custom(int rank, int world, int root, int total_voices, const skred_shard_ops_t *ops, skred_shard_t **out);
void skred_shard_destroy(skred_shard_t *shard);
skred_bank_t *skred_shard_bank(skred_shard_t *shard);        /* tables, globals, options, updates: through the bank ABI above */
int  skred_shard_range(const skred_shard_t *shard, int *lo, int *hi);
int  skred_shard_upload(skred_shard_t *shard, const skred_voice_bank_t *whole_bank);   /* this rank's block of the WHOLE bank */
int  skred_shard_set_ops(skred_shard_t *shard, const skred_shard_ops_t *ops, int always_reduce);   /* NULL members keep the current step */
/* RCCL owned by the library: rank 0 draws an id, the host program carries its 128 bytes to the other ranks, every
 * rank initialises with it (collective call). */
int  skred_shard_rccl_unique_id(void *out128);
int  skred_shard_init_rccl(skred_shard_t *shard, const void *unique_id128);
/* One block: render -> reduce -> master on the root.  `partial`: float[num_frames][2] scratch in the memory the steps
 * work on (NULL: the shard's own device scratch); `out` ([num_frames][num_channels]) is written on the root only.
 * Asynchronous on `stream` with the bank-backed steps. */
int  skred_shard_render_mix(skred_shard_t *shard, int num_frames, int interp, float *partial, float *out, int num_channels, void *stream);

/* The same block with the collective of block k overlapped with the render of block k + 1 (two partial buffers, the
 * collective and the root's master stage on a stream of the shard's own): throughput is bounded by max(render,
 * reduce + master) instead of their sum.  Host-paced: call k first waits (on the host) until block k - 2 has left the
 * collective's stream, so `out` of call k is complete -- for the host and for every stream -- once call k + 2 has
 * returned: alternate between two output buffers.  `stream` itself never waits for the collective's stream; to have
 * everything issued so far complete ON `stream` (e.g. to consume the latest block with a kernel or a copy queued
 * there) call skred_shard_flush(shard, stream).  Same samples as skred_shard_render_mix, bit for bit.  Custom steps
 * (host memory) run synchronously, in order. */
int  skred_shard_render_mix_pipelined(skred_shard_t *shard, int num_frames, int interp, float *out, int num_channels, void *stream);
int  skred_shard_flush(skred_shard_t *shard, void *stream);

/* Timing of the most recent skred_bank_render() on its stream, via hipEvents
 * recorded around the render kernel itself (ms; <0 if unavailable). Synchronises. */
float skred_bank_last_render_ms(skred_bank_t *bank);

/* The render kernel of every skred_bank_render() call is bracketed by a hipEvent pair on the
 * call's stream (ring of 256).  reset() starts a measurement window; summary() synchronises and
 * reports mean / min kernel duration (ms) over the calls since the reset (at most the last 256). */
void skred_bank_timing_reset(skred_bank_t *bank);
int  skred_bank_timing_summary(skred_bank_t *bank, float *mean_ms, float *min_ms, int *count);

#ifdef __cplusplus
}
#endif
#endif /* SKRED_AMD_H */
