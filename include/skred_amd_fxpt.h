/*
 * include/skred_amd_fxpt.h -- C ABI of the FIXED-POINT render path.
 *
 * The reference has no fixed-point render path at all (the notamy <name>_lutset_fxpt.h files are
 * data-only headers nobody includes), so this path is DEFINED by this project: the definition is
 * oracle/cpu_ref_fxpt.c (scalar C) and the HIP kernel must reproduce it bit for bit, mix included
 * (integer sums do not depend on the order of addition).  Parity against the reference: unpinned
 * upstream, by construction.
 *
 * Arithmetic (all integer, two's complement, `>>` on signed values is arithmetic):
 *   LUT      int16 single-cycle tables of 2^L entries (the notamy *_fxpt pyramids), one pool
 *   phase    uint32, 2^32 = one table cycle; per frame  phase += phase_inc  (mod 2^32), THEN sampled
 *   index    i = phase >> (32-L);  truncate: s = lut[i]
 *            linear:   f = (phase << L) >> 17  (Q15),  s = a + (((b - a) * f) >> 15),  b = lut[(i+1) & (2^L-1)]
 *   ADSR     t = sat32(now - sample_start), linear stages on integer frame counts A, D, R and Q15
 *            sustain S with reciprocals rX = floor(2^32 / X):
 *              t < A        e = (t * rA) >> 17
 *              t < A + D    e = 32768 - ((((t-A) * rD) >> 17) * (32768 - S) >> 15)
 *              held         e = S                      (sample_release == 0)
 *              tr < R       e = S - ((((tr * rR) >> 17) * S) >> 15),  tr = sat32(now - sample_release)
 *              else         e = 0, is_active = 0
 *   gain     target = (amp_q15 * ((e * velocity_q15) >> 15)) >> 15        (amp_q15 <= 65535; this product in 64 bits)
 *            smoother (optional): g += ((target - g) * k_q15) >> 15, gain = g
 *   output   v = (s * gain) >> 15 (product in 64 bits) ; L = (v * pan_left_q15) >> 15 ; R = (v * pan_right_q15) >> 15
 *            every other product is an int32 one (keep it inside 32 bits: Q15 gains, velocity <= 65535)
 *   range    PROMISED only while each of those int32 products stays inside int32 -- e * velocity, the two envelope products,
 *            (target - g) * k_q15, v * pan_left_q15, v * pan_right_q15 -- with gains, velocity and smoother state >= 0:
 *            beyond that the scalar definition is signed overflow in C and defines nothing (skred_fxbank_upload checks only
 *            the table window, amp_q15 and the delay line; a smoother state of 2^20 with a pan of 8192 is already outside).
 *            (b - a) * f of the linear lookup cannot leave int32 (|b - a| <= 65535, f < 32768).  sample_start and
 *            sample_release may lie AHEAD of the clock: now - sample_start wraps and saturates, so the note plays its
 *            sustain level until now reaches sample_start and attacks then; a release ahead of the clock has run out
 *   mix      int64 sum of L and of R over all voices, per frame
 *   skipped  amp_q15 == 0 or finished: v = 0, state frozen (as synth.c:531-542 does for the float path)
 *   one-shot a voice with one_shot != 0 plays ONE cycle of its table: in the frame where phase + phase_inc carries out of
 *            32 bits the phase is left at 0xFFFFFFFF, that frame is still rendered from the table's last entry (linear:
 *            the neighbour does not fold back to entry 0, b = a), `finished` is set and from the next frame on the voice
 *            is skipped -- the image of osc_next()'s finish rule for forward playback (synth.c:241-256)
 *   biquad   filter_mode != 0: direct form I on the (interpolated) table sample s, |s| <= 32767, in the order of the
 *            float path (synth.c:349-364: after the oscillator, before the gain).  Coefficients Q2.30 in int32 (the RBJ
 *            b/a0, a/a0 of mmf_set_params, synth.c:929-1008: all inside (-2, 2)); delay line in Q12 sample units, int32,
 *            |x|, |y| < 2^29; accumulation in int64 (five products < 2^60 each):
 *              x0  = s << 12
 *              acc = b0*x0 + b1*x1 + b2*x2 - a1*y1 - a2*y2
 *              y0  = clamp((acc + 2^29) >> 30, -2^29, 2^29 - 1)       round to nearest, saturating
 *              x2 = x1, x1 = x0, y2 = y1, y1 = y0
 *              s   = clamp(y0 >> 12, -32768, 32767)                   back to sample units: a resonant overshoot saturates
 *   master   the image of the master-volume stage (synth.c:616-624: vg += k * (target - vg); out = sum * vg), after the mix:
 *            g is Q31 held in int64, target in [0, 2^31), k_q15 in [0, 32768]; per frame
 *              g   += ((target_q31 - g) * k_q15) >> 15
 *              out  = (mix * (g >> 16)) >> 15                         per channel, int64 (|mix| < 2^38 for 2^20 voices: 53 bits)
 *            defaults: target 0.025 (volume_user 1 x AMY_FACTOR), k 66/32768 (0.002), g 0 -- the float path's
 *   stamps   note-on: sample_start = now, sample_release = 0, is_active = 1; note-off: if is_active, sample_release = now
 *            (amp_envelope_trigger / _release, synth.c:383-395), now = the bank's synth_sample_count when the stamp runs
 */
#ifndef SKRED_AMD_FXPT_H
#define SKRED_AMD_FXPT_H

#include <stdint.h>
#include <stddef.h>

#include "skred_amd.h"   /* skred_owner_match_t and the SKRED_EACH_* bits, shared with the float bank */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct skred_fxpt_bank {
  int32_t n_voices;
  uint32_t *phase;              /* rw */
  uint32_t *phase_inc;
  int32_t  *table_offset;       /* first entry of the voice's table inside the int16 pool */
  int32_t  *log2_size;          /* 3..15 */
  int32_t  *amp_q15;            /* 0..65535 */
  int32_t  *pan_left_q15, *pan_right_q15;
  int32_t  *disconnect;
  int32_t  *use_envelope;
  uint32_t *attack_frames, *decay_frames, *release_frames;
  int32_t  *sustain_q15, *velocity_q15;
  uint64_t *sample_start, *sample_release;
  int32_t  *is_active;          /* rw */
  int32_t  *smoother_enable;
  int32_t  *smoother_k_q15;
  int32_t  *smoother_gain_q15;  /* rw */
  int32_t  *voice_sample;       /* rw: v of the last rendered frame */
  int32_t  *one_shot;           /* plays one cycle, then finishes */
  int32_t  *finished;           /* rw */
  int32_t  *filter_mode;        /* 0 = no filter (the kind of filter is in the coefficients) */
  int32_t  *b0_q30, *b1_q30, *b2_q30, *a1_q30, *a2_q30;
  int32_t  *x1, *x2, *y1, *y2;  /* rw: delay line, Q12 sample units */
} skred_fxpt_bank_t;

typedef struct skred_fxbank skred_fxbank_t;   /* opaque device-side bank */

int  skred_fxbank_create(int device, int n_voices, skred_fxbank_t **out);
void skred_fxbank_destroy(skred_fxbank_t *fx);
int  skred_fxbank_set_tables_i16(skred_fxbank_t *fx, const int16_t *pool, size_t n_entries);
int  skred_fxbank_upload(skred_fxbank_t *fx, const skred_fxpt_bank_t *host, int src_first, int dst_first, int count);
int  skred_fxbank_download(skred_fxbank_t *fx, skred_fxpt_bank_t *host, int src_first, int dst_first, int count);
int  skred_fxbank_set_sample_count(skred_fxbank_t *fx, uint64_t synth_sample_count);
uint64_t skred_fxbank_get_sample_count(const skred_fxbank_t *fx);

/* Render num_frames frames; d_mix = device int64[num_frames][2]; d_stems = device int32
 * [num_frames][n_voices][2] or NULL.  interp: 0 truncate, 1 linear.  Asynchronous on `stream`. */
int  skred_fxbank_render(skred_fxbank_t *fx, int num_frames, int interp, int64_t *d_mix, int32_t *d_stems, void *stream);
/* Render + mix-down + master stage in ONE launch (the render kernel's last-arriving workgroups add the rows up and apply the
 * gain of each frame): d_out = device int64[num_frames][2], post-master. */
int  skred_fxbank_render_mix(skred_fxbank_t *fx, int num_frames, int interp, int64_t *d_out, int32_t *d_stems, void *stream);
/* The master stage alone, for a sum that travelled (multi-GPU: on the root, after the int64 reduce of the ranks'
 * skred_fxbank_render outputs -- an exact sum, whatever the order): must follow a skred_fxbank_render of the same block on
 * this bank, which walked the block's gains.  d_out may equal d_sum. */
int  skred_fxbank_master(skred_fxbank_t *fx, const int64_t *d_sum, int num_frames, int64_t *d_out, void *stream);
int  skred_fxbank_set_master(skred_fxbank_t *fx, int64_t target_q31, int32_t k_q15, int64_t gain_q31);   /* synchronous */
int64_t skred_fxbank_get_master_gain(skred_fxbank_t *fx);                                                  /* synchronous; < 0: error */
/* Note-ons / note-offs on device-resident voices (the float path's SKRED_STAMP_TRIGGER / _RELEASE), on `stream`; the ids travel
 * through the staging ring of the live-control calls below: the call does not synchronise the stream. */
enum { SKRED_FX_STAMP_TRIGGER = 1, SKRED_FX_STAMP_RELEASE = 2 };
int  skred_fxbank_stamp(skred_fxbank_t *fx, const int32_t *voices, int n_voices, int which, void *stream);
/* ---- live control: updates, the free-voice list, note-ons --------------------------------------------------------------
 *
 * The control plane of the float bank (include/skred_amd.h: skred_bank_update, skred_bank_find_idle, skred_bank_notes_on_list
 * and their kin) on the fixed-point planes, with the same vocabulary: SKRED_DIRTY_* / SKRED_STAMP_*, SKRED_IDLE_*, SKRED_NOTE_*
 * keep their bit values.  Everything is asynchronous on the caller's stream, ordered like the renders queued on it; nothing here
 * waits for the device.  The calls work on a shard through skred_fxshard_bank(), with that rank's LOCAL voice indices.
 * Note owners and controllers have a section of their own below.  Not here (yet): the deferred queue and the step clock, taps,
 * slots of more than one voice.
 *
 * Transport.  Records travel through a ring of SKRED_FX_RING_SLOTS pinned staging slots: one hipMemcpyAsync per batch into the
 * slot's device twin on `stream`, then the kernels, then an event of the slot's own.  The caller's arrays are free again when a
 * call returns.  A call that finds its slot still in flight -- the bank is SKRED_FX_RING_SLOTS batches ahead of the device --
 * waits for that slot's event, for as long as it takes: there is no wall-clock limit after which an update would be dropped.
 * (Consequence: do not issue more than SKRED_FX_RING_SLOTS batches on a stream that is blocked behind something the same
 * thread has yet to submit.)  One stream at a time per bank, as for its renders.
 *
 * skred_fxbank_update -- the `dirty` parts of the listed voices, from the host view, onto the resident voices:
 *   SKRED_DIRTY_PARAMS        phase_inc, table_offset, log2_size, the flags (use_envelope, smoother_enable, disconnect, filter_mode,
 *                             one_shot), amp_q15, attack / decay / release frames and their reciprocals, sustain_q15, b0..a2,
 *                             smoother_k_q15, velocity_q15.  Not the pans, not the envelope clock.
 *   SKRED_DIRTY_PAN           pan_left_q15, pan_right_q15
 *   SKRED_DIRTY_PHASE         phase, finished
 *   SKRED_DIRTY_ENV_STATE     is_active
 *   SKRED_DIRTY_FILTER_STATE  x1 x2 y1 y2
 *   SKRED_DIRTY_SMOOTHER      smoother_gain_q15
 *   SKRED_DIRTY_SAMPLE        voice_sample
 *   SKRED_DIRTY_ENV_CLOCK     sample_start, sample_release as the host has them
 *   SKRED_STAMP_TRIGGER / _RELEASE   the stamps of skred_fxbank_stamp with now = the bank's sample count at the call, applied
 *                             after an ENV_CLOCK write of the same record
 *   SKRED_DIRTY_HOLD          refused (SKRED_E_BAD_ARG): the definition has no sample-and-hold
 * Everything not named keeps the value the device last computed (skred_fxbank_upload would overwrite the running phase, the
 * smoother, voice_sample, is_active / finished and the delay line with the host's stale copies).  A voice may be listed more than
 * once: the copies take effect in order.  n == 0: SKRED_OK.  Refused before anything touches the device: SKRED_E_BAD_ARG -- NULL
 * bank, host view or list, n < 0, no bit or unknown bits in dirty; SKRED_E_RANGE -- a voice outside the bank or the host view,
 * and, per listed voice and only for the kinds named, what skred_fxbank_upload refuses: the table window and amp_q15 outside
 * 0..65535 under PARAMS, a delay line outside +-2^29 under FILTER_STATE. */
enum { SKRED_FX_RING_SLOTS = 8 };
int  skred_fxbank_update(skred_fxbank_t *fx, const skred_fxpt_bank_t *host, const int32_t *voices, int n, uint32_t dirty, void *stream);

/* The free-voice list: skred_bank_find_idle's contract (ascending from `from`, wrapping to `first`; d_count[0] = written =
 * min(total, max_out), d_count[1] = total; entries past `written` are not touched; reads the bank only; the same state gives the
 * same bytes; two launches, no workgroup waits for another) with the criteria read on the fixed-point fields, exactly:
 *   SKRED_IDLE_FINISHED   finished != 0
 *   SKRED_IDLE_ENV_DONE   use_envelope != 0 && is_active == 0 && (smoother_enable == 0 || |smoother_gain_q15| <= settle_q15)
 *                         (the absolute value taken in 64 bits)
 *   SKRED_IDLE_AMP_ZERO   amp_q15 == 0
 * settle_q15 = 0 IS a usable level here, unlike the float path's: with k_q15 > 0 the integer smoother g += ((0 - g) * k) >> 15
 * moves a positive g down by at least 1 per frame (the shift is arithmetic: -(g * k) >> 15 <= -1 whenever g * k > 0), so after a
 * release has ended the gain reaches exactly 0 in at most g frames.  (A NEGATIVE g -- outside the promised range -- moves up by
 * floor(-g * k / 2^15), which is 0 once |g| * k < 2^15: it stalls.)
 * skred_fx_idle_check is pure host: SKRED_E_BAD_ARG -- NULL query, negative max_out, no criterion, unknown bits, among them
 * SKRED_IDLE_UNNAMED (the definition has no modulators), a negative settle_q15; SKRED_E_RANGE -- count <= 0, a range outside
 * [0, n_voices), `from` outside the range.  The bank calls add: NULL bank or d_count, NULL d_voices with max_out > 0. */
typedef struct skred_fx_idle_query {
  int32_t first, count; uint32_t which; int32_t settle_q15; int32_t from; int32_t max_out;
} skred_fx_idle_query_t;
int  skred_fx_idle_check(const skred_fx_idle_query_t *q, int n_voices);
int  skred_fxbank_find_idle(skred_fxbank_t *fx, const skred_fx_idle_query_t *q, int32_t *d_voices, uint32_t *d_count, void *stream);
/* The same into host memory; waits for `stream` only.  Returns `written` (>= 0) or a SKRED_E_* code; *total_out may be NULL. */
int  skred_fxbank_find_idle_host(skred_fxbank_t *fx, const skred_fx_idle_query_t *q, int32_t *voices, int *total_out, void *stream);

/* Device-side note-ons: skred_bank_notes_on_list / _note_on_idle / _stamp_list, argument for argument.  Note k goes to voice
 * d_voices[first_entry + k] if first_entry + k < d_count[0] and that entry lies in [0, n_voices); otherwise it is dropped.  A
 * placed note stores, as words: phase_inc and velocity_q15; with SKRED_NOTE_SET_PHASE the phase, and `finished` is cleared; with
 * SKRED_NOTE_SET_PAN the two pans; then the trigger stamp (sample_start = the bank's sample count at the call, sample_release = 0,
 * is_active = 1).  Nothing else: amp, table, smoother k, filter and delay line keep what they hold.  d_assigned[k] (device
 * int32[n], may be NULL) = the voice or -1; d_result (device uint32[2], required) = placed, dropped.  Integer sums: the same bytes
 * in any arrival order.  The list must name distinct voices.  The notes are staged before the call returns.  n == 0: SKRED_OK,
 * nothing is done.  skred_fx_notes_check (pure host) refuses with SKRED_E_BAD_ARG: NULL notes, n < 0, unknown flags, non-zero
 * reserved words, velocity_q15 outside 0..65535, and under SET_PAN a pan outside 0..65535. */
typedef struct skred_fx_note {            /* 32 bytes */
  uint32_t phase_inc; int32_t velocity_q15; uint32_t phase; int32_t pan_left_q15, pan_right_q15;
  uint32_t flags, reserved[2];            /* SKRED_NOTE_SET_PHASE / SKRED_NOTE_SET_PAN; reserved 0 */
} skred_fx_note_t;
int  skred_fx_notes_check(const skred_fx_note_t *notes, int n);
int  skred_fxbank_notes_on_list(skred_fxbank_t *fx, const skred_fx_note_t *notes, int n, const int32_t *d_voices,
                                const uint32_t *d_count, int first_entry, int32_t *d_assigned, uint32_t *d_result, void *stream);
/* The query `q` into scratch the bank owns (q->max_out is ignored: the library uses n), then the placement with first_entry = 0.
 * SKRED_IDLE_AMP_ZERO is refused: a note-on leaves amp_q15 alone, so such a voice would stay silent and be listed again. */
int  skred_fxbank_note_on_idle(skred_fxbank_t *fx, const skred_fx_idle_query_t *q, const skred_fx_note_t *notes, int n,
                               int32_t *d_assigned, uint32_t *d_result, void *stream);
/* SKRED_STAMP_TRIGGER and / or _RELEASE on the first min(n, *d_count_or_null) entries of a list in device memory (NULL: n
 * entries); entries outside the bank -- the -1 of a dropped note -- are skipped. */
int  skred_fxbank_stamp_list(skred_fxbank_t *fx, const int32_t *d_voices, int n, const uint32_t *d_count_or_null, uint32_t stamps,
                             void *stream);

/* ---- voice stealing: which sounding voices matter least, ranked on the device ------------------------------------------
 *
 * skred_bank_find_steal / _find_steal_host / _note_on_steal (include/skred_amd.h), argument for argument, on the fixed-point
 * fields as the device holds them at that point of the stream; SKRED_STEAL_OLDEST / _QUIETEST, SKRED_STEAL_RELEASED_FIRST /
 * _RELEASED_ONLY and SKRED_STEAL_MAX keep their values.  `now` is the bank's sample count when the call is made (the clock the
 * stamps use).  Every comparison is exact:
 *   released   sample_release != 0
 *   age        sample_start > now ? 0 : now - sample_start      (a start ahead of the clock, which this path allows, has age 0)
 *   candidate  the voice lies in [first, first + count)  &&  use_envelope != 0  &&  is_active != 0  &&  age >= min_age
 *              &&  (released, under SKRED_STEAL_RELEASED_ONLY)
 *              &&  the voice does NOT satisfy skred_fxbank_find_idle's predicate for (which = exclude_idle, settle_q15);
 *                  exclude_idle = 0 excludes nobody
 *   class      0 if SKRED_STEAL_RELEASED_FIRST is set and the voice is released, else 1
 *   primary    SKRED_STEAL_OLDEST:    sample_release for class 0, sample_start otherwise, as full 64-bit counts
 *              SKRED_STEAL_QUIETEST:  min(|smoother_gain_q15| taken in 64 bits, 0x7fffffff) when smoother_enable != 0, else 0x7fffffff
 *   key        class << 62 | min(primary, 2^62 - 1)
 *   order      ascending key, ties by ascending voice index
 * d_count[0] = written = min(total, max_out), d_count[1] = total candidates; entries past `written` are not touched; the query
 * reads the bank only; the same state gives the same bytes; max_out == 0 counts only.  SKRED_STEAL_DIGITS + 3 = nine launches
 * whatever the data (one with max_out == 0), no workgroup waits for another, nothing waits for the device.  Only the first launch
 * reads the bank -- SKX_OSC's flags and the read-write flags always, the envelope clock for OLDEST, min_age > 0 or a RELEASED_*
 * flag, the smoother's gain for QUIETEST or an ENV_DONE exclusion, amp_q15 for an AMP_ZERO exclusion -- and leaves one key per
 * voice; the rest is the float bank's select.  The bank owns the scratch (8 bytes per voice, allocated by the first query): one
 * stream at a time.  The calls work on a shard through skred_fxshard_bank(), with that rank's LOCAL voice indices.
 * skred_fx_steal_check is pure host: SKRED_E_BAD_ARG -- NULL query, unknown policy, unknown bits in flags or exclude_idle, among
 * them SKRED_STEAL_UNNAMED and SKRED_IDLE_UNNAMED (the definition has no modulators), reserved != 0, max_out outside
 * [0, SKRED_STEAL_MAX], a negative settle_q15; SKRED_E_RANGE -- count <= 0, a range outside [0, n_voices).  The bank calls add:
 * NULL bank or d_count, NULL d_voices with max_out > 0.  All refusals come before anything touches the device. */
typedef struct skred_fx_steal_query {     /* 40 bytes */
  int32_t first, count; uint32_t policy, flags; uint64_t min_age;
  uint32_t exclude_idle; int32_t settle_q15; int32_t max_out; int32_t reserved;
} skred_fx_steal_query_t;
int  skred_fx_steal_check(const skred_fx_steal_query_t *q, int n_voices);
int  skred_fxbank_find_steal(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, int32_t *d_voices, uint32_t *d_count, void *stream);
/* The same into host memory; waits for `stream` only.  Returns `written` (>= 0) or a SKRED_E_* code; *total_out may be NULL. */
int  skred_fxbank_find_steal_host(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, int32_t *voices, int *total_out, void *stream);
/* Notes at full polyphony: the idle query (max_out = n) into the bank's own list, the steal query with exclude_idle =
 * idle_q->which, settle_q15 = idle_q->settle_q15 and max_out = min(n, SKRED_STEAL_MAX) (the library overrides those three fields
 * of *steal_q: a victim is never a voice the idle list already offers), the victims appended behind the idle entries as far as
 * the batch reaches, then the placement of skred_fxbank_notes_on_list with first_entry = 0: idle voices take the first notes,
 * victims the next ones in victim order, the rest is dropped.  d_assigned as there; d_result (device uint32[3], required) =
 * placed, dropped, placed on stolen voices.  The notes travel through the staging ring as skred_fxbank_notes_on_list's do.
 * n == 0: SKRED_OK, nothing is done.  Refused before anything touches the device: what skred_fxbank_note_on_idle refuses
 * (SKRED_IDLE_AMP_ZERO among it), what skred_fx_steal_check refuses, what skred_fx_notes_check refuses. */
int  skred_fxbank_note_on_steal(skred_fxbank_t *fx, const skred_fx_idle_query_t *idle_q, const skred_fx_steal_query_t *steal_q,
                                const skred_fx_note_t *notes, int n, int32_t *d_assigned, uint32_t *d_result, void *stream);

/* ---- note owners and controllers: note-offs and control changes that cannot hit a stolen voice ------------------------------
 *
 * The float bank's two sections of the same names (include/skred_amd.h: skred_bank_tag_slots .. skred_bank_download_owners,
 * skred_bank_ctl_range / _ctl_slots / _ctl_owned) on the fixed-point planes.  This bank has NO SLOTS: every call is per voice,
 * which is the float call at K = slot_voices = 1 and voice_mask = 1; slots (K > 1) are out of scope here.  Everything is
 * asynchronous on the caller's stream and ordered like skred_fxbank_update; host arrays (tags, the controller record) travel through
 * the ring of SKRED_FX_RING_SLOTS staging slots, so the caller's array is free on return and nothing waits for the device.  The
 * calls work on a shard through skred_fxshard_bank(), with that rank's LOCAL voice indices.  n == 0 (count == 0 for _ctl_range and
 * _owner_clear): SKRED_OK, nothing is done.  Every refusal comes before anything touches the device and leaves the bank usable.
 *
 * Owner words.  owner[n_voices] is a uint32 array in device memory that only the calls of this section read or write; 0 means
 * "nobody".  The first call of this section other than _owner_clear and _download_owners allocates it (4 bytes per voice, plus the
 * scratch of _release_tags) and zero-fills it; that one call may wait for the device.  skred_fxbank_upload, _update, the renders,
 * notes, stamps and steals never touch it and sk_fx_render_kernel never reads it: a bank that makes owner calls renders the blocks
 * of a bank that makes none, bit for bit.  The host's sequence is the float bank's: draw a non-zero tag per note, place the burst
 * (skred_fxbank_note_on_idle / _note_on_steal), then skred_fxbank_tag_list(d_assigned, tags) on the same stream -- a thief's tags
 * overwrite its victims'.  Note-off by id: skred_fxbank_release_tags; note-off or "this chord only" on a kept d_assigned:
 * skred_fxbank_stamp_owned / _ctl_owned with the tags the entries are expected to carry.  Tags are checked with
 * skred_owner_tags_check (include/skred_amd.h; SKRED_OWNER_MAX_TAGS, SKRED_OWNER_ALLOW_ZERO, SKRED_OWNER_UNIQUE as they are).
 *
 * skred_fxbank_tag_list      owner[d_voices[k]] = tags[k] (host uint32[n]; 0 clears) for the first min(n, *d_count_or_null) entries
 *                            (NULL: n) that lie in [0, n_voices): a d_assigned with its -1 holes is the natural argument.  A voice
 *                            named twice with different tags ends up with one of them.  d_result (device uint32[2], may be NULL),
 *                            cleared on the stream ahead of the kernel: [0] voices tagged, [1] entries that are no voice.
 *                            SKRED_E_BAD_ARG: NULL bank, list or tags, n < 0 or n > INT32_MAX / 64.
 * skred_fxbank_find_owned    d_voices_out[k] (device int32[n]) = the LOWEST voice of [first, first + count) whose owner equals
 *                            tags[k], or -1.  1 <= n <= SKRED_OWNER_MAX_TAGS, no zero tag, no tag twice.  An unsigned minimum: the
 *                            same state gives the same bytes, and no workgroup waits for another.  SKRED_E_BAD_ARG: NULL bank, tags
 *                            or d_voices_out, what skred_owner_tags_check(SKRED_OWNER_UNIQUE) refuses; SKRED_E_RANGE: count <= 0 or
 *                            a range outside the bank.
 * skred_fxbank_stamp_owned   skred_fxbank_stamp_list with the guard owner[voice] == tags[k] (tags non-zero: an untagged voice never
 *                            matches).  The stores are exactly that call's, `now` the bank's sample count at the call.  d_result
 *                            (device uint32[3], required), cleared on the stream ahead of the kernel: [0] voices stamped, [1] voices
 *                            whose owner differs, [2] entries that are no voice.  SKRED_E_BAD_ARG: NULL bank, list, tags or result,
 *                            n < 0 or n > INT32_MAX / 64, a zero tag, no or unknown stamp bits.
 * skred_fxbank_release_tags  note-off by id: skred_fxbank_find_owned into scratch the bank owns, then skred_fxbank_stamp_owned on
 *                            that list with the same tags.  Each tag stamps at most one voice, the lowest that carries it.
 *                            d_result as there: [2] counts the tags nobody in the range carries, [1] is 0.  One stream at a time
 *                            per bank.  Refusals of both calls.
 * skred_fxbank_owner_clear   owner[first .. first + count) = 0 on `stream` (nothing to do on a bank that was never tagged).
 *                            SKRED_E_RANGE: count < 0 or a range outside the bank.
 * skred_fxbank_download_owners  the owner words of a range into host_u32; synchronous (waits for the device); zeros on a bank that
 *                            was never tagged.
 *
 * Controllers.  skred_fx_ctl_t is ONE record (this bank has no slots): `which` names the fields it stores with the float bank's
 * SKRED_CTL_* bits, reserved words are 0.  Each field stores exactly the words named here and nothing else -- the running phase, the
 * delay line, the smoother's gain, the envelope clock, every flag, the table window and filter_mode keep what the device holds:
 *   SKRED_CTL_PHASE_INC   phase_inc
 *   SKRED_CTL_INC_SCALE   phase_inc = ((uint64)phase_inc * inc_scale_q16) >> 16, the product in 64 bits, 65536 = 1.0.  A result
 *                         above 0xFFFFFFFF is NOT stored (the voice keeps its increment) and is counted in d_result[1].  Together
 *                         with PHASE_INC the scale applies to the new value; when that product is withheld the new value stays.
 *   SKRED_CTL_AMP         amp_q15, 1..65535, stored only on voices whose amp_q15 != 0 ON THE DEVICE; the others keep 0 and are
 *                         counted in d_result[1] (the float bank's rule: one host drives both banks)
 *   SKRED_CTL_PAN         pan_left_q15, pan_right_q15, each 0..65535
 *   SKRED_CTL_FILTER      b0_q30 b1_q30 b2_q30 a1_q30 a2_q30 (Q2.30, any int32).  filter_mode and the delay line are untouched, so
 *                         the choice of the render instantiation stays right; on a voice without a filter the coefficients are
 *                         stored and inert
 *   SKRED_CTL_ENV_TIMES   attack_frames, decay_frames, release_frames, their reciprocals floor(2^32 / X) (0 for X == 0) as
 *                         skred_fxbank_upload makes them, and sustain_q15 (0..32768)
 *   SKRED_CTL_VELOCITY    velocity_q15, 0..65535
 *   SKRED_CTL_SMOOTHING   smoother_k_q15, 0..32768
 * SKRED_CTL_FM_DEPTH .. SKRED_CTL_CZ_DIST are refused: the definition has no modulators.  skred_fx_ctl_check is pure host:
 * SKRED_E_BAD_ARG for a NULL record, which == 0, unknown or refused bits, a non-zero reserved word, a named value outside its range.
 * Values a field does not name are not looked at.
 *
 * skred_fxbank_ctl_range  the record on every voice of [first, first + count).  d_result (device uint32[2], may be NULL), cleared on
 *                         the stream ahead of the kernel: [0] voices written, [1] stores withheld by the two guards.  Refused: what
 *                         skred_fx_ctl_check refuses, a NULL bank; SKRED_E_RANGE: count < 0 or a range outside the bank.
 * skred_fxbank_ctl_list   the record on the first min(n, *d_count_or_null) entries of a list in device memory that lie in
 *                         [0, n_voices); -1 holes are skipped.  A voice listed twice gets the absolute stores twice, which is the same
 *                         as once, and is counted twice; with SKRED_CTL_INC_SCALE its increment is UNSPECIFIED (scaled once or twice).
 *                         d_result as for _ctl_range.  SKRED_E_BAD_ARG: NULL bank or list, n < 0 or n > INT32_MAX / 64.
 * skred_fxbank_ctl_owned  skred_fxbank_ctl_list under the guard owner[voice] == tags[k].  d_result (device uint32[3], may be NULL):
 *                         [0] voices written, [1] stores withheld, [2] voices whose owner differs.  Refused: what _ctl_list refuses,
 *                         NULL tags, a zero tag.
 * LIMIT, as for notes: the host view goes stale; mirror the values before a later skred_fxbank_update with SKRED_DIRTY_PARAMS or
 * SKRED_DIRTY_PAN of such a voice.  skred_fxbank_download_params reads them back where the host cannot know them (a scaled
 * increment, a withheld amp): every parameter field of the host view that skred_fxbank_download leaves out -- phase_inc,
 * table_offset, log2_size, amp_q15, the pans, the five flags (as 0 / 1), the envelope's frame counts, sustain_q15, velocity_q15,
 * smoother_k_q15, sample_start, sample_release, the five coefficients -- as the device holds it; recip_out (may be NULL) receives
 * the three reciprocals of each voice, uint32[count][3].  Synchronous; windows as skred_fxbank_download. */
typedef struct skred_fx_ctl {             /* 80 bytes */
  uint32_t which;                         /* SKRED_CTL_* of the fields below */
  uint32_t phase_inc, inc_scale_q16;
  int32_t  amp_q15, pan_left_q15, pan_right_q15;
  int32_t  b0_q30, b1_q30, b2_q30, a1_q30, a2_q30;
  uint32_t attack_frames, decay_frames, release_frames;
  int32_t  sustain_q15, velocity_q15, smoother_k_q15;
  uint32_t reserved[3];                   /* 0 */
} skred_fx_ctl_t;
int  skred_fxbank_tag_list(skred_fxbank_t *fx, const int32_t *d_voices, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                           uint32_t *d_result, void *stream);
int  skred_fxbank_find_owned(skred_fxbank_t *fx, int first, int count, const uint32_t *tags, int n, int32_t *d_voices_out, void *stream);
int  skred_fxbank_stamp_owned(skred_fxbank_t *fx, const int32_t *d_voices, const uint32_t *tags, int n, const uint32_t *d_count_or_null,
                              uint32_t stamps, uint32_t *d_result, void *stream);
int  skred_fxbank_release_tags(skred_fxbank_t *fx, int first, int count, const uint32_t *tags, int n, uint32_t stamps,
                               uint32_t *d_result, void *stream);
int  skred_fxbank_owner_clear(skred_fxbank_t *fx, int first, int count, void *stream);
int  skred_fxbank_download_owners(skred_fxbank_t *fx, uint32_t *host_u32, int first, int count);
int  skred_fx_ctl_check(const skred_fx_ctl_t *ctl);
int  skred_fxbank_ctl_range(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, int first, int count, uint32_t *d_result, void *stream);
int  skred_fxbank_ctl_list(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const int32_t *d_voices, int n, const uint32_t *d_count_or_null,
                           uint32_t *d_result, void *stream);
int  skred_fxbank_ctl_owned(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const int32_t *d_voices, const uint32_t *tags, int n,
                            const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
int  skred_fxbank_download_params(skred_fxbank_t *fx, skred_fxpt_bank_t *host, uint32_t *recip_out, int src_first, int dst_first, int count);

/* ---- channels and per-note expression: masked owner matches, per-entry controller values -----------------------------------
 *
 * The fixed-point twin of the float bank's section of the same name (include/skred_amd.h: skred_bank_find_match .. _ctl_tags_each),
 * with the same vocabulary: a host that tags notes as channel << 24 | note id has "all notes off on channel 3", "mod wheel on
 * channel 3", "how many notes does channel 3 hold" and n different bends on n notes as ONE device call each, instead of
 * skred_fxbank_download_owners behind a device wait, a pick on the host and an uploaded list, or n skred_fxbank_ctl_owned calls.
 * This bank has no slots: everything is per voice (the float calls at K = 1, voice_mask = 1).
 *
 * Every call is asynchronous on the caller's stream and ordered like skred_fxbank_update; host arrays travel through the ring of
 * SKRED_FX_RING_SLOTS staging slots, so the caller's memory is free on return and nothing waits for the device -- except
 * skred_fxbank_find_match_host, which waits for its stream ONLY.  The owner array is the one of the section above, allocated by the
 * first call that needs it exactly as there; these calls read it and never write it.  No render kernel reads anything these calls
 * add: a bank that makes match queries renders the blocks of a bank that makes none, bit for bit.  Every refusal comes before
 * anything touches the device.  One stream at a time per bank, as for the queries (the list shares their scratch).  On a shard:
 * through skred_fxshard_bank(), with that rank's local indices.
 * Out of scope: slots (K > 1), the deferred queue and pattern steps, the drop-in mode.
 *
 * A. Masked matches.  skred_owner_match_t and skred_owner_match_check are the float bank's, as they are.  A voice MATCHES m when
 * owner != 0 && (owner & m->mask) == m->value: mask 0 with value 0 is every tagged voice, mask 0xFF000000 a channel byte, mask
 * 0xFFFFFFFF one note.  An untagged voice matches nothing.
 *
 * skred_fxbank_find_match       the matching voices of [first, first + count), ascending, into d_voices[0 .. min(total, max_out))
 *                               (device int32); d_count[0] (device uint32[1]) = the TOTAL, whether or not the list was cut short.
 *                               max_out == 0: the count alone (d_voices may be NULL).  Entries past min(total, max_out) are not
 *                               written.  The same state gives the same bytes: the compaction is ordered by index, no workgroup
 *                               waits for another, and it is the float bank's (sk_match_count_kernel / _scatter_kernel) on the
 *                               scratch of skred_fxbank_find_idle.  SKRED_E_BAD_ARG: NULL bank, match or d_count, what
 *                               skred_owner_match_check refuses, max_out < 0, NULL d_voices with max_out > 0; SKRED_E_RANGE:
 *                               count <= 0 or a range outside the bank.
 * skred_fxbank_find_match_host  the same into host memory, waiting for `stream` only: returns the number of voices written to
 *                               voices[0 .. max_out) or a negative SKRED_E_* code; *total_out (may be NULL) = the total.
 * skred_fxbank_stamp_match      skred_fxbank_stamp_list's stores on EVERY matching voice of the range -- all notes off on a channel
 *                               -- in one pass, with no list in between; `now` is the bank's sample count at the call.  d_result
 *                               (device uint32[2], required), cleared on the stream ahead of the kernel: [0] voices stamped,
 *                               [1] voices of the range that did not match.  Refusals of _find_match about bank, match and range;
 *                               SKRED_E_BAD_ARG for a NULL d_result, no or unknown stamp bits.
 * skred_fxbank_ctl_match        skred_fxbank_ctl_range under the match guard: the same stores, the same two withheld-store rules,
 *                               on the matching voices only.  d_result (device uint32[3], may be NULL): [0] voices written,
 *                               [1] stores withheld, [2] voices of the range that did not match.  Refused: what skred_fx_ctl_check
 *                               and skred_owner_match_check refuse, a NULL bank; SKRED_E_RANGE as for _find_match.
 *
 * B. Per-entry controller values.  skred_fxbank_ctl_owned stores ONE record on all n listed notes; here entry k of the list brings a
 * small record of its own (skred_fx_ctl_each_t, `set` made of the float bank's SKRED_EACH_* bits, reserved words 0), whose named
 * values replace or scale the record's for that entry alone.  Exact integer arithmetic, field by field:
 *   SKRED_EACH_INC_SCALE  phase_inc = ((uint64)phase_inc * inc_scale_q16) >> 16 on the DEVICE's value, the product in 64 bits,
 *                         65536 = 1.0 -- SKRED_CTL_INC_SCALE's rule: a result above 0xFFFFFFFF is NOT stored (the voice keeps its
 *                         increment) and is counted in d_result[1]; exactly 0xFFFFFFFF is stored.  Per-note pitch bend.
 *   SKRED_EACH_AMP_SCALE  needs the record to name SKRED_CTL_AMP: the amp stored is ((uint64)ctl->amp_q15 * amp_scale_q16) >> 16,
 *                         under SKRED_CTL_AMP's device-side guard (a voice whose amp_q15 is 0 keeps it and is counted).  A result
 *                         of 0 or above 65535 is withheld and counted in d_result[1], and the voice's amp is left alone -- the amp
 *                         guard then does not look at the voice, so it cannot count it a second time; exactly 1 and exactly 65535
 *                         are stored.  amp_scale_q16 == 0 is refused.  Polyphonic aftertouch.
 *   SKRED_EACH_VELOCITY   the entry's velocity_q15 (0..65535) replaces the record's, or supplies it where the record does not
 *                         name the field.
 *   SKRED_EACH_PAN        the same for pan_left_q15, pan_right_q15, each 0..65535.
 * The withheld stores add up to at most 2 per voice (one for the increment, one for the amp).  Everything else the record names is
 * stored as skred_fxbank_ctl_owned stores it.  `ctl` may be NULL: no base record, the entries supply everything (AMP_SCALE is then
 * refused).
 *
 * skred_fx_ctl_each_check       pure host: SKRED_OK, or SKRED_E_BAD_ARG for NULL each, n < 0; with ctl != NULL what
 *                               skred_fx_ctl_check refuses; in an entry: unknown bits in set, set == 0, a non-zero reserved word, a
 *                               named value outside its range, amp_scale_q16 == 0 under AMP_SCALE; AMP_SCALE where ctl is NULL or
 *                               does not name SKRED_CTL_AMP; INC_SCALE where ctl names SKRED_CTL_PHASE_INC or SKRED_CTL_INC_SCALE.
 *                               Values an entry does not name are not looked at (and never shipped).
 * skred_fxbank_ctl_owned_each   entry k (of the first min(n, *d_count_or_null)) acts only if d_voices[k] lies in [0, n_voices) AND
 *                               owner[voice] == tags[k] (non-zero); -1 holes and entries outside the bank are skipped.  On that
 *                               voice it performs skred_fxbank_ctl_owned's stores with each[k] laid over the record.  d_result
 *                               (device uint32[3], may be NULL): [0] voices written, [1] stores withheld (the two guards and the
 *                               amp products), [2] voices whose owner differs.  A voice listed twice gets the absolute stores twice;
 *                               a scaled increment on such a voice is UNSPECIFIED, as for skred_fxbank_ctl_list.  Refused: what
 *                               skred_fx_ctl_each_check refuses, NULL bank, list or tags, a zero tag, n > INT32_MAX / 64.
 *                               n == 0: SKRED_OK, nothing is done.
 * skred_fxbank_ctl_tags_each    expression by note id: skred_fxbank_find_owned of the tags over [first, first + count) into the
 *                               scratch of skred_fxbank_release_tags, then the call above on that list -- built as _release_tags
 *                               is.  each[k] goes with tags[k]: the tags travel sorted, and the entries are permuted with them on
 *                               the host.  Tags unique, none zero, n <= SKRED_OWNER_MAX_TAGS; each tag reaches at most ONE voice,
 *                               the lowest that carries it.  d_result as above; [2] is 0 (a tag nobody carries is a -1 entry and
 *                               is not counted).  Refusals of both calls.
 * LIMIT, as for the controllers: the host view goes stale; skred_fxbank_download_params reads the values back. */
typedef struct skred_fx_ctl_each {        /* 32 bytes */
  uint32_t set;                           /* SKRED_EACH_* of the values below */
  uint32_t inc_scale_q16, amp_scale_q16;
  int32_t  velocity_q15, pan_left_q15, pan_right_q15;
  uint32_t reserved[2];                   /* 0 */
} skred_fx_ctl_each_t;
int  skred_fxbank_find_match(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, int max_out, int32_t *d_voices,
                             uint32_t *d_count, void *stream);
int  skred_fxbank_find_match_host(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, int max_out, int32_t *voices,
                                  int *total_out, void *stream);
int  skred_fxbank_stamp_match(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, uint32_t stamps, uint32_t *d_result,
                              void *stream);
int  skred_fxbank_ctl_match(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, int first, int count, const skred_owner_match_t *m,
                            uint32_t *d_result, void *stream);
int  skred_fx_ctl_each_check(const skred_fx_ctl_each_t *each, int n, const skred_fx_ctl_t *ctl);
int  skred_fxbank_ctl_owned_each(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const skred_fx_ctl_each_t *each, const int32_t *d_voices,
                                 const uint32_t *tags, int n, const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
int  skred_fxbank_ctl_tags_each(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl, const skred_fx_ctl_each_t *each, int first, int count,
                                const uint32_t *tags, int n, uint32_t *d_result, void *stream);

/* C. Per-note timbre: per-entry filter coefficients.  The per-voice twin of the float bank's section C (include/skred_amd.h:
 * skred_bank_ctl_owned_each_filter / _ctl_tags_each_filter) at K = 1, without masks: the two calls of B with one more array, entry k
 * also bringing the five Q2.30 coefficients of its voice -- key tracking, velocity-to-cutoff, MPE timbre (CC 74), n notes with n
 * cutoffs in one call instead of n skred_fxbank_ctl_owned calls.  The five words are stored as SKRED_CTL_FILTER stores them on this
 * bank: any int32; filter_mode and the delay line are untouched, and on a voice without a filter the words are inert.  Entry k
 * acts exactly as it does in B (a voice of the bank whose owner is tags[k]); the record and each[k] are stored as there, under the
 * same withheld-store rules.  `each` may be NULL here: the coefficients only; `ctl` may be NULL as in B.  d_result keeps its three
 * words and their meaning.
 *
 * skred_fx_filter_each_check          pure host: SKRED_OK, or SKRED_E_BAD_ARG for NULL filt, n < 0, a non-zero reserved word; with
 *                                     ctl != NULL what skred_fx_ctl_check refuses, and a ctl that itself names SKRED_CTL_FILTER
 *                                     (two sets of coefficients for one voice: ambiguous).
 * skred_fxbank_ctl_owned_each_filter  skred_fxbank_ctl_owned_each with filt[k] beside each[k]; the arrays and the tags travel in one
 *                                     staged batch, one kernel reads them.  Refused: what _ctl_owned_each refuses (a NULL `each`
 *                                     excepted) and what skred_fx_filter_each_check refuses.  n == 0: SKRED_OK.
 * skred_fxbank_ctl_tags_each_filter   skred_fxbank_ctl_tags_each with filt[k] beside tags[k]: the tags travel sorted, and filt is
 *                                     permuted on the host with each by the same permutation.  Refusals of both.
 * Out of scope: the deferred queue and pattern steps, the drop-in mode.  Coefficients computed on the device, in integers, from a
 * cutoff kept beside the voice: section "filter cutoff" below (these calls go on bringing finished words, which the host makes with
 * skred_filter_coeffs of include/skred_amd.h in fp32 and converts to Q2.30 itself, as for skred_fxbank_upload).
 * LIMIT, as for the controllers: the host view goes stale; skred_fxbank_download_params reads the values back. */
typedef struct skred_fx_filter_each {     /* 32 bytes */
  int32_t  b0_q30, b1_q30, b2_q30, a1_q30, a2_q30;
  uint32_t reserved[3];                   /* 0 */
} skred_fx_filter_each_t;
int  skred_fx_filter_each_check(const skred_fx_filter_each_t *filt, int n, const skred_fx_ctl_t *ctl_or_null);
int  skred_fxbank_ctl_owned_each_filter(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl_or_null, const skred_fx_ctl_each_t *each_or_null,
                                        const skred_fx_filter_each_t *filt, const int32_t *d_voices, const uint32_t *tags, int n,
                                        const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
int  skred_fxbank_ctl_tags_each_filter(skred_fxbank_t *fx, const skred_fx_ctl_t *ctl_or_null, const skred_fx_ctl_each_t *each_or_null,
                                       const skred_fx_filter_each_t *filt, int first, int count, const uint32_t *tags, int n,
                                       uint32_t *d_result, void *stream);

/* ---- channel polyphony: stealing inside one channel, note-ons under a cap ---------------------------------------------------
 *
 * The fixed-point twin of the float bank's section of the same name (include/skred_amd.h: skred_bank_find_steal_slots_match ..
 * skred_bank_note_on_channel).  A channel can be swept, bent and silenced (the section above); these calls let it ALLOCATE.
 * skred_fxbank_find_steal ranks every sounding voice of a range, whoever owns it -- a burst on the pad channel takes the bass line's
 * notes -- and nothing limits how many voices a channel holds.  The host cannot enforce a limit: the number of sounding voices of a
 * channel is device state, and the only correct host route is skred_fxbank_download_owners plus skred_fxbank_download behind a device
 * wait.  This bank has no slots: every call is per voice (the float call at K = 1, voice_mask = 1).  skred_owner_match_t,
 * skred_owner_match_check, SKRED_CHAN_NO_CAP and the SKRED_STEAL_* / SKRED_IDLE_* bits keep their meaning and values.
 *
 * On the words AS THE DEVICE HOLDS THEM at that point of the stream, every comparison exact (q: the skred_fx_steal_query_t, m: the
 * match; released, age, class, primary, key and order are exactly those of skred_fxbank_find_steal):
 *   match(o)      o != 0  &&  (o & m.mask) == m.value                          (skred_owner_match_t's rule)
 *   sounding(v)   v lies in [first, first + count)  &&  match(owner[v])  &&  use_envelope != 0  &&  is_active != 0
 *                 &&  NOT (exclude_idle != 0  &&  v satisfies skred_fxbank_find_idle's predicate for (exclude_idle, settle_q15))
 *   candidate(v)  sounding(v)  &&  age >= min_age  &&  (released, under SKRED_STEAL_RELEASED_ONLY)
 *   order         ascending key, ties by ascending voice index
 * An untagged voice (owner 0) is never sounding in this sense: it is neither counted nor stolen.  A voice that does not match costs
 * one owner word and no plane read.
 *
 * skred_fxbank_find_steal_match is skred_fxbank_find_steal under its contract (asynchronous, reads the bank and the owner array only,
 * the same state gives the same bytes, the bank's steal scratch -- one stream at a time --, no workgroup ever waits for another),
 * restricted to the match: d_voices[0 .. written) = the first min(total, max_out) victims; d_count (device, uint32[3]):
 *   [0]  written = min(total, max_out)
 *   [1]  total candidates
 *   [2]  the sounding voices of the match in the range -- the channel's current polyphony
 * Entries past `written` are not touched.  max_out == 0: a census of the channel in one launch.  With mask == 0 and every sounding
 * voice tagged the list and d_count[0..1] are skred_fxbank_find_steal's bytes.  The first call allocates the owner array as the note
 * owners' section says.  Refused before anything touches the device: what skred_fx_steal_check and skred_owner_match_check refuse, and
 * SKRED_E_BAD_ARG for a NULL bank, query or d_count, or a NULL d_voices with max_out > 0. */
int  skred_fxbank_find_steal_match(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, const skred_owner_match_t *m,
                                   int32_t *d_voices, uint32_t *d_count, void *stream);
/* The same into host memory; waits for `stream` only.  Returns `written` (>= 0) or a SKRED_E_* code; *total_out and *sounding_out
 * may be NULL. */
int  skred_fxbank_find_steal_match_host(skred_fxbank_t *fx, const skred_fx_steal_query_t *q, const skred_owner_match_t *m,
                                        int32_t *voices, int *total_out, int *sounding_out, void *stream);
/* A burst of n notes of ONE channel under a polyphony cap: skred_fxbank_note_on_steal with three differences, all decided on the
 * device.  With
 *   I = the idle voices idle_q lists, at most n,
 *   S = the channel's sounding count: d_count[2] of the matched query above, run with steal_q and m,
 *   V = the victims that query wrote,
 * the burst is split as
 *   a = min(n, I, cap > S ? cap - S : 0)   notes take the first a idle voices            (idle voices are limited by the cap),
 *   b = min(n - a, V)                      notes take the channel's own victims, in victim order (stealing stays inside the channel),
 *   the remaining n - a - b notes are dropped,
 * and every placed note k's voice gets owner = tags[k], as skred_fxbank_tag_list on d_assigned would write it (a thief's tag
 * overwrites its victim's).  d_result (device, uint32[4], required): [0] placed, [1] dropped, [2] stolen (b), [3] S as seen before the
 * burst.  d_assigned as for skred_fxbank_notes_on_list.
 * Consequences: a channel at or below its cap never exceeds it; a channel above a lowered cap does not grow (a = 0: every note
 * steals one of its own); a burst cannot steal from itself (both lists are made before a note is placed, and they are disjoint: a
 * victim is never a voice the idle list offers) or from another channel (only voices that match are ranked); cap = 1 with
 * min_age = 0 is mono mode -- the new note takes the old one's voice; SKRED_CHAN_NO_CAP never limits.  There is no bank-wide fallback:
 * victims come from the channel only -- a host that wants one calls skred_fxbank_note_on_steal.
 * The library overrides steal_q's exclude_idle, settle_q15 and max_out exactly as skred_fxbank_note_on_steal does.  Five steps on
 * `stream`: the idle query, the matched key pass and its select, one one-workgroup join kernel, the note launch, the owner-tag launch.
 * The notes and the tags travel through the staging ring (two slots); the host never learns the counts and waits for nothing.
 * skred_fx_chan_check is the pure-host statement of what is refused before anything touches the device: what skred_fx_idle_check
 * (with max_out = n), skred_fx_steal_check (with the overrides) and skred_owner_match_check refuse; SKRED_E_BAD_ARG for a NULL query,
 * n < 0, SKRED_IDLE_AMP_ZERO in idle_q->which, NULL tags, n > INT32_MAX / 64 (skred_fxbank_tag_list's bound), a tag that is 0 or does
 * not satisfy m (such a note would not count towards its own channel).  Every cap is accepted.  The entry point also refuses a NULL
 * bank, notes or d_result and what skred_fx_notes_check refuses.  n == 0: SKRED_OK, nothing is done.  On a shard: through
 * skred_fxshard_bank(), with that rank's local indices. */
int  skred_fx_chan_check(const skred_fx_idle_query_t *idle_q, const skred_fx_steal_query_t *steal_q, const skred_owner_match_t *m,
                         uint32_t cap, const uint32_t *tags, int n, int n_voices);
int  skred_fxbank_note_on_channel(skred_fxbank_t *fx, const skred_fx_idle_query_t *idle_q, const skred_fx_steal_query_t *steal_q,
                                  const skred_owner_match_t *m, uint32_t cap, const skred_fx_note_t *notes, const uint32_t *tags,
                                  int n, int32_t *d_assigned, uint32_t *d_result, void *stream);

/* ---- pedals: sustain and sostenuto hold note-offs back on the device --------------------------------------------------------
 *
 * The fixed-point, per-voice twin of the float bank's section "pedals" (include/skred_amd.h: skred_pedal_check ..
 * skred_bank_download_pedals): that section read at slot_voices = 1, voice_mask = 1 -- this bank has no slots.  SKRED_PEDAL_PENDING /
 * _LATCHED, SKRED_PEDAL_LIFT_SUSTAIN / _LIFT_SOSTENUTO / _SUSTAIN_DOWN, SKRED_PEDAL_CALL_*, skred_owner_match_t,
 * skred_owner_match_check and skred_owner_tags_check are that header's, values and meaning unchanged.  A host that plays this bank
 * through skred_fxbank_note_on_channel steals on the device, so a pending note-off kept on the host would release the wrong note
 * after a theft; the only other correct route is skred_fxbank_download_owners plus skred_fxbank_download behind a device wait on
 * every pedal-up.
 *
 * pedal[n_voices] is a uint32 array in device memory, one word per voice, that only the calls of this section read or write.
 * SKRED_PEDAL_PENDING: a note-off arrived and was held back.  SKRED_PEDAL_LATCHED: sostenuto caught this note.  The first call of
 * this section other than _pedal_clear and _download_pedals allocates it (4 bytes per voice) and zero-fills it, and ensures the owner
 * array too; that call waits for the device once, as the first owner call does.  It is freed with the bank.  No render kernel reads
 * the word: blocks rendered with and without pedal calls that hold nothing are bit-identical, and a bank that never makes a pedal
 * call launches nothing more than it did before this section existed.
 *
 * A NEW NOTE CLEARS THE WORD.  Once the array exists, every tag launch of the bank (skred_fxbank_tag_list, the tags of
 * skred_fxbank_note_on_channel) is followed on its stream by a launch that stores 0 into the pedal word of every voice it tagged --
 * the same list, the same min(n, *d_count) rule, the same "is a voice" rule.  So a thief's tags clear its victim's bits, and a key
 * struck again under the pedal (the same voice in mono mode) starts clean: the pedal-up releases the old note-off's voice only if the
 * old note is still the one that sounds there.
 *
 * HELD(v):  use_envelope != 0  &&  is_active != 0  &&  sample_release == 0  -- the terms candidate and released of
 * skred_fxbank_find_steal, on the words as the device holds them at that point of the stream.
 *
 * PARTICULAR TO THIS BANK: SKRED_STAMP_RELEASE writes the release clock only while is_active is set (skred_fxbank_stamp_list's rule).
 * skred_fxbank_pedal_up and skred_fxbank_stamp_owned_pedal count a voice whose envelope is not active as released or stamped all the
 * same, exactly as skred_fxbank_stamp_owned counts it today; its clock stays as it was, and PENDING is cleared.
 *
 * All calls are asynchronous on `stream` and ordered like skred_fxbank_update; host arrays travel through the staging ring; nothing
 * waits for the device; results are pure functions of the state, whatever the order of arrival; one stream at a time per bank.  On a
 * shard: through skred_fxshard_bank(), with that rank's local indices.
 *
 * Stated behaviour: a pending note ranks in the steal queries as the held note it is (its envelope has no release clock).
 * skred_fxbank_stamp_match / _release_tags / _stamp_owned on a pending voice stamp at once and LEAVE the bit: a later pedal_up stamps
 * again -- "all notes off" under a pedal is therefore skred_fxbank_pedal_up or _pedal_clear first.
 * Out of scope: the drop-in mode, deferred items, pattern steps.
 *
 * skred_fx_pedal_check            pure host, no device: what the entry point named by `call` refuses about everything but its
 *                                 pointers to the bank, the list and the result, in the order it checks -- the return codes and the
 *                                 order of skred_pedal_check(call, n_voices, first, count, 1, 1, m, flags, tags, n).  Every entry
 *                                 point below calls it before anything touches the device; a refused call writes nothing.
 * skred_fxbank_stamp_owned_pedal  looks at the entries below min(n, *d_count_or_null).  An entry that is no voice of the bank: [2].
 *                                 owner[v] != tags[k]: [1].  Otherwise, hold_all != 0 or a LATCHED word: pedal[v] |= PENDING,
 *                                 nothing is stamped, [3].  Otherwise skred_fxbank_stamp_owned's SKRED_STAMP_RELEASE with the bank's
 *                                 sample count as the clock, [0].  d_result (device, uint32[4], required) is cleared on the stream
 *                                 ahead of the kernel.  An entry named twice stores the same words twice and is counted twice.  With
 *                                 hold_all == 0 and nothing latched, the bank's bytes and words 0..2 are those of
 *                                 skred_fxbank_stamp_owned(..., SKRED_STAMP_RELEASE, ...).  n == 0: SKRED_OK, nothing is done.
 *                                 Refused: NULL bank, list or result, what skred_fx_pedal_check(STAMP_OWNED) refuses.
 * skred_fxbank_release_tags_pedal note-off by note id: skred_fxbank_release_tags' find pass into the same scratch -- the lowest voice
 *                                 of [first, first + count) per tag, or -1 -- then the call above on that list, in one staged batch.
 *                                 [1] is 0; [2] counts the tags nobody in the range carries.  Refused: NULL bank or result, what
 *                                 skred_fx_pedal_check(RELEASE_TAGS) refuses.
 * skred_fxbank_pedal_latch        sostenuto down, one pass over the range, no list: a voice that matches m gets LATCHED when its
 *                                 PENDING bit is clear and it is HELD.  Notes struck later are not caught (their tags clear the
 *                                 word), nor notes whose note-off is already pending.  d_result (device, uint32[2], required),
 *                                 cleared ahead of the kernel: [0] voices that satisfy the rule (latched now or before), [1] voices
 *                                 of the range that did not match.  Only matching voices read a plane; no plane is written.
 *                                 Refused: NULL bank or result, what skred_fx_pedal_check(LATCH) refuses.
 * skred_fxbank_pedal_up           a pedal goes up, one pass over the matching voices of the range.  flags: at least one of
 *                                 LIFT_SUSTAIN and LIFT_SOSTENUTO; SUSTAIN_DOWN is refused together with LIFT_SUSTAIN.
 *                                 LIFT_SOSTENUTO clears LATCHED.  A voice that is then PENDING, not LATCHED and not kept by
 *                                 SUSTAIN_DOWN gets the release stamp with THIS call's clock and loses PENDING.  d_result (device,
 *                                 uint32[3], required), cleared ahead of the kernel: [0] voices released, [1] voices still pending,
 *                                 [2] voices of the range that did not match.  The word is stored only when it changed.
 *                                 Refused: NULL bank or result, what skred_fx_pedal_check(UP) refuses.
 * skred_fxbank_pedal_clear        pedal[first .. first + count) = 0 on `stream`; nothing to do on a bank without the array.
 *                                 SKRED_E_RANGE: count < 0 or a range outside the bank.
 * skred_fxbank_download_pedals    the words of [first, first + count) into host_u32; waits for the device, like
 *                                 skred_fxbank_download_owners; zeros on a bank without the array. */
int  skred_fx_pedal_check(int call, int n_voices, int first, int count, const skred_owner_match_t *m, uint32_t flags,
                          const uint32_t *tags, int n);
int  skred_fxbank_stamp_owned_pedal(skred_fxbank_t *fx, const int32_t *d_voices, const uint32_t *tags, int n,
                                    const uint32_t *d_count_or_null, int hold_all, uint32_t *d_result, void *stream);
int  skred_fxbank_release_tags_pedal(skred_fxbank_t *fx, int first, int count, const uint32_t *tags, int n, int hold_all,
                                     uint32_t *d_result, void *stream);
int  skred_fxbank_pedal_latch(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, uint32_t *d_result, void *stream);
int  skred_fxbank_pedal_up(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, uint32_t flags, uint32_t *d_result,
                           void *stream);
int  skred_fxbank_pedal_clear(skred_fxbank_t *fx, int first, int count, void *stream);
int  skred_fxbank_download_pedals(skred_fxbank_t *fx, uint32_t *host_u32, int first, int count);

/* ---- portamento: pitch glides that advance and land on the device, in integers ------------------------------------------------
 *
 * The fixed-point twin of the float bank's section "portamento" (include/skred_amd.h: skred_glide_check .. skred_bank_download_glide),
 * per voice -- this bank has no slots, so no slot_voices and no masks.  The float definition rests on one fp32 product per step, on
 * signs and on non-finite values; none of that exists here.  THIS is the place of record for the integer definition: the same bits on
 * every machine, an exact landing, and increments that do not depend on how the host cuts its blocks.  The only other route on this
 * bank is one skred_fxbank_ctl_tags_each(SKRED_EACH_INC_SCALE) per block from the host, which must keep the list of gliding notes,
 * never lands on the struck key's increment (a Q16 multiply of a truncated product), and stalls outright on small increments,
 * where (inc * 65542) >> 16 == inc.
 *
 * STATE.  glide[n_voices] is an array of four uint32 per voice in device memory (one 16-byte word): target, up_q32, down_q32, carry.
 * target == 0 means "not gliding": a phase_inc of 0 is a voice without pitch and is never a legal start or target.  The first call
 * that starts a glide (skred_fxbank_glide_owned / _glide_tags with n > 0) allocates the array (16 bytes per voice) beside the owner
 * and pedal arrays and zero-fills it, and ensures the owner array too; that call waits for the device once.  It is freed with the
 * bank.  Only the calls of this section (and the clear below) read or write it, and the only bank word they store is phase_inc, as a
 * word store: its neighbours in the plane keep their bits.  No render kernel reads the array; a bank that never starts a glide
 * allocates nothing more and launches nothing more than it did before this section existed.
 *
 * ENTRY.  skred_fx_glide_t: `set` holds exactly one of three bits.  With inc = the voice's phase_inc as the device holds it:
 *   SKRED_FX_GLIDE_FROM_SCALE  target = inc, then inc = ((uint64)inc * scale_q16) >> 16 -- slide INTO the note from the previous key.
 *                              scale_q16 is SKRED_EACH_INC_SCALE's Q16: 65536 = 1.0.
 *   SKRED_FX_GLIDE_TO_SCALE    target = ((uint64)(gliding ? the old target : inc) * scale_q16) >> 16; inc stays.  A chain of these
 *                              composes on the old target, not on wherever the glide happens to be.
 *   SKRED_FX_GLIDE_TO_INC      target = target_inc; inc stays.  Legato onto a key whose increment the host knows -- the bank is per
 *                              voice, so it does -- and the glided note lands on the struck note's bits.  Q16 TO_SCALE cannot promise
 *                              that landing.
 * up_q32 and down_q32 (both non-zero) are the rates: 1 + up_q32 / 2^32 and 1 - down_q32 / 2^32 per 64 frames, far finer than Q16.
 * A start whose inc, new inc or target would be 0 or above 0xFFFFFFFF stores nothing and is counted as withheld: the voice and its
 * glide words stay as they were.  A start that stores sets carry = 0 and replaces a glide the voice was in.
 *
 * ADVANCE BY F FRAMES.  For every voice of [first, first + count) with target != 0:
 *   1. c = carry + F; c >> 6 steps are taken; the new carry is c & 63.
 *   2. Before the first step (and when there is none to take), a voice with inc == 0 or inc == target arrives at once.
 *   3. A step with inc < target:  next = inc + max(1, ((uint64)inc * up_q32) >> 32), in 64 bits; the voice arrives when next >= target.
 *   4. A step with inc > target:  next = inc - max(1, ((uint64)inc * down_q32) >> 32); the voice arrives when next <= target.
 *      (down_q32 <= 2^32 - 1: the subtrahend never exceeds inc.)
 *   5. On arrival the target's bits are stored in phase_inc and the four words are zeroed.
 *   6. Otherwise the last `next` is stored (only if it differs from what the voice held) and carry is written.
 * max(1, ...) guarantees progress: an LFO-rate increment cannot stall.  The loop runs at most F / 64 + 1 times.  Because of the
 * carry, the increment at every multiple of 64 frames does not depend on the block sizes the host advances by.
 *
 * A NEW NOTE CLEARS THE WORDS.  Once the array exists, every tag launch of the bank (skred_fxbank_tag_list, the tags of
 * skred_fxbank_note_on_channel) is followed on its stream by a launch that zeroes the four words of every voice it tagged -- the same
 * list under the same list rule, right where the pedal word is cleared.  A thief or a re-struck key does not inherit a glide.  The
 * order for mono legato is therefore skred_fxbank_note_on_channel, then skred_fxbank_glide_tags(FROM_SCALE).
 *
 * All calls are asynchronous on `stream` and ordered like skred_fxbank_update; host arrays travel through the staging ring; nothing
 * waits for the device except the download and the first allocation; results are pure functions of the state, whatever the order of
 * arrival; one stream at a time per bank.  On a shard: through skred_fxshard_bank(), with that rank's local indices.
 *
 * skred_fx_glide_check       pure host: SKRED_OK, or SKRED_E_BAD_ARG for NULL glide, n < 0, and per entry: `set` not exactly one of
 *                            the three bits, a non-zero reserved word, up_q32 == 0 or down_q32 == 0, scale_q16 == 0 on the two scale
 *                            forms, target_inc == 0 on TO_INC.  Values the form does not use are not looked at.
 * skred_fxbank_glide_owned   looks at the entries below min(n, *d_count_or_null); entry k starts glide[k] on d_voices[k] where that is
 *                            a voice of the bank whose owner is tags[k].  d_result (device uint32[3], may be NULL; cleared on the
 *                            stream ahead of the kernel): [0] voices set gliding, [1] starts withheld, [2] voices whose owner differs.
 *                            A voice listed twice is UNSPECIFIED.  Refused before anything touches the device: NULL bank or list,
 *                            what skred_owner_tags_check refuses (NULL tags, n < 0, a zero tag), n > INT32_MAX / 64, what
 *                            skred_fx_glide_check refuses -- in that order.  n == 0: SKRED_OK, nothing is done.
 * skred_fxbank_glide_tags    glides by note id: skred_fxbank_release_tags' find pass over [first, first + count) into the same
 *                            scratch -- the lowest voice of the range per tag, or -1 -- then the call above on that list.  glide[k]
 *                            goes with tags[k]: the tags travel sorted, and the entries are permuted with them on the host.  Tags
 *                            unique, none zero, n <= SKRED_OWNER_MAX_TAGS.  d_result as above; [2] is 0.  Refused: NULL bank, the
 *                            tags, n and the entries as above, then SKRED_E_RANGE for an empty range or one outside the bank.
 * skred_fxbank_glide_advance the advance pass; call it once per rendered block with the block's frames.  num_frames 1 .. 65536.
 *                            d_result (device uint32[2], may be NULL; cleared ahead of the kernel): [0] voices still gliding,
 *                            [1] voices that arrived.  It ships no bytes and takes no slot of the ring.  On a bank without the array:
 *                            SKRED_OK, and d_result is cleared on the stream.  Refused: NULL bank, num_frames out of range
 *                            (SKRED_E_BAD_ARG), an empty range or one outside the bank (SKRED_E_RANGE).
 * skred_fxbank_glide_stop    glide[first .. first + count) = 0 on `stream`; snap != 0: a gliding voice's phase_inc = its target
 *                            first.  Nothing to do on a bank without the array.  SKRED_E_RANGE: count < 0 or a range outside the bank.
 * skred_fxbank_download_glide  the words of [first, first + count) into host_u32x4 (4 * count words); waits for the device; zeros on
 *                            a bank without the array.
 * LIMITS, documented, not fixed: a SKRED_CTL_PHASE_INC / _INC_SCALE bend of a gliding voice is undone on arrival (the target's bits
 * are stored) -- a bend of the section "pitch wheel" below is not: the glide then runs on the key and lands on target * ratio;
 * the host view of phase_inc goes stale -- skred_fxbank_download_params reads it back; glides belong with tagged notes
 * (an untagged voice cannot be reached).  Out of scope: the drop-in mode, deferred items, pattern steps, per-frame glides. */
#define SKRED_FX_GLIDE_FROM_SCALE (1u << 0)
#define SKRED_FX_GLIDE_TO_SCALE   (1u << 1)
#define SKRED_FX_GLIDE_TO_INC     (1u << 2)
typedef struct skred_fx_glide {           /* 32 bytes */
  uint32_t set;                           /* exactly one SKRED_FX_GLIDE_* */
  uint32_t up_q32, down_q32;              /* per 64 frames: x (1 + up / 2^32), x (1 - down / 2^32); both non-zero */
  uint32_t scale_q16;                     /* FROM_SCALE, TO_SCALE: 65536 = 1.0 */
  uint32_t target_inc;                    /* TO_INC */
  uint32_t reserved[3];                   /* 0 */
} skred_fx_glide_t;
int  skred_fx_glide_check(const skred_fx_glide_t *glide, int n);
int  skred_fxbank_glide_owned(skred_fxbank_t *fx, const skred_fx_glide_t *glide, const int32_t *d_voices, const uint32_t *tags, int n,
                              const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
int  skred_fxbank_glide_tags(skred_fxbank_t *fx, const skred_fx_glide_t *glide, int first, int count, const uint32_t *tags, int n,
                             uint32_t *d_result, void *stream);
int  skred_fxbank_glide_advance(skred_fxbank_t *fx, int first, int count, int num_frames, uint32_t *d_result, void *stream);
int  skred_fxbank_glide_stop(skred_fxbank_t *fx, int first, int count, int snap, void *stream);
int  skred_fxbank_download_glide(skred_fxbank_t *fx, uint32_t *host_u32x4, int first, int count);

/* ---- pitch wheel: bends that return to the key's bits and compose with glides, in integers ---------------------------------------
 *
 * The fixed-point twin of the float bank's section "pitch wheel" (include/skred_amd.h: skred_bend_check .. skred_bank_download_bend),
 * per voice -- this bank has no slots, so no slot_voices and no masks.  THIS is the place of record for the integer definition.  The
 * only other bend route on this bank is SKRED_CTL_INC_SCALE / SKRED_EACH_INC_SCALE, phase_inc = (phase_inc * q16) >> 16 on whatever
 * the device holds, and it (a) never comes back: every message truncates, so up by r and back by 1/r leaves a smaller increment, the
 * loss has one sign and grows with every wheel message, and after a sweep the channel is flat against a freshly struck key; (b) is
 * relative: the host must remember the last position per channel and send ratios of ratios, and a note stolen and struck again between
 * two messages gets the wrong one; (c) is coarse: Q16 resolves 0.026 cent at unity, a 14-bit wheel over +-2 semitones steps by 0.024
 * cent, so adjacent positions collide, and on small increments (inc * 65542) >> 16 == inc, the stall the glide section names; (d) is
 * undone on arrival when the voice glides.  A bend of this section is ABSOLUTE: the wheel at centre gives the key's bits, on every
 * machine, after any number of messages.
 *
 * STATE.  bend[n_voices] is an array of two uint32 per voice in device memory (one 8-byte word): key, ratio_q24.  key == 0 means "not
 * bent": a phase_inc of 0 is a voice without pitch and is never a legal key.  The first skred_fxbank_bend_match / _bend_owned_each /
 * _bend_tags_each call with work to do allocates the array (8 bytes per voice) beside the owner, pedal and glide arrays and zero-fills
 * it, and ensures the owner array too; that call waits for the device once.  It is freed with the bank.  Only the calls of this
 * section, the clear below and the glide calls read or write it, and the only bank word they store is phase_inc, as a word store: its
 * neighbours in the plane keep their bits.  No render kernel reads the array; a bank that never bends allocates nothing more and
 * launches nothing more than it did before this section existed.
 *
 * RATIO.  Q24: SKRED_FX_BEND_ONE = 1 << 24 is the centre; legal values are 1 .. 0xFFFFFFFF (just under 8 octaves up).  Q24 and not
 * SKRED_CTL_INC_SCALE's Q16 because Q16 cannot tell adjacent positions of a 14-bit wheel apart (above): Q24 resolves 0.0001 cent at
 * unity.  The product key * ratio_q24 is below 2^64 for every key and ratio, so it is formed exactly in 64 bits.
 *
 * THE RULE.  The absolute bend of voice v to r, with inc = phase_inc as the device holds it:
 *   1. k = key[v] ? key[v] : inc -- the first bend captures the key.
 *   2. r == SKRED_FX_BEND_ONE: where key[v] != 0, phase_inc = key[v] is stored; both words are cleared.  The voice counts as restored
 *      only if key[v] != 0: the centre on a voice that was never bent stores nothing and counts nothing.
 *   3. Otherwise p = ((uint64)k * r) >> 24.  k == 0, p == 0 or p > 0xFFFFFFFF: the bend is WITHHELD and counted, and the voice and its
 *      words stay exactly as they were.  Else phase_inc = p, key[v] = k, ratio[v] = r.  Exactly 0xFFFFFFFF and exactly 1 are stored.
 * The same message twice gives the same bits twice; any sequence of bends followed by the centre gives the key's bits and zero words.
 *
 * A NEW NOTE CLEARS THE WORDS.  Once the array exists, every tag launch of the bank (skred_fxbank_tag_list, the tags of
 * skred_fxbank_note_on_channel) is followed on its stream by a launch that zeroes the two words of every voice it tagged -- the same
 * list under the same list rule, right where the pedal word and the glide words are cleared.  Without it a thief's first bend would
 * find its victim's key and the centre would restore it.  A note struck under a deflected wheel is therefore, in this order:
 * skred_fxbank_note_on_channel, skred_fxbank_bend_tags_each with the channel's ratio, optionally skred_fxbank_glide_tags(FROM_SCALE).
 *
 * GLIDES UNDER A BEND.  On a bank that has a bend array the glide calls read it.  On a voice with key != 0, every place the portamento
 * section says `inc` reads and writes `key` instead: FROM_SCALE: target = key, key = (key * scale_q16) >> 16; TO_SCALE: target =
 * ((gliding ? the old target : key) * scale_q16) >> 16; TO_INC unchanged; the advance's steps, its arrive-at-once test and its
 * "stored only if it differs" rule run on key, and on arrival key = target; a stop with snap: key = target.  The sounding increment is
 * then stored again as phase_inc = ((uint64)key * ratio_q24) >> 24 at three points: after a start that was not withheld, after every
 * advance of a gliding voice, after a snap.  Where that product is 0 or above 0xFFFFFFFF only that one store is withheld, uncounted;
 * key and the glide words stand.  So a glide under a bend lands on (target * ratio_q24) >> 24, and the centre then gives the target's
 * bits.  Voices with key == 0, and banks without a bend array, store the bytes they stored before this section existed.
 *
 * All calls are asynchronous on `stream` and ordered like skred_fxbank_update; host arrays travel through the staging ring; nothing
 * waits for the device except the download and the first allocation; results are pure functions of the state, whatever the order of
 * arrival; one stream at a time per bank.  On a shard: through skred_fxshard_bank(), with that rank's local indices.  Every d_result
 * is a device uint32[3], may be NULL, and is cleared on the stream ahead of the kernel: [0] voices stored or restored, [1] bends
 * withheld, [2] see each call.
 *
 * skred_fx_bend_check          pure host: SKRED_OK, or SKRED_E_BAD_ARG for a NULL array, n < 0, or a ratio of 0.
 * skred_fxbank_bend_match      the channel wheel: THE RULE to ratio_q24 on every voice of [first, first + count) with owner != 0 and
 *                              (owner & m->mask) == m->value; geometry, guard and counting as skred_fxbank_ctl_match.  d_result[2]:
 *                              voices of the range that did not match.  It ships no bytes and takes no slot of the ring.  Refused, in
 *                              this order: NULL bank or match, ratio 0, what skred_owner_match_check refuses, SKRED_E_RANGE for an
 *                              empty range or one outside the bank.
 * skred_fxbank_bend_owned_each looks at the entries below min(n, *d_count_or_null); entry k bends d_voices[k] to ratios_q24[k] where
 *                              that is a voice of the bank whose owner is tags[k].  d_result[2]: voices whose owner differs.  A voice
 *                              listed twice is UNSPECIFIED.  Refused, in skred_fxbank_glide_owned's order: NULL bank or list, what
 *                              skred_owner_tags_check refuses (NULL tags, n < 0, a zero tag), n > INT32_MAX / 64, what
 *                              skred_fx_bend_check refuses.  n == 0: SKRED_OK, nothing is done.
 * skred_fxbank_bend_tags_each  bends by note id, built as skred_fxbank_glide_tags is: skred_fxbank_release_tags' find pass over
 *                              [first, first + count) into the same scratch -- the lowest voice of the range per tag, or -1 -- then
 *                              the call above on that list.  ratios_q24[k] goes with tags[k]: the tags travel sorted, and the ratios
 *                              are permuted with them on the host.  Tags unique, none zero, n <= SKRED_OWNER_MAX_TAGS.  d_result[2] is
 *                              0.  Refused: NULL bank, the tags, n and the ratios as above, then SKRED_E_RANGE for an empty range or
 *                              one outside the bank.
 * skred_fxbank_bend_clear      bend[first .. first + count) = 0 on `stream`; snap != 0: a bent voice's phase_inc = its key first.
 *                              Nothing to do on a bank without the array.  SKRED_E_RANGE: count < 0 or a range outside the bank.
 * skred_fxbank_download_bend   the words of [first, first + count) into host_u32x2 (2 * count words); waits for the device; zeros on a
 *                              bank that never bent.
 * LIMITS, documented, not fixed: a SKRED_CTL_PHASE_INC / _INC_SCALE store on a bent voice is overwritten by the next bend, centre or
 * glide step of that voice (the key's bits rule); the host view of phase_inc goes stale -- skred_fxbank_download_params reads it
 * back; the per-note calls belong with tagged notes.  Out of scope: the drop-in mode, deferred items, pattern steps. */
#define SKRED_FX_BEND_ONE (1u << 24)
int  skred_fx_bend_check(const uint32_t *ratios_q24, int n);
int  skred_fxbank_bend_match(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, uint32_t ratio_q24, uint32_t *d_result,
                             void *stream);
int  skred_fxbank_bend_owned_each(skred_fxbank_t *fx, const uint32_t *ratios_q24, const int32_t *d_voices, const uint32_t *tags, int n,
                                  const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
int  skred_fxbank_bend_tags_each(skred_fxbank_t *fx, const uint32_t *ratios_q24, int first, int count, const uint32_t *tags, int n,
                                 uint32_t *d_result, void *stream);
int  skred_fxbank_bend_clear(skred_fxbank_t *fx, int first, int count, int snap, void *stream);
int  skred_fxbank_download_bend(skred_fxbank_t *fx, uint32_t *host_u32x2, int first, int count);

/* ---- filter cutoff: key-tracked cutoffs that glide and land, coefficients computed on the device, in integers ----------------------
 *
 * The fixed-point twin of the float bank's section "filter cutoff on the device" (include/skred_amd.h: skred_filter_coeffs_w ..
 * skred_bank_download_cutoff), per voice -- no slots, no masks.  THIS is the place of record for the integer definition.  The other
 * filter route of this bank (SKRED_CTL_FILTER, skred_fx_filter_each_t) brings five finished Q2.30 words that the host made with libm in
 * fp32: "cutoff = 4 x the note's own frequency" after a glide or a bend needs a download of phase_inc, a sweep is one upload per
 * block, and the words depend on the host's libm.  The calls of this section keep the CUTOFF beside the voice and compute the five
 * words on the device with the integer arithmetic below: the same bits on every machine.
 *
 * FORMATS.  w_q29: uint32, the angular cutoff 2 pi f / rate in radians per frame, Q29; THE BOX is [SKRED_FX_CUTOFF_W_MIN,
 * SKRED_FX_CUTOFF_W_MAX] = [2^19, 3 * 2^29], the float box [2^-10, 3].  q_q16: uint32, box [2^10, 2^26] = [2^-6, 2^10].  mode 1 .. 5 as
 * in the float section (low-pass, high-pass, band-pass, notch, all-pass).
 *
 * THE ARITHMETIC (skred_fx_filter_coeffs_w(mode, w_q29, q_q16)).  Integers only.  A SIGNED product x is rounded by (x + 2^(s-1)) >> s
 * with an arithmetic shift (a floor): to nearest, ties towards plus infinity.  With each step, the bound of what it forms:
 *   1. range reduction: w_q29 > SKRED_FX_CUTOFF_HALF_PI_Q29: r = SKRED_FX_CUTOFF_PI_Q29 - w_q29 (exact; the cosine below changes its
 *      sign), else r = w_q29.  r <= 843314857 < 2^30.
 *   2. z = (r * r + 2^27) >> 28: (r / 2)^2 in Q32 (r^2 in Q30).  r * r < 2^60; z <= 2.4675 * 2^30 < 2^32: a uint32.  The polynomials
 *      run in (r / 2)^2 < 0.617, so that no power of z amplifies the rounding of a constant.
 *   3. sine, Horner in z on Q31 words:  p = S5;  p = ((p * z + 2^31) >> 32) + S4;  .. + S3;  .. + S2;  .. + S1;
 *      sinc = 2^31 + ((p * z + 2^31) >> 32) -- sin(r) / r in Q31, in [0.6366 * 2^31, 2^31).  |p| <= |S1| < 2^30.5 at every step, every
 *      product |p * z| < 2^62.5: an int64.  rs = r * sinc: sin(w) in Q60, < 2^61.
 *   4. cosine, Horner in z on Q31 words:  c = C6;  c = ((c * z + 2^31) >> 32) + C5;  .. + C4;  .. + C3;  .. + C2;
 *      t = (c * z + 2^31) >> 32;  cos = 2^31 - z + ((t * z + 2^31) >> 32) -- cos(r) in Q31; the term -2 (r / 2)^2 is z itself in Q31 and
 *      is taken exactly, outside the Horner chain (its coefficient 2 would not fit a Q31 word).  |c| <= C2 < 2^30.5, |c * z| < 2^62.5,
 *      |t| < 2^30, |t * z| < 2^62; 0 < cos <= 2^31.  cs = -cos behind the reduction of step 1, else cos: cos(w) in Q31.
 *   5. skred_filter_coeffs' sequence in integers.  alpha = (rs + (den >> 1)) / den with den = q_q16 << 15 (2 q in Q30; <= 2^41): sn /
 *      (2 q) in Q30 to nearest, straight from the Q60 sine -- a sine rounded to Q30 first would have its half unit multiplied by up to
 *      32.  rs + (den >> 1) < 2^62.  alpha lies in [2^9, 2^35 + 64) -- near pi / 2 the sine's polynomial overshoots 1 by up to 5e-10, which
 *      1 / (2 q) = 32 turns into 17 units --: 36 bits.  a0 = 2^30 + alpha: in (2^30, 2^30 + 2^35 + 64), 36 bits.
 *      The numerators, signed, |n| <= a0 or <= 2^32:
 *        mode 1:  d = 2^31 - cs (Q31);  b0 = d / 2,  b1 = d,  b2 = b0            mode 2:  s = 2^31 + cs (Q31);  b0 = s / 2,  b1 = -s,  b2 = b0
 *        mode 3:  b0 = alpha,  b1 = 0,  b2 = -alpha                              mode 4:  b0 = 2^30,  b1 = -cs (-2 cos w in Q30),  b2 = b0
 *        mode 5:  b0 = 2^30 - alpha,  b1 = -cs,  b2 = a0 (36 bits)
 *        a1 = -cs,  a2 = 2^30 - alpha  in every mode.
 *   6. FIVE ROUNDED QUOTIENTS by a0, each Q(n, s) = round(|n| * 2^(s + 2) / a0) with the sign of n put back -- ONE rule for negative
 *      numerators: the magnitude is rounded to nearest, ties away from zero.  s = 28 for a Q30 numerator, 27 for a Q31 one (d, s), 26
 *      for its half (d / 2, s / 2: no bit of d is dropped).  |n| * 2^30 does not fit 64 bits (a0 * 2^30 is 2^66), so the divide is
 *      made in two steps:  qa = (|n| << s) / a0,  ra = the remainder;  Q = (qa << 2) + ((ra << 2) + (a0 >> 1)) / a0.
 *      |n| << s < (2^30 + 2^35 + 64) * 2^28 < 2^63.05: an unsigned 64-bit word holds it.  qa < 2^29 (|n| < 2 a0 everywhere);  ra < a0;
 *      (ra << 2) + (a0 >> 1) < 2^38.2;  Q < 2^31.1, clamped to int32 (only mode 1's b1 and mode 2's -b1 reach the clamp, at 2 - 2^-30).
 *      Mode 3's b1 is 0 and mode 5's b2 is 2^30 exactly.  No divisor is zero.
 * Nothing above leaves 64 bits anywhere in the box; tests/test_fx_cutoff_cpu.py evaluates every step in unbounded integers on the grid,
 * a random set and all corners and holds each to the width stated here.  Nine 64-bit divides per voice at most.
 *
 * ACCURACY, measured by tests/test_fx_cutoff_cpu.py on the float section's grid mapped to these formats (201 values of w_q29: both
 * ends, 72 spread geometrically, the pi / 2 seam and its 64 neighbours on either side; 17 values of q_q16; 5 modes) against an fp64
 * evaluation of the RBJ formulas on the exact rationals w_q29 / 2^29 and q_q16 / 2^16: the largest absolute error of each word in
 * units of 2^-30, of this function and of the route this bank had before (the same inputs converted to fp32, skred_filter_coeffs,
 * rounded to Q2.30 as the host rounds them).  The test holds every entry of the first table to at most 4 x the second's.
 *                     skred_fx_filter_coeffs_w                      fp32 skred_filter_coeffs, rounded (the yardstick)
 *   mode    b0     b1     b2     a1     a2                 b0      b1      b2      a1      a2
 *   1     0.80   1.31   0.80   2.12   1.45               99.4   198.8    99.4   243.8    93.8
 *   2     1.02   1.67   1.02   2.12   1.45              113.1   226.2   113.1   243.8    93.8
 *   3     0.98   0      0.98   2.12   1.45               89.0     0      89.0   243.8    93.8
 *   4     0.98   2.12   0.98   2.12   1.45               89.5   243.8    89.5   243.8    93.8
 *   5     1.45   2.12   0      2.12   1.45               93.8   243.8     0     243.8    93.8
 * The largest ratio is 0.015: the integer route is some 70 times closer to fp64 than fp32 coefficients rounded to Q2.30 can be.
 * Stability (|a2| < 2^30 and |a1| < 2^30 + a2) holds on the whole grid for modes 1 .. 5, and every word fits int32.
 *
 * STATE.  cut[n_voices] is an array of eight uint32 per voice (two 16-byte words): w_q29 (0: "no device cutoff"), target_q29 (0: "not
 * moving"), up_q32, down_q32 | carry (0 .. 63), q_q16, mode, a reserved 0.  The first skred_fxbank_cutoff_match / _cutoff_owned_each /
 * _cutoff_tags_each call with work to do allocates it (32 bytes per voice; the owner array first, when no owner call came before) and
 * zero-fills it; that call waits for the device once.  It is freed with the bank.  Only the calls of this section and the clear below
 * read or write it.  The only bank words they store are b0_q30 b1_q30 b2_q30 a1_q30 a2_q30 (the whole coefficient plane word and the
 * a2 word): filter_mode, the delay line and every neighbouring word keep their bits, so the render instantiation stays right, and a
 * voice with filter_mode == 0 keeps the words without reading them.  A bank that never calls these allocates nothing more and
 * launches nothing more than it did before this section existed.
 *
 * A RECORD ON VOICE v (skred_fx_cutoff_t), the float section's steps 1 - 4 in integers:
 *   1. v has no cutoff word (w_q29 == 0) and the record does not name BOTH SKRED_FX_CUTOFF_Q and SKRED_FX_CUTOFF_MODE: WITHHELD and
 *      counted.
 *   2. q = the record's with SKRED_FX_CUTOFF_Q, else the voice's; mode likewise with SKRED_FX_CUTOFF_MODE.
 *   3. SKRED_FX_CUTOFF_ABS: wn = value (a w_q29 in the box).  SKRED_FX_CUTOFF_TRACK: k = the key word of a bent voice (section "pitch
 *      wheel"), else phase_inc -- the word a glide runs on.  k == 0: WITHHELD and counted.  wn = ((uint64)k * value) >> 27 with value
 *      = track_q24 = harmonic * 2 pi in Q24: phase_inc / 2^32 is cycles per frame, so w = 2 pi * harmonic * k / 2^32 radians per frame
 *      and in Q29 that is k * (harmonic * 2 pi * 2^24) / 2^27.  A uint32 track_q24 reaches harmonic 256 / 2 pi, about the 40th; the
 *      product is below 2^64.  wn outside the box is CLAMPED to the nearer end and counted.
 *   4. SKRED_FX_CUTOFF_GLIDE on a voice that has a cutoff word: target = wn, the rates are the record's, carry = 0; w and the
 *      coefficients stand until the next advance.  Otherwise (no GLIDE, or the voice's first cutoff): w = wn, target = up = down =
 *      carry = 0 -- any movement stops -- and the five words = THE ARITHMETIC(mode, wn, q).
 * A withheld record leaves the voice and all eight words exactly as they were.
 *
 * ADVANCE BY F FRAMES (skred_fxbank_cutoff_advance), the portamento's rule on w, for every moving voice of a range: c = carry + F, and
 * c >> 6 steps are taken, stopping at arrival.  w == target: arrived at once.  Up: next = w + max(1, ((uint64)w * up_q32) >> 32),
 * arrived if next >= target.  Down: next = w - max(1, ((uint64)w * down_q32) >> 32), arrived if next <= target.  On arrival w = THE
 * TARGET'S BITS and target, rates and carry are zeroed; else carry = c & 63.  Then the coefficients are computed ONCE from that final
 * w (also when no step was taken).  w at every multiple of 64 frames does not depend on how the host cuts its blocks; a voice that
 * has landed holds the bits of a voice set with SKRED_FX_CUTOFF_ABS at the target.  A voice that does not move costs one 16-byte load.
 *
 * A NEW NOTE CLEARS THE WORDS.  Once the array exists, every tag launch of the bank is followed on its stream by a launch that zeroes
 * all eight words of every voice it tagged, beside the pedal, glide and bend clears: a thief or a key struck again does not inherit
 * a moving cutoff.  The coefficients stay what they were.  The order for a tracked note is skred_fxbank_note_on_channel, then
 * skred_fxbank_bend_tags_each / skred_fxbank_glide_tags, then skred_fxbank_cutoff_tags_each.
 *
 * All calls are asynchronous on `stream` and ordered like skred_fxbank_update; host arrays travel through the staging ring; nothing
 * waits for the device but the download and the first allocation; the same state gives the same bytes; one stream at a time per
 * bank.  On a shard: through skred_fxshard_bank(), with that rank's local indices.  d_result of the three record calls (device,
 * uint32[4], may be NULL; cleared on the stream ahead of the kernel): [0] voices set or started, [1] records withheld, [2] voices not
 * owned (the _each calls) or voices of the range that did not match, [3] cutoffs clamped.
 *
 * skred_fx_filter_coeffs_w        pure host, THE ARITHMETIC.  out5 = b0 b1 b2 a1 a2.  SKRED_OK; 1 for mode 0 (bypass: out5 is left as it
 *                                 is); SKRED_E_BAD_ARG for a NULL out5 or a mode outside 0 .. 5; SKRED_E_RANGE for a w_q29 or q_q16
 *                                 outside the box.
 * skred_fx_cutoff_check           pure host: SKRED_OK, or what the record calls refuse about n records, in this order.
 *                                 SKRED_E_BAD_ARG: a NULL array, n < 0; in a record: unknown bits in set, ABS with TRACK or neither,
 *                                 first_time != 0 and not both Q and MODE, a reserved word that is not 0; SKRED_E_RANGE: a named
 *                                 q_q16 outside the box, an ABS value outside the box, a TRACK value of 0, a named mode outside
 *                                 1 .. 5; SKRED_E_BAD_ARG: a zero up_q32 or down_q32 under GLIDE.  first_time: the caller states that
 *                                 the voices have no cutoff word yet -- the entry points cannot know (they pass 0), and there the
 *                                 kernel withholds and counts instead.
 * skred_fxbank_cutoff_match       the channel sweep: the record on every voice of [first, first + count) with owner != 0 and (owner &
 *                                 m->mask) == m->value; geometry, guard and counting as skred_fxbank_bend_match; the record is a
 *                                 kernel argument and takes no slot of the ring.  Refused, in this order: NULL bank, match or record,
 *                                 what skred_fx_cutoff_check refuses, what skred_owner_match_check refuses, SKRED_E_RANGE for an
 *                                 empty range or one outside the bank.
 * skred_fxbank_cutoff_owned_each  looks at the entries below min(n, *d_count_or_null); entry k brings recs[k] to d_voices[k] where
 *                                 that is a voice of the bank whose owner is tags[k].  A voice listed twice is UNSPECIFIED.  Refused,
 *                                 in skred_fxbank_bend_owned_each's order: NULL bank or list, what skred_owner_tags_check refuses,
 *                                 n > INT32_MAX / 64, what skred_fx_cutoff_check refuses.  n == 0: SKRED_OK, nothing is done.
 * skred_fxbank_cutoff_tags_each   by note id: skred_fxbank_release_tags' find pass over [first, first + count) into the same scratch,
 *                                 then the call above on that list.  recs[k] goes with tags[k]: the tags travel sorted, the records
 *                                 are permuted with them on the host.  Tags unique, none zero, n <= SKRED_OWNER_MAX_TAGS; d_result[2]
 *                                 is 0.  Refused: as above, then SKRED_E_RANGE for an empty range or one outside the bank.
 * skred_fxbank_cutoff_advance     the advance pass over [first, first + count).  d_result (device, uint32[2], may be NULL; cleared on
 *                                 the stream ahead of the kernel): [0] voices still moving, [1] voices that arrived.  On a bank
 *                                 without the array: SKRED_OK, d_result (if given) is cleared on the stream, nothing is launched.
 *                                 SKRED_E_BAD_ARG: NULL bank, num_frames outside 1 .. 65536; SKRED_E_RANGE: count <= 0 or a range
 *                                 outside the bank.
 * skred_fxbank_cutoff_stop        every movement of [first, first + count) ends on `stream`: target, rates and carry are cleared, w,
 *                                 q and mode stay; snap != 0: a moving voice's w = its target and its coefficients are computed
 *                                 first.  Nothing to do on a bank without the array.  SKRED_E_RANGE: count < 0 or a range outside.
 * skred_fxbank_download_cutoff    the words of [first, first + count) into host_u32x8 (8 * count words); waits for the device; zeros
 *                                 on a bank that never set a cutoff.
 * LIMITS, documented, not fixed: a tracked cutoff is computed when the call runs and does not follow later bends or glides: send it
 * again.  A SKRED_CTL_FILTER store (or per-entry coefficients) on a voice with a cutoff word is overwritten by that voice's next
 * moving advance, and otherwise leaves w stale.  A release leaves the words alone -- unless the voice has a filter envelope (the next
 * section).  Out of scope: the drop-in mode, deferred items, pattern steps. */
#define SKRED_FX_CUTOFF_W_MIN (1u << 19)
#define SKRED_FX_CUTOFF_W_MAX (3u << 29)
#define SKRED_FX_CUTOFF_Q_MIN (1u << 10)
#define SKRED_FX_CUTOFF_Q_MAX (1u << 26)
#define SKRED_FX_CUTOFF_PI_Q29 1686629713u          /* round(pi * 2^29) */
#define SKRED_FX_CUTOFF_HALF_PI_Q29 843314857u      /* round(pi / 2 * 2^29) */
#define SKRED_FX_CUTOFF_S1 (-1431655761ll)          /* Q31 coefficients of sin(r) / r - 1 in (r / 2)^2: about -4/3!, 16/5!, -64/7!, .. */
#define SKRED_FX_CUTOFF_S2 286331072ll
#define SKRED_FX_CUTOFF_S3 (-27269072ll)
#define SKRED_FX_CUTOFF_S4 1513217ll
#define SKRED_FX_CUTOFF_S5 (-52533ll)
#define SKRED_FX_CUTOFF_C2 1431655759ll             /* Q31 coefficients of cos(r) - 1 + 2 (r / 2)^2: about 16/4!, -64/6!, 256/8!, .. */
#define SKRED_FX_CUTOFF_C3 (-190887371ll)
#define SKRED_FX_CUTOFF_C4 13634516ll
#define SKRED_FX_CUTOFF_C5 (-605274ll)
#define SKRED_FX_CUTOFF_C6 17511ll
enum { SKRED_FX_CUTOFF_ABS = 1u << 0,     /* w = value, a w_q29 */
       SKRED_FX_CUTOFF_TRACK = 1u << 1,   /* w = (k * value) >> 27, k the voice's key increment, value a track_q24: exactly one of ABS and TRACK */
       SKRED_FX_CUTOFF_GLIDE = 1u << 2,   /* the computed w is the TARGET, reached by up_q32 / down_q32 per 64 frames */
       SKRED_FX_CUTOFF_Q = 1u << 3,       /* the record names q_q16 */
       SKRED_FX_CUTOFF_MODE = 1u << 4 };  /* the record names mode (1 .. 5) */
typedef struct skred_fx_cutoff {          /* 32 bytes */
  uint32_t set, value, q_q16, mode, up_q32, down_q32;
  uint32_t reserved[2];                   /* 0 */
} skred_fx_cutoff_t;
int  skred_fx_filter_coeffs_w(int mode, uint32_t w_q29, uint32_t q_q16, int32_t out5[5]);
int  skred_fx_cutoff_check(const skred_fx_cutoff_t *rec, int n, int first_time);
int  skred_fxbank_cutoff_match(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, const skred_fx_cutoff_t *rec,
                               uint32_t *d_result, void *stream);
int  skred_fxbank_cutoff_owned_each(skred_fxbank_t *fx, const skred_fx_cutoff_t *recs, const int32_t *d_voices, const uint32_t *tags, int n,
                                    const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
int  skred_fxbank_cutoff_tags_each(skred_fxbank_t *fx, const skred_fx_cutoff_t *recs, int first, int count, const uint32_t *tags, int n,
                                   uint32_t *d_result, void *stream);
int  skred_fxbank_cutoff_advance(skred_fxbank_t *fx, int first, int count, int num_frames, uint32_t *d_result, void *stream);
int  skred_fxbank_cutoff_stop(skred_fxbank_t *fx, int first, int count, int snap, void *stream);
int  skred_fxbank_download_cutoff(skred_fxbank_t *fx, uint32_t *host_u32x8, int first, int count);

/* ---- filter envelope: per-note cutoff contours that follow the gate, in integers -----------------------------------------------------
 *
 * The fixed-point twin of the float bank's section "filter envelope" (include/skred_amd.h: skred_fenv_check ..
 * skred_bank_download_fenv), per voice -- no slots, no masks.  THIS is the place of record for the integer definition.  With the cutoff
 * calls alone a host sends one SKRED_FX_CUTOFF_GLIDE per stage and times them itself, and the last one it cannot time: under a pedal,
 * after skred_fxbank_stamp_match, skred_fxbank_release_tags or a steal it does not know when, or whether, a voice's release clock was
 * stamped.  The device knows: sample_release (SKX_TIME words 2, 3) lies beside every voice and every note-off path stamps it.  So the
 * contour is a small program kept beside the voice; skred_fxbank_cutoff_advance, the per-block pass the cutoff already has, steps it,
 * and the release is entered from the voice's own release clock.  The envelope has NO ARITHMETIC OF ITS OWN: a step is the cutoff
 * section's 64-frame step with up_q32 = down_q32 = the stage's rate, a level is compared as the uint32 it is, and a coefficient store
 * is THE ARITHMETIC(mode, w_q29, q_q16) of the cutoff section.  No render kernel reads the array.
 *
 * STATE.  fenv[n_voices] is an array of eight uint32 per voice (two 16-byte words):
 *     stage | w_peak | w_sustain | w_end          the levels are w_q29 values inside THE BOX of the cutoff section
 *     rate_attack_q32 | rate_decay_q32 | rate_release_q32 | 0
 * stage: 0 off (then all eight words are 0), 1 attack, 2 decay, 3 sustain, 4 release.  The first skred_fxbank_fenv_match /
 * _fenv_owned_each / _fenv_tags_each call with work to do allocates it (32 bytes per voice; the owner and cutoff arrays first, when
 * they do not exist yet) and zero-fills it; that call may wait for the device once.  It is freed with the bank.  Only the calls of
 * this section, the cutoff calls and the clear below read or write it.  The array has the shape of the float bank's fenv array
 * (checked at compile time), so the float bank's clear kernel serves it at one voice per slot, as it serves cut[].  A bank that never
 * calls these allocates nothing more and launches nothing more, and every entry point behaves on it as it did, to the byte.
 *
 * ENTERING A STAGE with level T and rate r (a Q32 fraction of w per 64 frames), from the voice's w.  An integer rate has no direction:
 * the direction is w < T (up) or w > T (down).
 *   The stage LANDS AT ONCE iff w == T; the next stage is then entered by this same rule.  Otherwise target = T and up_q32 = down_q32
 *   = r.  (T is in the box, so T != 0: "target == 0" goes on meaning "not moving".)
 *     attack (1):  T = w_peak,    r = rate_attack_q32;   next: decay
 *     decay (2):   T = w_sustain, r = rate_decay_q32;    next: sustain
 *     sustain (3): target = up_q32 = down_q32 = 0: the voice rests, not moving, and the stage word stays 3
 *     release (4): T = w_end,     r = rate_release_q32;  next: off -- when the release lands ALL EIGHT fenv words are cleared, target,
 *                  rates and carry become 0, and w keeps the bits of w_end: the voice is bit-identical, in all eight cutoff words and
 *                  the five coefficients, to one set with SKRED_FX_CUTOFF_ABS at w_end.
 *   carry survives stage changes: the note keeps its 64-frame grid from the record to the end of the release.
 *
 * A RECORD ON VOICE v (skred_fx_fenv_t: set, start, peak, sustain, end, rate_attack_q32, rate_decay_q32, rate_release_q32):
 *   1. v has no cutoff word (w_q29 == 0): WITHHELD and counted; both arrays of the voice stay untouched.  The base cutoff, q and mode
 *      come from skred_fxbank_cutoff_* first.
 *   2. w_now = the voice's w_q29 when the kernel runs.  SKRED_FX_FENV_ABS: the four levels are w_q29 values in the box.
 *      SKRED_FX_FENV_REL: each level = ((uint64)w_now * value_q16) >> 16, value_q16 a uint32 ratio in Q16 (2^16 is "the present
 *      cutoff"; up to 65536 x).  w_now <= 3 * 2^29 < 2^31 and value_q16 < 2^32, so THE PRODUCT IS BELOW 2^63 and the shifted level below
 *      2^47: both fit a uint64, and the clamp is made on the 64-bit value before it is narrowed.  A level outside the box is CLAMPED to
 *      the nearer end, and the VOICE is counted once however many of its levels were clamped.  Exactly one of ABS and REL is named.
 *      Without SKRED_FX_FENV_START the start level is neither computed nor clamped (and must be 0 in the record).
 *   3. Any movement the voice had ends and carry = 0.  SKRED_FX_FENV_START: w = the start level at once; otherwise the contour starts
 *      from w_now.
 *   4. The fenv words = 1, the three levels, the three rates, 0, and the attack is ENTERED by the rule above.  Stages that land at once
 *      chain as far as sustain (peak == w: decay is entered; sustain == peak too: the voice rests in sustain).  The release is entered
 *      by the advance pass only.
 *   5. If w changed, the five coefficient words = THE ARITHMETIC(mode, w, q), once, from the final w.
 *
 * ADVANCE BY F FRAMES.  skred_fxbank_cutoff_advance stays the one per-block pass.  On a bank with an fenv array, for every voice of
 * the range with stage != 0:
 *   1. stage is 1 .. 3 and the voice's sample_release != 0 (lo | hi): the release is ENTERED first (it may land at once, which ends the
 *      contour).
 *   2. c = carry + F (carry <= 63, F <= 65536: below 2^17).  Then c >> 6 times, while the voice has a target: one step of the cutoff
 *      section -- up: next = w + max(1, ((uint64)w * r) >> 32), arrived if next >= target; down: next = w - max(1, ((uint64)w * r) >>
 *      32), arrived if next <= target.  w <= 3 * 2^29 and r < 2^32: the product is below 2^63, the step at most w - 1 (down cannot
 *      wrap), next going up below 2 w <= 3 * 2^30 < 2^32 (formed in 64 bits all the same, as the cutoff section forms it).  On arrival w
 *      = THE TARGET'S BITS and the next stage is ENTERED; the remaining steps continue in that stage.  (Sustain has no target: the
 *      remaining steps do nothing.)  A stage with a target was entered with w != target and a step that does not arrive leaves w !=
 *      target, so the step is never taken on w == target.
 *   3. carry = c & 63 -- through sustain as well, which is what makes the property below hold -- or 0 when the contour ended.
 *   4. If the voice had a target when the pass began, or step 1 entered the release, the coefficients are computed ONCE from the final
 *      w.  A voice resting in sustain stores nothing.
 * A voice with stage == 0 follows the cutoff section's rule unchanged.  d_result keeps its meaning: [0] voices with a target after the
 * pass (a voice resting in sustain has none), [1] voices that arrived at any level in the pass, stepped or at once; each such voice
 * counts once.  A trigger stamp alone does not restart a contour (a releasing contour goes on releasing); a new record does.
 * THE STATED PROPERTY: for a fixed sequence of control calls at fixed frame positions and a block cut at every call, w at every
 * multiple of 64 frames from the record on does not depend on where else the host cuts its blocks.
 * Cost: on a bank with the array a voice with stage == 0 costs its 16-byte cutoff load and one more 4-byte load (its stage word); one
 * with a contour the two fenv words, its second cutoff word and the 8 bytes of its release clock.  On a bank without the array the
 * pass is the kernel it was.
 *
 * DECIDED HERE, beyond the proposal's text: (a) REL value_q16 is Q16 and the clamp precedes the narrowing, as step 2 states; (b) the
 * record's steps 2 and 3 are ordered so that every REL level, the start included, is taken from w_now and not from the start level;
 * (c) a record on a voice that already has a contour replaces it (carry = 0: the new note's grid starts at the record); (d) the
 * advance compares a contoured voice's up_q32 only -- the two rates of such a voice are one word twice, since every cutoff record
 * that could split them ends the contour; (e) a release that lands in the pass that enters it counts in [1] once and computes the
 * coefficients, whether it landed at once or by steps; (f) a zero rate is refused by the check (a stage must move), a rate so small that
 * ((uint64)w * r) >> 32 is 0 moves by 1 per 64 frames, as in the cutoff section.
 *
 * WHO ENDS AN ENVELOPE.  Once the array exists, every tag launch of the bank is followed on its stream by a launch that zeroes all
 * eight fenv words of every voice it tagged, beside the pedal, glide, bend and cutoff clears: a thief or a key struck again inherits no
 * contour.  skred_fxbank_cutoff_match / _cutoff_owned_each / _cutoff_tags_each zero the fenv words of the voices they set or start (a
 * withheld record leaves them), skred_fxbank_cutoff_stop those of every voice of its range, moving or resting: a cutoff call on an
 * enveloped voice ends the contour and then does what it always did.  The order for a note is skred_fxbank_note_on_channel, then
 * skred_fxbank_bend_tags_each / skred_fxbank_glide_tags, then skred_fxbank_cutoff_tags_each, then skred_fxbank_fenv_tags_each.
 *
 * All calls are asynchronous on `stream` and ordered like skred_fxbank_update; host arrays travel through the staging ring; nothing
 * waits for the device but the download and the first allocation; the same state gives the same bytes; one stream at a time per
 * bank.  On a shard: through skred_fxshard_bank(), with that rank's local indices.  d_result of the three record calls (device,
 * uint32[4], may be NULL; cleared on the stream ahead of the kernel): [0] voices started, [1] records withheld, [2] voices not owned
 * (the _each calls) or voices of the range that did not match, [3] voices clamped.
 *
 * skred_fx_fenv_check             pure host: SKRED_OK, or what the record calls refuse about n records, in this order.
 *                                 SKRED_E_BAD_ARG: a NULL array, n < 0; then record by record: SKRED_E_BAD_ARG: unknown bits in set;
 *                                 ABS together with REL, or neither; start != 0 without START; SKRED_E_RANGE: an ABS level outside
 *                                 the box (start only with START); a REL value of 0 (start only with START); SKRED_E_BAD_ARG: a zero
 *                                 rate.
 * skred_fxbank_fenv_match         the channel sweep: the record on every voice of [first, first + count) with owner != 0 and (owner &
 *                                 m->mask) == m->value; geometry, guard and counting as skred_fxbank_cutoff_match; the record is a
 *                                 kernel argument and takes no slot of the ring.  Refused, in skred_fxbank_cutoff_match's order: NULL
 *                                 bank, match or record, what skred_fx_fenv_check refuses, what skred_owner_match_check refuses,
 *                                 SKRED_E_RANGE for an empty range or one outside the bank.
 * skred_fxbank_fenv_owned_each    looks at the entries below min(n, *d_count_or_null); entry k brings recs[k] to d_voices[k] where
 *                                 that is a voice of the bank whose owner is tags[k].  A voice listed twice is UNSPECIFIED.  Refused,
 *                                 in skred_fxbank_cutoff_owned_each's order: NULL bank or list, what skred_owner_tags_check refuses,
 *                                 n > INT32_MAX / 64, what skred_fx_fenv_check refuses.  n == 0: SKRED_OK, nothing is done.
 * skred_fxbank_fenv_tags_each     by note id: skred_fxbank_release_tags' find pass over [first, first + count) into the same scratch,
 *                                 then the call above on that list.  recs[k] goes with tags[k]: the tags travel sorted, the records
 *                                 are permuted with them on the host.  Tags unique, none zero, n <= SKRED_OWNER_MAX_TAGS; d_result[2]
 *                                 is 0.  Refused: as above, then SKRED_E_RANGE for an empty range or one outside the bank.
 * skred_fxbank_download_fenv      the fenv words of [first, first + count) into host_u32x8 (8 * count words); waits for the device;
 *                                 zeros on a bank without the array.
 * LIMITS, documented, not fixed: REL levels are computed when the record runs and do not follow later bends or glides: send the record
 * again.  A SKRED_CTL_FILTER store on a voice with a moving contour is overwritten by the next advance.  Out of scope: the drop-in
 * mode, deferred items, pattern steps. */
enum { SKRED_FX_FENV_ABS = 1u << 0,      /* the four levels are w_q29 values inside the box */
       SKRED_FX_FENV_REL = 1u << 1,      /* each level = (w_now * value_q16) >> 16, clamped: exactly one of ABS and REL */
       SKRED_FX_FENV_START = 1u << 2 };  /* w = the start level at once; without it `start` must be 0 */
typedef struct skred_fx_fenv {           /* 32 bytes */
  uint32_t set, start, peak, sustain, end, rate_attack_q32, rate_decay_q32, rate_release_q32;
} skred_fx_fenv_t;
int  skred_fx_fenv_check(const skred_fx_fenv_t *recs, int n);
int  skred_fxbank_fenv_match(skred_fxbank_t *fx, int first, int count, const skred_owner_match_t *m, const skred_fx_fenv_t *rec,
                             uint32_t *d_result, void *stream);
int  skred_fxbank_fenv_owned_each(skred_fxbank_t *fx, const skred_fx_fenv_t *recs, const int32_t *d_voices, const uint32_t *tags, int n,
                                  const uint32_t *d_count_or_null, uint32_t *d_result, void *stream);
int  skred_fxbank_fenv_tags_each(skred_fxbank_t *fx, const skred_fx_fenv_t *recs, int first, int count, const uint32_t *tags, int n,
                                 uint32_t *d_result, void *stream);
int  skred_fxbank_download_fenv(skred_fxbank_t *fx, uint32_t *host_u32x8, int first, int count);

/* Same on host buffers (synchronous). */
int  skred_fxbank_render_host(skred_fxbank_t *fx, int num_frames, int interp, int64_t *mix, int32_t *stems_or_null);
float skred_fxbank_last_render_ms(skred_fxbank_t *fx);

/* ---- the fixed-point bank sharded over the GPUs of one node (include/skred_amd.h: skred_shard_*) ----
 * skred_fxshard_create() makes an skred_shard_t whose steps are this path's: every rank renders its block of the bank into an
 * int64 pre-master sum, the one collective is ncclReduce(ncclSum, ncclInt64) -- an exact sum: the sharded render equals the
 * unsharded one BIT FOR BIT for every number of ranks --, the root applies the master stage.  Drive it with
 * skred_shard_render_mix (partial / out: int64[num_frames][2] behind the float pointers), skred_shard_init_rccl,
 * skred_shard_set_ops, skred_shard_destroy. */
struct skred_shard;
int  skred_fxshard_create(int device, int rank, int world, int root, int total_voices, struct skred_shard **out);
skred_fxbank_t *skred_fxshard_bank(struct skred_shard *shard);
int  skred_fxshard_upload(struct skred_shard *shard, const skred_fxpt_bank_t *whole_bank);

#ifdef __cplusplus
}
#endif
#endif
