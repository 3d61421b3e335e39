/* skred_fxbank_priv.h -- what the host files of the fixed-point bank share (skred_fxbank.c: planes, uploads, rendering;
 * skred_fx_stage.c: the staging ring and the batch path; skred_fx_live.c: updates, the free-voice list, note-ons; skred_fx_steal.c:
 * voice stealing; skred_fx_owner.c: note owners; skred_fx_ctl.c: controllers; skred_fx_expr.c: channels and per-note expression;
 * skred_fx_pedal.c: pedals; skred_fx_glide.c: portamento; skred_fx_bend.c: the pitch wheel; skred_fx_cutoff.c: filter cutoff; skred_fx_fenv.c:
 * the filter envelope; channel polyphony lives in skred_fx_steal.c). */
#ifndef SKRED_FXBANK_PRIV_H
#define SKRED_FXBANK_PRIV_H

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <stdint.h>
#include <stddef.h>

#include "skred_amd.h"
#include "skred_amd_fxpt.h"
#include "skred_fx_layout.h"

/* One staging slot of the control ring: a pinned host buffer, its device twin, and an event recorded behind the slot's copy and
 * the kernels that read the twin.  A slot that is still in flight is waited for through ITS event alone: the host never waits
 * for the device, and never gives up after some wall-clock time -- a stream that is legitimately backlogged (a long offline
 * block, a profiled run) holds the caller back exactly as long as it takes. */
#define SKX_RING SKRED_FX_RING_SLOTS
typedef struct {
  void *h, *d;
  size_t cap;
  hipEvent_t ev;
  int in_flight;
} skx_slot_t;

struct skred_fxbank {
  int device, n_voices, n_padded, n_groups;
  skx_plane_t *d_ro[SKX_COUNT];
  skx_plane_t *d_rw[SKX_RW_COUNT];
  int n_filter;                 /* voices with filter_mode != 0 (recounted on whole-bank uploads, grown otherwise) */
  int16_t *d_tables;
  size_t table_entries, table_bytes_padded;
  long long *d_partial; size_t partial_cap;  /* [n_wg][F][2] rows, [SKX_FINISH_SLABS][F][2] slab sums, then int32 gains[F] */
  uint32_t *d_tickets;          /* [SKX_FINISH_SLABS + 1] arrival counters of the in-kernel mix-down */
  long long *d_gain_state;      /* [0] Q31 master gain carried between blocks; [1] the gain a sum-only render prepared for skred_fxbank_master */
  long long master_target_q31;  /* default: 0.025 (the float path's volume_final) in Q31 */
  int32_t master_k_q15;         /* default: 0.002 in Q15 */
  int gains_frames;             /* > 0: the latest sum-only render left the gains of a block of this many frames */
  size_t gains_offset;          /* ... at this int64 offset into d_partial */
  skx_slot_t ring[SKX_RING];    /* staging of every host-written batch (skred_fx_stage.c) */
  unsigned ring_head;
  uint32_t *upd_mark; uint32_t upd_epoch;    /* per-voice epoch marks: a batch that names a voice twice is split into launches */
  uint32_t *d_idle; int idle_wgs;            /* the query's scratch: SKX_IDLE_W_COUNT words, idle_wgs counts, idle_wgs offsets */
  int32_t *d_idle_out, *h_idle_out; size_t idle_out_cap;   /* skred_fxbank_find_idle_host: counts + list, device and pinned */
  uint32_t *d_note_list; size_t note_list_cap;             /* skred_fxbank_note_on_idle / _note_on_steal: SKX_NOTE_LIST_WORDS words (the idle
                                                            * query's two counts, the joined list's length), then the list */
  uint32_t *d_steal; int steal_wgs;          /* skred_fxbank_find_steal's scratch, laid out as the float bank's (skred_bank_steal.c) */
  int32_t *d_steal_out, *h_steal_out;        /* [2] counts (a matched query: [3]), then SK_STEAL_MAX victims: the _host queries' list and the note-on bursts' */
  uint32_t *d_owner;                         /* note owners (skred_fx_owner.c): one word per voice, 0 nobody; NULL until the first call that needs it */
  int32_t *d_owner_found;                    /* ... and behind it skred_fxbank_release_tags' list, SKRED_OWNER_MAX_TAGS entries */
  uint32_t *d_match_pair;                    /* ... and behind that the two words the count pass of skred_fxbank_find_match fills */
  uint32_t *d_pedal;                         /* pedals (skred_fx_pedal.c): one word per voice, SKRED_PEDAL_*; NULL until the first call that needs it */
  skx_glide_t *d_glide;                      /* portamento (skred_fx_glide.c): four words per voice; NULL until the first call that starts a glide */
  skx_bend_t *d_bend;                        /* the pitch wheel (skred_fx_bend.c): two words per voice; NULL until the first call that bends */
  skx_cut_t *d_cut;                          /* filter cutoff (skred_fx_cutoff.c): eight words per voice; NULL until the first call that sets a cutoff */
  skx_fenv_t *d_fenv;                        /* the filter envelope (skred_fx_fenv.c): eight words per voice; NULL until the first record call */
  long long *d_mix; size_t mix_cap;
  int32_t *d_stems; size_t stems_cap;
  uint64_t count;
  hipEvent_t ev0, ev1;
  int timed;
};

int skred_amd_set_error(int code, const char *fmt, ...);   /* skred_bank.c */

#define HIP_TRY(call)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) return skred_amd_set_error(SKRED_E_NO_DEVICE, "%s -> %s", #call, hipGetErrorString(e_)); \
  } while (0)

/* the fields the biquad and the one-shots brought (filter_mode .. y2): a caller that zero-initialises the struct and leaves
 * them NULL gets what it got before they existed -- no filter, no one-shot, a delay line at rest */
#define FX_OPT(arr, v) ((arr) ? (arr)[v] : 0)

/* skred_fxbank.c: voice v of the host view as the planes hold it.  `check`: SKRED_DIRTY_PARAMS -- the table window and the amp
 * range, SKRED_DIRTY_FILTER_STATE -- the delay line; refusals as skred_fxbank_upload states them. */
int skx_pack_voice(const skred_fxbank_t *fx, const skred_fxpt_bank_t *h, int v, uint32_t check, skx_plane_t ro[SKX_COUNT],
                   skx_plane_t rw[SKX_RW_COUNT]);

/* skred_fx_live.c */
#define SKX_NOTE_LIST_WORDS 4      /* in front of the bank's note list: the idle query's two counts, the joined list's length, padding */
void skx_live_free(skred_fxbank_t *fx);
int skx_stamp_ids(skred_fxbank_t *fx, const int32_t *voices, int n, int which, const char *who, hipStream_t s);
/* ... for skred_fxbank_note_on_steal: the idle query's launches (q checked by the caller), room for n entries in d_note_list, and
 * the checked notes through the batch path into the placement kernel (`who`, here and below: the entry point, for the error text) */
int skx_idle_launch(skred_fxbank_t *fx, const skred_fx_idle_query_t *q, int32_t *d_voices, uint32_t *d_count, hipStream_t s);
/* ... for skred_fxbank_find_match too: the query scratch (SKX_IDLE_W_COUNT words, idle_wgs counts, idle_wgs offsets; allocated once,
 * for the whole bank, the words zeroed on `s`), and room for 2 + need entries in d_idle_out / h_idle_out */
int skx_idle_scratch(skred_fxbank_t *fx, hipStream_t s);
int skx_idle_out_room(skred_fxbank_t *fx, size_t need);
int skx_note_list_room(skred_fxbank_t *fx, int n);
int skx_notes_launch(skred_fxbank_t *fx, const skred_fx_note_t *notes, int n, const int32_t *d_voices, const uint32_t *d_count,
                     int first_entry, int32_t *d_assigned, uint32_t *d_result, const char *who, hipStream_t s);

/* skred_fx_stage.c, the batch path every staged launch takes.  begin: a slot of the ring with room for `bytes`, not in flight, filled
 * through bt->h.  send: the copy on `s`; returns the slot's device twin, or NULL with the error set.  end: the slot's event behind
 * everything queued, failed launch or not, then the verdict: `e`, the first launch that failed, fails the call under `who` */
typedef struct { skx_slot_t *sl; void *h; } skx_batch_t;
int skx_batch_begin(skred_fxbank_t *fx, size_t bytes, skx_batch_t *bt);
const void *skx_batch_send(skx_batch_t *bt, size_t bytes, hipStream_t s);
int skx_batch_end(skx_batch_t *bt, hipError_t e, const char *who, hipStream_t s);

/* skred_fx_steal.c */
void skx_steal_free(skred_fxbank_t *fx);

/* skred_fx_owner.c: the owner array (allocated and zero-filled by the first call that needs it), for the guarded controller too */
void skx_owner_free(skred_fxbank_t *fx);
int skx_owner_ensure(skred_fxbank_t *fx);
/* ... and skred_fxbank_tag_list behind its checks, for the channel burst of skred_fx_steal.c: n >= 1 tags through the batch path
 * into the tag kernel */
int skx_owner_tag_launch(skred_fxbank_t *fx, const int32_t *d_voices, const uint32_t *tags, int n, const uint32_t *d_count,
                         uint32_t *d_result, const char *who, hipStream_t s);
/* ... and the find pass of skred_fxbank_release_tags, for the pedals: begins the batch `bt` with sorted | perm (| the tags as given,
 * with_tags) of n checked tags and queues the find pass over a checked range into d_out; *err is that launch's verdict.  The caller
 * queues what else reads the slot (bt->sl->d), then ends the batch */
int skx_owner_find_launch(skred_fxbank_t *fx, int first, int count, const uint32_t *tags, int n, int with_tags, int32_t *d_out, hipStream_t s,
                          skx_batch_t *bt, hipError_t *err);
/* skred_fx_pedal.c: the pedal array, freed with the bank */
void skx_pedal_free(skred_fxbank_t *fx);
/* skred_fx_glide.c: the glide array, freed with the bank; and the checked entries as they travel -- out[j] = glide[perm[j]] (perm NULL:
 * j), the five named words as they stand, the rest zero.  Pure host */
void skx_glide_free(skred_fxbank_t *fx);
void skx_glide_pack(const skred_fx_glide_t *glide, int n, const uint32_t *perm, skx_glide_each_t *out);
/* skred_fx_bend.c: the bend array, freed with the bank; and the checked ratios as they travel -- out[j] = ratios[perm[j]] (perm NULL:
 * j).  Pure host */
void skx_bend_free(skred_fxbank_t *fx);
void skx_bend_pack(const uint32_t *ratios_q24, int n, const uint32_t *perm, uint32_t *out);
/* skred_fx_cutoff.c: the cutoff array, freed with the bank (skred_fxbank.c); and the checked records as they travel -- out[j] =
 * rec[perm[j]] (perm NULL: j), set and value as they stand, q_q16, mode and the rates where named, the rest zero.  Pure host */
void skx_cutoff_free(skred_fxbank_t *fx);
void skx_cutoff_pack(const skred_fx_cutoff_t *rec, int n, const uint32_t *perm, skx_cut_each_t *out);
/* ... and the allocation of the array by the first call that needs it (the owner array first), for the filter envelope too */
int skx_cutoff_ensure(skred_fxbank_t *fx);
/* skred_fx_fenv.c: the filter-envelope array, freed with the bank (skred_fxbank.c); and the checked records as they travel -- out[j] =
 * rec[perm[j]] (perm NULL: j), word for word.  Pure host */
void skx_fenv_free(skred_fxbank_t *fx);
void skx_fenv_pack(const skred_fx_fenv_t *rec, int n, const uint32_t *perm, skx_fenv_each_t *out);
/* skred_fx_ctl.c: the checked record as it travels (the reserved words carry the reciprocals).  Pure host */
void skx_ctl_pack(const skred_fx_ctl_t *ctl, skx_ctl_t *out);
/* skred_fx_expr.c: the checked entries as they travel -- out[j] = each[perm[j]] (perm NULL: j), the named values word for word, the
 * others zeroed.  Pure host */
void skx_each_pack(const skred_fx_ctl_each_t *each, int n, const uint32_t *perm, skx_each_t *out);
/* ... and n checked sets of per-entry filter coefficients the same way: out[j] = filt[perm[j]], five words, the rest zero.  Pure host */
void skx_filt_pack(const skred_fx_filter_each_t *filt, int n, const uint32_t *perm, skx_filt_each_t *out);
/* skred_bank_owner.c: the find pass's view of n <= SKRED_OWNER_MAX_TAGS tags (sorted ascending as unsigned numbers, and where each stood) */
int sk_owner_pack(const uint32_t *tags, int n, uint32_t *sorted, uint32_t *perm);
/* skred_bank_checks.c, the float bank's argument checks this bank shares (`who`: the entry point, with its "fx " in front): the stamp
 * bits, a list's length, a range of voices (K = 1) inside the bank, empty only where allowed, a plain window */
int sk_check_stamps(uint32_t stamps, const char *who);
int sk_check_list_n(int n, const char *who);
int sk_check_slot_range(int n_voices, int first, int count, int K, int allow_empty, const char *who);
int sk_check_window(int n_voices, int first, int count, const char *who);
/* skred_bank_stage.c: the ending of a _host query -- returns the entries copied to `out`, or an error; and room for `need` entries
 * behind `head` words in a grow-on-demand answer buffer (h_buf NULL: no pinned twin) */
int sk_read_back(const int32_t *d_out, int32_t *h_out, int counts, int max_out, int bound, int32_t *out, hipStream_t s, const char *who);
int sk_answer_room(void **d_buf, void **h_buf, size_t *cap, size_t head, size_t need);
/* ... and the per-voice side arrays (owners, pedals): allocated and zeroed for every stream, a checked window cleared on a stream, a
 * checked window downloaded (zeros when d_arr is NULL) */
int sk_side_alloc(void **d_arr, size_t bytes, const char *what);
int sk_side_clear(void *d_arr, size_t elem, int device, int n_voices, int first, int count, hipStream_t s, const char *who);
int sk_side_download(const void *d_arr, size_t elem, int device, int n_voices, void *host, int first, int count, const char *who);

/* skred_fx_kernels.hip, skred_fx_live_kernels.hip */
int skx_launch_stamp(const int32_t *d_ids, int n, int which, skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now, hipStream_t stream);
int skx_launch_update(const skx_update_t *d_updates, int n, skx_plane_t *const ro[SKX_COUNT], skx_plane_t *const rw[SKX_RW_COUNT],
                      uint64_t now, hipStream_t stream);
int skx_idle_workgroups(int first, int count);
int skx_launch_idle(const skx_idle_args_t *args, hipStream_t stream);
int skx_launch_notes(const skx_note_t *d_notes, int n, const int32_t *d_voices, const uint32_t *d_count, int first_entry, int n_voices,
                     skx_plane_t *const ro[SKX_COUNT], skx_plane_t *const rw[SKX_RW_COUNT], uint64_t now, int32_t *d_assigned,
                     uint32_t *d_result, hipStream_t stream);
int skx_launch_stamp_list(const int32_t *d_voices, int n, const uint32_t *d_count, int n_voices, uint32_t stamps,
                          skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now, hipStream_t stream);


/* skred_fx_owner_kernels.hip, skred_fx_ctl_kernels.hip */
int skx_launch_stamp_owned(const uint32_t *owner, const int32_t *d_voices, const uint32_t *d_tags, int n, const uint32_t *d_count,
                           int n_voices, uint32_t stamps, skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now, uint32_t *d_result,
                           hipStream_t stream);
int skx_launch_ctl_range(const skx_ctl_t *d_rec, int first, int count, skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result,
                         hipStream_t stream);
int skx_launch_ctl_list(const skx_ctl_t *d_rec, const int32_t *d_voices, const uint32_t *d_tags, const uint32_t *owner, int n,
                        const uint32_t *d_count, int n_voices, skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result, hipStream_t stream);
/* skred_fx_expr_kernels.hip (the ordered list of the matches is the float bank's sk_launch_match_find, skred_launch.h) */
int skx_launch_match_stamps(const uint32_t *owner, uint32_t value, uint32_t mask, int first, int count, uint32_t stamps,
                            skx_plane_t *time_plane, skx_plane_t *rw0, uint64_t now, uint32_t *d_result, hipStream_t stream);
int skx_launch_ctl_match(const skx_ctl_t *d_rec, int first, int count, const uint32_t *owner, uint32_t value, uint32_t mask,
                         skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result, hipStream_t stream);
/* the per-entry controller: d_filt == NULL the FILT = false instantiation (d_each required), else FILT = true (d_each may be NULL) */
int skx_launch_ctl_owned_each_filter(const skx_ctl_t *d_rec, const skx_each_t *d_each, const skx_filt_each_t *d_filt, const int32_t *d_voices,
                                     const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count, int n_voices,
                                     skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result, hipStream_t stream);
/* skred_fx_glide_kernels.hip (the clear behind a tag launch is the float bank's sk_launch_glide_clear at slot_voices = 1,
 * skred_launch.h).  d_each: 16-byte aligned; each d_result may be NULL and is zeroed on `stream` ahead of its kernel.  bend: the
 * bank's pitch-wheel array, or NULL on a bank without one (the BEND = false instantiations: the kernels as they were).  With the
 * array, on a voice whose key word is not 0 the glide runs on the key, and phase_inc is stored again as (key * ratio_q24) >> 24 */
/* entry k starts d_each[k]'s glide on d_voices[k] where that is a voice whose owner is d_tags[k]; d_result[3] += voices set gliding,
 * starts withheld, voices whose owner differs */
int skx_launch_glide_start(skx_glide_t *glide, skx_bend_t *bend, const skx_glide_each_t *d_each, const int32_t *d_voices, const uint32_t *d_tags,
                           const uint32_t *owner, int n, const uint32_t *d_count, int n_voices, skx_plane_t *osc, uint32_t *d_result,
                           hipStream_t stream);
/* the advance pass by num_frames over [first, first + count) (inside the bank); d_result[2] += voices still gliding, voices that arrived */
int skx_launch_glide_advance(skx_glide_t *glide, skx_bend_t *bend, skx_plane_t *osc, int first, int count, int num_frames, uint32_t *d_result,
                             hipStream_t stream);
/* glide[first .. first + count) = 0; snap != 0: a gliding voice's increment (bend: its key) = its target first */
int skx_launch_glide_stop(skx_glide_t *glide, skx_bend_t *bend, skx_plane_t *osc, int first, int count, int snap, hipStream_t stream);
/* skred_fx_bend_kernels.hip (the clear behind a tag launch is the float bank's sk_launch_bend_clear at slot_voices = 1, skred_launch.h).
 * Each d_result[3] may be NULL and is zeroed on `stream` ahead of its kernel: voices stored or restored, bends withheld, and */
/* ... the absolute bend to ratio_q24 on the voices of [first, first + count) (inside the bank) whose owner matches; [2]: voices of
 * the range that did not match */
int skx_launch_bend_match(skx_bend_t *bend, uint32_t ratio_q24, int first, int count, const uint32_t *owner, uint32_t value, uint32_t mask,
                          skx_plane_t *osc, uint32_t *d_result, hipStream_t stream);
/* ... entry k bends d_voices[k] to d_ratios[k] where that is a voice whose owner is d_tags[k]; [2]: voices whose owner differs */
int skx_launch_bend_each(skx_bend_t *bend, const uint32_t *d_ratios, const int32_t *d_voices, const uint32_t *d_tags, const uint32_t *owner,
                         int n, const uint32_t *d_count, int n_voices, skx_plane_t *osc, uint32_t *d_result, hipStream_t stream);
/* bend[first .. first + count) = 0; snap != 0: a bent voice's increment = its key first */
int skx_launch_bend_range_clear(skx_bend_t *bend, skx_plane_t *osc, int first, int count, int snap, hipStream_t stream);
/* skred_fx_cutoff_kernels.hip (the clear behind a tag launch is the float bank's sk_launch_cutoff_clear at slot_voices = 1,
 * skred_launch.h).  bend: the bank's pitch-wheel array or NULL (TRACK reads a bent voice's key).  ro: the bank's planes -- phase_inc is
 * read, the five coefficient words are stored.  Each d_result may be NULL and is zeroed on `stream` ahead of its kernel: [4] voices set
 * or started, records withheld, [2] below, cutoffs clamped.  fenv: the bank's filter-envelope array or NULL (a voice set, started or
 * stopped loses its contour: its eight fenv words = 0; the advance hands a voice with a contour to skx_fenv_advance) */
/* ... the record on the voices of [first, first + count) (inside the bank) whose owner matches; [2]: voices that did not match */
int skx_launch_cutoff_match(skx_cut_t *cut, const skx_bend_t *bend, skx_fenv_t *fenv, const skx_cut_each_t *rec, int first, int count,
                            const uint32_t *owner, uint32_t value, uint32_t mask, skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result, hipStream_t stream);
/* ... entry k brings d_each[k] (16-byte aligned) to d_voices[k] where that is a voice whose owner is d_tags[k]; [2]: voices whose owner differs */
int skx_launch_cutoff_each(skx_cut_t *cut, const skx_bend_t *bend, skx_fenv_t *fenv, const skx_cut_each_t *d_each, const int32_t *d_voices,
                           const uint32_t *d_tags, const uint32_t *owner, int n, const uint32_t *d_count, int n_voices, skx_plane_t *const ro[SKX_COUNT],
                           uint32_t *d_result, hipStream_t stream);
/* the advance pass by num_frames over [first, first + count) (inside the bank); d_result[2] += voices still moving, voices that arrived.
 * fenv == NULL: the plain instantiation, the kernel of a bank without a filter-envelope array */
int skx_launch_cutoff_advance(skx_cut_t *cut, skx_fenv_t *fenv, skx_plane_t *const ro[SKX_COUNT], int first, int count, int num_frames,
                              uint32_t *d_result, hipStream_t stream);
/* every movement of the range ends; snap != 0: a moving voice's w = its target and its coefficients computed first */
int skx_launch_cutoff_stop(skx_cut_t *cut, skx_fenv_t *fenv, skx_plane_t *const ro[SKX_COUNT], int first, int count, int snap, hipStream_t stream);
/* skred_fx_fenv_kernels.hip (the clear behind a tag launch is the float bank's sk_launch_fenv_clear at slot_voices = 1, skred_launch.h).
 * ro: the bank's planes -- the five coefficient words are stored.  Each d_result may be NULL and is zeroed on `stream` ahead of its
 * kernel: [4] voices started, records withheld, [2] below, voices clamped */
/* ... the record on the voices of [first, first + count) (inside the bank) whose owner matches; [2]: voices that did not match */
int skx_launch_fenv_match(skx_fenv_t *fenv, skx_cut_t *cut, const skx_fenv_each_t *rec, int first, int count, const uint32_t *owner, uint32_t value,
                          uint32_t mask, skx_plane_t *const ro[SKX_COUNT], uint32_t *d_result, hipStream_t stream);
/* ... entry k brings d_each[k] (16-byte aligned) to d_voices[k] where that is a voice whose owner is d_tags[k]; [2]: voices whose owner differs */
int skx_launch_fenv_each(skx_fenv_t *fenv, skx_cut_t *cut, const skx_fenv_each_t *d_each, const int32_t *d_voices, const uint32_t *d_tags,
                         const uint32_t *owner, int n, const uint32_t *d_count, int n_voices, skx_plane_t *const ro[SKX_COUNT],
                         uint32_t *d_result, hipStream_t stream);

#endif
