/*
 * skred_bank_priv.h -- internals shared by the translation units behind include/skred_amd.h.  Not installed.
 *   skred_bank.c         lifecycle, tables, upload / download, options, class and tape plan
 *   skred_bank_render.c  one block from request to kernels, as skred_bank_plan.c picks them
 *   skred_bank_stage.c   the staging ring and the batch path: the one way a host-written batch reaches a kernel; the _host queries' read-back;
 *                        the per-voice side arrays (owners, pedals, glides) of both banks: sk_side_alloc / _clear / _download
 *   skred_bank_checks.c  the argument checks the control calls share (pure host; the fixed-point bank uses them too)
 *   skred_bank_update.c  block-granular updates and the deferred queue
 *   skred_bank_idle.c    the free-voice query                  skred_bank_steal.c  the victim query
 *   skred_bank_notes.c   note-ons and stamps on voices a device-resident list names
 *   skred_bank_slots.c   the same for the slots of a tiled patch, slot stealing, and channel polyphony (matched stealing, capped note-ons)
 *   skred_bank_ctl.c     patch controllers                     skred_bank_owner.c  note owners
 *   skred_bank_expr.c    channels and per-note expression: masked owner matches, per-entry controller values and filter coefficients
 *   skred_bank_pedal.c   pedals: note-offs held back per slot, sostenuto's latch, the pedal-up
 *   skred_bank_glide.c   portamento: per-voice glides, started under the owner guard, advanced and landed on the device
 *   skred_bank_bend.c    the pitch wheel: absolute bends that keep the key's bits beside the sounding increment
 *   skred_bank_cutoff.c  filter cutoff on the device: key-tracked cutoffs that glide and land, coefficients computed where the voice lives
 *   skred_bank_fenv.c    filter envelope: per-note cutoff contours, stepped by the cutoff's advance pass, released by the voice's clock
 */
#ifndef SKRED_BANK_PRIV_H
#define SKRED_BANK_PRIV_H

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "skred_amd.h"
#include "skred_bank_plan.h"
#include "skred_device_layout.h"
#include "skred_launch.h"

#define SK_TIMING_RING 256
#define SK_REPORT_RING 64
#define SK_UPD_RING 8

typedef struct {
  void *h, *d;                /* pinned host buffer and its device twin */
  size_t cap;                 /* bytes */
  uint32_t seq;               /* != 0: a batch read from this slot is in flight; its last kernel stores this number into the bank's
                                 h_upd_done[slot] when it has run (no event: skred_update_kernels.hip, sk_batch_done) */
} sk_upd_slot_t;

struct skred_bank {
  int device;
  int n_cus;                  /* compute units of the device (the two-per-lane kernel's passes come one per CU, then two) */
  int n_voices, n_padded, n_groups;
  sk_plane_t *d_planes;       /* the slab behind d_ro[] / d_rw[] */
  sk_plane_t *d_ro[SKP_COUNT];
  sk_plane_t *d_rw[SKS_COUNT];
  float *d_tables;
  float *h_tables;            /* host copy of the pool (sk_pack_voice looks for guard samples: SKF_GUARD) */
  size_t table_floats;        /* real pool size       */
  size_t table_floats_padded; /* rounded up to 4      */
  float *d_partial;           /* [n_wg][F][2] workgroup rows, then [SK_FINISH_SLABS][F][2] slab sums, then [F] master gains */
  size_t partial_cap;         /* floats */
  uint32_t *d_tickets;        /* [SK_FINISH_SLABS + 1] arrival counters of the in-kernel mix-down */
  int timing_every;           /* SKRED_OPT_KERNEL_TIMING: bracket every n-th launch's render kernels with an event pair (0: none) */
  float *d_gain_state;        /* [0] master smoother gain carried between blocks; [1] the gain a sum-only render prepared for skred_bank_master */
  float *d_pp_gains;          /* [2][pp_gains_cap]: the per-frame master gains of the pipelined sum-only form's two blocks in flight (fixed rows:
                                 block k's master stage reads its row while block k + 1 renders, whatever kernel and block length that one has) */
  size_t pp_gains_cap;        /* floats per row */
  int pp_parity;              /* >= 0 only inside sk_bank_render_sum_pp: which of the two gain rows the sum-only render fills */
  int gains_frames;           /* > 0: the latest skred_bank_render() left the master gains of a block of this many frames in d_partial */
  size_t gains_offset;        /* ... at this float offset */
  float *d_out, *d_stems;     /* scratch of skred_bank_render_host */
  size_t out_cap, stems_cap;
  uint16_t *h_class;          /* per-voice SKC_* bits, shadow used to pick the kernel */
  int8_t *h_mod;              /* [4][n_padded] modulator lane inside the 64-voice group (fm, am, pm, cz) or -1 */
  int *h_level;               /* [n_padded] dependency level of each voice (modulated banks) */
  int *d_level;
  int32_t *d_env_list;        /* the voices on the motion list, in ascending order (sk_collect_expand_kernel) */
  int32_t *d_env_off;         /* per 128-voice wave slice: where its voices start in d_env_list; one more slot: their number */
  int32_t *d_group_flag;      /* per 128-voice wave slice: listed voices; one more slot: the one-voice family's "an envelope moved" ticket */
  /* THE MOTION LIST of the two-per-lane family (skred_device_layout.h: mask_cur): a bit per voice, double-buffered -- the
   * block reads d_mask[mask_p] and builds d_mask[mask_p ^ 1] (survivors), control actions OR into d_mask[mask_p] */
  uint64_t *d_mask[2];
  int mask_p;
  int mask_dirty;             /* the list must be rebuilt from the planes before the next two-per-lane block (upload, clock change,
                                 a stretch on another kernel family, a violation report) */
  int list_empty;             /* STRUCTURAL: the last list the device built was empty and nothing was added since (no control action);
                                 the envelope kernel is then not launched -- with an empty list it has nothing to render */
  uint32_t *d_violations;     /* sticky device counter: sk_render_fast2_kernel found a moving voice that was not listed; the word behind
                                 it: sk_gain_kernel's row counter (skred_device_layout.h: env_count) */
  /* listed voices rendered in place (skred_bank_plan.c: sk_plan_finish): the gain rows, and a proven upper bound on the current list's length --
   * the length launch t reported plus the voices control actions have touched since launch t was issued */
  float *d_env_gain;
  size_t env_gain_cap;        /* floats */
  uint64_t touched_total;     /* voices named by control actions so far (every one of them goes on the list: sk_list_voice) */
  uint64_t bound_touched;     /* ... when the launch that reported bound_len was issued */
  uint32_t bound_len, bound_min_ticket;   /* reports of launches before bound_min_ticket (the last rebuild of the list) do not count */
  int bound_valid;
  int last_in_place;          /* the latest block took that path */
  int32_t *d_probe_ids;       /* skred_bank_set_probe: the probed voices on the device, their number, the caller's buffer */
  int n_probe;
  float *d_probe_out;
  int32_t *d_tap_ids;         /* skred_bank_set_taps: the same for the tapped voices (a bank has a probe or taps, never both) */
  int n_taps;
  float *d_taps_out;
  int last_taps;              /* taps the latest block wrote */
  uint32_t *d_form_counts;    /* skred_bank_set_form_counter: the caller's [2] counters, or NULL */
  int split_mode;             /* SKRED_OPT_SPLIT: 0 never (default), 1 where it is the faster form, 2 whenever the bank qualifies */
  int split_pairs;            /* SKRED_OPT_SPLIT_PAIRS: 0 the library's choice, 2 / 4 forced (tests) */
  int last_split;             /* the latest block ran sk_render_split_kernel */
  /* packed lanes of sparse banks (skred_device_layout.h: pack_mask; skred_bank.c: sk_pack_refresh, skred_bank_plan.c: sk_plan_finish) */
  int pack_mode;              /* SKRED_OPT_PACK: 0 never, 1 where it pays (default) */
  int fm_skew;                /* SKRED_OPT_FM_SKEW: modulator lanes a block ahead of their carriers (default 1) */
  uint64_t *h_pack_mask;      /* [n_padded / 64] per aligned 64-voice group: voices that can sound, and the modulators they name */
  uint64_t *d_pack_mask;
  uint8_t *h_pack_dirty;      /* [n_padded / 64] a voice of the group changed class or modulator: its word is recomputed */
  int pack_any_dirty;
  int pack_hist[65];          /* groups per number of set bits in their word (the highest non-empty bin sizes the lane slots) */
  int pack_upload;            /* the device copy of the words is stale */
  int pack_zero;              /* a voice without a lane may hold a voice_sample the reference's skip rule would have cleared */
  int last_pack;              /* lanes per 64-voice group in the latest block (0: not packed) */
  int in_place_mode;          /* SKRED_OPT_IN_PLACE: 0 never, 1 where it is the faster path (default), 2 wherever the rows provably suffice */
  uint32_t violations_seen;   /* ... as last read back */
  hipStream_t side;           /* the envelope kernel's stream, beside the caller's */
  hipEvent_t ev_fork, ev_join;
  int last_family;            /* SKRED_KERNEL_* of the previous block (the list is only maintained while the two-per-lane family renders) */
  int max_level;
  int class_dirty;
  int cnt_real, cnt_filter, cnt_env, cnt_exotic, cnt_stops, cnt_fm;   /* voices per SKC_* bit (kept incrementally) */
  int cnt_guard;              /* real voices with SKC_GUARD */
  uint32_t tables_epoch, guard_epoch;   /* pools set so far; the pool the whole bank was last packed against (guard flags are a property of the pool) */
  int cnt_pair_ap;            /* pair-shaped carriers whose amplitude or pan is modulated too (SKC_PAIR_AP) */
  int cnt_fm_odd;             /* SKC_FM voices that are not the even half of a (carrier, next voice) pair (SKC_FM_ODD) */
  int cnt_cz;                 /* SKC_CZ voices: CZ phase distortion the one-voice kernel can render (they count in cnt_exotic too) */
  int cnt_cz_src;             /* ... of them, voices that read a previous-frame source (SKC_CZ_SRC) */
  uint32_t fast_mode_cz;      /* sk_classify(): the class mode with the SKC_CZ voices taken off the exotic count, | SKM_CZ; 0 when other
                                 exotic voices remain or the bank has no such voice.  Kept whatever SKRED_OPT_CZ_FAST says */
  int cnt_mod;                /* voices (real or not, like cnt_escapes) with SKC_MOD */
  int cz_fast;                /* SKRED_OPT_CZ_FAST */
  int last_cz;                /* the latest block ran a CZ instantiation of the one-voice kernel */
  int cnt_escapes;            /* voices naming a modulator outside their aligned 64-voice group (SKC_ESCAPES) */
  int cnt_outside;            /* ... of them, voices naming a modulator outside the bank (SKC_OUTSIDE): refused even with cross_group */
  /* cross-group modulation (SKRED_OPT_CROSS_GROUP; skred_device_layout.h: sk_tape_args_t; skred_bank.c: tape_plan) */
  int cross_group;            /* SKRED_OPT_CROSS_GROUP: 0 refuse such banks (default), 1 render them through the tape */
  int32_t *h_esc;             /* [4][n_padded] each voice's fm / am / pan / cz modulator when it sits in another group of the bank, else -1;
                                 allocated when the first such routing appears (NULL until then) */
  int esc_nomem;              /* ... that allocation failed: the bank refuses to render */
  int tape_dirty;             /* h_esc changed: the sources, the group graph and the pre-pass levels are planned again */
  int tape_rc;                /* != 0: the current plan was refused (a cycle, too deep); tape_msg says why */
  char tape_msg[256];
  int32_t *h_slot, *d_slot;   /* [n_padded] voice -> its tape slot, -1: not a source (allocated with h_esc) */
  int32_t *d_tape_groups;     /* the source groups, level by level (ascending inside a level) */
  size_t tape_groups_cap;     /* entries */
  int tape_level_off[SK_TAPE_MAX_LEVELS + 1];   /* level l: d_tape_groups[off[l], off[l + 1]) */
  int tape_sources, tape_levels;                /* of the current plan */
  float *d_tape;              /* [tape_sources][num_frames + 1] */
  size_t tape_cap;            /* floats */
  int last_tape_sources, last_tape_levels;      /* of the latest block (0, 0: it read no tape) */
  int mod_dirty;              /* modulator lanes changed: dependency levels must be recomputed */
  uint32_t fast_mode;         /* SKM_* from sk_classify() */
  int force_generic;          /* SKRED_OPT_FORCE_GENERIC */
  int fast2_min_voices;       /* SKRED_OPT_FAST2_MIN_VOICES */
  int fm2_min_voices;         /* SKRED_OPT_FM2_MIN_VOICES */
  int fast2_min_user;         /* ... was set by the caller (then it also applies to global-table banks) */
  int last_kernel;            /* SKRED_KERNEL_* used by the most recent render */
  skred_globals_t g;
  uint32_t features;
  hipEvent_t ev0[SK_TIMING_RING], ev1[SK_TIMING_RING]; /* around the render kernel of each call */
  int n_timed;                /* render calls since the last timing reset */
  /* what a launch found, reported by its final arriver into two pinned host words (no copy, no event): one-voice family --
   * "did an envelope move" (picks the lean instantiation: a speed hint); two-per-lane family -- the length of the list it
   * rendered, and the violation counter */
  uint32_t launch_ticket;     /* one per render launch */
  uint32_t control_epoch;     /* bumped by every upload / update / globals change */
  int env_quiet;              /* one-voice family: the last answered launch saw no envelope move and nothing changed since */
  volatile uint64_t *h_report;            /* pinned: [0] ticket << 32 | finding, [1] ticket << 32 | violations */
  uint32_t report_seen;                   /* ticket of the last report taken */
  uint32_t report_ticket[SK_REPORT_RING], report_epoch[SK_REPORT_RING];   /* what the launches that will report were issued under */
  uint8_t report_kind[SK_REPORT_RING];
  uint64_t report_touched[SK_REPORT_RING];   /* touched_total when the launch was issued */
  skred_seq_t *seq;             /* the pattern step clock (skred_seq.c), created on first use */
  struct sk_pat_step *pat;      /* [SKRED_PATTERNS_MAX][SKRED_SEQ_STEPS_MAX] batches the steps apply (skred_bank_update.c) */
  float seq_rate;               /* sample rate the step clock counts blocks in (0: the reference's 44100) */
  struct sk_queue_item *queue;  /* deferred updates (skred_bank_update.c), singly linked in arrival order */
  struct sk_queue_item *queue_tail;
  int queue_len;
  sk_upd_slot_t upd[SK_UPD_RING];   /* staging ring of host-written batches (skred_bank_stage.c) */
  uint32_t upd_head;
  volatile uint32_t *h_upd_done;    /* pinned [SK_UPD_RING]: the sequence number of the last batch each slot's kernels have finished with */
  uint32_t *d_upd_cnt;              /* device [SK_UPD_RING]: arrival counters of those kernels' workgroups */
  uint32_t upd_seq;
  uint32_t *upd_mark, upd_epoch;    /* per-voice epoch marks: duplicate voices inside one batch */
  /* the free-voice query (skred_bank_idle.c), everything allocated on first use */
  uint32_t *d_idle;                 /* SK_IDLE_W_COUNT words, idle_wgs counts, idle_wgs offsets (skred_launch.h) */
  int idle_wgs;
  uint64_t *d_named;                /* [n_padded / 64] the named set: bit v = some voice of the bank names voice v as a modulator */
  int named_dirty;                  /* the routing changed since d_named was built (sk_apply_meta): rebuilt by the next query that asks */
  int32_t *d_idle_out;              /* skred_bank_find_idle_host: [2] counts, then the list, and its pinned twin */
  int32_t *h_idle_out;
  size_t idle_out_cap;              /* entries of the list */
  /* skred_bank_note_on_idle (skred_bank_notes.c): the list its query leaves for its placement, allocated on first use */
  uint32_t *d_note_list;            /* [4] words (the query's d_count in the first two; skred_bank_note_on_steal: the joined list's length
                                       in the third), then note_list_cap voice indices */
  size_t note_list_cap;
  /* voice stealing (skred_bank_steal.c), everything allocated on first use */
  uint32_t *d_steal;                /* the radix select's scratch (skred_launch.h: SK_STEAL_W_*, histogram, counts, offsets, winners, keys) */
  int steal_wgs;
  int32_t *d_steal_out;             /* [2] counts (a matched query: [3]), then SK_STEAL_MAX victims: the _host queries' list and the note-on bursts' */
  int32_t *h_steal_out;             /* ... its pinned twin */
  /* note owners (skred_bank_owner.c), allocated and zeroed by the first call that needs them */
  uint32_t *d_owner;                /* [n_voices] a slot's tag at its first voice, 0: nobody; no render kernel reads it */
  int32_t *d_owner_slots;           /* [SKRED_OWNER_MAX_TAGS] skred_bank_release_tags: the list its find pass leaves for its stamps (behind d_owner) */
  uint32_t *d_match_pair;           /* [2] skred_bank_find_match: where the shared count pass leaves (written, total) (behind d_owner_slots) */
  /* pedals (skred_bank_pedal.c), allocated and zeroed by the first pedal call */
  uint32_t *d_pedal;                /* [n_voices] a slot's SKRED_PEDAL_* bits at its first voice; NULL: no pedal call yet, and the tag
                                       launches clear nothing; no render kernel reads it */
  /* portamento (skred_bank_glide.c), allocated and zeroed by the first call that starts a glide */
  sk_glide_t *d_glide;              /* [n_voices] target, rate_up, rate_down, carry per voice; target 0: not gliding; NULL: no glide was
                                       ever started, and the tag launches clear nothing; no render kernel reads it */
  /* the pitch wheel (skred_bank_bend.c), allocated and zeroed by the first call that bends */
  sk_bend_t *d_bend;                /* [n_voices] key, ratio per voice; key 0: not bent; NULL: no voice was ever bent, the tag launches
                                       clear nothing and the glide launches run as they always ran; no render kernel reads it */
  /* filter cutoff (skred_bank_cutoff.c), allocated and zeroed by the first call that sets a cutoff */
  sk_cut_t *d_cut;                  /* [n_voices] w, target, rate_up, rate_down, carry, q, mode, 0 per voice; w 0: no device cutoff; NULL:
                                       no cutoff was ever set, and the tag launches clear nothing; no render kernel reads it */
  /* filter envelope (skred_bank_fenv.c), allocated and zeroed by the first record call */
  sk_fenv_t *d_fenv;                /* [n_voices] stage, w_peak, w_sustain, w_end, rate_attack, rate_decay, rate_release, 0 per voice; stage
                                       0: no contour; NULL: no record was ever sent, the tag launches clear nothing and the cutoff
                                       launches run as they always ran; no render kernel reads it */
};

/* per-voice classification (host shadow) */
#define SKC_REAL   1u   /* a voice was uploaded into this slot and it can sound (has a table) */
#define SKC_FILTER 2u
#define SKC_ENV    4u
#define SKC_EXOTIC 8u   /* needs the generic kernel: see sk_plan_class_mode() */
#define SKC_FM    32u   /* carrier of a higher-indexed modulator of its 64-voice group, nothing else modulated */
#define SKC_STOPS 16u   /* one-shot without loop (plays to its table end and finishes) or reverse playback: the one-per-lane kernel's extended instantiation */
#define SKC_FM_ODD 256u /* an SKC_FM voice that is anything but: even index, frequency-modulated by the voice after it and by nothing else
                          -- the shape sk_render_fast2_kernel<FMP> renders with carrier and modulator in one lane */
#define SKC_PAIR_AP 512u /* a pair-shaped carrier whose amplitude or pan is modulated (by the voice after it or by itself) */
#define SKC_GUARD 64u   /* loops over its whole table with a guard sample behind it (SKF_GUARD): when every real voice does, the
                           linear lookup runs the instantiations without the fold test */
#define SKC_LIVE 1024u  /* can sound as far as its parameters say: a usable table and voice_amp != 0 (synth.c:537; a voice that has
                           finished is a matter of state, not of class) */
#define SKC_ESCAPES 128u /* names a modulator outside its aligned 64-voice group: the bank cannot be rendered until that is fixed
                            (SKRED_OPT_CROSS_GROUP: unless the modulator is in the bank -- then it is read from the tape) */
#define SKC_CZ 4096u    /* (with SKC_EXOTIC) a CZ voice of the fast family: cz_mode 1..7, finite phase data, its CZ source absent or a
                           higher-indexed voice of its aligned 64-voice group (the previous-frame read), its FM / AM / pan modulators
                           as SKC_FM asks (above it in the group; AM / pan also the voice itself) */
#define SKC_CZ_SRC 8192u /* an SKC_CZ voice with any such source: the launch exchanges voice_sample (SKM_FM) */
#define SKC_MOD 16384u  /* modulated in a way only the modulated kernel serves: what asks for SKB_ANY_MOD, as a bit that can be counted
                           (the feature word is only ever set; with SKRED_OPT_CZ_FAST on the count decides: skred_bank_plan.c) */
#define SKC_OUTSIDE 2048u /* with SKC_ESCAPES: the modulator is outside the bank (md < 0 or md >= n_voices): always refused */


int skred_amd_set_error(int code, const char *fmt, ...);
#define fail skred_amd_set_error
#define HIP_TRY(call)                                                              \
  do {                                                                             \
    hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess)                                                          \
      return fail(SKRED_E_NO_DEVICE, "%s -> %s", #call, hipGetErrorString(e_));   \
  } while (0)

/* One voice of the host view -> its device planes.  Pure: nothing in the bank changes; what the voice
 * means for kernel selection comes back in `meta` and is applied by sk_apply_meta() when the planes are
 * written.  phase_known: the host's voice_phase is the voice's current phase (an upload); 0 when only
 * parameters are being pushed and the phase lives on the device. */
typedef struct {
  uint16_t cls;         /* SKC_* */
  int8_t mod_lane[4];   /* modulator lane inside the 64-voice group (fm, am, pan, cz) or -1 */
  int32_t esc[4];       /* the modulator's voice index when it sits in another group of the bank (a tape source), else -1 */
  uint32_t features;    /* SKB_* this voice needs */
} sk_voice_meta_t;

int sk_pack_voice(const skred_bank_t *b, const skred_voice_bank_t *h, int v, int dst, int phase_known,
                  sk_plane_t ro[SKP_COUNT], sk_plane_t rw[SKS_COUNT], sk_voice_meta_t *meta);
/* params_travel: the parameter planes were written, so `meta` applies (a pure clock / state update leaves the classes alone) */
void sk_apply_meta(skred_bank_t *b, int dst, const sk_voice_meta_t *meta, int params_travel);
/* skred_bank.c, for render_block: the class mode, dependency levels and tape plan, made again where the voices changed; the lane
 * words of the groups whose voices changed (returns the most lanes a group needs) */
int sk_classify(skred_bank_t *b);
int sk_pack_refresh(skred_bank_t *b);
/* the pipelined multi-GPU form's two halves of a block (skred_bank_render.c; used by skred_shard.c) */
int sk_bank_render_sum_pp(skred_bank_t *b, int num_frames, int interp, float *d_sum, int parity, void *stream);
int sk_bank_master_pp(skred_bank_t *b, const float *d_sum, int num_frames, int num_channels, float *d_out, int parity, void *stream);
void sk_queue_free(skred_bank_t *b);
void sk_patterns_free(skred_bank_t *b);
void sk_idle_free(skred_bank_t *b);          /* skred_bank_idle.c: the query's scratch (skred_bank_destroy) */
void sk_steal_free(skred_bank_t *b);         /* skred_bank_steal.c: the victim query's scratch (skred_bank_destroy) */
/* skred_bank_idle.c: the named set is current on `s` (allocated and rebuilt when the routing changed) */
int sk_named_ensure(skred_bank_t *b, hipStream_t s);
/* skred_bank_steal.c, for skred_bank_note_on_steal: the query's checks (`voices`: where the list would go), and the query into the
 * bank's own d_steal_out (counts in its first two words) */
int sk_steal_check_bank(const skred_bank_t *b, const skred_steal_query_t *q, const void *voices, const void *count, const char *who);
int sk_steal_into_scratch(skred_bank_t *b, const skred_steal_query_t *q, hipStream_t s);
/* ... for skred_bank_slots.c (slot stealing): the scratch (allocated by the first query) and every argument of a query's launches
 * (`now` as the stamps take it); the bank's d_steal_out / h_steal_out */
int sk_steal_prepare(skred_bank_t *b, const skred_steal_query_t *q, int32_t *d_voices, uint32_t *d_count, hipStream_t s, sk_steal_args_t *a);
int sk_steal_out_buffers(skred_bank_t *b);
void sk_notes_free(skred_bank_t *b);         /* skred_bank_notes.c: the list scratch of skred_bank_note_on_idle (skred_bank_destroy) */
/* skred_bank_notes.c, for skred_bank_slots.c: skred_notes_check's rules on one record; room for n entries in d_note_list */
int sk_note_check_one(const skred_note_t *t, int k);
int sk_note_list_room(skred_bank_t *b, int n);
#define SK_NOTE_LIST_WORDS 4       /* in front of d_note_list's entries: a query's two counts, the joined list's length (note_on_steal), padded to 16 bytes */
/* skred_bank_ctl.c: the K records of a checked controller as they travel (masked ones word for word, the others zeroed); returns the
 * mask of the voices whose record puts them on the motion list.  Pure host */
uint64_t sk_ctl_pack(const skred_ctl_t *ctl, int slot_voices, uint64_t voice_mask, sk_ctl_t *out);
/* skred_bank_owner.c: the owner array (skred_bank_destroy); n <= SKRED_OWNER_MAX_TAGS tags as the find pass reads them -- sorted[j]
 * ascending as unsigned numbers, perm[j] the index that tag has in `tags`; returns 0, or 1 + the index of a repeated tag.  Pure host */
void sk_owner_free(skred_bank_t *b);
int sk_owner_pack(const uint32_t *tags, int n, uint32_t *sorted, uint32_t *perm);
/* ... and the array itself with the scratch behind it, allocated and zeroed by the first call that needs them (skred_bank_expr.c too) */
int sk_owner_ensure(skred_bank_t *b);
/* ... the find pass of n checked tags (1 .. SKRED_OWNER_MAX_TAGS, none zero, none twice) over a checked range into d_out on the
 * device (skred_bank_pedal.c: into d_owner_slots, as skred_bank_release_tags does) */
int sk_owner_find_launch(skred_bank_t *b, int first, int count, int slot_voices, const uint32_t *tags, int n, int32_t *d_out, hipStream_t s);
/* ... and skred_bank_tag_slots behind its checks, for the channel burst of skred_bank_slots.c: n >= 1 tags through the batch path
 * into the tag kernel (`who`: the caller, for the error text) */
int sk_owner_tag_launch(skred_bank_t *b, const int32_t *d_slots, const uint32_t *tags, int n, const uint32_t *d_count, int slot_voices,
                        uint32_t *d_result, const char *who, hipStream_t s);
/* skred_bank_pedal.c: the pedal array (skred_bank_destroy) */
void sk_pedal_free(skred_bank_t *b);
/* skred_bank_glide.c: the glide array (skred_bank_destroy); n checked entries as they travel -- out[j] = glide[perm[j]] (perm NULL:
 * glide[j]), the four named words as they stand, the reserved ones zero.  Pure host */
void sk_glide_free(skred_bank_t *b);
void sk_glide_pack(const skred_glide_t *glide, int n, const uint32_t *perm, sk_glide_each_t *out);
/* skred_bank_bend.c: the bend array (skred_bank_destroy); n checked ratios as they travel -- out[j] = the bits of ratios[perm[j]]
 * (perm NULL: ratios[j]).  Pure host */
void sk_bend_free(skred_bank_t *b);
void sk_bend_pack(const float *ratios, int n, const uint32_t *perm, uint32_t *out);
/* skred_bank_cutoff.c: the cutoff array (skred_bank_destroy); n checked records as they travel -- out[j] = rec[perm[j]] (perm NULL:
 * rec[j]), the named words as they stand, the others zero.  Pure host */
void sk_cutoff_free(skred_bank_t *b);
void sk_cutoff_pack(const skred_cutoff_t *rec, int n, const uint32_t *perm, sk_cut_each_t *out);
/* ... the array, allocated and zeroed if it does not exist yet (the owner array first; the bank's device is current); the planes the
 * cutoff and fenv launches touch; every lane of a slot (what the entry points hold filter_mask against) */
int sk_cutoff_ensure(skred_bank_t *b);
sk_cut_planes_t sk_cutoff_planes(const skred_bank_t *b);
uint64_t sk_all_lanes(int K);
/* skred_bank_fenv.c: the filter-envelope array (skred_bank_destroy); n checked records as they travel -- out[j] = rec[perm[j]] (perm
 * NULL: rec[j]), word for word, `start` zero where it is not named.  Pure host */
void sk_fenv_free(skred_bank_t *b);
void sk_fenv_pack(const skred_fenv_t *rec, int n, const uint32_t *perm, sk_fenv_each_t *out);
/* skred_bank_expr.c: n checked per-entry records as they travel -- out[j] = each[perm[j]] (perm NULL: each[j]), named values word for
 * word, the others zeroed; returns the SKRED_EACH_* bits of all of them together.  Pure host */
uint32_t sk_each_pack(const skred_ctl_each_t *each, int n, const uint32_t *perm, sk_each_t *out);
/* ... and n checked sets of per-entry filter coefficients the same way: out[j] = filt[perm[j]], five words, the rest zero.  Pure host */
void sk_filt_pack(const skred_filter_each_t *filt, int n, const uint32_t *perm, sk_filt_each_t *out);
/* skred_bank_idle.c, for skred_bank_slots.c: the scratch both list queries share (allocated on first use), the kernels' view of a
 * query on this bank, and room for `need` entries in d_idle_out / h_idle_out */
int sk_idle_scratch(skred_bank_t *b, hipStream_t s);
void sk_idle_args(const skred_bank_t *b, sk_idle_args_t *a, int first, int count, int from, int max_out, uint32_t which,
                  float settle_level, int32_t *d_voices, uint32_t *d_count);
int sk_idle_out_room(skred_bank_t *b, size_t need);
/* skred_bank_idle.c: everything skred_bank_find_idle refuses, without the device (`voices` / `count`: where the list and the
 * counts would go; `who` names the caller in the error text) */
int sk_idle_check(const skred_bank_t *b, const skred_idle_query_t *q, const void *voices, const void *count, const char *who);
/* skred_bank_stage.c, the staging ring of host-written batches: a free slot of at least `bytes` (waits for the batch that last
 * used it); where the kernel reads the staged bytes from (the pinned buffer itself, or its device twin behind a copy on `s`) */
int sk_staging_slot(skred_bank_t *b, size_t bytes, hipStream_t s, sk_upd_slot_t **out);
const void *sk_stage(sk_upd_slot_t *sl, size_t bytes, hipStream_t s);
/* ... and the batch path every staged launch takes.  begin: a slot with room for `bytes`, filled through bt->h.  send: where the
 * kernel reads from -- sk_stage's rule, or, `wide` (many workgroups read every byte), the device twin behind a copy -- and the
 * batch's number; NULL when the copy failed.  end: the launch's verdict -- failed: the stream is waited for (what is queued still
 * reads the slot) and the call fails under `who`; else the slot is the batch's until its kernel has run */
typedef struct {
  sk_upd_slot_t *sl;
  void *h;                      /* the slot's pinned buffer */
  uint32_t *cnt, *done, seq;    /* what a launcher takes as cnt, done, seq */
} sk_batch_t;
int sk_batch_begin(skred_bank_t *b, size_t bytes, hipStream_t s, sk_batch_t *bt);
const void *sk_batch_send(skred_bank_t *b, sk_batch_t *bt, size_t bytes, int wide, hipStream_t s);
int sk_batch_end(sk_batch_t *bt, hipError_t e, const char *who, hipStream_t s);
/* ... the ending of a _host query (plain pointers: the fixed-point bank's too): returns the entries copied to `out`, or an error; and
 * room for `need` entries behind `head` words in a grow-on-demand answer buffer (h_buf NULL: no pinned twin), both banks' */
int sk_read_back(const int32_t *d_out, int32_t *h_out, int counts, int max_out, int bound, int32_t *out, hipStream_t s, const char *who);
int sk_answer_room(void **d_buf, void **h_buf, size_t *cap, size_t head, size_t need);
/* ... and the per-voice side arrays (owners, pedals, glides; plain pointers: the fixed-point bank's too).  alloc: `bytes`, zeroed for
 * every stream, or a failure under `what`.  clear: the checked window of `elem`-byte elements zeroed on `s`.  download: the checked
 * window to `host`, zeros when the array was never allocated (d_arr NULL, which clear takes too) */
int sk_side_alloc(void **d_arr, size_t bytes, const char *what);
int sk_side_clear(void *d_arr, size_t elem, int device, int n_voices, int first, int count, hipStream_t s, const char *who);
int sk_side_download(const void *d_arr, size_t elem, int device, int n_voices, void *host, int first, int count, const char *who);
/* skred_bank_checks.c (`who`: the entry point, for the error text): K and -- `what` != NULL, its name -- a mask over the K voices;
 * the stamp bits; a list's length (n * K stays an int); a range of whole slots of K voices inside the bank, empty only where
 * allowed; a plain window for the clears and downloads */
int sk_check_slot_shape(int slot_voices, uint64_t mask, const char *what, const char *who);
int sk_check_stamps(uint32_t stamps, const char *who);
int sk_check_list_n(int n, const char *who);
int sk_check_slot_range(int n_voices, int first, int count, int K, int allow_empty, const char *who);
int sk_check_window(int n_voices, int first, int count, const char *who);
/* a control action reached the bank: what earlier launches reported about envelope activity no longer holds (the voices it
 * touched went on the motion list on the device: skred_update_kernels.hip) */
static inline void sk_control_changed(skred_bank_t *b) { b->control_epoch++; b->env_quiet = 0; b->list_empty = 0; }
/* ... and may have put this many more voices on the motion list (an upper bound: touched_total is what the in-place rule rests on) */
static inline void sk_touched(skred_bank_t *b, uint64_t voices) { b->touched_total += voices; sk_control_changed(b); }

#endif
