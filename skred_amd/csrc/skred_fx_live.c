/*
 * skred_fx_live.c -- live control of the fixed-point bank (include/skred_amd_fxpt.h: skred_fxbank_update, _find_idle /
 * _find_idle_host, _notes_on_list / _note_on_idle / _stamp_list; skred_fxbank_stamp's transport).
 *
 * The host side of skred_fx_live_kernels.hip: the checks (made before anything touches the device), the batch path
 * (skred_fx_stage.c), the launches.  Everything is queued on the caller's stream; the only waits are for a staging slot's own event,
 * when the ring has gone round, and -- in skred_fxbank_find_idle_host -- for the caller's stream.  The bank keeps no shadow of the
 * voices: all state the render kernel reads lives in the planes, except n_filter, which selects the biquad instantiation and is grown here.
 */
#include <stdlib.h>
#include <string.h>

#include "skred_fxbank_priv.h"

#define fail skred_amd_set_error

_Static_assert(sizeof(skx_update_t) == 160, "update record layout");
_Static_assert(sizeof(skred_fx_note_t) == sizeof(skx_note_t) && sizeof(skred_fx_note_t) == 32 &&
               offsetof(skred_fx_note_t, phase_inc) == 4 * SKX_NOTE_PHASE_INC && offsetof(skred_fx_note_t, velocity_q15) == 4 * SKX_NOTE_VELOCITY &&
               offsetof(skred_fx_note_t, phase) == 4 * SKX_NOTE_PHASE && offsetof(skred_fx_note_t, pan_left_q15) == 4 * SKX_NOTE_PAN_LEFT &&
               offsetof(skred_fx_note_t, pan_right_q15) == 4 * SKX_NOTE_PAN_RIGHT && offsetof(skred_fx_note_t, flags) == 4 * SKX_NOTE_FLAGS,
               "the device's note record must be skred_fx_note_t word for word");
/* the kernels spell the public bits out (skred_fx_live_kernels.hip: SKXU_*, SKXI_*, SKXN_*) */
_Static_assert(SKRED_DIRTY_PARAMS == 1u << 0 && SKRED_DIRTY_PHASE == 1u << 1 && SKRED_DIRTY_ENV_STATE == 1u << 2 && SKRED_DIRTY_PAN == 1u << 3 &&
               SKRED_DIRTY_FILTER_STATE == 1u << 4 && SKRED_DIRTY_SMOOTHER == 1u << 5 && SKRED_DIRTY_SAMPLE == 1u << 7 &&
               SKRED_STAMP_TRIGGER == 1u << 8 && SKRED_STAMP_RELEASE == 1u << 9 && SKRED_DIRTY_ENV_CLOCK == 1u << 10 &&
               SKRED_IDLE_FINISHED == 1u << 0 && SKRED_IDLE_ENV_DONE == 1u << 1 && SKRED_IDLE_AMP_ZERO == 1u << 2 &&
               SKRED_NOTE_SET_PHASE == 1u << 0 && SKRED_NOTE_SET_PAN == 1u << 1, "device bits must equal the public values");
/* sk_fx_stamp_kernel's `which` (skred_fxbank_stamp) against the stamp bits of an update */
_Static_assert(SKRED_FX_STAMP_TRIGGER == SKRED_STAMP_TRIGGER >> 8 && SKRED_FX_STAMP_RELEASE == SKRED_STAMP_RELEASE >> 8, "stamp bits");

#define SKX_STAMPS (SKRED_STAMP_TRIGGER | SKRED_STAMP_RELEASE)
#define SKX_IDLE_CRITERIA (SKRED_IDLE_FINISHED | SKRED_IDLE_ENV_DONE | SKRED_IDLE_AMP_ZERO)

void skx_live_free(skred_fxbank_t *fx) {
  for (int i = 0; i < SKX_RING; i++) {
    skx_slot_t *sl = &fx->ring[i];
    if (sl->d) hipFree(sl->d);
    if (sl->h) hipHostFree(sl->h);
    if (sl->ev) hipEventDestroy(sl->ev);
    memset(sl, 0, sizeof(*sl));
  }
  free(fx->upd_mark);
  fx->upd_mark = NULL;
  if (fx->d_idle) hipFree(fx->d_idle);
  if (fx->d_idle_out) hipFree(fx->d_idle_out);
  if (fx->h_idle_out) hipHostFree(fx->h_idle_out);
  if (fx->d_note_list) hipFree(fx->d_note_list);
  fx->d_idle = NULL; fx->d_idle_out = NULL; fx->h_idle_out = NULL; fx->d_note_list = NULL;
  fx->idle_wgs = 0; fx->idle_out_cap = 0; fx->note_list_cap = 0;
  skx_steal_free(fx);
  skx_owner_free(fx);
  skx_pedal_free(fx);
  skx_glide_free(fx);
  skx_bend_free(fx);
}

/* note-ons / note-offs of voices the host names: ids only (stamping a voice twice with the same clock is idempotent) */
int skx_stamp_ids(skred_fxbank_t *fx, const int32_t *voices, int n, int which, const char *who, hipStream_t s) {
  const size_t bytes = (size_t)n * sizeof(int32_t);
  skx_batch_t bt;
  const int rc = skx_batch_begin(fx, bytes, &bt);
  if (rc) return rc;
  memcpy(bt.h, voices, bytes);
  const int32_t *src = (const int32_t *)skx_batch_send(&bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)skx_launch_stamp(src, n, which, fx->d_ro[SKX_TIME], fx->d_rw[0], fx->count, s);
  return skx_batch_end(&bt, e, who, s);
}

/* ------------------------------------------------------------------ updates */

/* n packed, checked records (n_filter of them bring a biquad; upd_mark allocated) -> a staging slot -> the update kernel */
static int update_launch(skred_fxbank_t *fx, const skx_update_t *rec, int n, int n_filter, hipStream_t s) {
  HIP_TRY(hipSetDevice(fx->device));
  const size_t bytes = (size_t)n * sizeof(skx_update_t);
  skx_batch_t bt;
  const int rc = skx_batch_begin(fx, bytes, &bt);
  if (rc) return rc;
  memcpy(bt.h, rec, bytes);
  const skx_update_t *src = (const skx_update_t *)skx_batch_send(&bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  if (fx->n_filter < (1 << 30)) fx->n_filter += n_filter;   /* as a partial upload grows it: the next block must run the biquad */
  /* a voice named twice is applied in order: one launch per run of distinct voices, found with a per-voice epoch mark */
  hipError_t e = hipSuccess;
  int start = 0;
  while (start < n && e == hipSuccess) {
    if (++fx->upd_epoch == 0) { memset(fx->upd_mark, 0, (size_t)fx->n_voices * sizeof(uint32_t)); fx->upd_epoch = 1; }
    int end = start;
    for (; end < n; end++) {
      uint32_t *m = &fx->upd_mark[rec[end].voice];
      if (*m == fx->upd_epoch) break;                   /* named before in this run: the next launch takes it */
      *m = fx->upd_epoch;
    }
    e = (hipError_t)skx_launch_update(src + start, end - start, fx->d_ro, fx->d_rw, fx->count, s);
    start = end;
  }
  return skx_batch_end(&bt, e, "fx update", s);
}

int skred_fxbank_update(skred_fxbank_t *fx, const skred_fxpt_bank_t *h, const int32_t *voices, int n, uint32_t dirty, void *stream) {
  if (!fx || !h || n < 0 || (n > 0 && !voices)) return fail(SKRED_E_BAD_ARG, "fx update: bad arguments");
  if (n == 0) return SKRED_OK;
  if (!dirty || (dirty & ~(uint32_t)SKRED_DIRTY_VALID_MASK)) return fail(SKRED_E_BAD_ARG, "fx update: dirty mask 0x%x", dirty);
  if (dirty & SKRED_DIRTY_HOLD) return fail(SKRED_E_BAD_ARG, "fx update: SKRED_DIRTY_HOLD -- the fixed-point definition has no sample-and-hold");
  for (int i = 0; i < n; i++)
    if (voices[i] < 0 || voices[i] >= fx->n_voices || voices[i] >= h->n_voices)
      return fail(SKRED_E_RANGE, "fx update: voice %d outside the bank", voices[i]);
  hipStream_t s = (hipStream_t)stream;
  if (!(dirty & ~(uint32_t)SKX_STAMPS)) {               /* stamps carry no values: nothing to pack */
    HIP_TRY(hipSetDevice(fx->device));
    return skx_stamp_ids(fx, voices, n, (int)(dirty >> 8), "fx update", s);
  }
  /* pack and check every record before anything touches the device */
  skx_update_t *rec = (skx_update_t *)calloc((size_t)n, sizeof(skx_update_t));
  if (!rec) return fail(SKRED_E_NO_MEM, "fx update staging");
  int n_filter = 0;
  for (int i = 0; i < n; i++) {
    const int v = voices[i];
    const int rc = skx_pack_voice(fx, h, v, dirty, rec[i].ro, rec[i].rw);
    if (rc) { free(rec); return rc; }
    rec[i].voice = v;
    rec[i].dirty = dirty;
    if ((dirty & SKRED_DIRTY_PARAMS) && FX_OPT(h->filter_mode, v)) n_filter++;
  }
  if (!fx->upd_mark) {
    fx->upd_mark = (uint32_t *)calloc((size_t)fx->n_voices, sizeof(uint32_t));
    if (!fx->upd_mark) { free(rec); return fail(SKRED_E_NO_MEM, "fx update marks"); }
  }
  const int rc = update_launch(fx, rec, n, n_filter, s);
  free(rec);
  return rc;
}

/* ------------------------------------------------------------------ the free-voice list */

int skred_fx_idle_check(const skred_fx_idle_query_t *q, int n_voices) {
  if (!q) return fail(SKRED_E_BAD_ARG, "fx find_idle: no query");
  if (q->max_out < 0) return fail(SKRED_E_BAD_ARG, "fx find_idle: max_out %d", q->max_out);
  if (q->which & SKRED_IDLE_UNNAMED) return fail(SKRED_E_BAD_ARG, "fx find_idle: SKRED_IDLE_UNNAMED -- the fixed-point definition has no modulators");
  if (q->which & ~(uint32_t)SKX_IDLE_CRITERIA) return fail(SKRED_E_BAD_ARG, "fx find_idle: unknown bits in which = 0x%x", q->which);
  if (!(q->which & SKX_IDLE_CRITERIA)) return fail(SKRED_E_BAD_ARG, "fx find_idle: which = 0x%x selects no criterion", q->which);
  if (q->settle_q15 < 0) return fail(SKRED_E_BAD_ARG, "fx find_idle: settle_q15 %d", q->settle_q15);
  const int rc = sk_check_slot_range(n_voices, q->first, q->count, 1, 0, "fx find_idle");
  if (rc) return rc;
  if (q->from < q->first || q->from - q->first >= q->count)
    return fail(SKRED_E_RANGE, "fx find_idle: from = %d outside the range [%d,+%d)", q->from, q->first, q->count);
  return SKRED_OK;
}

static int idle_check_bank(const skred_fxbank_t *fx, const skred_fx_idle_query_t *q, const void *voices, const void *count, const char *who) {
  if (!fx || !q) return fail(SKRED_E_BAD_ARG, "%s: no bank or no query", who);
  if (!count) return fail(SKRED_E_BAD_ARG, "%s: nowhere to put the counts", who);
  const int rc = skred_fx_idle_check(q, fx->n_voices);
  if (rc) return rc;
  if (q->max_out > 0 && !voices) return fail(SKRED_E_BAD_ARG, "%s: max_out %d and no list to fill", who, q->max_out);
  return SKRED_OK;
}

int skx_idle_scratch(skred_fxbank_t *fx, hipStream_t s) {
  if (fx->d_idle) return SKRED_OK;
  /* sized once, for the whole bank from any `first` (a range's spans start at `first` rounded down to 64) */
  const int wgs = skx_idle_workgroups(63, fx->n_padded);
  HIP_TRY(hipMalloc((void **)&fx->d_idle, ((size_t)SKX_IDLE_W_COUNT + 2 * (size_t)wgs) * sizeof(uint32_t)));
  fx->idle_wgs = wgs;
  HIP_TRY(hipMemsetAsync(fx->d_idle, 0, (size_t)SKX_IDLE_W_COUNT * sizeof(uint32_t), s));   /* the ticket: zero once, re-armed by every last arriver */
  return SKRED_OK;
}

int skx_idle_launch(skred_fxbank_t *fx, const skred_fx_idle_query_t *q, int32_t *d_voices, uint32_t *d_count, hipStream_t s) {
  HIP_TRY(hipSetDevice(fx->device));
  const int rc = skx_idle_scratch(fx, s);
  if (rc) return rc;
  if (skx_idle_workgroups(q->first, q->count) > fx->idle_wgs) return fail(SKRED_E_RANGE, "fx find_idle: scratch too small");   /* (unreachable: sized above) */
  skx_idle_args_t a;
  memset(&a, 0, sizeof(a));
  a.osc = fx->d_ro[SKX_OSC];
  a.rw0 = fx->d_rw[0];
  a.words = fx->d_idle;
  a.counts = fx->d_idle + SKX_IDLE_W_COUNT;
  a.offsets = a.counts + fx->idle_wgs;
  a.d_voices = d_voices;
  a.d_count = d_count;
  a.first = q->first;
  a.end = q->first + q->count;
  a.from = q->from;
  a.max_out = q->max_out;
  a.which = q->which;
  a.settle_q15 = q->settle_q15;
  const hipError_t e = (hipError_t)skx_launch_idle(&a, s);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx find_idle launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}

int skred_fxbank_find_idle(skred_fxbank_t *fx, const skred_fx_idle_query_t *q, int32_t *d_voices, uint32_t *d_count, void *stream) {
  const int rc = idle_check_bank(fx, q, d_voices, d_count, "fx find_idle");
  if (rc) return rc;
  return skx_idle_launch(fx, q, d_voices, d_count, (hipStream_t)stream);
}

int skx_idle_out_room(skred_fxbank_t *fx, size_t need) {
  return sk_answer_room((void **)&fx->d_idle_out, (void **)&fx->h_idle_out, &fx->idle_out_cap, 2, need);
}

int skred_fxbank_find_idle_host(skred_fxbank_t *fx, const skred_fx_idle_query_t *q, int32_t *voices, int *total_out, void *stream) {
  int dummy = 0;
  int rc = idle_check_bank(fx, q, voices, &dummy, "fx find_idle_host");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_idle_out_room(fx, (size_t)q->max_out))) return rc;
  rc = skx_idle_launch(fx, q, fx->d_idle_out + 2, (uint32_t *)fx->d_idle_out, s);
  if (rc) return rc;
  const int written = sk_read_back(fx->d_idle_out, fx->h_idle_out, 2, q->max_out, q->max_out, voices, s, "fx find_idle_host");
  if (written >= 0 && total_out) *total_out = fx->h_idle_out[1];
  return written;
}

/* ------------------------------------------------------------------ note-ons */

int skred_fx_notes_check(const skred_fx_note_t *notes, int n) {
  if (!notes || n < 0) return fail(SKRED_E_BAD_ARG, "fx notes: no notes or n = %d", n);
  for (int k = 0; k < n; k++) {
    const skred_fx_note_t *t = &notes[k];
    if (t->flags & ~(uint32_t)(SKRED_NOTE_SET_PHASE | SKRED_NOTE_SET_PAN)) return fail(SKRED_E_BAD_ARG, "fx note %d: unknown bits in flags = 0x%x", k, t->flags);
    if (t->reserved[0] || t->reserved[1]) return fail(SKRED_E_BAD_ARG, "fx note %d: reserved words must be 0", k);
    if (t->velocity_q15 < 0 || t->velocity_q15 > 65535) return fail(SKRED_E_BAD_ARG, "fx note %d: velocity_q15 %d outside 0..65535", k, t->velocity_q15);
    if ((t->flags & SKRED_NOTE_SET_PAN) && (t->pan_left_q15 < 0 || t->pan_left_q15 > 65535 || t->pan_right_q15 < 0 || t->pan_right_q15 > 65535))
      return fail(SKRED_E_BAD_ARG, "fx note %d: pan (%d, %d) outside 0..65535", k, t->pan_left_q15, t->pan_right_q15);
  }
  return SKRED_OK;
}

/* the checked notes -> a staging slot -> the placement kernel */
int skx_notes_launch(skred_fxbank_t *fx, const skred_fx_note_t *notes, int n, const int32_t *d_voices, const uint32_t *d_count,
                     int first_entry, int32_t *d_assigned, uint32_t *d_result, const char *who, hipStream_t s) {
  const size_t bytes = (size_t)n * sizeof(skred_fx_note_t);
  skx_batch_t bt;
  const int rc = skx_batch_begin(fx, bytes, &bt);
  if (rc) return rc;
  memcpy(bt.h, notes, bytes);
  const skx_note_t *src = (const skx_note_t *)skx_batch_send(&bt, bytes, s);
  if (!src) return SKRED_E_NO_DEVICE;
  const hipError_t e = (hipError_t)skx_launch_notes(src, n, d_voices, d_count, first_entry, fx->n_voices, fx->d_ro, fx->d_rw, fx->count,
                                                    d_assigned, d_result, s);
  return skx_batch_end(&bt, e, who, s);
}

int skred_fxbank_notes_on_list(skred_fxbank_t *fx, const skred_fx_note_t *notes, int n, const int32_t *d_voices, const uint32_t *d_count,
                               int first_entry, int32_t *d_assigned, uint32_t *d_result, void *stream) {
  if (!fx || !notes || !d_voices || !d_count || !d_result) return fail(SKRED_E_BAD_ARG, "fx notes_on_list: no bank, notes, list, count or result");
  if (n < 0 || first_entry < 0) return fail(SKRED_E_BAD_ARG, "fx notes_on_list: n = %d, first_entry = %d", n, first_entry);
  if (n == 0) return SKRED_OK;
  const int rc = skred_fx_notes_check(notes, n);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(fx->device));
  return skx_notes_launch(fx, notes, n, d_voices, d_count, first_entry, d_assigned, d_result, "fx notes_on_list", (hipStream_t)stream);
}

/* room for n entries in the bank's own list */
int skx_note_list_room(skred_fxbank_t *fx, int n) {
  return sk_answer_room((void **)&fx->d_note_list, NULL, &fx->note_list_cap, SKX_NOTE_LIST_WORDS, (size_t)n);
}

int skred_fxbank_note_on_idle(skred_fxbank_t *fx, const skred_fx_idle_query_t *q, const skred_fx_note_t *notes, int n, int32_t *d_assigned,
                              uint32_t *d_result, void *stream) {
  if (!fx || !q || !notes || !d_result) return fail(SKRED_E_BAD_ARG, "fx note_on_idle: no bank, query, notes or result");
  if (n < 0) return fail(SKRED_E_BAD_ARG, "fx note_on_idle: n = %d", n);
  if (q->which & SKRED_IDLE_AMP_ZERO)
    return fail(SKRED_E_BAD_ARG, "fx note_on_idle: SKRED_IDLE_AMP_ZERO -- a note-on leaves amp_q15 alone: the voice would stay silent and be listed again");
  skred_fx_idle_query_t qq = *q;
  qq.max_out = n;
  int rc = skred_fx_idle_check(&qq, fx->n_voices);
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  if ((rc = skred_fx_notes_check(notes, n))) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(fx->device));
  if ((rc = skx_note_list_room(fx, n))) return rc;
  uint32_t *d_count = fx->d_note_list;
  int32_t *d_list = (int32_t *)(fx->d_note_list + SKX_NOTE_LIST_WORDS);
  if ((rc = skx_idle_launch(fx, &qq, d_list, d_count, s))) return rc;
  return skx_notes_launch(fx, notes, n, d_list, d_count, 0, d_assigned, d_result, "fx note_on_idle", s);
}

int skred_fxbank_stamp_list(skred_fxbank_t *fx, const int32_t *d_voices, int n, const uint32_t *d_count_or_null, uint32_t stamps,
                            void *stream) {
  if (!fx || !d_voices || n < 0) return fail(SKRED_E_BAD_ARG, "fx stamp_list: no bank, no list or n = %d", n);
  const int rc = sk_check_stamps(stamps, "fx stamp_list");
  if (rc) return rc;
  if (n == 0) return SKRED_OK;
  HIP_TRY(hipSetDevice(fx->device));
  const hipError_t e = (hipError_t)skx_launch_stamp_list(d_voices, n, d_count_or_null, fx->n_voices, stamps, fx->d_ro[SKX_TIME], fx->d_rw[0],
                                                         fx->count, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SKRED_E_NO_DEVICE, "fx stamp_list launch -> %s", hipGetErrorString(e));
  return SKRED_OK;
}
