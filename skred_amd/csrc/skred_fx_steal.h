/* skred_fx_steal.h -- voice stealing on the fixed-point bank: what skred_fx_steal.c and skred_fx_steal_kernels.hip share
 * (include/skred_amd_fxpt.h: skred_fxbank_find_steal).
 *
 * Only the key pass knows the bank: sk_fx_steal_keys_kernel turns the fixed-point planes into one 64-bit key per voice and counts
 * the first digit.  Everything behind it is the float bank's select (skred_launch.h: sk_launch_steal_select), entered with the same
 * sk_steal_args_t -- its float `idle` member and env_s stay zero: nothing behind the key pass reads them -- over a scratch of the
 * same layout, owned by the fixed-point bank. */
#ifndef SKRED_FX_STEAL_H
#define SKRED_FX_STEAL_H

#include "skred_fx_layout.h"
#include "skred_launch.h"

typedef struct {
  sk_steal_args_t s;               /* scratch, d_voices / d_count, now, min_age, range, max_out, policy, flags */
  skx_idle_args_t idle;            /* the exclusion: osc, rw0, which = exclude_idle, settle_q15 (first / end filled by the launcher) */
  const skx_plane_t *time;         /* SKX_TIME: sample_start, sample_release */
} skx_steal_args_t;

#ifdef __cplusplus
extern "C" {
#endif
/* the key pass, then sk_launch_steal_select: SK_STEAL_DIGITS + 3 launches whatever the data, the key pass alone with max_out == 0.
 * `owner` != NULL (one word per voice of the bank): the MATCHED query of channel polyphony -- a voice takes part when owner[v] != 0
 * and (owner[v] & mask) == value, and d_count is uint32[3]: written, total candidates, sounding voices of the match in the range
 * (the key pass writes all three with max_out == 0).  NULL: value and mask are not looked at, d_count is uint32[2] */
int skx_launch_steal(const skx_steal_args_t *args, const uint32_t *owner, uint32_t value, uint32_t mask, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
