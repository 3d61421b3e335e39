/*
 * skred_chan.h -- C-linkage launch entry points of skred_chan_kernels.hip (internal to libskred_amd.so, beside skred_launch.h; the
 * public ABI is include/skred_amd.h, section "channel polyphony").  Called by skred_bank_chan.c.
 */
#ifndef SKRED_CHAN_H
#define SKRED_CHAN_H

#include "skred_launch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the word of the steal scratch (skred_launch.h: SK_STEAL_W_*; zeroed once with the others) in which the workgroups of the matched
 * key pass add up their sounding slots; its last arriver reads it, stores it to d_count[2] and re-arms it */
#define SK_CHAN_W_SOUNDING 6
#ifdef __cplusplus
static_assert(SK_CHAN_W_SOUNDING > SK_STEAL_W_PREFIX_HI && SK_CHAN_W_SOUNDING < SK_STEAL_W_COUNT, "a word of the steal scratch that the select does not use");
#else
_Static_assert(SK_CHAN_W_SOUNDING > SK_STEAL_W_PREFIX_HI && SK_CHAN_W_SOUNDING < SK_STEAL_W_COUNT, "a word of the steal scratch that the select does not use");
#endif

/* sk_launch_slot_steal with the owner guard and the sounding count: a slot takes part when owner[first voice] != 0 and
 * (owner & mask) == value; d_count (uint32[3]) = written, total candidates, sounding slots of the match in the range.  `owner`:
 * one word per voice of the bank.  max_out == 0: the key pass alone, which writes all three words */
int sk_launch_chan_steal(const sk_steal_args_t *args, uint64_t member_mask, int slot_voices, const uint32_t *owner, uint32_t value,
                         uint32_t mask, hipStream_t stream);
/* One workgroup.  I = min(idle_count[0], n), S = victim_count[2], V = min(victim_count[0], SK_STEAL_MAX):
 * a = min(n, I, cap > S ? cap - S : 0), b = min(n - a, V); list[a + t] = victims[t] for t < b; out_count[0] = a + b;
 * d_result[2] = b, d_result[3] = S.  `list` has room for n entries */
int sk_launch_chan_join(int32_t *list, const uint32_t *idle_count, const int32_t *victims, const uint32_t *victim_count, int n,
                        uint32_t cap, uint32_t *out_count, uint32_t *d_result, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
