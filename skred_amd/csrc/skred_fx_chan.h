/*
 * skred_fx_chan.h -- C-linkage launch entry point of skred_fx_chan_kernels.hip (internal to libskred_amd.so, beside skred_fx_steal.h;
 * the public ABI is include/skred_amd_fxpt.h, section "channel polyphony").  Called by skred_fx_chan.c.  The word of the steal scratch
 * that holds the sounding count (SK_CHAN_W_SOUNDING) and the join of a burst (sk_launch_chan_join) are the float bank's, skred_chan.h.
 */
#ifndef SKRED_FX_CHAN_H
#define SKRED_FX_CHAN_H

#include "skred_chan.h"
#include "skred_fx_steal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* skx_launch_steal with the owner guard and the sounding count: a voice takes part when owner[v] != 0 and (owner[v] & mask) == value;
 * d_count (uint32[3]) = written, total candidates, sounding voices of the match in the range.  `owner`: one word per voice of the
 * bank.  max_out == 0: the key pass alone, which writes all three words */
int skx_launch_chan_steal(const skx_steal_args_t *args, const uint32_t *owner, uint32_t value, uint32_t mask, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
