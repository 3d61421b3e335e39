/*
 * skred_bank_checks.c -- the argument checks the control calls of both banks share: the shape of a slot, the stamp bits, the length
 * of a list, a range of whole slots, a plain window.  Pure host: no HIP call, and nothing of a bank but its voice count, so the
 * stand-alone test programs (tests/c_*_host.c) link it as it is.  `who` names the calling entry point in the error text; every
 * message carries the offending values.  A caller keeps the ORDER of its checks: a call that is wrong in two ways gets the code of
 * the first.
 */
#include "skred_bank_priv.h"

/* K, and -- `what` != NULL: its name in the text -- a mask over the K voices */
int sk_check_slot_shape(int slot_voices, uint64_t mask, const char *what, const char *who) {
  if (slot_voices < 1 || slot_voices > 64 || (slot_voices & (slot_voices - 1)))
    return fail(SKRED_E_RANGE, "%s: slot_voices = %d (a power of two, 1 .. 64)", who, slot_voices);
  if (!what) return SKRED_OK;
  if (!mask) return fail(SKRED_E_BAD_ARG, "%s: %s is 0", who, what);
  if (slot_voices < 64 && (mask >> slot_voices))
    return fail(SKRED_E_BAD_ARG, "%s: %s = 0x%llx has bits at or above slot_voices = %d", who, what, (unsigned long long)mask, slot_voices);
  return SKRED_OK;
}

int sk_check_stamps(uint32_t stamps, const char *who) {
  if (!stamps || (stamps & ~(uint32_t)(SKRED_STAMP_TRIGGER | SKRED_STAMP_RELEASE)))
    return fail(SKRED_E_BAD_ARG, "%s: stamps = 0x%x (SKRED_STAMP_TRIGGER and / or SKRED_STAMP_RELEASE)", who, stamps);
  return SKRED_OK;
}

/* the entries of a list: n * K stays an int for every K */
int sk_check_list_n(int n, const char *who) {
  if (n < 0 || n > INT32_MAX / 64) return fail(SKRED_E_BAD_ARG, "%s: n = %d", who, n);
  return SKRED_OK;
}

static int window_check(int n_voices, int first, int count, int least, const char *who) {
  if (count < least || first < 0 || first > n_voices || count > n_voices - first)
    return fail(SKRED_E_RANGE, "%s: range [%d,+%d) outside the bank of %d voices", who, first, count, n_voices);
  return SKRED_OK;
}

/* [first, +count) inside n_voices, empty or not, anywhere up to the end (the clears and the downloads) */
int sk_check_window(int n_voices, int first, int count, const char *who) { return window_check(n_voices, first, count, 0, who); }

/* a range of whole slots of K voices inside the bank (K checked by the caller; 1: any range of voices); an empty one only where
 * the caller allows it -- the queries, finds and matches do not */
int sk_check_slot_range(int n_voices, int first, int count, int K, int allow_empty, const char *who) {
  const int rc = window_check(n_voices, first, count, !allow_empty, who);
  if (rc) return rc;
  if ((first & (K - 1)) || (count & (K - 1)))
    return fail(SKRED_E_RANGE, "%s: range [%d,+%d) is not made of whole slots of %d voices", who, first, count, K);
  return SKRED_OK;
}
