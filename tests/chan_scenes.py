"""The scenes of the channel-polyphony tests (tests/test_chan_cpu.py runs them on the oracle alone and asserts that none is vacuous,
tests/test_chan.py runs them on the device).  Owner words are tag = channel << 24 | note id.

  owners()      an owner array for a bank cut into slots of K voices: channels A and B interleaved, every seventh slot untagged,
                every eleventh tagged by a third channel nobody asks for.
  burst_bank()  tests/test_slot_steal.py's playing_patch (two channels sharing a full bank: every fourth copy comes to rest inside
                the first blocks, the others sound), the sounding copies tagged A and B in turn, the copies at rest carrying the
                stale tags of the notes that ended there.
  BURSTS        the script of bursts, each stated against the channel's CURRENT sounding count S (known to the model only): the
                six kinds -- under the cap, at the cap, above a lowered cap, dropped, no idle slot, mono.
"""
import numpy as np

import chan_model as CM
import slot_steal_model as M
from steal_model import OLDEST, QUIETEST, RELEASED_FIRST, FIN, ENV

A, B, C3, MONO = 1, 2, 3, 4
WHICH = FIN | ENV
SETTLE = 1e-3
F = 64
KINDS = {"under", "at", "above", "dropped", "no idle", "mono"}


def tag_of(channel, note):
    return (channel << 24) | (note & 0xFFFFFF)


def owners(n, K, seed=0):
    """One word per voice; only the words at first voices mean anything, the others hold junk that matches channel A."""
    rng = np.random.default_rng(4100 + n + 7 * K + seed)
    own = np.full(n, tag_of(A, 0xABCDEF), np.uint32)                  # a kernel that read a member's word would see channel A everywhere
    heads = np.arange(0, n - n % K, K)
    s = heads // K
    ch = np.where(s % 2 == 0, A, B)
    own[heads] = (ch.astype(np.uint32) << np.uint32(24)) | (1 + s.astype(np.uint32))
    own[heads[s % 7 == 3]] = 0
    own[heads[s % 11 == 5]] = tag_of(C3, 9)
    own[heads[rng.integers(0, len(heads), max(1, len(heads) // 16))]] = np.uint32(0xFFFFFFFF)   # all 32 bits: one note, channel 255
    return own


def matches(own, K):
    """The matches every scene runs: channel A, channel B, everybody (mask 0), one note by all 32 bits, one note that is not there,
    a channel nobody is on."""
    heads = np.arange(0, len(own) - len(own) % K, K)
    tagged = own[heads][(own[heads] != 0) & (own[heads] >> 24 == A)]
    one = int(tagged[len(tagged) // 2]) if len(tagged) else tag_of(A, 1)
    return [CM.channel(A), CM.channel(B), (0, 0), (one, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (tag_of(A, 0xFFFFFE), 0xFFFFFFFF),
            CM.channel(77)]


def burst_bank(patch, members):
    """(bank, tables, g, K, owner array before any block).  n = 512."""
    import test_slot_steal as G
    n = 512
    bank, tables, g, K = G.playing_patch(patch, n, members)
    own = np.zeros(n, np.uint32)
    copy = np.arange(n // K)
    heads = copy * K
    sounding = copy % 4 != 0
    turn = np.cumsum(sounding) % 2                                     # the sounding copies in turn: A, B, A, B, ...
    own[heads] = np.where(sounding, np.where(turn == 1, A, B), np.where(copy % 8 == 0, A, B)).astype(np.uint32) << np.uint32(24)
    own[heads] |= (100 + copy).astype(np.uint32)
    return bank, tables, g, K, own


# (name, channel, n or (what, delta), cap rule, idle range, steal range, policy, flags): ranges in copies; cap rule: ("S", d) = the
# channel's sounding count over the steal range + d, or a number; n rule: a number, or ("V", d) = the victims of the steal range + d
WHOLE = None
BURSTS = (
    ("under", A, 2, ("S", 3), WHOLE, WHOLE, OLDEST, RELEASED_FIRST),
    ("at", A, 3, ("S", 0), WHOLE, WHOLE, QUIETEST, 0),
    ("above", A, 2, ("S", -2), WHOLE, WHOLE, OLDEST, 0),
    ("other channel under", B, 1, CM.NO_CAP, WHOLE, WHOLE, OLDEST, 0),
    ("dropped", B, ("V", 2), ("S", 0), WHOLE, (0, 8), OLDEST, RELEASED_FIRST),
    ("no idle", A, 2, CM.NO_CAP, (1, 1), WHOLE, OLDEST, RELEASED_FIRST),
    ("mono first", MONO, 1, 1, WHOLE, WHOLE, OLDEST, 0),
    ("mono", MONO, 1, 1, WHOLE, WHOLE, OLDEST, 0),
    ("mono again", MONO, 1, 1, WHOLE, WHOLE, OLDEST, 0),
)


def burst_args(step, host, now, own, K, mmask, n_voices):
    """The arguments of burst `step` of BURSTS on the current state: (iq, sq, match, cap, n, tags)."""
    from skred_amd.bank import slot_query
    name, ch, n_rule, cap_rule, irange, srange, policy, flags = BURSTS[step]
    whole = (0, n_voices // K)
    i0, ic = irange or whole
    s0, sc = srange or whole
    iq = slot_query(i0 * K, ic * K, K, mmask, WHICH, SETTLE, i0 * K, 0)
    sq = M.SlotQuery(s0 * K, sc * K, K, mmask, policy, flags, max_out=5)
    match = CM.channel(ch)
    order, sounding = CM.victim_slots(host, now, sq.but(exclude_idle=WHICH, settle_level=SETTLE), own, match)
    cap = cap_rule if isinstance(cap_rule, int) else sounding + cap_rule[1]
    n = n_rule if isinstance(n_rule, int) else len(order) + n_rule[1]
    tags = np.array([tag_of(ch, 1000 * (step + 1) + k) for k in range(n)], np.uint32)
    return iq, sq, match, cap, n, tags
