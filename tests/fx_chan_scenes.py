"""The scenes of the fixed-point channel-polyphony tests (tests/test_fx_chan_cpu.py runs them on the oracle alone and asserts that
none is vacuous, tests/test_fx_chan.py runs them on the device).  Owner words are tag = channel << 24 | note id.  The banks are
tests/fx_steal_scenes.py's (a role per voice, v mod 8), by import.

  owners()       channels A and B in turn by groups of eight voices (so each channel holds every role), every seventh group
                 untagged, every eleventh on a third channel nobody asks for, a few words with all 32 bits set.
  queries()      the (query, match) pairs of the 1 500-voice scene.
  ties_owners()  A and B interleaved voice by voice in the 70 000-voice bank in which all starts, and all releases, are equal.
  burst_bank()   1 024 voices; the sounding ones tagged A and B in turn, the ones at rest carrying the stale tags of notes that ended.
  BURSTS         the script of bursts, each stated against the channel's CURRENT sounding count S (known to the model only): the seven
                 kinds tests/chan_model.kind distinguishes -- under the cap, mixed, at the cap, above a lowered cap, dropped, no idle
                 voice, mono -- and SKRED_CHAN_NO_CAP.
"""
import numpy as np

import fx_chan_model as CM
import fx_steal_scenes as sc
from fx_steal_model import ENV, FIN, OLDEST, QUIETEST, RELEASED_FIRST, RELEASED_ONLY, STEAL_MAX, Query
from skred_amd import fxbank as fxb

A, B, C3, MONO, NOBODY = 1, 2, 3, 4, 77
WHICH, SETTLE = FIN | ENV, 3
F = 64
KINDS = {"under", "mixed", "at", "above", "dropped", "no idle", "mono"}
N_QUERY, N_TIES, N_BURST = 1500, 70000, 1024
MIN_AGE = 20000


def tag_of(channel, note):
    return (channel << 24) | (note & 0xFFFFFF)


def owners(n):
    v = np.arange(n)
    g = v // 8
    own = (np.where(g % 2 == 0, A, B).astype(np.uint32) << np.uint32(24)) | (1 + v).astype(np.uint32)
    own[g % 7 == 3] = 0
    own[g % 11 == 5] = tag_of(C3, 9)
    own[(v % 97) == 13] = np.uint32(0xFFFFFFFF)                         # all 32 bits: one note id, channel 255
    return own


def matches(own, truth):
    """Channel A, channel B, everybody tagged (mask 0), one sounding note by all 32 bits, the all-ones word, a note that is not there, a
    channel with no voice at all."""
    snd = (truth["use_envelope"] != 0) & (truth["is_active"] != 0) & (own >> np.uint32(24) == A)
    one = int(own[np.flatnonzero(snd)[len(np.flatnonzero(snd)) // 2]])
    return [CM.channel(A), CM.channel(B), (0, 0), (one, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (tag_of(A, 0xFFFFFE), 0xFFFFFFFF),
            CM.channel(NOBODY)]


def queries(n=N_QUERY):
    """The queries every match of the scene runs."""
    whole, part = Query(0, n, max_out=16), Query(70, 1300, max_out=16)      # neither end of `part` on a wave or workgroup edge
    return [whole, part, whole.but(max_out=0), whole.but(max_out=1), whole.but(max_out=STEAL_MAX), part.but(max_out=STEAL_MAX),
            whole.but(policy=QUIETEST), part.but(policy=QUIETEST, max_out=STEAL_MAX),
            whole.but(flags=RELEASED_FIRST, max_out=STEAL_MAX), part.but(flags=RELEASED_ONLY),
            whole.but(policy=QUIETEST, flags=RELEASED_FIRST | RELEASED_ONLY),
            whole.but(min_age=MIN_AGE, max_out=STEAL_MAX), part.but(min_age=MIN_AGE, flags=RELEASED_ONLY, max_out=0),
            whole.but(exclude_idle=ENV, settle_q15=0, max_out=STEAL_MAX), part.but(exclude_idle=FIN | ENV, settle_q15=0),
            whole.but(exclude_idle=FIN | ENV | fxb.IDLE_AMP_ZERO, settle_q15=SETTLE, min_age=MIN_AGE, flags=RELEASED_FIRST, max_out=1)]


def query_scene():
    """(bank, pool, c0, the oracle's bank after the scene's blocks, now, owner array)"""
    b, pool, c0, truth, now, role, special = sc.scene(N_QUERY, "plain")
    return b, pool, c0, truth, now, owners(N_QUERY)


def ties_owners(n=N_TIES):
    v = np.arange(n)
    return (np.where(v % 2 == 0, A, B).astype(np.uint32) << np.uint32(24)) | (1 + v).astype(np.uint32)


def ties_queries(n=N_TIES):
    return [Query(0, n, max_out=STEAL_MAX), Query(0, n, max_out=1), Query(0, n, flags=RELEASED_FIRST, max_out=STEAL_MAX),
            Query(11, n - 30, flags=RELEASED_FIRST, max_out=STEAL_MAX), Query(0, n, max_out=0)]


def burst_bank():
    """(bank, pool, c0, owner array before any block)."""
    n = N_BURST
    b, pool, c0, role, _ = sc.steal_bank(n)
    v = np.arange(n)
    sounding = np.isin(role, (0, 1, 5, 6))
    turn = np.cumsum(sounding) % 2                                      # the sounding voices in turn: A, B, A, B, ...
    ch = np.where(sounding, np.where(turn == 1, A, B), np.where(v % 16 < 8, A, B))
    own = (ch.astype(np.uint32) << np.uint32(24)) | (100 + v).astype(np.uint32)
    own[role == 3] = 0                                                  # the voices without an envelope never held a note
    return b, pool, c0, own


# (name, channel, n or ("V", d), cap rule, idle range, steal range, policy, flags, min_age): ranges (first, count) in voices, None the
# whole bank; cap rule: ("S", d) = the channel's sounding count over the steal range + d, or a number; n rule: a number, ("V", d) = the
# candidates of the steal range + d, or ("IV", d) = the idle voices of the idle range + those candidates + d
WHOLE = None
BURSTS = (
    ("under", A, 2, ("S", 3), WHOLE, WHOLE, OLDEST, RELEASED_FIRST, 64),
    ("mixed", A, 3, ("S", 1), WHOLE, WHOLE, OLDEST, 0, 64),
    ("at", A, 3, ("S", 0), WHOLE, WHOLE, QUIETEST, 0, 64),
    ("above", A, 2, ("S", -2), WHOLE, WHOLE, OLDEST, 0, 64),
    ("other channel under, no cap", B, 1, CM.NO_CAP, WHOLE, WHOLE, OLDEST, 0, 64),
    ("dropped", B, ("V", 2), ("S", 0), WHOLE, (0, 64), OLDEST, RELEASED_FIRST, 64),
    ("dropped, no cap", B, ("IV", 2), CM.NO_CAP, (16, 8), (40, 24), QUIETEST, 0, 64),
    ("no idle", A, 2, CM.NO_CAP, (8, 1), WHOLE, OLDEST, RELEASED_FIRST, 64),
    ("mono first", MONO, 1, 1, WHOLE, WHOLE, OLDEST, 0, 0),
    ("mono", MONO, 1, 1, WHOLE, WHOLE, OLDEST, 0, 0),
    ("mono again", MONO, 1, 1, WHOLE, WHOLE, OLDEST, 0, 0),
)


def burst_args(step, truth, now, own):
    """The arguments of burst `step` of BURSTS on the current state: (iq, sq, match, cap, n, tags)."""
    import fx_live_model as live
    name, ch, n_rule, cap_rule, irange, srange, policy, flags, min_age = BURSTS[step]
    i0, ic = irange or (0, truth.n)
    s0, sn = srange or (0, truth.n)
    iq = fxb.FxIdleQueryC(i0, ic, WHICH, SETTLE, i0, 0)
    sq = Query(s0, sn, policy, flags, min_age, max_out=5)
    match = CM.channel(ch)
    order, sounding = CM.victim_order(truth, now, sq.but(exclude_idle=WHICH, settle_q15=SETTLE), own, match)
    cap = cap_rule if isinstance(cap_rule, int) else sounding + cap_rule[1]
    if isinstance(n_rule, int):
        n = n_rule
    else:
        n = len(order) + n_rule[1] + (live.idle_list(truth, i0, ic, WHICH, SETTLE, i0)[1] if n_rule[0] == "IV" else 0)
    tags = np.array([tag_of(ch, 1000 * (step + 1) + k) for k in range(n)], np.uint32)
    return iq, sq, match, cap, n, tags


def burst_notes(n, step):
    return [fxb.FxNoteC(3000017 + 40009 * i + step, 9000 + 23 * i, (0x01234567 * (i + 1 + step)) & 0xFFFFFFFF, 700 + 31 * i, 32000 - 29 * i,
                        (fxb.NOTE_SET_PHASE, fxb.NOTE_SET_PHASE | fxb.NOTE_SET_PAN)[(i + step) & 1]) for i in range(n)]


def run_burst_script(on_burst=None):
    """The bursts of BURSTS on the oracle; on_burst(step, state, args, want, now) runs the device's side: step -1 before the first
    burst, then per burst once with its arguments and the model's (d_assigned, d_result), and once per block ("block", the oracle's
    (mix, stems)) behind it.  Returns (the kinds seen, a log)."""
    from oracle import cpuref
    import fx_live_model as live
    b, pool, c0, own = burst_bank()
    truth, cnt = b.copy(), c0
    for _ in range(2):
        _, _, cnt = cpuref.fx_render(truth, pool, cnt, F, 1)
    state = dict(bank=b, pool=pool, c0=c0, own=own, truth=truth)
    if on_burst:
        on_burst(-1, state, None, None, None)
    seen, log, mono = set(), [], None
    for step in range(len(BURSTS)):
        now = cnt
        iq, sq, match, cap, n, tags = burst_args(step, truth, now, own)
        want, res, n_idle = CM.burst(truth, now, own, iq, sq, match, cap, n)
        kind = CM.kind(n, n_idle, res, cap)
        seen.add(kind)
        log.append((BURSTS[step][0], n, cap, n_idle, res, kind))
        before = own.copy()
        everybody = Query(0, truth.n, exclude_idle=WHICH, settle_q15=SETTLE)
        v, snd_all, _, _ = CM.terms(truth, now, everybody, before, (0, 0))
        other = v[snd_all & ~CM.matches(before[v], match)]                 # the sounding voices of the other channels
        clocks = (truth["sample_start"][other].copy(), truth["sample_release"][other].copy())
        notes = burst_notes(n, step)
        if on_burst:
            on_burst(step, state, (iq, sq, match, cap, n, tags, notes), (want, res), now)
        placed, counts = live.place_notes(truth, notes, want, res[0], 0, now)
        assert np.array_equal(placed, want) and list(counts) == res[:2]
        CM.tag(own, want, tags)
        # victims come from the channel only (the others keep their tags and clocks), and a burst never names a voice twice
        stolen = want[res[0] - res[2]:res[0]]
        assert CM.matches(before[stolen], match).all() and (own[other] == before[other]).all()
        assert (truth["sample_start"][other] == clocks[0]).all() and (truth["sample_release"][other] == clocks[1]).all()
        assert len(set(want[:res[0]].tolist())) == res[0]
        after = CM.victim_order(truth, now, Query(0, truth.n, exclude_idle=WHICH, settle_q15=SETTLE), own, match)[1]
        if BURSTS[step][5] is None:                                        # (the steal range is the whole bank: S is the channel's count)
            assert after <= max(cap, res[3]), (step, after, cap, res)      # at or below the cap: never above it; above it: no growth
        if BURSTS[step][1] == MONO:                                        # mono mode: the new note takes the old one's voice
            assert res[:3] == ([1, 0, 0] if mono is None else [1, 0, 1]) and (mono is None or want[0] == mono) and after == 1, (step, res, want, mono)
            mono = int(want[0])
        for _ in range(2):
            ref = cpuref.fx_render(truth, pool, cnt, F, 1, want_stems=on_burst is not None)
            cnt = ref[2]
            if on_burst:
                on_burst(step, state, "block", ref, None)
    return seen, log
