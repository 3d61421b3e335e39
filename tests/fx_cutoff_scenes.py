"""The randomised performance the cutoff tests of the fixed-point bank share: written against the stage interface of
tests/fx_cutoff_model.py (FxCutoffStage), so the same calls run on the model alone (tests/test_fx_cutoff_cpu.py asserts there that the
scene is not vacuous) and on a device stage that compares every call with the model (tests/test_fx_cutoff.py).

Banks of 65 voices and more carry the whole scene: at most a quarter of the records are withheld or clamped, some voice lands, some
voice still moves, one goes up and one goes down.  A bank of one voice cannot hold four such voices at once; there the scene is the
calls alone."""
import numpy as np

import fx_cutoff_model as M

R = M.Rec
BOTH = M.BOTH
CH = 3
CHAN = (CH << 24, 0xFF000000)
HARMONICS = (1, 1, 2, 2, 4, 4, 8, 40)                            # 40 x a key above 570 Hz leaves the box: some records clamp


def silent_voice(bank):
    """a voice without pitch (k == 0: its tracked records are withheld), on banks that can spare one"""
    if bank.n >= 65:
        bank["phase_inc"][5] = 0
    return bank


def random_performance(st, gen, blocks=True):
    n = st.n
    tally = dict(records=0, withheld=0, clamped=0, landed=0, still=0, up=0, down=0)

    def count(res, sent):
        tally["records"] += sent
        tally["withheld"] += res[1]
        tally["clamped"] += res[3]

    v = np.arange(n, dtype=np.int32)
    tags = (((v % 2 + CH).astype(np.uint32)) << np.uint32(24)) | (1 + v).astype(np.uint32)      # channels 3 and 4 interleaved
    st.tag(v, tags)
    mine = int((v % 2 == 0).sum())
    # a record without Q and MODE on voices that have no cutoff yet: all withheld (the one part of the scene that is)
    few = max(1, mine // 12)
    res = st.cut_match(CHAN, R(M.ABS, 1 << 25), (0, min(n, 2 * few)))
    assert res[0] == 0 and res[1] == (min(n, 2 * few) + 1) // 2
    count(res, res[1])
    # the channel sweep: every voice of channel 3 gets a tracked low-pass
    res = st.cut_match(CHAN, R(M.TRACK | BOTH, M.track_q24(2), 3 << 15, 1))
    assert res[0] + res[1] == mine and res[2] == n - mine
    count(res, mine)
    # one record per note on every voice, in no order, with holes, entries outside the bank and one stolen voice
    perm = gen.permutation(n)
    recs = [R(M.TRACK | BOTH, M.track_q24(int(gen.choice(HARMONICS))), int(np.exp2(gen.uniform(10, 26))), 1 + int(gen.integers(0, 5)))
            if gen.integers(0, 3) else R(M.ABS | BOTH, int(np.exp2(gen.uniform(19, 30.5))), int(np.exp2(gen.uniform(12, 20))), 1 + int(gen.integers(0, 5)))
            for _ in range(n)]
    lst = v[perm].tolist() + [-1, n, n + 7]
    ltags = tags[perm].tolist() + [5, 6, 7]
    if n > 1:
        ltags[0] ^= 1
    lrecs = recs + [R(M.ABS | BOTH, 1 << 24, 1 << 16, 1)] * 3
    res = st.cut_list(lrecs, lst, ltags, count=max(1, n // 2))
    count(res, res[0] + res[1])
    res = st.cut_list(lrecs, lst, ltags)
    assert res[2] == (1 if n > 1 else 0) and res[0] + res[1] == n - res[2]
    count(res, n - res[2])
    st.cut_list(lrecs, lst, ltags, count=5000)
    if blocks:
        st.block()
    # sweeps: v % 4 == 0 up and fast (they land), 1 down and slow, 2 up and slow (they go on moving), 3 rest
    fast, slow = M.rate_q32(700.0), M.rate_q32(3.0)
    has = st.cut[:, M.W] != 0
    movers = [int(x) for x in v if x % 4 != 3 and has[x]]
    grecs = []
    for x in movers:
        w = int(st.cut[x, M.W])
        if x % 4 == 0:
            grecs.append(R(M.ABS | M.GLIDE, min(M.W_MAX, w + (w >> 1) + 1), up_q32=fast[0], down_q32=fast[1]))
        elif x % 4 == 1:
            grecs.append(R(M.ABS | M.GLIDE, max(M.W_MIN, w >> 3), up_q32=slow[0], down_q32=slow[1]))
        else:
            grecs.append(R(M.ABS | M.GLIDE | M.SET_Q, M.W_MAX, 1 << 17, up_q32=slow[0], down_q32=slow[1]))
    for at in range(0, len(movers), 1024):
        part = slice(at, at + 1024)
        res = st.cut_tags(grecs[part], tags[movers[part]])
        assert res == [len(movers[part]), 0, 0, 0]
        count(res, res[0])
    moving = st.cut[:, M.TARGET] != 0
    tally["up"] = int((moving & (st.cut[:, M.W] < st.cut[:, M.TARGET])).sum())
    tally["down"] = int((moving & (st.cut[:, M.W] > st.cut[:, M.TARGET])).sum())
    for frames in (64, 100, 28, 1, 63, 640):
        res = st.cut_advance(frames)
        tally["landed"] += res[1]
        tally["still"] = res[0]
        if blocks:
            st.block()
    # a tracked record on a moving voice without GLIDE stops it where the record says; a stop with snap lands, one without stays
    if n > 1:
        res = st.cut_tags([R(M.TRACK, M.track_q24(1))], tags[1:2])
        count(res, 1)
    third = max(1, n // 3)
    st.cut_stop(True, (0, third))
    st.cut_stop(False, (third, n - third))
    assert not st.cut[:, M.TARGET].any() and not st.cut[:, M.CARRY].any()
    assert st.cut_advance(64) == [0, 0]
    if blocks:
        st.block()
    return tally
