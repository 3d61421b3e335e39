"""The list rule of the float bank's control kernels, pinned for every entry point that takes a slot list.

The rule -- entry i is looked at when i < min(n, *d_count) (no d_count: n); it names a slot when it is >= 0, a multiple of K and
slot + K <= n_voices; thread l of the entry's K threads serves voice entry + l -- is one function on the device
(skred_amd/csrc/skred_update_common.hpp: sk_list_looked, sk_entry_decode).  Here every entry point that goes through it gets the same
awkward list and is held to the model its own feature test uses: tag_slots (with the pedal-clear and glide-clear launches behind it,
on a bank that has both arrays), stamp_slots, stamp_owned, stamp_owned_pedal, ctl_slots, ctl_owned, ctl_owned_each,
ctl_owned_each_filter, glide_owned.

512 voices; K in {1, 4, 64}; the list has (256 >> log2 K) + 1 entries, so the LAST entry is the only one of a second workgroup (and at
K = 64 a slot fills a wavefront).  The entries: distinct slots, the last slot of the bank, -1, the first index past the bank, for
K > 1 a slot index plus 1 (whose slot is named by no entry), no slot twice.  d_count: absent, n - 1 (cuts off exactly the second
workgroup's entry, which is a slot whose owner word is the expected one), 0, n + 7 (n rules).  After every call: the result words, and
every controller word, state word, envelope clock, owner, pedal and glide word of the whole bank against the models; at the end the
words of every voice that no looked-at valid entry names must be what they were before the first call, bit for bit.
"""
import numpy as np
import pytest

import ctl_model as CM
import expr_model as EM
import glide_model as GM
import owner_model as OM
import pedal_model as PM
import slot_model as SM
import timbre_model as TM
from skred_amd import device
from skred_amd.device import ctl, ctl_each
from test_glide import GlideRig, glides_for
from test_slot_steal import plain_bank
from test_timbre import bank_words, cutoff, whole_bank_same

N = 512
SPAN = 256                                                           # threads per workgroup of the control kernels
REL, TRIG = SM.STAMP_RELEASE, SM.STAMP_TRIGGER


@pytest.fixture(scope="module")
def dev():
    assert device.load().skred_amd_device_count() > 0, "no GPU visible"
    return device


def awkward_list(K):
    """(entries, the slot the misaligned entry sits in or None): the last entry is a slot, alone in the second workgroup."""
    n = SPAN // K + 1
    rng = np.random.default_rng(K)
    inside = None if K == 1 else K                                   # slot K is named by no entry; K + 1 is the misaligned one
    special = [N - K, -1, N] + ([] if K == 1 else [K + 1])
    free = [int(s) for s in rng.permutation(np.arange(0, N - K, K)) if s != inside]
    body = special + free[:n - 1 - len(special)]
    entries = np.array([body[i] for i in rng.permutation(len(body))] + [free[n - 1 - len(special)]], np.int32)
    valid = [int(e) for e in entries if CM.slot_valid(int(e), K, N)]
    assert len(entries) == n and len(valid) == len(set(valid)) == n - len(special) + 1 and CM.slot_valid(int(entries[-1]), K, N)
    return entries, inside


class ListRig(GlideRig):
    """tests/test_glide.py's rig (owners, clocks, glide words, increments) with the model's pedal array beside it."""

    def __init__(self, dev, bank, tables, g):
        super().__init__(dev, bank, tables, g)
        self.pedal = PM.new(bank.n)

    def all_same(self, tag):
        whole_bank_same(self, tag)                                   # controller words, state, owners, clocks, glide words, increments
        got = self.db.download_pedals()
        bad = np.flatnonzero(got != self.pedal)
        assert not len(bad), f"{tag}: pedal words differ at {bad[:8].tolist()}: {got[bad[:8]].tolist()} / {self.pedal[bad[:8]].tolist()}"

    def count_word(self, count):
        import torch
        return None if count is None else torch.tensor([count, 4321], dtype=torch.int32, device="cuda")

    def tag(self, entries, tags, K, count=None, tag=""):
        for e in OM.looked(entries, len(tags), count):               # (pedal_model.tag_slots: the tagged slots' pedal words cleared)
            if CM.slot_valid(e, K, self.n):
                self.pedal[e] = 0
        super().tag(entries, tags, K, count, tag)                    # the glide words cleared, the owners tagged, d_result checked
        self.all_same(tag)

    def call(self, tag, words, launch, want):
        """one list call: launch(d_result) on the device, `want` the model's result words"""
        res = self.result(words)
        launch(res.data_ptr())
        got = self.read(res, words, tag)
        print(f"{tag}: d_result {got}, the model {want}")
        assert got == want, f"{tag}: d_result {got}, the model says {want}"
        self.all_same(tag)
        return want


def snapshot(r):
    start, release = r.db.download_env_clocks()
    return dict(words=bank_words(r.db, r.bank), start=start, release=release, owner=r.db.download_owners(), pedal=r.db.download_pedals(),
                glide=r.db.download_glide())


@pytest.mark.gpu
@pytest.mark.parametrize("count_kind", ["absent", "n-1", "zero", "n+7"])
@pytest.mark.parametrize("K", [1, 4, 64])
def test_every_list_call_obeys_one_rule(dev, K, count_kind):
    bank, tables, g, now = plain_bank(N)
    bank["voice_amp"][5::11] = 0.0                                   # zero-amp voices: the AMP guard withholds
    entries, inside = awkward_list(K)
    n = len(entries)
    count = {"absent": None, "n-1": n - 1, "zero": 0, "n+7": n + 7}[count_kind]
    full = (1 << K) - 1
    part = full if K == 1 else (1 << (K - 1)) | 1                    # voices 0 and K - 1 of a slot
    r = ListRig(dev, bank, tables, g)
    try:
        # every slot of the bank owned, held back by the pedal and gliding: the clears behind the tag launch have words to clear, and
        # an entry that must not be looked at is a slot whose guard would pass
        slots = np.arange(0, N, K, dtype=np.int32)
        first_tags = (np.uint32(0x0B000000) + np.arange(len(slots), dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        dl_all = r.dev_list(slots)
        r.tag(slots, first_tags, K, tag="setup: every slot tagged")
        r.call("setup: every note-off held back", 4,
               lambda res: r.db.stamp_owned_pedal(dl_all.data_ptr(), first_tags, K, full, True, res),
               PM.stamp_owned_pedal(r.owner, r.pedal, r.truth, slots, first_tags, None, K, full, True, r.now())[0])
        r.start_owned(glides_for(len(slots)), K, full, slots, first_tags, tag="setup: every slot gliding")
        r.all_same("setup")
        assert (r.pedal[slots] == PM.PENDING).all() and int((r.glide[:, 0] != 0).sum()) > N // 2
        before = snapshot(r)

        dl, dc = r.dev_list(entries), r.count_word(count)
        dcp = dc.data_ptr() if dc is not None else 0
        looked = [int(e) for e in OM.looked(entries, n, count)]
        named = np.array(sorted(e for e in looked if CM.slot_valid(e, K, N)), np.int64)
        holes = 2 if K == 1 else 3                                    # -1, the index past the bank, the misaligned one
        assert len(named) == {"absent": n - holes, "n-1": n - 1 - holes, "zero": 0, "n+7": n - holes}[count_kind]

        # 1. tag_slots, and the pedal and glide clears behind it
        new_tags = (np.uint32(0x0C000000) + np.arange(n, dtype=np.uint32) + np.uint32(1)).astype(np.uint32)
        r.tag(entries, new_tags, K, count, tag="tag_slots")
        assert not r.pedal[named].any() and not r.glide[(named[:, None] + np.arange(K)).ravel()].any()
        if inside is not None:
            assert r.pedal[inside] == PM.PENDING and r.owner[inside] == first_tags[inside // K], "the misaligned entry reached its slot"
        # the tags the guarded calls expect: what every entry that is a slot carries now (the cut-off entry too: its guard would
        # pass), every fifth one somebody else's
        etags = np.array([r.owner[e] if CM.slot_valid(int(e), K, N) else 0x70000000 + k for k, e in enumerate(entries)], np.uint32)
        etags[2::5] ^= np.uint32(0x00800000)
        assert OM.tags_check(etags) == 0

        # 2. stamp_slots
        r.db.stamp_slots(dl.data_ptr(), n, K, part, TRIG, dcp)
        SM.stamp(r.truth, SM.stamp_voices(entries, n, count, K, part, N), TRIG, r.now())
        r.all_same("stamp_slots")
        # 3. stamp_owned
        r.call("stamp_owned", 3, lambda res: r.db.stamp_owned(dl.data_ptr(), etags, K, part, REL, res, dcp),
               OM.stamp_owned(r.owner, r.truth, entries, etags, count, K, part, REL, r.now())[0])
        # 4. stamp_owned_pedal, stamping and holding back
        for hold in (False, True):
            r.call(f"stamp_owned_pedal hold {hold}", 4, lambda res: r.db.stamp_owned_pedal(dl.data_ptr(), etags, K, part, hold, res, dcp),
                   PM.stamp_owned_pedal(r.owner, r.pedal, r.truth, entries, etags, count, K, part, hold, r.now())[0])
        # 5. ctl_slots
        recs = [ctl(CM.AMP | CM.PAN | CM.SMOOTHING, amp=0.5 + 0.005 * l, pan_left=0.25, pan_right=0.625, smoothing=0.3) for l in range(K)]
        r.call("ctl_slots", 2, lambda res: r.db.ctl_slots(recs, part, dl.data_ptr(), n, dcp, res),
               CM.ctl_slots((r.truth,), recs, part, entries, n, count, N)[0])
        # 6. ctl_owned
        recs = [ctl(CM.AMP | CM.INC_SCALE | CM.ENV_TIMES, amp=0.3 + 0.005 * l, inc_scale=1.0594631, attack_time=30.0, decay_time=60.0 + l,
                    sustain_level=0.5, release_time=400.0) for l in range(K)]
        r.call("ctl_owned", 3, lambda res: r.db.ctl_owned(recs, part, dl.data_ptr(), etags, dcp, res),
               OM.ctl_owned(r.owner, (r.truth,), recs, part, entries, etags, count)[0])
        # 7. ctl_owned_each
        bits = [EM.EACH_INC_SCALE, EM.EACH_AMP_SCALE, EM.EACH_VELOCITY, EM.EACH_PAN, EM.EACH_ALL]
        each = [ctl_each(bits[k % 5], inc_scale=float(np.float32(2.0 ** ((k % 25 - 12) / 12.0))), amp_scale=0.25 + 0.001 * k,
                         velocity=0.3 + 0.0005 * k, pan_left=0.001 * (k % 1000), pan_right=0.9) for k in range(n)]
        recs = [ctl(CM.AMP | CM.SMOOTHING, amp=0.5 + 0.005 * l, smoothing=0.35) for l in range(K)]
        r.call("ctl_owned_each", 3, lambda res: r.db.ctl_owned_each(recs, each, part, dl.data_ptr(), etags, K, dcp, res),
               EM.ctl_owned_each(r.owner, (r.truth,), recs, each, K, part, entries, etags, count)[0])
        # 8. ctl_owned_each_filter
        filt = [cutoff(k, 1 + k % 5) for k in range(n)]
        r.call("ctl_owned_each_filter", 3,
               lambda res: r.db.ctl_owned_each_filter(recs, each, filt, part, part, dl.data_ptr(), etags, K, dcp, res),
               TM.ctl_owned_each_filter(r.owner, (r.truth,), recs, each, filt, K, part, part, entries, etags, count)[0])
        # 9. glide_owned
        r.start_owned(glides_for(n, 3), K, part, entries, etags, count, tag="glide_owned")
        r.all_same("glide_owned")

        # the voices no looked-at valid entry names: every word as it was before the first call
        quiet = np.ones(N, bool)
        for e in named:
            quiet[e:e + K] = False
        assert quiet.sum() == N - len(named) * K and (inside is None or quiet[inside:inside + K].all())
        after = snapshot(r)
        for field, sub in CM.CTL_WORDS:
            x, y = CM.word(before["words"], field, sub), CM.word(after["words"], field, sub)
            assert x[quiet].tobytes() == y[quiet].tobytes(), f"{field}.{sub}: a voice no entry names changed"
        assert before["words"]["voice_amp_envelope"]["is_active"][quiet].tobytes() == \
               after["words"]["voice_amp_envelope"]["is_active"][quiet].tobytes(), "is_active: a voice no entry names changed"
        for what in ("start", "release", "owner", "pedal", "glide"):
            assert before[what][quiet].tobytes() == after[what][quiet].tobytes(), f"{what}: a voice no entry names changed"
        if len(named):
            assert before["owner"][~quiet].tobytes() != after["owner"][~quiet].tobytes()
        assert r.db.list_violations() == 0
    finally:
        r.close()
