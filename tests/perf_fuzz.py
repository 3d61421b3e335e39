"""Whole performances for the float bank's control plane: performance(seed, cfg) is a script -- a list of blocks, each a length and the
calls queued in front of it -- that imitates a host playing four MIDI channels.  A pure function of the seed: nothing here looks at a
device or at the model's state.  The host knows only what a real host knows: per channel the pedals, the keys it holds down, the cap,
the glide rate, the tags it used and the place of its earlier bursts' d_assigned lists; which slot holds which note it never learns.

tests/perf_model.py runs a script on the composed model, tests/test_perf_fuzz.py on a device beside it.  A call is (the name of a
Stage method, its keyword arguments); `ref` arguments name an earlier call of the script by its serial number: that call's d_assigned
is the list.
"""
from dataclasses import dataclass

import numpy as np

import chan_model as CHM
import ctl_model as CTL
import expr_model as EM
import glide_model as GM
import owner_model as OM
import owner_scenes as OS
import pedal_model as PM
import slot_model as SM
import slot_steal_model as SSM
from skred_amd import device
from skred_amd.bank import slot_query
from steal_model import OLDEST

SEEDS = tuple(range(8))
BLOCKS = 24
FRAMES = (64, 128, 37, 27, 192, 512)
CHANNELS = (3, 5, 7, 9)
WHICH, SETTLE = OS.WHICH, OS.SETTLE
SEMI = 2.0 ** (1.0 / 12.0)
MIN_IN_PLACE = 4                                    # blocks of a plain2 performance the planner's rule pins to the in-place path
TOP_KEY = 96                                        # its increment times 3.4e38 is not finite: the withheld bend is aimed at it
KINDS = ("note_on_channel", "note_on_steal_slots", "note_on_idle_slots", "tag_slots", "release_tags", "release_tags_pedal",
         "stamp_owned_pedal", "pedal_latch", "pedal_up", "pedal_clear", "stamp_match", "ctl_range", "ctl_match", "ctl_owned_each",
         "ctl_tags_each", "ctl_owned_each_filter", "ctl_tags_each_filter", "glide_tags", "glide_owned", "glide_advance", "glide_stop",
         "census")


@dataclass(frozen=True)
class Cfg:
    name: str
    n: int
    K: int
    vmask: int
    mmask: int
    bounds: tuple                                   # channel c plays into [bounds[c], bounds[c + 1])
    two_per_lane: bool
    in_place: int = -1

    def ranges(self):
        return [(a, b - a) for a, b in zip(self.bounds, self.bounds[1:])]


# channel 1's range starts off a 64-voice boundary and crosses a 256-thread workgroup span (tests/test_pedal.py's SHAPES)
CONFIGS = {
    "patch": Cfg("patch", 1280, 4, OS.VMASK, OS.MMASK, (0, 296, 660, 960, 1280), False),
    "plain": Cfg("plain", 600, 1, 1, 1, (0, 37, 330, 470, 600), True),
    "plain2": Cfg("plain2", 1500, 2, 0b11, 0b11, (0, 38, 420, 900, 1500), True, 2),
}


def make_bank(cfg, seed):
    """The bank a performance starts on: every slot sounds since long ago and belongs to nobody, except a few per channel (drawn from
    the seed) that are at rest -- the polyphony the channels fight over."""
    rng = np.random.default_rng(1000 + seed)
    rest = []
    for first, count in cfg.ranges():
        heads = np.arange(first, first + count, cfg.K)
        rest.extend(rng.choice(heads, int(rng.integers(4, 9)), replace=False).tolist())
    rest = np.array(sorted(rest), np.int32)
    if cfg.name == "patch":
        return OS.bank(cfg.n, rest)
    from test_slot_steal import plain_bank
    bank, tables, g, _ = plain_bank(cfg.n)
    e = bank["voice_amp_envelope"]
    e["attack_time"], e["decay_time"], e["release_time"] = np.float32(20.0), np.float32(50.0), np.float32(200.0)
    e["sustain_level"] = np.float32(0.6)
    bank["voice_smoother_smoothing"] = np.float32(0.5)
    v = np.arange(cfg.n)
    e["sample_start"][:] = (int(g.synth_sample_count) - 40000 - ((v // cfg.K) * 37) % 1000).astype(np.uint64)
    at_rest = np.isin(v - v % cfg.K, rest)
    e["is_active"][at_rest] = 0
    bank["voice_smoother_gain"][at_rest] = np.float32(0.0)
    return bank, tables, g


def setup(cfg):
    """the options the device bank of a configuration is opened with"""
    def apply(db):
        if cfg.two_per_lane:
            db.fast2_min_voices(0)
        if cfg.in_place >= 0:
            db.in_place(cfg.in_place)
    return apply


def tag_of(ch, key):
    return (ch << 24) | key


def key_inc(key, lane):
    return np.float32(0.05 * 2.0 ** ((key - 36) / 12.0) * (1.0 + 0.5 * lane))


class Host:
    """what the host keeps per channel"""

    def __init__(self, ch, rng_range):
        self.ch, self.range = ch, rng_range
        self.sustain = self.sost = False
        self.down, self.lifted, self.struck, self.bent = [], [], [], set()
        self.cap, self.glide_until, self.last_burst, self.plans = 6, -1, None, {}


class Gen:
    def __init__(self, seed, cfg):
        self.rng = np.random.default_rng([seed, cfg.n, cfg.K])                    # (a configuration's script is its own)
        self.cfg, self.K = cfg, cfg.K
        self.hosts = [Host(c, r) for c, r in zip(CHANNELS, cfg.ranges())]
        self.serial, self.calls, self.used = 0, None, set()
        self.whole = (0, cfg.n - cfg.n % cfg.K)

    # ---- helpers
    def emit(self, kind, **kw):
        self.calls.append((kind, kw))
        self.used.add(kind)
        self.serial += 1
        return self.serial - 1

    def pick(self, seq, k=1):
        seq = list(seq)
        k = min(k, len(seq))
        return [seq[i] for i in self.rng.choice(len(seq), k, replace=False)] if k else []

    def chance(self, p):
        return self.rng.random() < p

    def notes(self, keys):
        out = []
        for j, key in enumerate(keys):
            for l in range(self.K):
                pan = (j + l) % 3 == 0
                out.append(device.NoteC(key_inc(key, l), np.float32(0.5 + 0.05 * ((key + l) % 10)), np.float32(0.25 * ((key + l) % 3)),
                                        np.float32(0.2 + 0.1 * l) if pan else np.float32(0), np.float32(0.8 - 0.1 * l) if pan else np.float32(0),
                                        SM.SET_PHASE | (SM.SET_PAN if pan else 0)))
        return out

    def tags(self, h, keys):
        t = np.array([tag_of(h.ch, k) for k in keys], np.uint32)
        assert (t != 0).all() and len(t) <= OM.MAX_TAGS, "a zero tag or too many tags: unspecified input"
        return t

    def unique(self, h, keys):
        t = self.tags(h, keys)
        assert len(set(t.tolist())) == len(t), "a tag twice in one by-id call: a slot could be named twice"
        return t

    def queries(self, h, min_age=0):
        first, count = h.range
        iq = slot_query(first, count, self.K, self.cfg.mmask, WHICH, SETTLE, first, 0)
        return iq, SSM.SlotQuery(self.whole[0], self.whole[1], self.K, self.cfg.mmask, OLDEST, 0, min_age)

    def new_keys(self, h, k):
        free = [key for key in range(40, TOP_KEY + 1) if key not in h.down]
        return sorted(self.pick(free, k))

    def rates(self):
        return GM.per_64(float(self.pick((150.0, 400.0, 1200.0))[0]))

    def glide_on(self, h, b, blocks=8):
        h.glide_until = max(h.glide_until, b + blocks)

    # ---- the events
    def burst(self, h, b, keys=None, cap=None, mono=False):
        rng = self.rng
        if keys is None:
            k = int(rng.choice((1, 1, 2, 3, 4, 6, 9)))
            keys = self.new_keys(h, k)
            if h.lifted and self.chance(0.5):                                     # a key struck again while its note-off may be held
                keys = sorted(set(keys[1:] + [h.lifted[-1]]))
            elif h.down and self.chance(0.4):                                     # struck twice: two slots will carry the tag
                keys = sorted(set(keys[1:] + [h.down[-1]]))
        if cap is None:
            count = len(h.down) + len(h.lifted)
            cap = int(rng.choice((count, count + len(keys), max(1, count - 2), h.cap, CHM.NO_CAP)))
        if mono or cap <= 1:
            cap, keys = 1, keys[:1]
        h.cap = cap if cap != CHM.NO_CAP else h.cap
        iq, sq = self.queries(h, 0 if cap == 1 else int(rng.choice((0, 0, 100))))
        tags = self.tags(h, keys)
        ref = self.emit("note_on_channel", notes=self.notes(keys), tags=tags, iq=iq, sq=sq, match=CHM.channel(h.ch), cap=cap)
        for key in keys:
            if key in h.lifted:
                h.lifted.remove(key)
            if key not in h.down:
                h.down.append(key)
            h.struck.append(key)
            h.bent.discard(key)
        h.last_burst = (ref, keys, tags)
        return ref, keys, tags

    def legato(self, h, b):
        """a new key slides in from the last one: note_on_channel, THEN the glide on the new tag"""
        prev = h.down[-1] if h.down else 60
        key = self.new_keys(h, 1)[0]
        mono = self.chance(0.4)
        ref, keys, tags = self.burst(h, b, [key], cap=1 if mono else None, mono=mono)
        if self.chance(0.5):                                                      # exact: rate 2 from 2^-k below arrives ON step k
            steps = int(self.rng.integers(1, 4))
            g = GM.Glide(GM.FROM_SCALE, 2.0, 0.5, 2.0 ** (-steps if self.chance(0.5) else steps))
            arrive = self.arrival(b, steps)
            if arrive is not None and self.chance(0.8):
                h.plans.setdefault(arrive, []).append(("off", key))
        else:
            up, down = self.rates()
            g = GM.Glide(GM.FROM_SCALE, up, down, np.float32(SEMI ** float(np.clip(prev - key, -12, 12) or 5)))
        if self.chance(0.5):
            self.emit("glide_tags", glides=[g], first=h.range[0], count=h.range[1], tags=self.unique(h, [key]))
        else:
            self.emit("glide_owned", glides=[g], ref=ref, tags=tags)
        h.bent.add(key)
        self.glide_on(h, b)

    def arrival(self, b, steps):
        """the block in whose front the advance lands a glide of `steps` steps that starts in front of block b"""
        c = 0
        for k in range(b, BLOCKS - 1):
            c += self.frames[k]
            if c >> 6 >= steps:
                return k
        return None

    def retarget(self, h, b):
        """legato onto a new key without a retrigger: TO_SCALE on a sounding note, chained"""
        keys = self.pick(h.down, 2)
        up, down = self.rates()
        glides = [GM.Glide(GM.TO_SCALE, up, down, np.float32(SEMI ** int(self.rng.choice((-7, -3, 2, 4, 7))))) for _ in keys]
        self.emit("glide_tags", glides=glides, first=h.range[0], count=h.range[1], tags=self.unique(h, keys))
        h.bent.update(keys)
        self.glide_on(h, b)

    def off(self, h, keys=None, plain=None):
        if keys is None:
            keys = self.pick(h.down, int(self.rng.integers(1, 4)))
            if self.chance(0.3) and h.struck:                                     # a tag nobody carries any more (or never lifted twice)
                keys = sorted(set(keys + self.pick(h.struck, 1)))
        keys = sorted(set(keys))
        if not keys:
            return
        tags = self.unique(h, keys)
        if self.chance(0.12) if plain is None else plain:
            self.emit("release_tags", first=h.range[0], count=h.range[1], tags=tags)
        else:
            self.emit("release_tags_pedal", first=h.range[0], count=h.range[1], tags=tags, hold_all=h.sustain)
        for key in keys:
            if key in h.down:
                h.down.remove(key)
                if h.sustain or h.sost:
                    h.lifted.append(key)

    def pedal(self, h, what=None):
        first, count = h.range
        m = CHM.channel(h.ch)
        r = self.rng.random()
        if what == "latch":
            h.sost = False
            r = 0.5 if h.sustain else 0.69
        if what == "up" and not (h.sustain or h.sost):
            h.sustain = True
            if h.down:
                self.off(h, plain=False)
            r = 0.9
        if not h.sustain and r < 0.45:
            h.sustain = True                                                      # (sustain down is the host's knowledge alone)
            return self.off(h) if h.down else None
        if not h.sost and r < 0.7:
            h.sost = True
            return self.emit("pedal_latch", first=first, count=count, match=m)
        if h.sustain and h.sost and r < 0.2:
            h.sustain = h.sost = False
            h.lifted = []
            return self.emit("pedal_up", first=first, count=count, match=m, flags=PM.LIFT_SUSTAIN | PM.LIFT_SOSTENUTO)
        if h.sost and (r < 0.6 or not h.sustain):
            h.sost = False
            if not h.sustain:
                h.lifted = []
            return self.emit("pedal_up", first=first, count=count, match=m, flags=PM.LIFT_SOSTENUTO | (PM.SUSTAIN_DOWN if h.sustain else 0))
        if h.sustain:
            h.sustain = False
            if not h.sost:
                h.lifted = []
            return self.emit("pedal_up", first=first, count=count, match=m, flags=PM.LIFT_SUSTAIN)

    def all_off(self, h, what=None):
        first, count = h.range
        if self.chance(0.5) if what is None else what:                                                      # the stated order: the pedal's bits first
            self.emit("pedal_clear", first=first, count=count)
            h.sustain = h.sost = False
        self.emit("stamp_match", first=first, count=count, match=CHM.channel(h.ch))
        h.down, h.lifted = [], []

    def sweep(self, h, what=None):
        first, count = h.range
        K = self.K
        what = int(self.rng.integers(0, 4)) if what is None else what
        if what == 0:
            c = device.filter_coeffs(1, float(self.rng.choice((400.0, 1600.0, 6400.0))), 0.8, 44100.0)
            ctls = [device.ctl(CTL.FILTER, b0=c[0], b1=c[1], b2=c[2], a1=c[3], a2=c[4])] * K
        elif what == 1:
            ctls = [device.ctl(CTL.AMP, amp=float(self.rng.choice((0.05, 0.1, 0.2))))] * K
        elif what == 2:
            ctls = [device.ctl(CTL.INC_SCALE, inc_scale=float(np.float32(SEMI ** float(self.rng.choice((-1, 1, 2))))))] * K
            h.bent.update(h.down + h.lifted + h.struck)
        else:
            ctls = [device.ctl(CTL.PAN, pan_left=0.3 + 0.1 * l, pan_right=0.7 - 0.1 * l) for l in range(K)]
            return self.emit("ctl_range", ctls=ctls, first=first, count=count)
        self.emit("ctl_match", ctls=ctls, first=first, count=count, match=CHM.channel(h.ch))

    def per_note(self, h, what=None):
        first, count = h.range
        K = self.K
        keys = self.pick(h.down + h.lifted, 3) or self.pick(h.struck, 1)
        if not keys:
            return
        keys = sorted(set(keys))
        tags = self.unique(h, keys)
        what = int(self.rng.integers(0, 5)) if what is None else what
        E = device.ctl_each
        if what == 0:                                                             # a bend per note
            each = [E(EM.EACH_INC_SCALE, inc_scale=float(np.float32(SEMI ** (0.25 * (1 + j % 4))))) for j in range(len(keys))]
            h.bent.update(keys)
            self.emit("ctl_tags_each", ctls=None, each=each, first=first, count=count, tags=tags)
        elif what == 1:                                                           # velocity (aftertouch), a pan
            each = [E(EM.EACH_VELOCITY | EM.EACH_PAN, velocity=0.3 + 0.1 * j, pan_left=0.4, pan_right=0.6) for j in range(len(keys))]
            self.emit("ctl_tags_each", ctls=None, each=each, first=first, count=count, tags=tags)
        elif what == 2:                                                           # an amp product that vanishes: the store is withheld
            each = [E(EM.EACH_AMP_SCALE | EM.EACH_VELOCITY, amp_scale=1e-30, velocity=0.9) for _ in keys]
            self.emit("ctl_tags_each", ctls=[device.ctl(CTL.AMP, amp=1e-30)] * K, each=each, first=first, count=count, tags=tags)
        elif what == 3:                                                           # a bend that overflows: the store is withheld
            top = [k for k in (h.down + h.lifted) if k == TOP_KEY and k not in h.bent]
            if not top:
                return self.timbre(h, keys, tags)
            each = [E(EM.EACH_INC_SCALE, inc_scale=3.4e38)]
            self.emit("ctl_tags_each", ctls=None, each=each, first=first, count=count, tags=self.unique(h, top[:1]))
        else:
            self.timbre(h, keys, tags)

    def timbre(self, h, keys, tags):
        filt = [device.filter_each(*device.filter_coeffs(1, 220.0 * 2.0 ** ((k - 40) / 12.0), 0.9, 44100.0)) for k in keys]
        fmask = 1 if self.K > 1 and self.chance(0.5) else self.cfg.vmask
        self.emit("ctl_tags_each_filter", ctls=None, each=None, filt=filt, fmask=fmask, first=h.range[0], count=h.range[1], tags=tags)

    def after_burst(self, h, b, what=None):
        """calls on the d_assigned of the channel's last burst: the host never reads it"""
        ref, keys, tags = h.last_burst
        what = int(self.rng.integers(0, 4)) if what is None else what
        if what == 0:
            each = [device.ctl_each(EM.EACH_VELOCITY, velocity=0.4 + 0.05 * j) for j in range(len(keys))]
            self.emit("ctl_owned_each", ctls=None, each=each, ref=ref, tags=tags)
        elif what == 1:
            filt = [device.filter_each(*device.filter_coeffs(1, 300.0 + 100.0 * j, 0.7, 44100.0)) for j in range(len(keys))]
            each = [device.ctl_each(EM.EACH_PAN, pan_left=0.5, pan_right=0.5) for _ in keys]
            self.emit("ctl_owned_each_filter", ctls=None, each=each, filt=filt, fmask=self.cfg.vmask, ref=ref, tags=tags)
        elif what == 2:
            up, down = self.rates()
            self.emit("glide_owned", glides=[GM.Glide(GM.FROM_SCALE, up, down, np.float32(SEMI ** -5))] * len(keys), ref=ref, tags=tags)
            h.bent.update(keys)
            self.glide_on(h, b)
        else:                                                                     # staccato: the chord is lifted through its own list
            self.emit("stamp_owned_pedal", ref=ref, tags=tags, hold_all=h.sustain)
            for key in keys:
                if key in h.down:
                    h.down.remove(key)
                    if h.sustain or h.sost:
                        h.lifted.append(key)

    def untargeted(self, h, steal):
        """a chord through the unmatched calls and skred_bank_tag_slots on their d_assigned (tagged, as every note-on of the range)"""
        keys = self.new_keys(h, int(self.rng.integers(1, 4)))
        iq, sq = self.queries(h)
        sq = sq.but(first=h.range[0], count=h.range[1])                           # (unmatched: it must not leave the channel's range)
        if steal:
            ref = self.emit("note_on_steal_slots", notes=self.notes(keys), n=len(keys), iq=iq, sq=sq)
        else:
            ref = self.emit("note_on_idle_slots", notes=self.notes(keys), n=len(keys), iq=iq)
        tags = self.tags(h, keys)
        self.emit("tag_slots", ref=ref, tags=tags)
        for key in keys:
            h.down.append(key)
            h.struck.append(key)
            h.bent.discard(key)
        h.last_burst = (ref, keys, tags)

    def census(self, h):
        _, sq = self.queries(h)
        self.emit("census", sq=sq, match=CHM.channel(h.ch))

    def glide_stop(self, h):
        self.emit("glide_stop", first=h.range[0], count=h.range[1], snap=bool(self.chance(0.5)))
        h.glide_until = -1

    # ---- one performance
    def run(self):
        rng = self.rng
        self.frames = [int(f) for f in rng.choice(FRAMES, BLOCKS)]
        for at, f in zip(rng.choice(np.arange(2, BLOCKS - 1), len(FRAMES), replace=False), FRAMES):   # every length occurs
            self.frames[int(at)] = f
        script = []
        menu = ("burst", "burst", "legato", "retarget", "off", "off", "pedal", "pedal", "all_off", "sweep", "per_note", "per_note",
                "after_burst", "steal", "idle", "census", "glide_stop")
        must = {}                                                                 # every call kind occurs: block -> (channel, act, variant)
        for act in (("legato", None), ("retarget", None), ("off", True), ("off", False), ("pedal", "latch"), ("pedal", "up"), ("all_off", 0),
                    ("all_off", 1), ("sweep", 0), ("sweep", 3), ("per_note", 0), ("per_note", 4), ("after_burst", 0), ("after_burst", 1),
                    ("after_burst", 2), ("after_burst", 3), ("steal", None), ("idle", None), ("census", None), ("glide_stop", None),
                    ("top", None)):
            must.setdefault(int(rng.integers(2, BLOCKS - 1)), []).append((int(rng.integers(0, len(self.hosts))),) + act)
        for b in range(BLOCKS):
            self.calls = []
            if 2 <= b < BLOCKS - 1:
                for h in self.hosts:
                    for what, key in h.plans.pop(b, []):
                        if key in h.down:
                            self.off(h, [key])
                    for act in self.pick(menu, int(rng.integers(1, 3))):
                        self.act(h, b, act)
                for c, act, what in must.get(b, ()):
                    self.act(self.hosts[c], b, act, what)
                for h in self.hosts:                                              # portamento: the advance ahead of the render
                    if h.glide_until >= b:
                        self.emit("glide_advance", first=h.range[0], count=h.range[1], frames=self.frames[b])
            script.append({"frames": self.frames[b], "calls": self.calls})
        return script

    def act(self, h, b, act, what=None):
        if act == "burst":
            self.burst(h, b)
        elif act == "top":                                                        # the top key, held and never bent: the overflow's aim
            if TOP_KEY not in h.down:
                self.burst(h, b, [TOP_KEY], cap=CHM.NO_CAP)
            each = [device.ctl_each(EM.EACH_INC_SCALE, inc_scale=3.4e38)]
            self.emit("ctl_tags_each", ctls=None, each=each, first=h.range[0], count=h.range[1], tags=self.unique(h, [TOP_KEY]))
        elif act == "legato":
            self.legato(h, b)
        elif act == "retarget":
            if not h.down:
                self.burst(h, b)
            self.retarget(h, b)
        elif act == "off":
            if not h.down:
                self.burst(h, b)
            self.off(h, plain=what)
        elif act == "pedal":
            self.pedal(h, what)
        elif act == "all_off":
            self.all_off(h, what)
        elif act == "sweep":
            self.sweep(h, what)
        elif act == "per_note":
            if not h.struck:
                self.burst(h, b)
            self.per_note(h, what)
        elif act == "after_burst":
            if h.last_burst is None:
                self.burst(h, b)
            self.after_burst(h, b, what)
        elif act in ("steal", "idle"):
            self.untargeted(h, act == "steal")
        elif act == "census":
            self.census(h)
        elif act == "glide_stop":
            self.glide_stop(h)


def performance(seed, cfg):
    script = Gen(seed, cfg).run()
    assert len(script) == BLOCKS and not script[0]["calls"] and not script[1]["calls"] and not script[-1]["calls"]
    return script


def check_input(script):
    """what the generator promises never to produce (the issue's list of unspecified input)"""
    flat = [c for blk in script for c in blk["calls"]]
    for i, (kind, kw) in enumerate(flat):
        if kind in ("note_on_steal_slots", "note_on_idle_slots"):               # tagged and untagged note-ons never share a range
            nxt, nkw = flat[i + 1]
            assert nxt == "tag_slots" and nkw["ref"] == i and len(nkw["tags"]) == kw["n"], "an untagged note-on"
    for blk in script:
        for kind, kw in blk["calls"]:
            tags = kw.get("tags")
            if tags is not None:
                assert len(tags) <= OM.MAX_TAGS and all(int(t) != 0 for t in tags), kind
                if kind in ("release_tags", "release_tags_pedal", "glide_tags", "ctl_tags_each", "ctl_tags_each_filter"):
                    assert len(set(int(t) for t in tags)) == len(tags), kind
            for c in kw.get("ctls") or ():
                assert all(np.isfinite(getattr(c, f)) for f in EM.Rec.FIELDS), kind
            for e in kw.get("each") or ():
                assert all(np.isfinite(getattr(e, f)) for f in ("inc_scale", "amp_scale", "velocity", "pan_left", "pan_right")), kind
            for g in kw.get("glides") or ():
                assert GM.check([g], 1, 1) == 0, kind
