#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ from the UNMODIFIED reference.

Runs only where /root/reference exists (the build container).  It drives
oracle/_ref/libskred_ref.so -- the reference sources compiled in place by
`make -C oracle ref` -- through its own control path (wire(), i.e. the same text
protocol a user types) and its own audio callback (synth_callback -> synth() + seq()),
and stores inputs + expected outputs as small .npz fixtures:

  tables / table_*      the wavetables the voices reference (float pool)
  s<k>_in_<field>       full voice state before segment k (field names of synth.def)
  s<k>_globals_in/out   JSON: synth_sample_count, noise LCG state, volume smoother
  s<k>_mix              reference output frames [F][2]  (post master volume)
  s<k>_stems_sha256     sha256 of the `user` stem buffer bytes [F][64][2]
  s<k>_stems            stems of the listed voices only (when few voices are active)
  s<k>_out_<field>      read-write voice state after segment k

No reference source text is stored: fixtures are data.  Each case runs in a fresh process
because synth() keeps function-static state (first-call latch, noise LCG: synth.c:503-511).

usage: python tests/golden/gen_golden.py [--case NAME] [--list]
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(HERE))                      # tests/: fuzz_banks, golden_io

import fuzz_banks  # noqa: E402
from skred_amd.bank import ENV_DTYPE, FIELDS, MMF_DTYPE, RW_FIELDS, GlobalsC, VoiceBank  # noqa: E402

REF_DIR = os.environ.get("SKRED_REFERENCE", "/root/reference")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libskred_ref.so")
LCG_A, LCG_C, M64 = 6364136223846793005, 1442695040888963407, (1 << 64) - 1


class Ref:
    """A skred process image driven through ctypes: by default the reference itself
    (oracle/_ref/libskred_ref.so); tests/test_dropin.py passes oracle/_ref/libskred_dropin_check.so,
    i.e. the reference's wire/seq/skred objects linked against OUR libskred_synth.so instead of synth.o."""

    def __init__(self, lib_path=None):
        if lib_path is None:
            subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
            lib_path = REF_SO
        self.L = C.CDLL(lib_path)
        self.L.ref_boot()
        self.L.ref_stems.restype = C.POINTER(C.c_float)
        self.L.ref_ext_table.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_float, C.c_float]
        self.V = self.L.ref_voice_max()
        self.W = self.L.ref_wave_table_max()
        assert self.L.ref_sizeof_mmf() == MMF_DTYPE.itemsize
        assert self.L.ref_sizeof_envelope() == ENV_DTYPE.itemsize
        self.frames_done = 0          # frames rendered so far == LCG draws so far (synth.c:525)

    # -- raw views of the reference's global arrays (synth.def) --
    def arr(self, name, dtype, n=None):
        n = self.V if n is None else n
        dt = np.dtype(dtype)
        raw = (C.c_char * (dt.itemsize * n)).in_dll(self.L, name)
        return np.frombuffer(raw, dtype=dt, count=n)

    def scalar(self, name, ctype):
        return ctype.in_dll(self.L, name)

    def wire(self, line: str):
        for part in line.split("\n"):
            if part.strip():
                r = self.L.ref_wire(part.encode())
                assert r == 0, (part, r)

    def load_patch(self, n: int):
        r = self.L.ref_load_patch(REF_DIR.encode(), n)
        assert r == 0, r

    def ext_table(self, slot, data, rate=44100.0, one_shot=0, loop_enabled=0, loop_start=0,
                  loop_end=None, midi_note=69.0, offset_hz=0.0):
        data = np.ascontiguousarray(data, np.float32)
        le = (len(data) - 1) if loop_end is None else loop_end
        r = self.L.ref_ext_table(slot, data.ctypes.data, len(data), rate, one_shot, loop_enabled,
                                 loop_start, le, midi_note, offset_hz)
        assert r == 0, r

    def noise_rng(self) -> int:
        s = 1                                     # audio_rng_init(&synth_random, 1), synth.c:508
        for _ in range(self.frames_done):
            s = (s * LCG_A + LCG_C) & M64
        return s

    def globals(self) -> GlobalsC:
        return GlobalsC(self.scalar("synth_sample_count", C.c_uint64).value, self.noise_rng(),
                        self.scalar("volume_final", C.c_float).value,
                        self.scalar("volume_smoother_gain", C.c_float).value,
                        self.scalar("volume_smoother_smoothing", C.c_float).value, 0.0)

    def snapshot(self):
        """(VoiceBank, tables pool) of the current reference state."""
        b = VoiceBank(self.V)
        tptr = self.arr("voice_table", "<u8")
        tsize = self.arr("voice_table_size", "<i4")
        pool, offs, seen = [], np.zeros(self.V, np.int64), {}
        pos = 0
        for v in range(self.V):
            p, n = int(tptr[v]), int(tsize[v])
            if p == 0 or n <= 0:
                continue
            if (p, n) not in seen:
                data = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n,)).copy()
                seen[(p, n)] = pos
                pool.append(data)
                pos += n
            offs[v] = seen[(p, n)]
        for name, dt, _ in FIELDS:
            if name == "voice_table_offset":
                b.a[name] = offs
            else:
                b.a[name] = self.arr(name, dt).copy()
        tables = np.concatenate(pool) if pool else np.zeros(1, np.float32)
        return b, tables.astype(np.float32)

    def render(self, frames: int, block: int = 512):
        """frames of audio through synth_callback in `block`-frame calls (skred.h:12 default)."""
        mix = np.zeros((frames, 2), np.float32)
        stems = np.zeros((frames, self.V, 2), np.float32)
        sp = self.L.ref_stems()
        p = 0
        while p < frames:
            n = min(block, frames - p)
            self.L.ref_callback(mix[p:].ctypes.data_as(C.c_void_p), n)
            stems[p:p + n] = np.ctypeslib.as_array(sp, shape=(n, self.V, 2))
            p += n
        self.frames_done += frames
        return mix, stems


def fnv1a32(b: bytes) -> str:
    h = 0x811C9DC5
    for x in b:
        h = ((h ^ x) * 0x01000193) & 0xFFFFFFFF
    return "%08x" % h


class Case:
    def __init__(self, name, desc):
        self.name, self.desc = name, desc
        self.out = {}
        self.meta = {"case": name, "description": desc, "sample_rate": 44100, "segments": [],
                     "generator": "tests/golden/gen_golden.py", "flags": "-O2 -ffp-contract=off"}
        self.k = 0
        self.tables = None

    def segment(self, ref: Ref, frames, block=512, keep_stems=(), note=""):
        bank, tables = ref.snapshot()
        # oracle/ref_driver.c owns an EMPTY pcm[] / pcm_map[] (the sample blob is absent from the mount), so the AMY
        # slots 100-199 of this reference build hold no data: no fixture may stand on them
        idx = bank.a["voice_wave_table_index"]
        assert not ((idx >= 100) & (idx <= 199)).any(), f"case {self.name}: a voice sits on an AMY slot (100-199)"
        if self.tables is None:
            self.tables = tables
            self.out["tables"] = tables
        else:
            assert tables.shape == self.tables.shape and (tables == self.tables).all(), \
                "table pool changed between segments"
        g_in = ref.globals()
        mix, stems = ref.render(frames, block)
        bank_out, _ = ref.snapshot()
        g_out = ref.globals()
        p = f"s{self.k}_"
        self.out.update(bank.to_arrays(p + "in_"))
        self.out.update(bank_out.to_arrays(p + "out_", RW_FIELDS))
        self.out[p + "mix"] = mix
        self.out[p + "globals_in"] = np.array(json.dumps(g_in.to_dict()))
        self.out[p + "globals_out"] = np.array(json.dumps(g_out.to_dict()))
        self.out[p + "stems_sha256"] = np.array(hashlib.sha256(stems.tobytes()).hexdigest())
        keep = list(keep_stems)
        if keep:
            self.out[p + "stems"] = np.ascontiguousarray(stems[:, keep, :])
            self.out[p + "stems_voices"] = np.array(keep, np.int32)
        self.meta["segments"].append({"frames": frames, "block": block, "note": note,
                                      "mix_fnv1a32": fnv1a32(mix.tobytes()),
                                      "mix_rms": float(np.sqrt((mix.astype(np.float64) ** 2).mean())),
                                      "mix_peak": float(np.abs(mix).max())})
        self.k += 1
        return mix, stems

    def extra(self, name, value):
        """Case-specific data next to the segments (input files, expected files); `x_` prefix in the npz."""
        self.out["x_" + name] = np.ascontiguousarray(value)

    def save(self):
        if self.name == "c0_0sk":
            assert self.meta["segments"][0]["mix_fnv1a32"] == "4160cd81", self.meta["segments"][0]
        self.out["meta"] = np.array(json.dumps(self.meta))
        path = os.path.join(HERE, self.name + ".npz")
        save_npz(path, self.out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes) segments={self.k}")
        for s in self.meta["segments"]:
            print("   ", s)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member times, so that the same arrays always give the same file.  Every case is written this
    way.  The ten fixtures older than the fuzz cases were written by np.savez_compressed itself, whose member times are the time of
    writing: regenerating one of them gives the same arrays in a file of other bytes, as it always did (no test compares file
    bytes; only the fuzz fixtures are byte-stable from their first commit)."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def lcg_uniform(n, seed):
    """n floats in [-1,1) from the reference's LCG recurrence (synth.c:110-123)."""
    out = np.zeros(n, np.float32)
    s = seed
    for i in range(n):
        s = (s * LCG_A + LCG_C) & M64
        hi = (s >> 32) & 0xFFFFFFFF
        if hi >= 1 << 31:
            hi -= 1 << 32
        out[i] = np.float32(hi) / np.float32(2147483648.0)
    return out


# ---------------------------------------------------------------- the cases

# the three lines of the reference patch 0.sk (BASELINE config 0), fed through wire() so that the
# case can also be replayed where the reference tree is absent (GPU box)
PATCH_0SK = ["S100", "v0 w0 f440 a4 F1,10", "v1 w0 f1 a50 m1"]


def case_c0_0sk(ref, Case):
    """BASELINE config 0: 0.sk, 1 s, 512-frame callbacks.  Anchor from SURVEY §8c: FNV-1a 4160cd81."""
    if os.path.isdir(REF_DIR):
        assert [l.rstrip("\n") for l in open(os.path.join(REF_DIR, "0.sk"))] == PATCH_0SK
    for line in PATCH_0SK:
        ref.wire(line)
    c = Case("c0_0sk", "reference patch 0.sk (sine carrier v0, FM by muted v1 > v0: one-frame-delay "
                        "modulator semantics), 44100 frames in 512-frame callbacks")
    c.segment(ref, 44100, 512, keep_stems=(0, 1))
    c.save()


def case_c1_sine_adsr(ref, Case):
    """BASELINE config 1 shape at N=64: sine + ADSR (+ default amp smoother), note-off mid-way,
    then long enough for the envelope to end and the smoother to decay through the subnormals."""
    u = (lcg_uniform(192, 0x5EED) + 1.0) * 0.5
    for v in range(64):
        f = 27.5 * 2.0 ** (7.0 * float(u[v]))
        pan = float(u[64 + v]) * 2.0 - 1.0
        amp = 0.25 + float(u[128 + v])
        ref.wire(f"v{v} w0 f{f:.6f} a{amp:.6f} p{pan:.6f} t0.01,0.1,0.7,0.2 l{0.5 + 0.5 * float(u[v]):.4f}")
    c = Case("c1_sine_adsr64", "64 sine voices (w0), distinct freq/amp/pan, ADSR t0.01,0.1,0.7,0.2 "
                               "triggered with l<vel>; note-off after 2048 frames; run past release end "
                               "and through the subnormal tail of the amp smoother")
    c.segment(ref, 2048, 512, note="attack+decay+sustain")
    for v in range(64):
        ref.wire(f"v{v} l0")
    c.segment(ref, 2048, 512, note="release starts")
    c.segment(ref, 8192, 512, note="release ends (8820 frames), is_active -> 0")
    c.segment(ref, 12288, 100, note="smoother tail decays through subnormals to 0; 100-frame callbacks")
    c.save()


def case_c2_mixed_filter(ref, Case):
    """BASELINE config 2 shape at N=64: mixed tables + biquad modes 1..5."""
    u = (lcg_uniform(256, 0xC2) + 1.0) * 0.5
    waves = [0, 4, 1, 2, 3]
    for v in range(64):
        f = 27.5 * 2.0 ** (6.0 * float(u[v]))
        pan = float(u[64 + v]) * 2.0 - 1.0
        k = 100.0 * (80.0 ** float(u[128 + v]))
        q = 0.5 + 3.5 * float(u[192 + v])
        ref.wire(f"v{v} w{waves[v % 5]} f{f:.6f} a1 p{pan:.6f} J{1 + v % 5} K{k:.4f} Q{q:.4f}")
    c = Case("c2_mixed_filter64", "64 voices cycling sine/triangle/square/saw tables (w0,w4,w1,w2,w3) "
                                  "through RBJ biquad modes 1..5 with varied K/Q")
    c.segment(ref, 4096, 512)
    c.save()


def case_c2_notamy(ref, Case):
    """Config 2/3 tables: the notamy float LUT pyramids installed into EXT slots (the reference
    itself never loads them: SURVEY D3), voices spread over all pyramid levels, filter on."""
    luts = np.load(os.path.join(HERE, "..", "..", "skred_amd", "data", "notamy_luts.npz"))
    names = json.loads(str(luts["names"]))
    slot = 200
    slots = []
    for nm in names:
        ref.ext_table(slot, luts["f32_" + nm])
        slots.append((slot, len(luts["f32_" + nm])))
        slot += 1
    u = (lcg_uniform(192, 0xA3) + 1.0) * 0.5
    for v in range(64):
        s, _ = slots[v % len(slots)]
        f = 55.0 * 2.0 ** (6.0 * float(u[v]))
        pan = float(u[64 + v]) * 2.0 - 1.0
        k = 200.0 * (30.0 ** float(u[128 + v]))
        ref.wire(f"v{v} w{s} f{f:.6f} a0.8 p{pan:.6f} J{1 + v % 4} K{k:.4f} Q{0.6 + (v % 7) * 0.4:.3f}")
    c = Case("c2_notamy64", "notamy sine/triangle/impulse float LUTs (all pyramid levels, sizes 8..1024) "
                            "as cyclic tables in EXT slots 200+, biquad modes 1..4")
    c.segment(ref, 4096, 512)
    c.save()


# geometry (length, loopstart, loopend, midinote) of a few pcm_map entries, notamy/pcm_large.h:11-20
PCM_GEOM = [(707, 342, 684, 89), (8186, 4282, 7439, 39), (2766, 1377, 2744, 45),
            (1311, 898, 1288, 52), (2276, 1164, 2254, 51)]


def install_pcm_tables(ref):
    """The five synthetic one-shot tables of the c4_pcm_oneshot case in EXT slots 200-204."""
    for i, (n, ls, le, note) in enumerate(PCM_GEOM):
        data = lcg_uniform(n, 0x9C3 + i)
        data = np.convolve(data, np.ones(5, np.float32) / 5.0, mode="same").astype(np.float32)
        data /= np.abs(data).max()
        hz = 440.0 * 2.0 ** ((note - 69.0) / 12.0)
        ref.ext_table(200 + i, data, rate=22050.0, one_shot=1, loop_enabled=0, loop_start=ls,
                      loop_end=le, midi_note=float(note), offset_hz=hz)


def case_c4_pcm(ref, Case):
    """BASELINE config 5 shape, truncate mode: one-shot PCM-like tables (synthetic, seeded) with the
    real pcm_map geometry: forward, reverse, looped, finishing mid-block."""
    install_pcm_tables(ref)
    lines = []
    v = 0
    for i, (n, ls, le, note) in enumerate(PCM_GEOM):
        hz = 440.0 * 2.0 ** ((note - 69.0) / 12.0)
        for mode in range(4):
            f = hz * [1.0, 0.37, 2.9, 7.3][(mode + i) % 4]
            pan = -0.9 + 0.09 * v
            if mode == 0:   # forward one-shot
                lines.append(f"v{v} w{200 + i} f{f:.5f} a1 p{pan:.3f} T")
            elif mode == 1:  # reverse one-shot
                lines.append(f"v{v} w{200 + i} f{f:.5f} a1 p{pan:.3f} b1 T")
            elif mode == 2:  # forward, looped between the map's loop points
                lines.append(f"v{v} w{200 + i} f{f:.5f} a1 p{pan:.3f} B1 T")
            else:            # reverse, looped
                lines.append(f"v{v} w{200 + i} f{f:.5f} a1 p{pan:.3f} B1 b1 T")
            v += 1
    for ln in lines:
        ref.wire(ln)
    c = Case("c4_pcm_oneshot", "20 voices on 5 synthetic one-shot tables with pcm_map geometry: forward / "
                               "reverse / looped / reverse-looped; several finish mid-block and freeze")
    c.segment(ref, 3000, 512, keep_stems=tuple(range(v)))
    # retrigger a few finished voices, change direction of a looping one
    ref.wire("v0 T\nv1 T\nv6 b1\nv9 T")
    c.segment(ref, 3000, 512, keep_stems=tuple(range(v)), note="after retrigger of v0 v1 v9, v6 reversed")
    c.save()


def case_edge_basic(ref, Case):
    """Edge cases without cross-voice modulation."""
    ref.wire("v0 w0 f440 a0")                              # amp == 0: skipped, state frozen
    ref.wire("v1 w0 f330 a1 h7")                           # sample & hold
    ref.wire("v2 w4 f220 a1 q4")                           # bit crush
    ref.wire("v3 w0 f500 a1 m1")                           # disconnected from the mix
    ref.wire("v4 w6 a0.5")                                 # shared per-frame LCG noise
    ref.wire("v5 w5 f3 a0.5 p-0.5")                        # noise table
    ref.wire("v6 w0 f440 a1 s0")                           # smoother off
    ref.wire("v7 w0 f441 a1 s0.5")                         # fast smoother
    ref.wire("v8 w3 f100 a1 b1")                           # cyclic table played backwards
    ref.wire("v9 w0 f30000 a1 p0.3")                       # inc > size/2
    ref.wire("v10 w2 f44000 a1 p-0.3")                     # inc ~ size: general fmodf wrap
    ref.wire("v11 w0 f440 a1 t0.001,0.002,0.5,0.003 l1")   # short envelope, released below
    ref.wire("v12 w1 f60 a1 J5 K1200 Q2")                  # all-pass
    ref.wire("v13 w0 f0 a1")                               # zero increment
    ref.wire("v14 w0 f1234.5 a1 h3 q6 J1 K900 Q1.5 p0.7")  # S&H + crush + filter together
    ref.wire("v15 w0 f880 a1 t0,0,1,0 l0.5")               # flat envelope with velocity
    ref.wire("v16 w0 f2 a1 p1")                            # sub-audio, hard right
    ref.wire("V0.5")                                       # master volume change (smoothed)
    c = Case("edge_basic", "skip/hold/crush/mute/noise/smoother/reverse/fast-wrap/short-ADSR/all-pass "
                           "voices, master volume step")
    c.segment(ref, 1024, 512, keep_stems=tuple(range(17)))
    ref.wire("v11 l0\nv0 a1\nv6 a0\nv2 f3000\nV1")
    c.segment(ref, 1024, 512, keep_stems=tuple(range(17)), note="v11 released, v0 un-muted, v6 amp 0")
    c.segment(ref, 700, 33, keep_stems=tuple(range(17)), note="odd block size 33")
    c.save()


def case_edge_mod(ref, Case):
    """Cross-voice modulation (FM/AM/pan/CZ) and phase distortion: SURVEY §8f rank 2."""
    ref.wire("v0 w0 f440 a1 F1,5")          # FM, modulator index > carrier (previous frame's value)
    ref.wire("v1 w0 f3 a20 m1")
    ref.wire("v2 w0 f2 a10 m1")             # FM, modulator index < carrier (this frame's value)
    ref.wire("v3 w0 f200 a1 F2,3")
    ref.wire("v4 w0 f300 a1 A5,0.5")        # AM
    ref.wire("v5 w0 f4 a1 m1")
    ref.wire("v6 w1 f250 a1 P7,0.8")        # pan modulation
    ref.wire("v7 w0 f1 a1 m1")
    for i in range(7):                      # CZ modes 1..7
        ref.wire(f"v{8 + i} w0 f{110 + 7 * i} a1 c{i + 1},{0.15 + 0.1 * i:.2f}")
    ref.wire("v15 w0 f110 a1 c1,0.2 C16,0.3")  # CZ amount modulated
    ref.wire("v16 w0 f0.5 a1 m1")
    ref.wire("v17 w0 f330 a1 A17,0.9")         # self amplitude modulation
    ref.wire("v18 w4 f120 a1 F19,2 A19,0.7 P19,0.5 J1 K800 Q2")  # everything from one modulator
    ref.wire("v19 w0 f5 a2 m1")
    ref.wire("v20 w0 f100 a1 F3,1")            # chain: v2 -> v3 -> v20
    c = Case("edge_mod", "FM / AM / pan-mod / CZ modes 1..7 / CZ-mod / self-AM / modulation chain")
    c.segment(ref, 2048, 512, keep_stems=tuple(range(21)))
    c.save()


# ---- WAV files in, stem recording out (SURVEY 8f "next" #3) ----

# (which, format, channels, sample rate, frames, extra): input files `<which>.wav` for `:w` (wire.c:801-814)
WAV_INPUTS = [
    (1, "s16", 1, 44100, 3000, ""),
    (2, "s16", 2, 22050, 2000, "list"),        # a LIST chunk sits between fmt and data
    (3, "u8", 1, 8000, 1000, ""),
    (4, "s24", 1, 48000, 1500, "extensible"),  # WAVE_FORMAT_EXTENSIBLE header
    (5, "s32", 2, 44100, 800, ""),
    (6, "f32", 1, 44100, 1200, ""),
    (7, "f32", 2, 32000, 901, "odd"),          # odd-sized LIST chunk (pad byte) before data
]
# (which, slot, ch): ch -1 is the parser's default (wire.c:804).  miniwav.c:130 compares it with an unsigned
# channel count, so -1 becomes `channels` and the copy at miniwav.c:137 reads channel 0 of the NEXT frame: the
# table is the file's channel 0 advanced by one sample, and its last element is read past the decoded buffer
# (undefined).  Kept, because it is what the reference plays; the undefined element is set to 0.0f below so
# that the fixture is reproducible (this build defines it as 0.0f).
WAV_LOADS = [(1, 200, -1), (2, 201, 0), (2, 202, 1), (3, 203, -1), (4, 204, 0), (5, 205, 1), (6, 206, -1),
             (7, 207, 0), (2, 208, -1)]


def wav_bytes(fmt, channels, rate, frames, extra, seed):
    """A small RIFF/WAVE file: seeded noise + a decaying sine, peak ~0.8."""
    import struct
    x = lcg_uniform(frames * channels, seed).astype(np.float64).reshape(frames, channels)
    t = np.arange(frames)[:, None] / float(rate)
    x = 0.45 * x + 0.35 * np.sin(2 * np.pi * 330.0 * (1 + np.arange(channels)[None, :]) * t) * np.exp(-3.0 * t)
    if fmt == "u8":
        data = np.clip(np.round(x * 127.0 + 128.0), 0, 255).astype(np.uint8).tobytes()
        tag, bits = 1, 8
    elif fmt == "s16":
        data = np.clip(np.round(x * 32767.0), -32768, 32767).astype("<i2").tobytes()
        tag, bits = 1, 16
    elif fmt == "s24":
        v = np.clip(np.round(x * 8388607.0), -8388608, 8388607).astype("<i4").reshape(-1)
        data = v.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
        tag, bits = 1, 24
    elif fmt == "s32":
        data = np.clip(np.round(x * 2147483647.0), -2147483648, 2147483647).astype("<i4").tobytes()
        tag, bits = 1, 32
    else:
        data = x.astype("<f4").tobytes()
        tag, bits = 3, 32
    align = channels * bits // 8
    if extra == "extensible":
        guid = struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
        fmt_chunk = struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * align, align, bits, 22, bits,
                                (1 << channels) - 1) + guid
    else:
        fmt_chunk = struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt_chunk)) + fmt_chunk
    if extra == "list":
        body = b"INFOISFT" + struct.pack("<I", 6) + b"skred\0"
        chunks += b"LIST" + struct.pack("<I", len(body)) + body
    if extra == "odd":
        body = b"INFOISFT" + struct.pack("<I", 5) + b"skre\0"      # 17 bytes -> one pad byte follows
        chunks += b"LIST" + struct.pack("<I", len(body)) + body + b"\0"
    chunks += b"data" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


WAVE_SLOT_FIELDS = [("wave_size", "<i4"), ("wave_rate", "<f4"), ("wave_one_shot", "<i4"),
                    ("wave_loop_enabled", "<i4"), ("wave_loop_start", "<i4"), ("wave_loop_end", "<i4"),
                    ("wave_midi_note", "<f4"), ("wave_offset_hz", "<f4"), ("wave_is_miniwav", "<i4")]


def wav_case_lines():
    """(the `:w` lines, the voice lines) of the wav_samples case; tests/test_wav.py feeds the same lines to
    this build's own patch reader."""
    loads = [f":w{which},{slot}" + (f",{ch}" if ch >= 0 else "") for which, slot, ch in WAV_LOADS]
    lines = []
    for v, (which, slot, ch) in enumerate(WAV_LOADS):
        pan = -0.8 + 0.2 * v
        f = [220.0, 440.0, 330.0, 1760.0, 440.0, 550.0, 110.0, 880.0, 440.0][v]
        mods = ["", " B1", " b1", "", " B1 b1", "", " B1", "", ""][v]
        lines.append(f"v{v} w{slot} f{f:.3f} a{1 + 0.25 * v:.2f} p{pan:.2f}{mods} T")
    lines += ["v0 r1", "v3 r1", "v5 r1"]
    return loads, lines


def case_wav_samples(ref, Case):
    """`:w` loads 7 WAV files (u8/s16/s24/s32/f32, mono/stereo, extra chunks) into EXT slots through the
    reference's loader (wire.c:406-441 -> miniwav.c:103-147); 9 voices play them (one-shot, looped, reverse);
    3 voices are stem-recorded (`r1`, `<`, `*`: wire.c:698,816-849 -> save_wav wire.c:94-185)."""
    import glob
    import tempfile
    c = Case("wav_samples", "9 voices on WAV files loaded with :w (all PCM widths + float, mono/stereo); "
                            "voices 0,3,5 stem-recorded to a 6-channel 16-bit WAV")
    old = os.getcwd()
    tmp = tempfile.mkdtemp(prefix="skred_wav_")
    os.chdir(tmp)
    try:
        for which, fmt, ch, rate, frames, extra in WAV_INPUTS:
            b = wav_bytes(fmt, ch, rate, frames, extra, 0xA5 + which)
            with open(f"{which}.wav", "wb") as f:
                f.write(b)
            c.extra(f"wav_in_{which}", np.frombuffer(b, np.uint8))
        load_lines, voice_lines = wav_case_lines()
        for ln in load_lines:
            ref.wire(ln)
        c.extra("wav_loads", np.array(WAV_LOADS, np.int32))
        slots = [w[1] for w in WAV_LOADS]
        for which, slot, ch in WAV_LOADS:
            if ch < 0:
                n = int(ref.arr("wave_size", "<i4", ref.W)[slot])
                p = int(ref.arr("wave_table_data", "<u8", ref.W)[slot])
                C.cast(p, C.POINTER(C.c_float))[n - 1] = 0.0
        for name, dt in WAVE_SLOT_FIELDS:
            c.extra("slot_" + name, ref.arr(name, dt, ref.W)[slots].copy())
        tp = ref.arr("wave_table_data", "<u8", ref.W)
        sz = ref.arr("wave_size", "<i4", ref.W)
        for slot in slots:
            c.extra(f"slot_table_{slot}", np.ctypeslib.as_array(
                C.cast(int(tp[slot]), C.POINTER(C.c_float)), shape=(int(sz[slot]),)).copy())
        for ln in voice_lines:
            ref.wire(ln)
        ref.L.synth_callback_init.argtypes = [C.c_float]
        if hasattr(ref.L, "synth_callback_init"):
            ref.L.synth_callback_init(C.c_float(1.0))           # skred.c:91-99 (the recorder buffer)
        ref.wire("<0.05")                                       # 0.05 s = 2205 frames of 64 stereo stems
        c.segment(ref, 2560, 512, keep_stems=tuple(range(len(WAV_LOADS))), note="recording stops inside block 5")
        ref.wire("*")
        out = sorted(glob.glob("skred-*.wav"))
        assert len(out) == 1, out
        with open(out[0], "rb") as f:
            c.extra("rec_wav", np.frombuffer(f.read(), np.uint8))
        os.remove(out[0])
        ref.wire("v1 T\nv5 T")
        c.segment(ref, 1024, 512, keep_stems=tuple(range(len(WAV_LOADS))), note="v1 v5 retriggered")
    finally:
        os.chdir(old)
    c.save()


def korg_lines():
    """64 voices over the Korg DW-8000 single cycles (wave slots 32-62, synth.c:1251-1268): every slot at least once,
    the slots the shipped patches use (w33, w36, w49 in 2/11/16/23/42.sk) also as FM carriers and modulators, filters,
    envelopes, reverse playback."""
    lines = []
    for v in range(64):
        slot = 32 + v % 31
        f = 41.2 * 2.0 ** (v / 11.0)
        ln = f"v{v} w{slot} f{f:.4f} a{0.4 + 0.02 * (v % 13):.2f} p{-0.9 + 1.8 * ((v * 29) % 64) / 63.0:.4f}"
        if v % 4 == 1:
            ln += f" J{1 + v % 5} K{180.0 + 55.0 * v:.1f} Q{0.7 + 0.1 * (v % 6):.1f}"
        if v % 5 == 2:
            ln += f" t0.005,0.05,0.6,0.08 l{0.6 + 0.1 * (v % 4):.1f}"
        if v % 9 == 4:
            ln += " b1"
        lines.append(ln)
    # the shapes of the shipped patches: carrier on w49 modulated by a muted slow sine above it; a muted w33 modulator
    lines += ["v60 w49 f440 a4 p1 F61,100", "v61 w0 f0.125 a100 m1", "v62 w36 f220 a2 A63,1", "v63 w33 f25 a50 m1"]
    return lines


def case_korg_waves(ref, Case):
    for ln in korg_lines():
        ref.wire(ln)
    c = Case("korg_waves", "64 voices on the Korg DW-8000 cycles of wave slots 32-62 (incl. w33/w36/w49 as the shipped "
                           "patches use them: FM carrier, AM carrier, muted modulators), filters, envelopes, reverse")
    c.segment(ref, 3072, 512, note="attack/decay/sustain")
    for v in range(2, 60, 5):
        ref.wire(f"v{v} l0")
    c.segment(ref, 4096, 512, note="note-off, release ends (3528 frames)")
    c.save()


def bank256_lines(part):
    """The 64 voice lines of part `part` (0..3) of the bank256_sum case: same tables per voice index in every part
    (so that all four snapshots share one table pool), everything else different."""
    lines = []
    for i in range(64):
        n = part * 64 + i
        f = 55.0 * 2.0 ** (n / 40.0)
        pan = -0.95 + 1.9 * ((n * 37) % 256) / 255.0
        k = 200.0 + 30.0 * i + 500.0 * part
        lines.append(f"v{i} w{[0, 4, 1][i % 3]} f{f:.5f} a{0.5 + 0.01 * i:.2f} p{pan:.4f} "
                     f"J{1 + (n % 4)} K{k:.2f} Q{0.6 + 0.05 * (n % 9):.2f} t0.01,0.1,0.7,0.2 l{0.5 + 0.125 * (n % 5):.3f}")
    return lines


def case_bank256_sum(ref, Case):
    """N > 64 pinned to the reference itself (SURVEY 8c "N > 64"): the reference renders four different 64-voice
    banks, one after the other; a build that renders all 256 voices at once must produce, per voice, the same
    stems, and as its pre-master sum the sum of the four runs' stems (accumulated here in f64)."""
    c = Case("bank256_sum", "4 x 64 voices (sine/triangle/square, biquad modes 1-4, ADSR in attack/decay): per-part "
                            "fixtures + the f64 sum of all 256 voices' stems over the same 1024 frames")
    frames = 1024
    total = np.zeros((frames, 2), np.float64)
    h = hashlib.sha256()
    parts = []
    for part in range(4):
        for ln in bank256_lines(part):
            ref.wire(ln)
        r = c.segment(ref, frames, 512, note=f"voices {part * 64}..{part * 64 + 63} of the 256-voice bank")
        if r is None:
            return                                   # control-path replay stops at the first segment
        _, stems = r
        total += stems.astype(np.float64).sum(axis=1)
        parts.append(stems)
    all_stems = np.ascontiguousarray(np.concatenate(parts, axis=1))          # [F][256][2]
    c.extra("sum64", total)
    c.extra("stems256_sha256", np.frombuffer(hashlib.sha256(all_stems.tobytes()).digest(), np.uint8))
    c.save()


# ---- fuzzed banks: state written straight into the reference's arrays (tests/fuzz_banks.py) ----

FUZZ_SLOTS = [0, 200, 201, 202, 203, 204]      # the sine and the five one-shot tables of install_pcm_tables()
FUZZ_SEEDS = {"fuzz_mod_0": 0, "fuzz_mod_1": 1, "fuzz_mod_2": 2, "fuzz_mod_3": 3}
FUZZ_BLOCKS = [512, 33, 64, 100, 1, 7, 65]


def fuzz_setup(ref):
    """Install the tables the fuzzed banks sit on; returns the (offset, size) catalogue fuzz_banks.wild_bank() draws from, entry
    k standing for wave slot FUZZ_SLOTS[k] (the offsets only tell the entries apart: snapshot() lays the pool out again)."""
    install_pcm_tables(ref)
    sizes = ref.arr("wave_size", "<i4", ref.W)[FUZZ_SLOTS]
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return [(int(o), int(n)) for o, n in zip(offs, sizes)]


def write_bank(ref, bank):
    """Every field of `bank` but the table binding into the reference's per-voice arrays."""
    for name, dt, _ in FIELDS:
        if name not in ("voice_table_offset", "voice_table_size"):
            ref.arr(name, dt)[:] = bank.a[name]


def inject_bank(ref, bank, cat, count0):
    """Make `bank` (64 voices drawn over the catalogue of fuzz_setup) the reference's state: each voice is bound to its table with
    `v<k> w<slot>` (voice_table is a pointer), everything else is stored into the arrays, the sample clock is set."""
    assert bank.n == ref.V
    slot_of = {o: FUZZ_SLOTS[k] for k, (o, _) in enumerate(cat)}
    for v in range(bank.n):
        ref.wire(f"v{v} w{slot_of[int(bank['voice_table_offset'][v])]}")
    assert (ref.arr("voice_table_size", "<i4") == bank["voice_table_size"]).all()
    write_bank(ref, bank)
    ref.scalar("synth_sample_count", C.c_uint64).value = count0


def apply_action(ref, action):
    """One fuzz_banks.Action on the reference's state as it stands."""
    mirror, _ = ref.snapshot()
    action.apply(mirror, ref.scalar("synth_sample_count", C.c_uint64).value)
    write_bank(ref, mirror)


def fuzz_plan(seed, cat):
    """(bank, [(frames, callback size, actions before the segment)]) of fuzz seed `seed`: four to six segments."""
    rng = np.random.default_rng(7000 + seed)
    bank, _ = fuzz_banks.wild_bank(rng, 64, cat, "any64")
    k = int(rng.integers(4, 7))
    acts = fuzz_banks.spread(rng, fuzz_banks.events(rng, bank, 2 * k), k)
    segs = [(int(rng.integers(60, 260)), int(rng.choice(FUZZ_BLOCKS)), acts[i]) for i in range(k)]
    return bank, segs, fuzz_banks.COUNT0


def fuzz_case(name):
    def case(ref, Case):
        cat = fuzz_setup(ref)
        bank, segs, count0 = fuzz_plan(FUZZ_SEEDS[name], cat)
        inject_bank(ref, bank, cat, count0)
        c = Case(name, f"fuzzed 64-voice bank, seed {FUZZ_SEEDS[name]} of tests/fuzz_banks.py: every feature at random, FM / AM / "
                       "pan / CZ modulators anywhere in the bank, control actions between the segments")
        for frames, block, acts in segs:
            for a in acts:
                apply_action(ref, a)
            r = c.segment(ref, frames, block, note=" ".join(a.kind for a in acts))
            assert np.isfinite(r[0]).all() and np.isfinite(r[1]).all(), f"{name}: the reference's output is not finite"
        c.save()
    return case


def check_fuzz_coverage():
    """Between them the fuzz fixtures drive all four modulator kinds and all seven CZ modes on voices that sound."""
    import golden_io as gio
    kinds, modes = set(), set()
    for name in FUZZ_SEEDS:
        for seg in gio.load(name).segments:
            b = seg.bank_in
            live = b["voice_amp"] != 0
            for f in ("voice_freq_mod_osc", "voice_amp_mod_osc", "voice_pan_mod_osc"):
                if ((b[f] >= 0) & live).any():
                    kinds.add(f)
            if ((b["voice_cz_mod_osc"] >= 0) & (b["voice_cz_mode"] != 0) & live).any():
                kinds.add("voice_cz_mod_osc")
            modes |= set(int(m) for m in b["voice_cz_mode"][live] if m)
    assert len(kinds) == 4 and modes == set(range(1, 8)), (kinds, modes)


CASES = {
    "c0_0sk": case_c0_0sk,
    "c1_sine_adsr64": case_c1_sine_adsr,
    "c2_mixed_filter64": case_c2_mixed_filter,
    "c2_notamy64": case_c2_notamy,
    "c4_pcm_oneshot": case_c4_pcm,
    "edge_basic": case_edge_basic,
    "edge_mod": case_edge_mod,
    "wav_samples": case_wav_samples,
    "bank256_sum": case_bank256_sum,
    "korg_waves": case_korg_waves,
}
CASES.update({name: fuzz_case(name) for name in FUZZ_SEEDS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--list", action="store_true")
    a = ap.parse_args()
    if a.list:
        print("\n".join(CASES))
        return
    if a.case:
        CASES[a.case](Ref(), Case)
        return
    for name in CASES:   # fresh process per case: synth() has function-static state
        subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], check=True)
    check_fuzz_coverage()   # over the four fuzz fixtures as just written (a run with --case may leave older siblings: not checked)


if __name__ == "__main__":
    main()
