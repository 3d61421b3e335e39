#!/usr/bin/env python3
"""tools/measure_banks.py SCENARIO... -- the one-off measurements quoted in DESIGN.md, reproducible (run on the GPU box).

  kernels    the users of the one-voice kernel at BASELINE sizes (C1/C2, 2^18 / 2^20 banks forced onto it, FM, one-shots)
  crossover  one voice per lane vs two per lane, 32 768 .. 262 144 voices  (SK_FAST2_MIN_VOICES)
  overhead   what the event pairs of the sampled kernel timing cost a small bank per block
  frames     kernel time vs frames per launch on a 4096-voice bank (per-frame cost of a lone wavefront + fixed cost)
  fm         2^20-voice two-operator FM banks (carrier v, modulator v+1)
  noise      2^20-voice banks with w6 voices, specialised vs generic kernel
  live       notes starting / ending every block on a 2^20-voice bank (cost of control)
  patches    2^20-voice banks made by tiling a reference patch (banks.bank_patch: the routings of 3.sk, 37.sk, 1.sk, 7.sk, 18.sk)
  linear     C1 / C2 / C3 with linear interpolation, pools with and without guard samples
  mid        mid-size enveloped banks: which kernel family renders them, steady
  cross      modulators in other 64-voice groups (SKRED_OPT_CROSS_GROUP: the source tape and its pre-pass launches): a 2^20-voice C3
             bank whose voice 0 modulates the amplitude and pan of every voice, 3.sk / 18.sk laid out back to back across group
             edges -- each beside the same routings kept inside the groups
  taps       what voice taps cost (skred_bank_set_taps): 18.sk tiled over 2^20 voices, 512 frames, packed lanes, with 0 and with 64
             taps (voices 0 and 10 -- a source and the carrier it modulates in its own frame -- of 32 copies spread over the bank)
  idle       the free-voice query (skred_bank_find_idle) on c2 banks of 65 536 and 2^20 voices after ten blocks of note traffic: (a) its
             launches between an event pair (every criterion, UNNAMED off and on, max_out 1 024; median and minimum of 50), beside one
             512-frame block of the same bank; (b) what a host does for the same answer without it: skred_bank_download of the bank
             plus the predicate in numpy
  steal      voice stealing on a 2^20-voice c2 bank whose polyphony is used up but for 64 idle voices, a burst of 256 notes: (a)
             skred_bank_note_on_steal between an event pair (median, minimum and maximum of 12; nothing is waited for); (b) the only
             way without it: skred_bank_download of the bank, the victim order in numpy, skred_bank_update -- host-held time, and the
             stream time of the update alone; (c) skred_bank_find_steal alone at max_out 0 (its first launch), 16 and 1 024
  cz         CZ phase distortion on the one-voice kernel (SKRED_OPT_CZ_FAST): one 512-frame block at 2^20 and 2^16 voices of (a) the C2
             recipe with `c1,0.5` on every voice, (b) a three-voice group shaped like 42.sk's v0-v2 (`v0 c1,0.5 C2,0.5 F1,1`, v1 and
             v2 `m1` modulators above it) tiled over the bank, each with the option 0 and 1.  Run from a directory that holds an
             older build of the package, it times option 0 only: the baseline
  fxlive     note-ons on the FIXED-POINT bank: 256 notes on a 2^20-voice fxbank.bank_fx bank with 64 idle voices ahead of every burst
             (medians of 12): (a) skred_fxbank_note_on_idle between an event pair -- stream time, and the time the call held the host;
             (b) the only route without it: skred_fxbank_download of the bank, picking on the CPU, skred_fxbank_upload of those voices,
             skred_fxbank_stamp -- host-held time and the stream time of upload + stamp; beside one 512-frame block of the bank
  fxowners   note-off by tag on the FIXED-POINT bank (release_tags) beside the read-back-and-map route; fxctl: a bank-wide cutoff
             change through ctl_range beside host-view writes + skred_fxbank_update, and ctl_list on 256 entries
  expr       channels and per-note expression on bank_patch("3sk", 2^20) tagged over 16 channels (medians of 12): ctl_match of one
             channel beside ctl_range of the range and beside download_owners + numpy pick + list upload + ctl_slots; stamp_match
             beside that route ending in stamp_slots; 256 bends through one ctl_tags_each beside 256 ctl_owned calls; the 64-frame
             block after a filter-only ctl_match beside the steady block
  fxexpr     the same on the FIXED-POINT bank: fxbank.bank_fx, 2^20 voices all sounding, tagged over 16 channels (medians of 12 with
             minimum and maximum): ctl_match of one channel beside download_owners + numpy pick + list upload + ctl_list; stamp_match
             beside that route ending in stamp_list; 256 bends through one ctl_tags_each beside 256 ctl_owned calls; the 64-frame
             block after the ctl_match beside the steady block
  fxsteal    voice stealing on the FIXED-POINT bank: 2^20 voices of fxbank.bank_fx whose polyphony is used up but for 64 idle voices,
             a burst of 256 notes (medians of 12 with minimum and maximum): (a) skred_fxbank_note_on_steal between an event pair --
             stream time, and the time the call held the host; nothing is waited for; (b) the only route without it:
             skred_fxbank_download of the bank, the idle pick and the victim order in numpy, skred_fxbank_upload of the chosen voices,
             skred_fxbank_stamp -- host-held time and the stream time of upload + stamp; (c) skred_fxbank_find_steal alone at max_out
             0 (its first launch), 16 and 1 024
  slots      patch notes: 256 notes on bank_patch("3sk", 2^20) with the three carriers of every copy enveloped and 600 copies at rest
             (medians of 12 with minimum and maximum): (a) skred_bank_note_on_idle_slots -- stream time between an event pair and
             the time the call held the host; (b) skred_bank_find_idle_host, the grouping of its voices into copies in numpy,
             skred_bank_update of the chosen copies' voices; (c) skred_bank_download, the predicate and the grouping in numpy,
             skred_bank_update -- (b) and (c): the time the route held the host

Each line: ms per block over the timed blocks (wall clock), voice-samples/s, and the render kernel's duration from the
library's own event pair around the latest bracketed launch (a bracketed launch runs alone).  kernels / fm / noise print
every bank once (round 1 printed two forms, with and without SKRED_OPT_OVERLAP_TAIL; a block is one launch now).
"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from skred_amd import banks, device  # noqa: E402


def run(name, bank, tables, g, interp=0, F=512, steps=60, min2=None, generic=False, overlap=None, timing=4, cross=False, taps=None, cz_fast=None):
    n = bank.n
    out = torch.zeros(F, 2, device="cuda")
    db = device.DeviceBank(n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    db.set_cross_group(cross)
    if cz_fast is not None:
        db.set_cz_fast(cz_fast)
    if taps is not None and len(taps):
        d_taps = torch.zeros(F, len(taps), 2, device="cuda")
        db.set_taps(taps, d_taps.data_ptr())
    if min2 is not None:
        db.fast2_min_voices(min2)
    db.force_generic(generic)
    db.kernel_timing(timing)
    for _ in range(25):
        db.render_mix(F, out.data_ptr(), 2, 0, interp)
    torch.cuda.synchronize()
    # spin-up: a GPU taken from idle needs tens of milliseconds of work before its clocks settle (bench.py: --spinup-ms);
    # then the best of three repetitions (short banks finish a repetition in a few milliseconds)
    t_spin = time.perf_counter()
    while time.perf_counter() - t_spin < 0.04:
        for _ in range(8):
            db.render_mix(F, out.data_ptr(), 2, 0, interp)
        torch.cuda.synchronize()
    best = None
    for _rep in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            db.render_mix(F, out.data_ptr(), 2, 0, interp)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        d_ = (time.perf_counter() - t0) / steps
        if best is None or d_ < best[0]:
            best = (d_, t0, t1)
    dt, t0, t1 = best
    k = f"{db.last_render_ms():.4f}" if timing else "-"
    tape = "  tape sources %d, pre-pass launches %d" % db.last_cross_group() if cross else ""
    if taps is not None:
        tape += f"  taps {db.last_taps()}, lanes per group {db.last_pack()}"
        db.set_taps([], 0)
    if cz_fast is not None:
        tape += f"  cz {int(db.last_cz())}, lanes per group {db.last_pack()}"
    print(f"{name:66s} kernel={db.last_kernel()} {dt * 1e3:.4f} ms/block {n * F / dt:.3e} voice-samples/s  "
          f"render kernel {k} ms  host issue {(t1 - t0) / steps * 1e6:.1f} us{tape}")
    db.close()


def kernels():
    b, t, g = banks.bank_c1(4096); run("c1 4096", b, t, g)
    b, t, g = banks.bank_c1(65536); run("c1 65536", b, t, g)
    b, t, g = banks.bank_c2(65536); run("c2 65536", b, t, g)
    b, t, g = banks.bank_c2(1 << 18); run("c2 2^18 two per lane", b, t, g, min2=1)
    b, t, g = banks.bank_c2(1 << 18); run("c2 2^18 one per lane", b, t, g, min2=1 << 30)
    b, t, g = banks.bank_c2(1 << 20); run("c2 2^20 one per lane", b, t, g, min2=1 << 30)
    b, t, g = banks.bank_c2(1 << 20)
    car = np.arange(0, 1 << 20, 8); b["voice_freq_mod_osc"][car] = car + 3; b["voice_freq_mod_depth"][car] = 0.2
    run("c2 2^20 FM (1/8 carriers)", b, t, g)
    b, t, g = banks.bank_c2(1 << 20)
    b["voice_one_shot"][::3] = 1; b["voice_loop_enabled"][::3] = 0
    run("c2 2^20 one-shots (1/3, finished after warm-up)", b, t, g)
    b, t, g = banks.bank_c2(1 << 20); run("c3 2^20 two per lane", b, t, g)
    b, t, g = banks.bank_c2(1 << 17)
    run("c3 131072 one per lane: the 8-GPU strong-scaling shard, event pairs on every 4th launch", b, t, g, min2=1 << 30, steps=200)
    run("c3 131072 one per lane: the 8-GPU strong-scaling shard, no event pairs", b, t, g, min2=1 << 30, steps=200, timing=0)
    b, t, g = banks.bank_c4(262144); run("c4 262144 linear", b, t, g, interp=1)
    b, t, g = banks.bank_c4(262144)
    b["voice_one_shot"][::3] = 1; b["voice_loop_enabled"][::3] = 0
    run("c4 262144 linear, one-shots (1/3, finished)", b, t, g, interp=1)
    b, t, g = banks.bank_c4(262144)
    b["voice_sample_hold_max"][::16] = 4
    run("c4 262144 linear, sample & hold on 1/16", b, t, g, interp=1)


def crossover():
    for rec in ("c1", "c2"):
        for n in (32768, 65536, 131072, 196608, 262144):
            b, t, g = banks.RECIPES[rec](n)
            run(f"{rec} {n} one per lane", b, t, g, min2=1 << 30, overlap=True)
            run(f"{rec} {n} two per lane", b, t, g, min2=1, overlap=True)


def overhead():
    for n in (4096, 65536):
        b, t, g = banks.bank_c1(n)
        run(f"c1 {n} an event pair on every 4th launch", b, t, g, steps=200)
        run(f"c1 {n} no event pairs", b, t, g, steps=200, timing=0)


def frames():
    for rec in ("c1", "c2"):
        for F in (64, 256, 512, 2048):
            b, t, g = banks.RECIPES[rec](4096)
            run(f"{rec} 4096 F={F}", b, t, g, F=F, steps=100, timing=1, overlap=True)


def fm():
    for rec in ("c1", "c2"):
        for mute in (False, True):
            b, t, g = banks.RECIPES[rec](1 << 20)
            car = np.arange(0, 1 << 20, 2)
            b["voice_freq_mod_osc"][car] = car + 1
            b["voice_freq_mod_depth"][car] = 0.2
            if mute:
                b["voice_disconnect"][car + 1] = 1
            run(f"{rec} 2^20 two-operator FM" + (", modulators muted (m1)" if mute else ""), b, t, g, steps=40)
    b, t, g = banks.bank_c2(1 << 20)
    car = np.arange(0, 1 << 20, 2)
    b["voice_pan_mod_osc"][car] = car + 1
    b["voice_pan_mod_depth"][car] = 0.5
    b["voice_disconnect"][car + 1] = 1
    run("c2 2^20 pan modulated by the next voice (P1 / m1)", b, t, g, steps=40)
    b["voice_freq_mod_osc"][car] = car + 1
    b["voice_freq_mod_depth"][car] = 0.2
    run("c2 2^20 two-operator FM + pan modulation (F1 P1 / m1)", b, t, g, steps=40)


def noise():
    n = 1 << 20
    for frac, label in ((0.05, "5% noise voices, scattered"), (0.0, "noise voices in the last 1/16 of the bank")):
        b, t, g = banks.bank_c2(n)
        v = np.arange(n)
        if frac:
            b["voice_wave_table_index"][(v * 2654435761 % 1000) < frac * 1000] = 6
        else:
            b["voice_wave_table_index"][n - n // 16:] = 6
        run("c2 2^20 " + label, b, t, g, steps=30)
        run("c2 2^20 " + label + " (generic kernel)", b, t, g, steps=30, generic=True)


def patches():
    for p in ("3sk", "37sk", "1sk", "7sk", "18sk"):
        b, t, g = banks.bank_patch(p, 1 << 20)
        run(f"patch {p} tiled over 2^20 voices", b, t, g, steps=20)


def straddle(patch, n, stride, offset):
    """`patch` laid out back to back: a copy every `stride` voices from `offset` on (copies straddle the 64-voice groups)."""
    one, t, g = banks.bank_patch(patch, 64)
    used = np.where((one["voice_amp"] != 0) & (one["voice_table_size"] > 0))[0]
    K = int(used.max()) + 1
    b = banks.VoiceBank(n)
    for c in range((n - offset) // stride):
        o = offset + c * stride
        if o + K > n:
            break
        for name in b.a:
            b.a[name][o:o + K] = one.a[name][:K]
        for f in ("voice_freq_mod_osc", "voice_amp_mod_osc", "voice_pan_mod_osc", "voice_cz_mod_osc"):
            m = one.a[f][:K]
            b.a[f][o:o + K] = np.where(m >= 0, m + o, m)
    return b, t, g


def cross():
    n = 1 << 20
    for label, src in (("voice 0 of the bank", lambda v: np.zeros_like(v)), ("voice 0 of each voice's own group", lambda v: v & ~63)):
        b, t, g = banks.bank_c2(n)
        v = np.arange(n)
        s = src(v)
        keep = v != s
        b["voice_phase_inc"][s[keep]] = np.float32(0.37)
        b["voice_amp_mod_osc"][keep], b["voice_amp_mod_depth"][keep] = s[keep], np.float32(0.8)
        b["voice_pan_mod_osc"][keep], b["voice_pan_mod_depth"][keep] = s[keep], np.float32(0.5)
        run(f"c3 2^20, AM + pan from {label}", b, t, g, steps=20, cross=True)
    # (18.sk at multiples of 4: a group edge never falls between its voices 0 and 1 or 1 and 2, which would make a cycle)
    for p, stride, offset in (("3sk", 13, 5), ("18sk", 12, 4)):
        b, t, g = straddle(p, n, stride, offset)
        run(f"patch {p} every {stride} voices from {offset} (across group edges)", b, t, g, steps=20, cross=True)
        b, t, g = banks.bank_patch(p, n)
        run(f"patch {p} tiled over 2^20 voices (inside the groups)", b, t, g, steps=20, cross=True)


def taps():
    n = 1 << 20
    b, t, g = banks.bank_patch("18sk", n)
    copies = (np.arange(32) * (n // 32) + 7000 * 16) % n                 # 16 voices per copy; the 7 000th copy among them
    ids = np.sort(np.concatenate([copies, copies + 10])).astype(np.int32)
    for _rep in range(2):
        run("patch 18sk tiled over 2^20 voices, no taps", b, t, g, steps=40, taps=[])
        run("patch 18sk tiled over 2^20 voices, 64 taps", b, t, g, steps=40, taps=ids)


def linear():
    for rec, n in (("c1", 4096), ("c2", 65536), ("c2", 1 << 20)):
        b, t, g = banks.RECIPES[rec](n)
        run(f"{rec} {n} truncating lookup", b, t, g, interp=0)
        run(f"{rec} {n} linear, guarded pool (INTERP 2)", b, t, g, interp=1)
        tn = t.copy()
        pos = np.unique(b["voice_table_offset"].astype(np.int64) + b["voice_table_size"].astype(np.int64))
        tn[pos[pos < len(tn)]] = 7.0
        run(f"{rec} {n} linear, pool without guard samples (general form)", b, tn, g, interp=1)


def mid():
    for n in (196608, 229376, 262144, 294912, 327680, 360448, 393216, 458752, 524288):
        b, t, g = banks.bank_c2(n)
        run(f"c2 {n} library's choice", b, t, g, steps=100)
        run(f"c2 {n} one per lane", b, t, g, min2=1 << 30, steps=100)
        run(f"c2 {n} two per lane", b, t, g, min2=1, steps=100)


def live():
    D = device
    n, F = 1 << 20, 512
    out = torch.zeros(F, 2, device="cuda")
    bank, tables, g = banks.bank_c2(n)
    db = device.DeviceBank(n)
    db.set_tables(tables)
    db.upload(bank)
    db.set_globals(g)
    db.kernel_timing(0)
    for _ in range(30):
        db.render_mix(F, out.data_ptr(), 2)
    rng = np.random.default_rng(1)
    for frac in (0.0, 0.0001, 0.0005, 0.005, 0.02):
        k = int(n * frac)
        res = {}
        for mode in ("stream", "sync"):          # blocks queued back to back (what bench.py's live_control times) / a host that waits for every block
            for _rep in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(60):
                    if k:
                        vs = rng.choice(n, k, replace=False).astype(np.int32)
                        db.update(bank, vs[:k // 2], D.STAMP_RELEASE)
                        db.update(bank, vs[k // 2:], D.STAMP_TRIGGER | D.DIRTY_PHASE | D.DIRTY_PARAMS)
                    db.render_mix(F, out.data_ptr(), 2)
                    if mode == "sync":
                        torch.cuda.synchronize()
                torch.cuda.synchronize()
                res[mode] = (time.perf_counter() - t0) / 60
        print(f"{frac * 100:.2f} % of the voices get a note-off / note-on per block: {res['stream'] * 1e3:.3f} ms/block queued back to back "
              f"({n * F / res['stream']:.3e} voice-samples/s), {res['sync'] * 1e3:.3f} ms/block when the host waits for every block"
              f"   [motion list {'in place' if db.last_in_place() else 'by the envelope kernel' if k else '-'}]")
    db.close()


def idle():
    D = device
    F, M = 512, 1024
    for n in (65536, 1 << 20):
        bank, tables, g = banks.bank_c2(n)
        bank["voice_amp_envelope"]["release_time"] = np.float32(300.0)
        db = device.DeviceBank(n)
        db.set_tables(tables); db.upload(bank); db.set_globals(g); db.kernel_timing(1)
        out = torch.zeros(F, 2, device="cuda")
        rng = np.random.default_rng(1)
        for _ in range(10):
            vs = rng.choice(n, n // 8, replace=False).astype(np.int32)
            db.update(bank, vs, D.STAMP_RELEASE)
            db.render_mix(F, out.data_ptr(), 2)
        torch.cuda.synchronize()
        block_ms = db.last_render_ms()
        dv = torch.full((M,), -1, dtype=torch.int32, device="cuda")
        dc = torch.zeros(2, dtype=torch.int32, device="cuda")
        crit = D.IDLE_FINISHED | D.IDLE_ENV_DONE | D.IDLE_AMP_ZERO
        for label, which, planes in (("UNNAMED off", crit, 4), ("UNNAMED on", crit | D.IDLE_UNNAMED, 4)):
            for _ in range(5):
                db.find_idle(0, n, which, 1e-3, n // 2, M, dv.data_ptr(), dc.data_ptr())
            torch.cuda.synchronize()
            ms = []
            for _ in range(50):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                db.find_idle(0, n, which, 1e-3, n // 2, M, dv.data_ptr(), dc.data_ptr())
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med, mn = float(np.median(ms)), float(np.min(ms))
            req = 2 * planes * 16 * n                            # both launches sweep the range; a word costs its 16-byte plane entry
            print(f"c2 {n} find_idle, every criterion, {label}, max_out {M}: median {med:.4f} ms, min {mn:.4f} ms for count + scatter "
                  f"(total idle {int(dc[1])}, written {int(dc[0])}); {2 * planes * 16} B requested per voice over both launches = "
                  f"{req / (mn * 1e-3) / 1e12:.3f} TB/s at the minimum ({req / (mn * 1e-3) / 8e12 * 100:.1f} % of the 8 TB/s HBM peak); "
                  f"one {F}-frame block of this bank: {block_ms:.4f} ms")
        got = bank.copy()
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            db.download(got)
            a, e = got.a, got.a["voice_amp_envelope"]
            lst = np.flatnonzero((a["voice_finished"] != 0) | (a["voice_amp"] == 0) |
                                 ((a["voice_use_amp_envelope"] != 0) & (e["is_active"] == 0) &
                                  ((a["voice_smoother_enable"] == 0) | (np.abs(a["voice_smoother_gain"]) <= np.float32(1e-3)))))
            ts.append(time.perf_counter() - t0)
        print(f"c2 {n} the same answer on the host: skred_bank_download of the bank + the predicate in numpy: best of 3 {min(ts) * 1e3:.3f} ms "
              f"({len(lst)} idle voices)")
        t0 = time.perf_counter()
        for _ in range(20):
            db.find_idle_host(0, n, crit, 1e-3, n // 2, M)
        print(f"c2 {n} find_idle_host (launches, copy of {M} entries, stream synchronise): {(time.perf_counter() - t0) / 20 * 1e3:.4f} ms per call")
        db.close()


def steal():
    D = device
    n, F, K, IDLE = 1 << 20, 512, 256, 64
    bank, tables, g = banks.bank_c2(n)
    db = device.DeviceBank(n)
    db.set_tables(tables); db.upload(bank); db.set_globals(g); db.kernel_timing(1)
    out = torch.zeros(F, 2, device="cuda")
    for _ in range(3):
        db.render_mix(F, out.data_ptr(), 2)
    torch.cuda.synchronize()
    block_ms = db.last_render_ms()
    free = (np.arange(IDLE, dtype=np.int32) * 16381 + 5) % n           # the 64 voices that are idle ahead of every burst
    rest = bank.copy()
    rest["voice_amp_envelope"]["is_active"][free] = 0
    rest["voice_smoother_gain"][free] = 0.0
    which = D.IDLE_FINISHED | D.IDLE_ENV_DONE
    notes = D.note_array([D.NoteC(0.4 + 0.001 * k, 0.8, 0.0, 0.5, 0.5, D.NOTE_SET_PHASE) for k in range(K)])
    iq = D.IdleQueryC(0, n, which, 1e-3, 0, 0)
    sq = D.steal_query(0, n, D.STEAL_OLDEST, D.STEAL_RELEASED_FIRST, 64)
    da = torch.full((K,), -1, dtype=torch.int32, device="cuda")
    dr = torch.zeros(3, dtype=torch.int32, device="cuda")

    def make_idle():
        db.update(rest, free, D.DIRTY_ENV_STATE | D.DIRTY_SMOOTHER)
        torch.cuda.synchronize()

    ms = []
    for it in range(3 + 12):                                             # three warm-up bursts, then the twelve that count
        make_idle()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        db.note_on_steal(notes, iq, sq, da.data_ptr(), dr.data_ptr())
        e1.record()
        e1.synchronize()
        if it >= 3:
            ms.append(e0.elapsed_time(e1))
    res = dr.cpu().numpy().tolist()
    print(f"c2 {n} note_on_steal, {K} notes, {IDLE} idle voices, OLDEST | RELEASED_FIRST, min_age 64: stream time median {np.median(ms):.4f} ms, "
          f"min {np.min(ms):.4f}, max {np.max(ms):.4f} of {len(ms)} (placed, dropped, stolen = {res}); nothing waited for; "
          f"one {F}-frame block of this bank: {block_ms:.4f} ms")
    got = bank.copy()
    held, upd = [], []
    for it in range(2 + 12):
        make_idle()
        t0 = time.perf_counter()
        db.download(got)
        a, e = got.a, got.a["voice_amp_envelope"]
        now = int(db.get_globals().synth_sample_count)
        idle = np.flatnonzero((a["voice_finished"] != 0) | ((a["voice_use_amp_envelope"] != 0) & (e["is_active"] == 0) &
                              ((a["voice_smoother_enable"] == 0) | (np.abs(a["voice_smoother_gain"]) <= np.float32(1e-3)))))[:K]
        start, release = bank["voice_amp_envelope"]["sample_start"], bank["voice_amp_envelope"]["sample_release"]   # (the host's own clocks)
        cand = (a["voice_use_amp_envelope"] != 0) & (e["is_active"] != 0) & (np.uint64(now) - np.minimum(start, np.uint64(now)) >= np.uint64(64))
        cand[idle] = False
        key = np.where(release != 0, release, start | np.uint64(1 << 62))
        c = np.flatnonzero(cand)
        part = c[np.argpartition(key[c], K)[:K]] if len(c) > K else c
        victims = part[np.lexsort((part, key[part]))]
        picks = np.concatenate([idle, victims])[:K].astype(np.int32)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        db.update(bank, picks, D.DIRTY_PARAMS | D.DIRTY_PHASE | D.STAMP_TRIGGER)
        e1.record()
        dt = time.perf_counter() - t0
        e1.synchronize()
        if it >= 2:
            held.append(dt * 1e3)
            upd.append(e0.elapsed_time(e1))
    print(f"c2 {n} the same notes without it: skred_bank_download of the bank (waits for the device) + the victim order in numpy + "
          f"skred_bank_update of {len(picks)} voices: host held median {np.median(held):.3f} ms, min {np.min(held):.3f}, max {np.max(held):.3f} "
          f"of {len(held)}; the update's stream time median {np.median(upd):.4f} ms")
    dv = torch.full((D.STEAL_MAX,), -1, dtype=torch.int32, device="cuda")
    dc = torch.zeros(2, dtype=torch.int32, device="cuda")
    for m in (0, 16, D.STEAL_MAX):
        q = D.steal_query(0, n, D.STEAL_OLDEST, D.STEAL_RELEASED_FIRST, 64, which, 1e-3, m)
        ms = []
        for it in range(3 + 12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            db.find_steal(q, dv.data_ptr(), dc.data_ptr())
            e1.record()
            e1.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        print(f"c2 {n} find_steal alone, max_out {m}: stream time median {np.median(ms):.4f} ms, min {np.min(ms):.4f}, max {np.max(ms):.4f} "
              f"of {len(ms)} (candidates {int(dc[1])}, written {int(dc[0])})")
    db.close()


def cz_banks(n):
    """(a) C2 with `c1,0.5` everywhere; (b) 42.sk's v0-v2 as a triple -- carrier, FM modulator, CZ source, the two `m1` -- 21 times per
    64-voice group (lane 63 silent)."""
    b, t, g = banks.bank_c2(n)
    b["voice_cz_mod_osc"] = -1
    b["voice_cz_mode"] = 1
    b["voice_cz_distortion"] = 0.5
    yield "c2 + c1,0.5 on every voice", b, t, g
    b, t, g = banks.bank_c2(n)
    v = np.arange(n)
    lane = v % 64
    role = np.where(lane < 63, lane % 3, 3)                # 0 carrier, 1 / 2 its modulators, 3 unused
    car = role == 0
    b["voice_cz_mod_osc"] = np.where(car, v + 2, -1).astype(np.int32)
    b["voice_cz_mod_depth"] = 0.5
    b["voice_cz_mode"] = car.astype(np.int32)
    b["voice_cz_distortion"] = 0.5
    b["voice_freq_mod_osc"] = np.where(car, v + 1, -1).astype(np.int32)
    b["voice_freq_mod_depth"] = 1.0
    b["voice_disconnect"] = ((role == 1) | (role == 2)).astype(np.int32)
    b["voice_amp"] = np.where(role == 3, 0.0, 1.0).astype(np.float32)
    yield "42.sk v0-v2 (c1,0.5 C2,0.5 F1,1; two m1 modulators) tiled", b, t, g


def cz():
    has_opt = hasattr(device.DeviceBank, "set_cz_fast")   # (an older build of the package: option 0 only -- the baseline)
    for n in (1 << 20, 1 << 16):
        for name, b, t, g in cz_banks(n):
            for opt in ((0, 1) if has_opt else (None,)):
                run(f"{n} {name}, option {'-' if opt is None else opt}", b, t, g, steps=30 if n > 100000 else 60, cz_fast=opt)


def fxlive():
    from skred_amd import fxbank as X
    n, F, K, IDLE = 1 << 20, 512, 256, 64
    bank, pool, c0 = X.bank_fx(n)
    db = X.DeviceFxBank(n)
    db.set_tables(pool); db.upload(bank); db.set_sample_count(c0)
    out = torch.zeros(F, 2, dtype=torch.int64, device="cuda")
    for _ in range(3):
        db.render_mix(F, out.data_ptr(), 1)
    torch.cuda.synchronize()
    block_ms = db.last_render_ms()
    free = ((np.arange(IDLE, dtype=np.int64) * 16381 + 5) % n).astype(np.int32)   # the 64 voices that are idle ahead of every burst
    rest = bank.copy()
    rest["is_active"][free] = 0
    rest["smoother_gain_q15"][free] = 0
    which = X.IDLE_FINISHED | X.IDLE_ENV_DONE
    notes = X.fx_note_array([X.FxNoteC(3000017 + 40009 * k, 26000, 0, 16384, 16384, X.NOTE_SET_PHASE) for k in range(K)])
    da = torch.full((K,), -1, dtype=torch.int32, device="cuda")
    dr = torch.zeros(2, dtype=torch.int32, device="cuda")

    def make_idle():
        db.update(rest, free, X.DIRTY_ENV_STATE | X.DIRTY_SMOOTHER)
        torch.cuda.synchronize()

    ms, held = [], []
    for it in range(3 + 12):                                             # three warm-up bursts, then the twelve that count
        make_idle()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        db.note_on_idle(notes, 0, n, which, 0, 0, da.data_ptr(), dr.data_ptr())
        dt = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        if it >= 3:
            ms.append(e0.elapsed_time(e1))
            held.append(dt * 1e3)
    res = dr.cpu().numpy().tolist()
    print(f"fx {n} note_on_idle, {K} notes, {IDLE} idle voices: stream time median {np.median(ms):.4f} ms, min {np.min(ms):.4f}, "
          f"max {np.max(ms):.4f} of {len(ms)}; host held median {np.median(held):.4f} ms, max {np.max(held):.4f} (placed, dropped = {res}); "
          f"nothing waited for; one {F}-frame block of this bank: {block_ms:.4f} ms")
    got = bank.copy()
    held, upd = [], []
    for it in range(2 + 12):
        make_idle()
        t0 = time.perf_counter()
        db.download(got)
        a = got.a
        picks = np.flatnonzero((a["finished"] != 0) | ((a["use_envelope"] != 0) & (a["is_active"] == 0) &
                               ((a["smoother_enable"] == 0) | (a["smoother_gain_q15"] == 0))))[:K].astype(np.int32)
        for k, v in enumerate(picks):                                    # the notes' values into the host view
            got["phase_inc"][v], got["velocity_q15"][v], got["phase"][v], got["finished"][v] = notes[k].phase_inc, notes[k].velocity_q15, 0, 0
        cb = got.as_c()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for v in picks:                                                  # (upload takes windows: one call per voice)
            X._check(db.L.skred_fxbank_upload(db.h, cb, int(v), int(v), 1), "skred_fxbank_upload")
        db.stamp(picks, X.FX_STAMP_TRIGGER)
        e1.record()
        dt = time.perf_counter() - t0
        e1.synchronize()
        if it >= 2:
            held.append(dt * 1e3)
            upd.append(e0.elapsed_time(e1))
    print(f"fx {n} the same notes without it: skred_fxbank_download of the bank (waits for the device) + the pick in numpy + "
          f"skred_fxbank_upload of {len(picks)} voices + skred_fxbank_stamp: host held median {np.median(held):.3f} ms, min {np.min(held):.3f}, "
          f"max {np.max(held):.3f} of {len(held)}; upload + stamp between the events: median {np.median(upd):.4f} ms")
    db.close()


def fxsteal():
    from skred_amd import fxbank as X
    n, F, K, IDLE = 1 << 20, 512, 256, 64
    bank, pool, c0 = X.bank_fx(n)
    db = X.DeviceFxBank(n)
    db.set_tables(pool); db.upload(bank); db.set_sample_count(c0)
    out = torch.zeros(F, 2, dtype=torch.int64, device="cuda")
    for _ in range(3):
        db.render_mix(F, out.data_ptr(), 1)
    torch.cuda.synchronize()
    block_ms = db.last_render_ms()
    now = db.sample_count()
    free = ((np.arange(IDLE, dtype=np.int64) * 16381 + 5) % n).astype(np.int32)   # the 64 voices that are idle ahead of every burst
    rest = bank.copy()
    rest["is_active"][free] = 0
    rest["smoother_gain_q15"][free] = 0
    which = X.IDLE_FINISHED | X.IDLE_ENV_DONE
    released = ((np.arange(4096, dtype=np.int64) * 257 + 11) % n).astype(np.int32)   # some voices in release: both classes occur
    db.stamp(released, X.FX_STAMP_RELEASE)
    notes = X.fx_note_array([X.FxNoteC(3000017 + 40009 * k, 26000, 0, 16384, 16384, X.NOTE_SET_PHASE) for k in range(K)])
    da = torch.full((K,), -1, dtype=torch.int32, device="cuda")
    dr = torch.zeros(3, dtype=torch.int32, device="cuda")
    iq = X.FxIdleQueryC(0, n, which, 0, 0, 0)
    sq = X.fx_steal_query(0, n, X.STEAL_OLDEST, X.STEAL_RELEASED_FIRST, 64)

    def make_idle():
        db.update(rest, free, X.DIRTY_ENV_STATE | X.DIRTY_SMOOTHER)
        torch.cuda.synchronize()

    ms, held = [], []
    for it in range(3 + 12):                                             # three warm-up bursts, then the twelve that count
        make_idle()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        db.note_on_steal(notes, iq, sq, da.data_ptr(), dr.data_ptr())
        dt = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        if it >= 3:
            ms.append(e0.elapsed_time(e1))
            held.append(dt * 1e3)
    res = dr.cpu().numpy().tolist()
    print(f"fx {n} note_on_steal, {K} notes, {IDLE} idle voices, OLDEST | RELEASED_FIRST, min_age 64: stream time median {np.median(ms):.4f} ms, "
          f"min {np.min(ms):.4f}, max {np.max(ms):.4f} of {len(ms)}; host held median {np.median(held):.4f} ms, max {np.max(held):.4f} "
          f"(placed, dropped, on stolen voices = {res}); nothing waited for; one {F}-frame block of this bank: {block_ms:.4f} ms")
    got = bank.copy()
    held, upd = [], []
    for it in range(2 + 12):
        make_idle()
        t0 = time.perf_counter()
        db.download(got)                                                 # (the read-write fields; the clocks are the host's own record)
        a = got.a
        idle = (a["finished"] != 0) | ((a["use_envelope"] != 0) & (a["is_active"] == 0) & ((a["smoother_enable"] == 0) | (a["smoother_gain_q15"] == 0)))
        start, release = a["sample_start"], a["sample_release"]
        cand = (a["use_envelope"] != 0) & (a["is_active"] != 0) & ~idle & (np.uint64(now) - np.minimum(start, np.uint64(now)) >= 64)
        key = np.where(release != 0, release, start | np.uint64(1 << 62))
        v = np.flatnonzero(cand)
        order = v[np.lexsort((v, key[v]))]
        picks = np.concatenate([np.flatnonzero(idle), order])[:K].astype(np.int32)
        for k, v in enumerate(picks):                                    # the notes' values into the host view
            got["phase_inc"][v], got["velocity_q15"][v], got["phase"][v], got["finished"][v] = notes[k].phase_inc, notes[k].velocity_q15, 0, 0
        cb = got.as_c()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for v in picks:                                                  # (upload takes windows: one call per voice)
            X._check(db.L.skred_fxbank_upload(db.h, cb, int(v), int(v), 1), "skred_fxbank_upload")
        db.stamp(picks, X.FX_STAMP_TRIGGER)
        e1.record()
        dt = time.perf_counter() - t0
        e1.synchronize()
        if it >= 2:
            held.append(dt * 1e3)
            upd.append(e0.elapsed_time(e1))
    print(f"fx {n} the same notes without it: skred_fxbank_download of the bank (waits for the device) + the idle pick and the victim "
          f"order in numpy + skred_fxbank_upload of {len(picks)} voices + skred_fxbank_stamp: host held median {np.median(held):.3f} ms, "
          f"min {np.min(held):.3f}, max {np.max(held):.3f} of {len(held)}; upload + stamp between the events: median {np.median(upd):.4f} ms")
    dv = torch.full((X.STEAL_MAX,), -1, dtype=torch.int32, device="cuda")
    dc = torch.zeros(2, dtype=torch.int32, device="cuda")
    for max_out in (0, 16, X.STEAL_MAX):
        q = X.fx_steal_query(0, n, X.STEAL_OLDEST, X.STEAL_RELEASED_FIRST, 64, which, 0, max_out)
        ms = []
        for it in range(3 + 12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            db.find_steal(q, dv.data_ptr(), dc.data_ptr())
            e1.record()
            e1.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        print(f"fx {n} find_steal alone, max_out {max_out}: stream time median {np.median(ms):.4f} ms, min {np.min(ms):.4f}, max {np.max(ms):.4f} "
              f"of {len(ms)} (written, total = {dc.cpu().numpy().tolist()})")
    db.close()


def slots():
    """256 patch notes on bank_patch("3sk", 2**20) -- the three carriers of every copy enveloped, a few hundred copies at rest -- through
    skred_bank_note_on_idle_slots, against the two routes a host had before it: find_idle_host + grouping in numpy + skred_bank_update,
    and skred_bank_download + the predicate and the grouping in numpy + skred_bank_update.  Medians of 12."""
    D = device
    n, K, NOTES, REST, REPS = 1 << 20, 4, 256, 600, 12
    MEMBERS, VOICES = 0x7, 0xF                                # the enveloped carriers; a note re-pitches the shared modulator too
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    lane = np.arange(n) % K
    sel = lane < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 100.0
    e["velocity"][sel], e["is_active"][sel], e["sample_start"][sel] = 1.0, 1, np.uint64(now - 40000)
    rng = np.random.default_rng(3)
    rest = np.sort(rng.choice(n // K, REST, replace=False)) * K
    for l in range(3):
        e["is_active"][rest + l] = 0                          # at rest: envelope over, smoother gain exactly 0
    db = device.DeviceBank(n)
    db.set_tables(tables); db.set_globals(g)
    which = D.IDLE_ENV_DONE
    q = D.slot_query(0, n, K, MEMBERS, which, 1e-3, n // 2, NOTES)
    notes = D.note_array([D.NoteC(0.4 + 0.001 * i, 0.8, 0.0, 0.5, 0.5, D.NOTE_SET_PHASE) for i in range(NOTES * K)])
    da = torch.full((NOTES,), -1, dtype=torch.int32, device="cuda")
    dr = torch.zeros(2, dtype=torch.int32, device="cuda")
    mirror = bank.copy()
    dirty = D.DIRTY_PARAMS | D.DIRTY_PHASE | D.STAMP_TRIGGER
    inc = np.array([t.phase_inc for t in notes], np.float32).reshape(NOTES, K)

    def place_on_host(picks):
        vs = (picks[:, None] + np.arange(K)[None, :]).astype(np.int32)
        mirror["voice_phase_inc"][vs] = inc[:len(picks)]
        mirror["voice_amp_envelope"]["velocity"][vs] = np.float32(0.8)
        mirror["voice_phase"][vs] = 0.0
        mirror["voice_finished"][vs] = 0
        db.update(mirror, vs.reshape(-1), dirty)

    def group(idle_voices):
        s, c = np.unique(idle_voices[(idle_voices % K) < 3] // K, return_counts=True)
        free = s[c == 3] * K
        k = int(np.searchsorted(free, n // 2))
        return np.concatenate([free[k:], free[:k]])[:NOTES]

    def device_route():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        db.note_on_idle_slots(notes, q, VOICES, da.data_ptr(), dr.data_ptr())
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1), dr.cpu().numpy().tolist()

    def list_route():
        t0 = time.perf_counter()
        voices, total = db.find_idle_host(0, n, which, 1e-3, None, 8192)
        assert total <= 8192
        picks = group(voices)
        place_on_host(picks)
        return (time.perf_counter() - t0) * 1e3, None, [len(picks), NOTES - len(picks)]

    got = bank.copy()

    def download_route():
        t0 = time.perf_counter()
        db.download(got)
        a, env = got.a, got.a["voice_amp_envelope"]
        idle = np.flatnonzero((a["voice_use_amp_envelope"] != 0) & (env["is_active"] == 0) &
                              ((a["voice_smoother_enable"] == 0) | (np.abs(a["voice_smoother_gain"]) <= np.float32(1e-3))))
        picks = group(idle)
        place_on_host(picks)
        return (time.perf_counter() - t0) * 1e3, None, [len(picks), NOTES - len(picks)]

    print(f"3sk {n} voices = {n // K} slots of {K}, {REST} slots at rest, {NOTES} patch notes ({NOTES * K} records), medians of {REPS}")
    for label, route in (("note_on_idle_slots (query + placement on the device)", device_route),
                         ("find_idle_host + grouping in numpy + skred_bank_update", list_route),
                         ("skred_bank_download + predicate and grouping in numpy + skred_bank_update", download_route)):
        host, stream, res = [], [], None
        for it in range(2 + REPS):
            db.upload(bank)
            torch.cuda.synchronize()
            h, s_ms, res = route()
            torch.cuda.synchronize()
            if it >= 2:
                host.append(h)
                if s_ms is not None:
                    stream.append(s_ms)
        line = f"  {label}: host time median {np.median(host):.4f} ms (min {np.min(host):.4f}, max {np.max(host):.4f})"
        if stream:
            line += f"; stream time between events median {np.median(stream):.4f} ms (min {np.min(stream):.4f}, max {np.max(stream):.4f})"
        print(line + f"; placed, dropped = {res}")
    db.close()


def slotsteal():
    """A burst of 256 patch notes on bank_patch("3sk", 2**20) -- the carriers enveloped, every copy sounding but 64 -- through
    skred_bank_note_on_steal_slots: 64 notes land on idle slots, 192 on stolen ones.  Every repetition uploads the bank and RENDERS a
    block of 64 frames first, so the calls meet the state a running instrument holds (the smoother gains ENV_DONE reads among it).
    The per-voice skred_bank_find_steal at max_out 16 runs on the same bank in the same run, for the comparison of the two key passes.  skred_bank_find_steal_slots alone at max_out 0,
    16 and 1024.  Against the only route a host had before: skred_bank_download + grouping and victim order in numpy +
    skred_bank_update.  Medians of 12 with minimum and maximum, stream events around the device calls."""
    D = device
    n, K, NOTES, REST, REPS = 1 << 20, 4, 256, 64, 12
    MEMBERS, VOICES = 0x7, 0xF
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    v = np.arange(n)
    sel = (v % K) < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 1e6
    e["velocity"][sel], e["is_active"][sel] = 1.0, 1
    e["sample_start"][sel] = (now - 40000 - ((v[sel] // K) * 7919) % 30000 - (v[sel] % K)).astype(np.uint64)   # every copy its own age
    rel = sel & ((v // K) % 3 == 0)
    e["sample_release"][rel] = (now - 2000 + ((v[rel] // K) * 104729) % 1000).astype(np.uint64)             # a third of them in release
    rng = np.random.default_rng(4)
    rest = np.sort(rng.choice(n // K, REST, replace=False)) * K
    for l in range(3):
        e["is_active"][rest + l] = 0
    db = device.DeviceBank(n)
    db.set_tables(tables); db.set_globals(g)
    which = D.IDLE_ENV_DONE
    iq = D.slot_query(0, n, K, MEMBERS, which, 1e-3, 0, NOTES)
    notes = D.note_array([D.NoteC(0.4 + 0.001 * i, 0.8, 0.0, 0.5, 0.5, D.NOTE_SET_PHASE) for i in range(NOTES * K)])
    da = torch.full((NOTES,), -1, dtype=torch.int32, device="cuda")
    dr = torch.zeros(3, dtype=torch.int32, device="cuda")
    dv = torch.full((D.STEAL_MAX,), -1, dtype=torch.int32, device="cuda")
    dc = torch.zeros(2, dtype=torch.int32, device="cuda")
    mirror = bank.copy()
    dirty = D.DIRTY_PARAMS | D.DIRTY_PHASE | D.STAMP_TRIGGER
    inc = np.array([t.phase_inc for t in notes], np.float32).reshape(NOTES, K)

    def sq(max_out):
        return D.slot_steal_query(0, n, K, MEMBERS, D.STEAL_OLDEST, D.STEAL_RELEASED_FIRST, 0, which, 1e-3, max_out)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1)

    def device_route():
        h, s_ms = timed(lambda: db.note_on_steal_slots(notes, iq, sq(0), VOICES, da.data_ptr(), dr.data_ptr()))
        return h, s_ms, dr.cpu().numpy().tolist()

    def query_only(max_out):
        def run():
            h, s_ms = timed(lambda: db.find_steal_slots(sq(max_out), dv.data_ptr(), dc.data_ptr()))
            return h, s_ms, dc.cpu().numpy().tolist()
        return run

    def voice_query():
        vq = D.steal_query(0, n, D.STEAL_OLDEST, D.STEAL_RELEASED_FIRST, 0, which, 1e-3, 16)
        h, s_ms = timed(lambda: db.find_steal(vq, dv.data_ptr(), dc.data_ptr()))
        return h, s_ms, dc.cpu().numpy().tolist()

    block = torch.zeros(64, 2, device="cuda")
    got = bank.copy()
    clocks = bank["voice_amp_envelope"]                       # (download returns the read-write fields; the clocks are the host's own)

    def download_route():
        t0 = time.perf_counter()
        db.download(got)
        a, env = got.a, got.a["voice_amp_envelope"]
        heads = np.arange(0, n, K)
        mv = heads[:, None] + np.arange(3)[None, :]
        use, act = a["voice_use_amp_envelope"][mv] != 0, env["is_active"][mv] != 0
        settled = (a["voice_smoother_enable"][mv] == 0) | (np.abs(a["voice_smoother_gain"][mv]) <= np.float32(1e-3))
        idle = use & ~act & settled
        free = heads[idle.all(1)][:NOTES]
        live = use & act
        rls = clocks["sample_release"][mv]
        allrel = ~(live & (rls == 0)).any(1)
        cand = live.any(1) & ~idle.all(1)
        primary = np.where(live, np.where(allrel[:, None], rls, clocks["sample_start"][mv]), np.uint64(0)).max(1)
        key = (np.where(allrel, 0, 1).astype(np.uint64) << np.uint64(62)) | primary.astype(np.uint64)
        need = NOTES - len(free)
        ch, ck = heads[cand], key[cand]
        part = ck <= np.partition(ck, need - 1)[need - 1] if 0 < need < len(ck) else np.ones(len(ck), bool)   # (ties at the cut: all of them)
        victims = ch[part][np.lexsort((ch[part], ck[part]))][:max(need, 0)]
        picks = np.concatenate([free, victims])[:NOTES]
        vs = (picks[:, None] + np.arange(K)[None, :]).astype(np.int32)
        mirror["voice_phase_inc"][vs] = inc[:len(picks)]
        mirror["voice_amp_envelope"]["velocity"][vs] = np.float32(0.8)
        mirror["voice_phase"][vs] = 0.0
        mirror["voice_finished"][vs] = 0
        db.update(mirror, vs.reshape(-1), dirty)
        return (time.perf_counter() - t0) * 1e3, None, [len(picks), NOTES - len(picks), len(picks) - len(free)]

    print(f"3sk {n} voices = {n // K} slots of {K}, {REST} slots at rest, a block of 64 frames, then a burst of {NOTES} patch notes ({NOTES * K} records), medians of {REPS}")
    for label, route in (("note_on_steal_slots (both queries, append and placement on the device)", device_route),
                         ("find_steal_slots alone, max_out 0 (the key pass)", query_only(0)),
                         ("find_steal_slots alone, max_out 16", query_only(16)),
                         ("find_steal_slots alone, max_out 1024", query_only(1024)),
                         ("find_steal (the per-voice query) on the same bank, max_out 16", voice_query),
                         ("skred_bank_download + grouping and victim order in numpy + skred_bank_update", download_route)):
        host, stream, res = [], [], None
        for it in range(2 + REPS):
            db.upload(bank)
            db.render_mix(64, block.data_ptr(), 2, 0, 0)
            torch.cuda.synchronize()
            h, s_ms, res = route()
            torch.cuda.synchronize()
            if it >= 2:
                host.append(h)
                if s_ms is not None:
                    stream.append(s_ms)
        line = f"  {label}: host time median {np.median(host):.4f} ms (min {np.min(host):.4f}, max {np.max(host):.4f})"
        if stream:
            line += f"; stream time between events median {np.median(stream):.4f} ms (min {np.min(stream):.4f}, max {np.max(stream):.4f})"
        print(line + f"; result words = {res}")
    db.close()


def ctl():
    """A cutoff change on every copy of bank_patch("3sk", 2**20) -- the three carriers of every copy filtered and enveloped -- through
    skred_bank_ctl_range, against the only route before it (host-view writes + skred_bank_update of those voices); ctl_slots on a
    256-slot list; the 64-frame block after the sweep beside the steady block of the same run; the blocks after a bank-wide AMP
    controller (every voice listed) until the block time is back at the steady one.  Medians of 12."""
    D = device
    n, K, REPS, F, LIST = 1 << 20, 4, 12, 64, 256
    CARRIERS = 0x7
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    sel = (np.arange(n) % K) < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 100.0
    e["velocity"][sel], e["is_active"][sel], e["sample_start"][sel] = 1.0, 1, np.uint64(now - 40000)
    co = banks.biquad_coeffs(np.array([1]), np.array([1200.0], np.float32), np.array([1.0], np.float32), 44100)
    bank["voice_filter_mode"][sel] = 1
    for k, v in co.items():
        bank["voice_filter"][k][sel] = v[0]
    db = device.DeviceBank(n)
    db.set_tables(tables); db.upload(bank); db.set_globals(g)
    out = torch.zeros(F, 2, device="cuda")
    dres = torch.zeros(2, dtype=torch.int32, device="cuda")
    dlist = torch.from_numpy((np.random.default_rng(5).choice(n // K, LIST, replace=False) * K).astype(np.int32)).cuda()
    mirror = bank.copy()
    carriers = np.flatnonzero(sel).astype(np.int32)

    def coeffs(i):
        c = banks.biquad_coeffs(np.array([1]), np.array([600.0 + 150.0 * i], np.float32), np.array([1.0], np.float32), 44100)
        return {k: float(v[0]) for k, v in c.items()}

    def sweep(i):
        c = coeffs(i)
        return D.ctl_array([D.ctl(D.CTL_FILTER if l < 3 else 0, **c) for l in range(K)])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        fn()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1)

    def block():
        return timed(lambda: db.render_mix(F, out.data_ptr(), 2, 0, 0))[1]

    def host_route(i):
        c = coeffs(i)
        for k, v in c.items():
            mirror["voice_filter"][k][carriers] = np.float32(v)
        db.update(mirror, carriers, D.DIRTY_PARAMS)

    def show(label, host, stream, extra=""):
        print(f"  {label}: host time median {np.median(host):.4f} ms (min {np.min(host):.4f}, max {np.max(host):.4f}); stream time between "
              f"events median {np.median(stream):.4f} ms (min {np.min(stream):.4f}, max {np.max(stream):.4f}){extra}")

    print(f"3sk {n} voices = {n // K} copies of {K}, carriers filtered and enveloped, {F}-frame blocks, medians of {REPS}")
    for _ in range(8):
        block()
    steady, after, host, stream = [], [], [], []
    for i in range(2 + REPS):
        b0 = block()
        arr = sweep(i)
        h, s_ms = timed(lambda: db.ctl_range(arr, 0, n, CARRIERS, dres.data_ptr()))
        b1 = block()
        if i >= 2:
            steady.append(b0); after.append(b1); host.append(h); stream.append(s_ms)
    show("1. ctl_range, FILTER on the carriers of every copy", host, stream, f"; d_result = {dres.cpu().numpy().tolist()}")
    print(f"  4. the block after it: median {np.median(after):.4f} ms (min {np.min(after):.4f}, max {np.max(after):.4f}); the steady block in front of it: "
          f"median {np.median(steady):.4f} ms (min {np.min(steady):.4f}, max {np.max(steady):.4f})")
    host, stream = [], []
    for i in range(2 + REPS):
        arr = sweep(i)
        h, s_ms = timed(lambda: db.ctl_slots(arr, CARRIERS, dlist.data_ptr(), LIST, 0, dres.data_ptr()))
        if i >= 2:
            host.append(h); stream.append(s_ms)
    show(f"3. ctl_slots, the same on a list of {LIST} slots", host, stream, f"; d_result = {dres.cpu().numpy().tolist()}")
    host, stream = [], []
    for i in range(1 + 3):
        h, s_ms = timed(lambda: host_route(i))
        if i >= 1:
            host.append(h); stream.append(s_ms)
        for _ in range(6):
            block()
    show(f"2. host-view writes + skred_bank_update of the {len(carriers)} carriers (3 runs)", host, stream)
    for _ in range(8):
        block()
    base = float(np.median([block() for _ in range(REPS)]))
    firsts, back = [], []
    for i in range(REPS):
        arr = D.ctl_array([D.ctl(D.CTL_AMP if l < 3 else 0, amp=0.5 + 0.01 * i) for l in range(K)])
        db.ctl_range(arr, 0, n, CARRIERS, dres.data_ptr())
        times = [block() for _ in range(24)]
        firsts.append(times[0])
        back.append(next((k for k, t in enumerate(times) if t <= 1.1 * base), len(times)))
    print(f"  5. the block after a bank-wide AMP controller: median {np.median(firsts):.4f} ms (min {np.min(firsts):.4f}, max {np.max(firsts):.4f}), steady "
          f"{base:.4f} ms; blocks until within 10 % of the steady time: median {np.median(back):.0f} (min {np.min(back)}, max {np.max(back)}; 24: not within 24)")
    db.close()


def owners():
    """Note-off by note id on bank_patch("3sk", 2**20), every copy sounding: a burst of 256 patch notes through
    skred_bank_note_on_steal_slots (all of them stolen) is tagged from its own d_assigned, two blocks of 64 frames pass, and the chord is
    released.  (a) skred_bank_release_tags of the 256 tags; (b) the only correct route before it: the burst's d_assigned copied to the
    host behind a stream wait, a key -> slot map kept in Python (a stolen slot's earlier key evicted), the note-off list uploaded and
    skred_bank_stamp_slots; (c) the 64-frame block after (a) beside the block after stamp_slots of the same slots.  Every repetition
    uploads the bank and renders a block first.  Medians of 12 with minimum and maximum, stream events around the device calls."""
    D = device
    n, K, NOTES, REPS, F = 1 << 20, 4, 256, 12, 64
    MEMBERS, VOICES = 0x7, 0xF
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    v = np.arange(n)
    sel = (v % K) < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 100.0
    e["velocity"][sel], e["is_active"][sel] = 1.0, 1
    e["sample_start"][sel] = (now - 40000 - ((v[sel] // K) * 7919) % 30000 - (v[sel] % K)).astype(np.uint64)   # every copy its own age
    db = device.DeviceBank(n)
    db.set_tables(tables); db.set_globals(g)
    which = D.IDLE_ENV_DONE
    iq = D.slot_query(0, n, K, MEMBERS, which, 1e-3, 0, NOTES)
    sq = D.slot_steal_query(0, n, K, MEMBERS, D.STEAL_OLDEST, 0, 0, which, 1e-3, NOTES)
    notes = D.note_array([D.NoteC(0.4 + 0.001 * i, 0.8, 0.0, 0.5, 0.5, D.NOTE_SET_PHASE) for i in range(NOTES * K)])
    tags = (0x80000000 + 17 * np.arange(NOTES)).astype(np.uint32)
    da = torch.full((NOTES,), -1, dtype=torch.int32, device="cuda")
    dr = torch.zeros(3, dtype=torch.int32, device="cuda")
    res = torch.zeros(3, dtype=torch.int32, device="cuda")
    out = torch.zeros(F, 2, device="cuda")

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1)

    def block():
        return timed(lambda: db.render_mix(F, out.data_ptr(), 2, 0, 0))[1]

    def by_tags():
        db.note_on_steal_slots(notes, iq, sq, VOICES, da.data_ptr(), dr.data_ptr())
        db.tag_slots(da.data_ptr(), tags, K)                       # (nothing waited for: the host never sees d_assigned)
        block(); block()
        torch.cuda.synchronize()
        h, s_ms = timed(lambda: db.release_tags(0, n, K, VOICES, tags, D.STAMP_RELEASE, res.data_ptr()))
        return h, s_ms, block(), res.cpu().numpy().tolist()

    key_of, slot_of = {}, {}

    def by_map():
        db.note_on_steal_slots(notes, iq, sq, VOICES, da.data_ptr(), dr.data_ptr())
        t0 = time.perf_counter()
        got = da.cpu().numpy()                                     # the stream wait a device-side note-on was built to remove
        for k, slot in enumerate(got.tolist()):
            if slot < 0:
                continue
            old = key_of.pop(slot, None)                           # a theft: the slot's earlier key no longer names it
            if old is not None:
                slot_of.pop(old, None)
            key_of[slot], slot_of[int(tags[k])] = int(tags[k]), slot
        h_map = (time.perf_counter() - t0) * 1e3
        block(); block()
        torch.cuda.synchronize()

        def off():
            lst = np.array([slot_of[int(t)] for t in tags if int(t) in slot_of], np.int32)
            dl = torch.from_numpy(lst).cuda()
            db.stamp_slots(dl.data_ptr(), len(lst), K, VOICES, D.STAMP_RELEASE)
        h, s_ms = timed(off)
        return h_map + h, s_ms, block(), [h_map, h]

    print(f"3sk {n} voices = {n // K} slots of {K}, every copy sounding; a block, a burst of {NOTES} stolen patch notes, two blocks of {F} frames, the note-off; medians of {REPS}")
    blocks = {}
    for label, route in (("(a) release_tags of 256 tags (find pass over the whole bank + guarded stamps, on the device)", by_tags),
                         ("(b) d_assigned read back behind a stream wait + key -> slot map in Python + list upload + stamp_slots", by_map)):
        host, stream, after, extra = [], [], [], None
        for it in range(2 + REPS):
            db.upload(bank)
            db.render_mix(F, out.data_ptr(), 2, 0, 0)
            torch.cuda.synchronize()
            key_of.clear(); slot_of.clear()
            h, s_ms, b, extra = route()
            torch.cuda.synchronize()
            if it >= 2:
                host.append(h); stream.append(s_ms); after.append(b)
        blocks[label[:3]] = after
        tail = f"d_result = {extra}" if label.startswith("(a)") else f"last run: readback and map {extra[0]:.4f} ms + note-off {extra[1]:.4f} ms"
        print(f"  {label}: host time held median {np.median(host):.4f} ms (min {np.min(host):.4f}, max {np.max(host):.4f}); stream time of the note-off "
              f"between events median {np.median(stream):.4f} ms (min {np.min(stream):.4f}, max {np.max(stream):.4f}); {tail}")
    for key, what in (("(a)", "release_tags"), ("(b)", "stamp_slots of the same slots")):
        t = blocks[key]
        print(f"  (c) the {F}-frame block after {what}: median {np.median(t):.4f} ms (min {np.min(t):.4f}, max {np.max(t):.4f})")
    db.close()


def _fx_timed(call, before=None, runs=12, warm=3):
    """(stream ms between events, host ms held) of `call`, `runs` times after `warm`; `before` runs untimed ahead of each"""
    ms, held = [], []
    for it in range(warm + runs):
        if before:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        if it >= warm:
            ms.append(e0.elapsed_time(e1))
            held.append(dt * 1e3)
    return ms, held


def _fx_stats(x):
    return f"median {np.median(x):.4f} ms (min {np.min(x):.4f}, max {np.max(x):.4f}) of {len(x)}"


def _fx_block_after(db, out, F, call=None, runs=12):
    t = []
    for _ in range(runs):
        if call:
            call()
        db.render_mix(F, out.data_ptr(), 1)
        torch.cuda.synchronize()
        t.append(db.last_render_ms())
    return t


def fxowners():
    from skred_amd import fxbank as X
    n, F, K = 1 << 20, 64, 256
    bank, pool, c0 = X.bank_fx(n)                                         # every voice sounding: a burst can only steal
    db = X.DeviceFxBank(n)
    db.set_tables(pool); db.upload(bank); db.set_sample_count(c0)
    out = torch.zeros(F, 2, dtype=torch.int64, device="cuda")
    notes = X.fx_note_array([X.FxNoteC(3000017 + 40009 * k, 26000, 0, 16384, 16384, X.NOTE_SET_PHASE) for k in range(K)])
    da = torch.full((K,), -1, dtype=torch.int32, device="cuda")
    dr = torch.zeros(3, dtype=torch.int32, device="cuda")
    iq = X.FxIdleQueryC(0, n, X.IDLE_FINISHED | X.IDLE_ENV_DONE, 0, 0, 0)
    sq = X.fx_steal_query(0, n, X.STEAL_OLDEST, 0, 64)
    burst = [0]

    def tags():
        return (1 + burst[0] * K + np.arange(K)).astype(np.uint32)

    def steal_and_tag():                                                  # 256 stolen notes tagged from their own d_assigned, two blocks
        burst[0] += 1
        db.note_on_steal(notes, iq, sq, da.data_ptr(), dr.data_ptr())
        db.tag_list(da.data_ptr(), tags())
        for _ in range(2):
            db.render_mix(F, out.data_ptr(), 1)

    def by_tag():
        db.release_tags(0, n, tags(), X.STAMP_RELEASE, dr.data_ptr())

    def by_host_map():                                                    # the parent's only correct route
        held = da.cpu().numpy()                                           # d_assigned read back behind a stream wait
        key_to_voice = {int(t): int(v) for t, v in zip(tags(), held)}     # the map a host would keep
        db.stamp(np.array([key_to_voice[int(t)] for t in tags()], np.int32), X.FX_STAMP_RELEASE)

    steady = _fx_block_after(db, out, F)
    print(f"fx {n} voices all sounding, bursts of {K} stolen notes tagged from their own d_assigned, two {F}-frame blocks, then the note-off")
    for label, call in (("(a) release_tags", by_tag), ("(b) d_assigned read back + a map in Python + skred_fxbank_stamp", by_host_map)):
        ms, held = _fx_timed(call, steal_and_tag)
        after = _fx_block_after(db, out, F, lambda: (steal_and_tag(), call()))
        print(f"  {label}: host held {_fx_stats(held)}; stream time between events {_fx_stats(ms)}; d_result = {dr.cpu().numpy().tolist()}")
        print(f"      the {F}-frame block after it: {_fx_stats(after)}; a steady block: {_fx_stats(steady)}")
    db.close()


def fxctl():
    from skred_amd import fxbank as X
    n, F, K = 1 << 20, 64, 256
    bank, pool, c0 = X.bank_fx(n)                                         # every voice filtered
    db = X.DeviceFxBank(n)
    db.set_tables(pool); db.upload(bank); db.set_sample_count(c0)
    out = torch.zeros(F, 2, dtype=torch.int64, device="cuda")
    co = X.q30_coeffs(np.array([1]), np.array([1200.0], np.float32), np.array([1.5], np.float32), 48000)
    c = X.fx_ctl(X.CTL_FILTER, **{k: int(v[0]) for k, v in co.items()})
    dr = torch.zeros(3, dtype=torch.int32, device="cuda")
    lst = torch.tensor(((np.arange(K, dtype=np.int64) * 4093 + 7) % n).astype(np.int32), dtype=torch.int32, device="cuda")
    everyone = np.arange(n, dtype=np.int32)
    h = bank.copy()

    def by_update():                                                      # the parent's only route: host-view writes + update of those voices
        for k, v in co.items():
            h[k][...] = v[0]
        db.update(h, everyone, X.DIRTY_PARAMS)

    steady = _fx_block_after(db, out, F)
    print(f"fx {n} voices, all filtered: a cutoff change on every voice")
    for label, call, runs in (("(a) ctl_range", lambda: db.ctl_range(c, 0, n, dr.data_ptr()), 12),
                              ("(b) host-view writes + skred_fxbank_update of every voice", by_update, 3),
                              (f"(c) ctl_list on a {K}-entry list", lambda: db.ctl_list(c, lst.data_ptr(), K, 0, dr.data_ptr()), 12)):
        ms, held = _fx_timed(call, None, runs, 1 if runs == 3 else 3)
        print(f"  {label}: host held {_fx_stats(held)}; stream time between events {_fx_stats(ms)}; d_result = {dr.cpu().numpy().tolist()[:2]}")
    after = _fx_block_after(db, out, F, lambda: db.ctl_range(c, 0, n, dr.data_ptr()))
    print(f"  (d) the {F}-frame block after ctl_range: {_fx_stats(after)}; a steady block: {_fx_stats(steady)}")
    db.close()


def expr():
    """Channels and per-note expression on bank_patch("3sk", 2**20), every copy sounding and tagged over 16 channels (tag = channel << 24
    | slot + 1).  (a) a cutoff change on ONE channel: skred_bank_ctl_match, beside skred_bank_ctl_range over the whole range and beside
    the only per-channel route before it -- skred_bank_download_owners (a device wait), a pick in numpy, the list uploaded,
    skred_bank_ctl_slots; (b) all notes off on one channel: skred_bank_stamp_match beside that route ending in skred_bank_stamp_slots;
    (c) 256 notes, 256 different bends: one skred_bank_ctl_tags_each beside 256 skred_bank_ctl_owned calls; (d) the 64-frame block after
    a filter-only ctl_match beside the steady block.  Medians of 12 with minimum and maximum; host time held, and stream time between
    events."""
    D = device
    n, K, REPS, F, CHANNELS, NOTES = 1 << 20, 4, 12, 64, 16, 256
    MEMBERS, VOICES = 0x7, 0xF
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    v = np.arange(n)
    sel = (v % K) < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 100.0
    e["velocity"][sel], e["is_active"][sel] = 1.0, 1
    e["sample_start"][sel] = np.uint64(now - 40000)
    db = device.DeviceBank(n)
    db.set_tables(tables); db.set_globals(g); db.upload(bank)
    slots = np.arange(0, n, K, dtype=np.int32)
    idx = np.arange(len(slots), dtype=np.uint32)
    tags = (((idx % CHANNELS) + 1) << 24 | (idx // CHANNELS + 1)).astype(np.uint32)
    dl_all = torch.from_numpy(slots).cuda()
    db.tag_slots(dl_all.data_ptr(), tags, K)
    res = torch.zeros(3, dtype=torch.int32, device="cuda")
    out = torch.zeros(F, 2, device="cuda")
    m = D.owner_match(3 << 24, 0xFF000000)
    co = banks.biquad_coeffs(np.array([1]), np.array([900.0], np.float32), np.array([1.2], np.float32), 48000)
    cut = [D.ctl(D.CTL_FILTER, b0=float(co["b0"][0]), b1=float(co["b1"][0]), b2=float(co["b2"][0]), a1=float(co["a1"][0]), a2=float(co["a2"][0]))
           for _ in range(K)]
    torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1)

    def stats(x):
        return f"median {np.median(x):.4f} ms (min {np.min(x):.4f}, max {np.max(x):.4f})"

    def series(call, before=None):
        host, stream = [], []
        for it in range(2 + REPS):
            if before is not None:
                before()
            torch.cuda.synchronize()
            h, s_ms = timed(call)
            if it >= 2:
                host.append(h); stream.append(s_ms)
        return f"host time held {stats(host)}; stream time between events {stats(stream)}"

    def parent_route(last):
        own = db.download_owners()[::K]                            # the device wait the channel calls were built to remove
        lst = slots[(own != 0) & ((own & np.uint32(0xFF000000)) == np.uint32(3 << 24))]
        dl = torch.from_numpy(lst).cuda()
        last(dl, len(lst))

    print(f"3sk {n} voices = {n // K} slots of {K}, every copy sounding, tagged over {CHANNELS} channels ({n // K // CHANNELS} notes each); medians of {REPS}")
    print(f"  (a) cutoff of one channel, ctl_match: {series(lambda: db.ctl_match(cut, 0, n, MEMBERS, m, res.data_ptr()))}; d_result = {res.cpu().numpy().tolist()}")
    print(f"  (a) cutoff of the whole range, ctl_range: {series(lambda: db.ctl_range(cut, 0, n, MEMBERS, res.data_ptr()))}")
    print(f"  (a) cutoff of one channel, download_owners + numpy pick + list upload + ctl_slots: "
          f"{series(lambda: parent_route(lambda dl, k: db.ctl_slots(cut, MEMBERS, dl.data_ptr(), k, 0, res.data_ptr())))}")
    retrig = lambda: db.stamp_slots(dl_all.data_ptr(), len(slots), K, VOICES, D.STAMP_TRIGGER)   # noqa: E731
    print(f"  (b) all notes off on one channel, stamp_match: {series(lambda: db.stamp_match(0, n, K, VOICES, m, D.STAMP_RELEASE, res.data_ptr()), retrig)}; "
          f"d_result = {res.cpu().numpy()[:2].tolist()}")
    print(f"  (b) the same, download_owners + numpy pick + list upload + stamp_slots: "
          f"{series(lambda: parent_route(lambda dl, k: db.stamp_slots(dl.data_ptr(), k, K, VOICES, D.STAMP_RELEASE)), retrig)}")
    note_tags = tags[3::CHANNELS * 7][:NOTES].copy()
    bends = [D.ctl_each(D.EACH_INC_SCALE, inc_scale=float(np.float32(2.0 ** ((k % 25 - 12) / 1200.0)))) for k in range(NOTES)]
    found = torch.full((NOTES,), -1, dtype=torch.int32, device="cuda")
    db.find_owned(0, n, K, note_tags, found.data_ptr())
    torch.cuda.synchronize()
    print(f"  (c) {NOTES} notes, {NOTES} bends, one ctl_tags_each: {series(lambda: db.ctl_tags_each(None, bends, 0, n, MEMBERS, note_tags, K, res.data_ptr()))}; "
          f"d_result = {res.cpu().numpy().tolist()}")

    def one_by_one():
        for k in range(NOTES):
            c = [D.ctl(D.CTL_INC_SCALE, inc_scale=bends[k].inc_scale)] * K
            db.ctl_owned(c, MEMBERS, found.data_ptr() + 4 * k, note_tags[k:k + 1])
    print(f"  (c) the same, {NOTES} ctl_owned calls on a list that is already on the device: {series(one_by_one)}")

    def block():
        return timed(lambda: db.render_mix(F, out.data_ptr(), 2, 0, 0))[1]
    db.upload(bank)
    for _ in range(8):
        block()
    steady = [block() for _ in range(REPS)]
    after = []
    for _ in range(REPS):
        db.ctl_match(cut, 0, n, MEMBERS, m, 0)
        after.append(block())
        block()
    print(f"  (d) the {F}-frame block after a filter-only ctl_match: {stats(after)}; a steady block: {stats(steady)}; kernel {db.last_kernel()}, "
          f"list violations {db.list_violations()}")
    db.close()


def fxexpr():
    """Channels and per-note expression on bank_fx(2**20), every voice sounding and tagged over 16 channels (tag = channel << 24 |
    voice + 1).  (a) a cutoff change on ONE channel: skred_fxbank_ctl_match beside the only per-channel route before it --
    skred_fxbank_download_owners (a device wait), a pick in numpy, the list uploaded, skred_fxbank_ctl_list; (b) all notes off on one
    channel: skred_fxbank_stamp_match beside that route ending in skred_fxbank_stamp_list; (c) 256 notes, 256 different bends: one
    skred_fxbank_ctl_tags_each beside 256 skred_fxbank_ctl_owned calls; (d) the 64-frame block after (a) beside the steady block.
    Medians of 12 with minimum and maximum; host time held, and stream time between events."""
    from skred_amd import fxbank as X
    n, F, CHANNELS, NOTES = 1 << 20, 64, 16, 256
    bank, pool, c0 = X.bank_fx(n)
    db = X.DeviceFxBank(n)
    db.set_tables(pool); db.upload(bank); db.set_sample_count(c0)
    out = torch.zeros(F, 2, dtype=torch.int64, device="cuda")
    v = np.arange(n, dtype=np.int64)
    tags = (((v % CHANNELS) + 1) << 24 | (v // CHANNELS + 1)).astype(np.uint32)
    everyone = torch.arange(n, dtype=torch.int32, device="cuda")
    db.tag_list(everyone.data_ptr(), tags)
    value, mask = 3 << 24, 0xFF000000
    co = X.q30_coeffs(np.array([1]), np.array([900.0], np.float32), np.array([1.2], np.float32), 48000)
    cut = X.fx_ctl(X.CTL_FILTER, **{k: int(x[0]) for k, x in co.items()})
    dr = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def parent_route(last):
        own = db.download_owners()                                        # the device wait the channel calls were built to remove
        lst = np.flatnonzero((own != 0) & ((own & np.uint32(mask)) == np.uint32(value))).astype(np.int32)
        dl = torch.from_numpy(lst).cuda()
        last(dl, len(lst))

    def line(label, call, before=None, words=3):
        ms, held = _fx_timed(call, before)
        print(f"  {label}: host held {_fx_stats(held)}; stream time between events {_fx_stats(ms)}; d_result = {dr.cpu().numpy().tolist()[:words]}")

    retrig = lambda: db.stamp_list(everyone.data_ptr(), n, X.STAMP_TRIGGER)   # noqa: E731
    print(f"fx {n} voices all sounding, tagged over {CHANNELS} channels ({n // CHANNELS} notes each)")
    line("(a) cutoff of one channel, ctl_match", lambda: db.ctl_match(cut, 0, n, value, mask, dr.data_ptr()))
    line("(a) the same, download_owners + numpy pick + list upload + ctl_list",
         lambda: parent_route(lambda dl, k: db.ctl_list(cut, dl.data_ptr(), k, 0, dr.data_ptr())), None, 2)
    line("(b) all notes off on one channel, stamp_match", lambda: db.stamp_match(0, n, value, mask, X.STAMP_RELEASE, dr.data_ptr()), retrig, 2)
    line("(b) the same, download_owners + numpy pick + list upload + stamp_list",
         lambda: parent_route(lambda dl, k: db.stamp_list(dl.data_ptr(), k, X.STAMP_RELEASE)), retrig, 0)
    note_tags = tags[2::CHANNELS * 7][:NOTES].copy()
    bends = [X.fx_each(X.EACH_INC_SCALE, inc_scale_q16=int(round(65536 * 2.0 ** ((k % 25 - 12) / 1200.0)))) for k in range(NOTES)]
    found = torch.full((NOTES,), -1, dtype=torch.int32, device="cuda")
    db.find_owned(0, n, note_tags, found.data_ptr())
    torch.cuda.synchronize()
    line(f"(c) {NOTES} notes, {NOTES} bends, one ctl_tags_each", lambda: db.ctl_tags_each(None, bends, 0, n, note_tags, dr.data_ptr()))

    def one_by_one():
        for k in range(NOTES):
            db.ctl_owned(X.fx_ctl(X.CTL_INC_SCALE, inc_scale_q16=bends[k].inc_scale_q16), found.data_ptr() + 4 * k, note_tags[k:k + 1])
    line(f"(c) the same, {NOTES} ctl_owned calls on a list that is already on the device", one_by_one, None, 0)
    db.upload(bank)
    _fx_block_after(db, out, F, None, 4)
    steady = _fx_block_after(db, out, F)
    after = _fx_block_after(db, out, F, lambda: db.ctl_match(cut, 0, n, value, mask))
    print(f"  (d) the {F}-frame block after ctl_match of one channel: {_fx_stats(after)}; a steady block: {_fx_stats(steady)}")
    db.close()


def timbre():
    """Per-note timbre on bank_patch("3sk", 2**20), every copy sounding and tagged over 16 channels (tag = channel << 24 | slot + 1):
    256 notes with 256 cutoffs.  (a) one skred_bank_ctl_tags_each_filter beside the only route before it, 256 skred_bank_ctl_owned calls
    with SKRED_CTL_FILTER on a list that is already on the device; (b) the 64-frame block after the call beside the steady block.
    Medians of 12 with minimum and maximum; host time held, and stream time between events."""
    D = device
    n, K, REPS, F, CHANNELS, NOTES = 1 << 20, 4, 12, 64, 16, 256
    MEMBERS = 0x7
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    sel = (np.arange(n) % K) < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 100.0
    e["velocity"][sel], e["is_active"][sel] = 1.0, 1
    e["sample_start"][sel] = np.uint64(now - 40000)
    bank["voice_filter_mode"][sel] = 1                             # the carriers filtered: the coefficients are heard
    for name, x in zip(("b0", "b1", "b2", "a1", "a2"), D.filter_coeffs(1, 2000.0, 0.707, 44100.0)):
        bank["voice_filter"][name][sel] = x
    db = device.DeviceBank(n)
    db.set_tables(tables); db.set_globals(g); db.upload(bank)
    slots = np.arange(0, n, K, dtype=np.int32)
    idx = np.arange(len(slots), dtype=np.uint32)
    tags = (((idx % CHANNELS) + 1) << 24 | (idx // CHANNELS + 1)).astype(np.uint32)
    db.tag_slots(torch.from_numpy(slots).cuda().data_ptr(), tags, K)
    res = torch.zeros(3, dtype=torch.int32, device="cuda")
    out = torch.zeros(F, 2, device="cuda")
    note_tags = tags[3::CHANNELS * 7][:NOTES].copy()
    coeffs = [D.filter_coeffs(1, 220.0 * 2.0 ** (k / 48.0), 0.9, 44100.0) for k in range(NOTES)]
    filt = D.filter_each_array([D.filter_each(*c) for c in coeffs])
    found = torch.full((NOTES,), -1, dtype=torch.int32, device="cuda")
    db.find_owned(0, n, K, note_tags, found.data_ptr())
    torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1)

    def stats(x):
        return f"median {np.median(x):.4f} ms (min {np.min(x):.4f}, max {np.max(x):.4f})"

    def series(call):
        host, stream = [], []
        for it in range(2 + REPS):
            torch.cuda.synchronize()
            h, s_ms = timed(call)
            if it >= 2:
                host.append(h); stream.append(s_ms)
        return f"host time held {stats(host)}; stream time between events {stats(stream)}"

    one_call = lambda: db.ctl_tags_each_filter(None, None, filt, 0, n, MEMBERS, MEMBERS, note_tags, K, res.data_ptr())   # noqa: E731
    print(f"3sk {n} voices = {n // K} slots of {K}, every copy sounding, tagged over {CHANNELS} channels; medians of {REPS}")
    print(f"  (a) {NOTES} notes, {NOTES} cutoffs, one ctl_tags_each_filter: {series(one_call)}; d_result = {res.cpu().numpy().tolist()}")

    # the records of the old route built ahead of the timed region, as the new call's array is
    singles = [D.ctl_array([D.ctl(D.CTL_FILTER, **dict(zip(("b0", "b1", "b2", "a1", "a2"), (float(x) for x in coeffs[k]))))] * K) for k in range(NOTES)]
    single_tags = [note_tags[k:k + 1].copy() for k in range(NOTES)]

    def one_by_one():
        for k in range(NOTES):
            db.ctl_owned(singles[k], MEMBERS, found.data_ptr() + 4 * k, single_tags[k])
    print(f"  (a) the same, {NOTES} ctl_owned calls on a list that is already on the device: {series(one_by_one)}")

    def block():
        return timed(lambda: db.render_mix(F, out.data_ptr(), 2, 0, 0))[1]
    db.upload(bank)
    for _ in range(8):
        block()
    steady = [block() for _ in range(REPS)]
    after = []
    for _ in range(REPS):
        one_call()
        after.append(block())
        block()
    print(f"  (b) the {F}-frame block after ctl_tags_each_filter: {stats(after)}; a steady block: {stats(steady)}; kernel {db.last_kernel()}, "
          f"list violations {db.list_violations()}")
    db.close()


def fxtimbre():
    """Per-note timbre on bank_fx(2**20), every voice sounding and tagged over 16 channels: 256 notes with 256 cutoffs.  (a) one
    skred_fxbank_ctl_tags_each_filter beside 256 skred_fxbank_ctl_owned calls with SKRED_CTL_FILTER; (b) the 64-frame block after the
    call beside the steady block.  Medians of 12 with minimum and maximum; host time held, and stream time between events."""
    from skred_amd import fxbank as X
    n, F, CHANNELS, NOTES = 1 << 20, 64, 16, 256
    bank, pool, c0 = X.bank_fx(n)
    db = X.DeviceFxBank(n)
    db.set_tables(pool); db.upload(bank); db.set_sample_count(c0)
    out = torch.zeros(F, 2, dtype=torch.int64, device="cuda")
    v = np.arange(n, dtype=np.int64)
    tags = (((v % CHANNELS) + 1) << 24 | (v // CHANNELS + 1)).astype(np.uint32)
    db.tag_list(torch.arange(n, dtype=torch.int32, device="cuda").data_ptr(), tags)
    dr = torch.zeros(3, dtype=torch.int32, device="cuda")
    note_tags = tags[2::CHANNELS * 7][:NOTES].copy()
    names = ("b0_q30", "b1_q30", "b2_q30", "a1_q30", "a2_q30")
    q30 = [[int(max(-(1 << 31), min((1 << 31) - 1, round(float(x) * (1 << 30))))) for x in device.filter_coeffs(1, 220.0 * 2.0 ** (k / 48.0), 0.9, 48000.0)]
           for k in range(NOTES)]
    filt = X.fx_filter_each_array([X.fx_filter_each(*c) for c in q30])
    found = torch.full((NOTES,), -1, dtype=torch.int32, device="cuda")
    db.find_owned(0, n, note_tags, found.data_ptr())
    torch.cuda.synchronize()

    def line(label, call, words=3):
        ms, held = _fx_timed(call, None)
        print(f"  {label}: host held {_fx_stats(held)}; stream time between events {_fx_stats(ms)}; d_result = {dr.cpu().numpy().tolist()[:words]}")

    one_call = lambda: db.ctl_tags_each_filter(None, None, filt, 0, n, note_tags, dr.data_ptr())   # noqa: E731
    print(f"fx {n} voices all sounding, tagged over {CHANNELS} channels ({n // CHANNELS} notes each)")
    line(f"(a) {NOTES} notes, {NOTES} cutoffs, one ctl_tags_each_filter", one_call)

    # the records of the old route built ahead of the timed region, as the new call's array is
    singles = [X.fx_ctl(X.CTL_FILTER, **dict(zip(names, q30[k]))) for k in range(NOTES)]
    single_tags = [note_tags[k:k + 1].copy() for k in range(NOTES)]

    def one_by_one():
        for k in range(NOTES):
            db.ctl_owned(singles[k], found.data_ptr() + 4 * k, single_tags[k])
    line(f"(a) the same, {NOTES} ctl_owned calls on a list that is already on the device", one_by_one, 0)
    db.upload(bank)
    _fx_block_after(db, out, F, None, 4)
    steady = _fx_block_after(db, out, F)
    after = _fx_block_after(db, out, F, one_call)
    print(f"  (b) the {F}-frame block after ctl_tags_each_filter: {_fx_stats(after)}; a steady block: {_fx_stats(steady)}")
    db.close()


def chan():
    """Channel polyphony on bank_patch("3sk", 2**20), every copy sounding and tagged over 16 channels (tag = channel << 24 | slot + 1).
    (a) a burst of 256 patch notes on ONE channel with the cap at the channel's current count, so that all 256 steal inside the
    channel: skred_bank_note_on_channel, beside the only route before it -- skred_bank_download_owners and skred_bank_download behind a
    device wait, the channel pick and the victim order in numpy, skred_bank_update, skred_bank_tag_slots; (b) the key pass:
    skred_bank_find_steal_slots_match beside skred_bank_find_steal_slots on the same range at max_out 0 and 16; (c) the 64-frame block
    after the burst beside the block after the equivalent skred_bank_note_on_steal_slots.  Medians of 12 with minimum and maximum;
    host time held, and stream time between events."""
    D = device
    from skred_amd.bank import slot_query, slot_steal_query
    n, K, REPS, F, CHANNELS, NOTES = 1 << 20, 4, 12, 64, 16, 256
    MEMBERS, VOICES = 0x7, 0xF
    WHICH = D.IDLE_FINISHED | D.IDLE_ENV_DONE
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    v = np.arange(n)
    sel = (v % K) < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 100.0
    e["velocity"][sel], e["is_active"][sel] = 1.0, 1
    e["sample_start"][sel] = (now - 40000 - ((v[sel] // K) * 37) % 1000).astype(np.uint64)
    db = device.DeviceBank(n)
    db.set_tables(tables); db.set_globals(g); db.upload(bank)
    slots = np.arange(0, n, K, dtype=np.int32)
    idx = np.arange(len(slots), dtype=np.uint32)
    tags = (((idx % CHANNELS) + 1) << 24 | (idx // CHANNELS + 1)).astype(np.uint32)
    dl_all = torch.from_numpy(slots).cuda()
    db.tag_slots(dl_all.data_ptr(), tags, K)
    out = torch.zeros(F, 2, device="cuda")
    m = D.owner_match(3 << 24, 0xFF000000)
    per_channel = n // K // CHANNELS
    iq = slot_query(0, n, K, MEMBERS, WHICH, 1e-3, 0, 0)
    sq = slot_steal_query(0, n, K, MEMBERS)
    notes = D.note_array([D.NoteC(0.01 + 1e-5 * (k % 97), 0.8, 0.0, 0.5, 0.5, 1) for k in range(NOTES * K)])   # (built once: a ctypes array passes through)
    note_tags = ((3 << 24) | (0x800000 + np.arange(NOTES))).astype(np.uint32)
    da = torch.full((NOTES,), -1, dtype=torch.int32, device="cuda")
    dr = torch.zeros(4, dtype=torch.int32, device="cuda")
    dv = torch.full((16,), -1, dtype=torch.int32, device="cuda")
    dc = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1)

    def stats(x):
        return f"median {np.median(x):.4f} ms (min {np.min(x):.4f}, max {np.max(x):.4f})"

    def series(call):
        host, stream = [], []
        for it in range(2 + REPS):
            torch.cuda.synchronize()
            h, s_ms = timed(call)
            if it >= 2:
                host.append(h); stream.append(s_ms)
        return f"host time held {stats(host)}; stream time between events {stats(stream)}"

    mirror, state = bank.copy(), bank.copy()
    starts = e["sample_start"].astype(np.int64).copy()

    def parent_route():
        own = db.download_owners()[::K]                            # the device waits the channel call was built to remove
        db.download(state)
        mine = (own != 0) & ((own & np.uint32(0xFF000000)) == np.uint32(3 << 24))
        live = (state["voice_amp_envelope"]["is_active"].reshape(-1, K)[:, :3] != 0).any(1)
        heads = slots[mine & live]
        key = starts.reshape(-1, K)[:, :3].max(1)[heads // K]
        picks = heads[np.lexsort((heads, key))][:NOTES]
        touched = (picks[:, None] + np.arange(K)[None, :]).reshape(-1).astype(np.int32)
        db.update(mirror, touched, D.DIRTY_PARAMS | D.DIRTY_PHASE | D.STAMP_TRIGGER)
        dl = torch.from_numpy(picks).cuda()
        db.tag_slots(dl.data_ptr(), note_tags[:len(picks)], K)

    print(f"3sk {n} voices = {n // K} slots of {K}, every copy sounding, tagged over {CHANNELS} channels ({per_channel} notes each); medians of {REPS}")
    burst = lambda: db.note_on_channel(notes, note_tags, iq, sq, m, per_channel, VOICES, da.data_ptr(), dr.data_ptr())   # noqa: E731
    print(f"  (a) {NOTES} notes on one channel at its cap, note_on_channel: {series(burst)}; d_result = {dr.cpu().numpy().tolist()}")
    print(f"  (a) the same, download_owners + download + numpy pick and order + update + tag_slots: {series(parent_route)}")
    for mo in (0, 16):
        q = slot_steal_query(0, n, K, MEMBERS, max_out=mo)
        print(f"  (b) max_out {mo}, find_steal_slots_match on one channel: {series(lambda: db.find_steal_slots_match(q, m, dv.data_ptr(), dc.data_ptr()))}; "
              f"d_count = {dc.cpu().numpy().tolist()}")
        print(f"  (b) max_out {mo}, find_steal_slots on the whole range: {series(lambda: db.find_steal_slots(q, dv.data_ptr(), dc.data_ptr()))}; "
              f"d_count = {dc.cpu().numpy()[:2].tolist()}")

    def block():
        return timed(lambda: db.render_mix(F, out.data_ptr(), 2, 0, 0))[1]

    def block_after(call):
        db.upload(bank)
        db.tag_slots(dl_all.data_ptr(), tags, K)
        for _ in range(8):
            block()
        after = []
        for _ in range(REPS):
            call()
            after.append(block())
            block()
        return after
    after_chan = block_after(burst)
    after_steal = block_after(lambda: db.note_on_steal_slots(notes, iq, sq, VOICES, da.data_ptr(), dr.data_ptr()))
    print(f"  (c) the {F}-frame block after the channel burst: {stats(after_chan)}; after note_on_steal_slots of {NOTES} notes: {stats(after_steal)}; "
          f"kernel {db.last_kernel()}, list violations {db.list_violations()}")
    db.close()


def fxchan():
    """Channel polyphony on bank_fx(2**20), every voice sounding and tagged over 16 channels (tag = channel << 24 | voice // 16 + 1).
    (a) a burst of 256 notes on ONE channel with the cap at the channel's current count, so that all 256 steal inside the channel:
    skred_fxbank_note_on_channel, beside the only route before it -- skred_fxbank_download_owners and skred_fxbank_download behind a
    device wait, the channel pick and the victim order in numpy, skred_fxbank_update, skred_fxbank_tag_list; (b) the key pass:
    skred_fxbank_find_steal_match beside skred_fxbank_find_steal on the same range at max_out 0 and 16; (c) the 64-frame block after
    the burst beside the block after the equivalent skred_fxbank_note_on_steal.  Medians of 12 with minimum and maximum; host time
    held, and stream time between events."""
    from skred_amd import fxbank as X
    n, F, CHANNELS, NOTES = 1 << 20, 64, 16, 256
    bank, pool, c0 = X.bank_fx(n)                                         # every voice sounding: a burst can only steal
    db = X.DeviceFxBank(n)
    db.set_tables(pool); db.upload(bank); db.set_sample_count(c0)
    out = torch.zeros(F, 2, dtype=torch.int64, device="cuda")
    v = np.arange(n, dtype=np.int64)
    tags = (((v % CHANNELS) + 1) << 24 | (v // CHANNELS + 1)).astype(np.uint32)
    everyone = torch.arange(n, dtype=torch.int32, device="cuda")
    db.tag_list(everyone.data_ptr(), tags)
    value, mask = 3 << 24, 0xFF000000
    per_channel = n // CHANNELS
    iq = X.FxIdleQueryC(0, n, X.IDLE_FINISHED | X.IDLE_ENV_DONE, 0, 0, 0)
    sq = X.fx_steal_query(0, n, X.STEAL_OLDEST, 0, 64)
    notes = X.fx_note_array([X.FxNoteC(3000017 + 40009 * k, 26000, 0, 16384, 16384, X.NOTE_SET_PHASE) for k in range(NOTES)])
    note_tags = ((3 << 24) | (0x800000 + np.arange(NOTES))).astype(np.uint32)
    da = torch.full((NOTES,), -1, dtype=torch.int32, device="cuda")
    dr = torch.zeros(4, dtype=torch.int32, device="cuda")
    dv = torch.full((16,), -1, dtype=torch.int32, device="cuda")
    dc = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mirror, state = bank.copy(), bank.copy()
    starts = bank["sample_start"].astype(np.int64).copy()

    def parent_route():
        own = db.download_owners()                                        # the device waits the channel call was built to remove
        db.download(state)
        mine = (own != 0) & ((own & np.uint32(mask)) == np.uint32(value)) & (state["is_active"] != 0)
        voices = np.flatnonzero(mine)
        picks = voices[np.lexsort((voices, starts[voices]))][:NOTES].astype(np.int32)
        db.update(mirror, picks, X.DIRTY_PARAMS | X.DIRTY_PHASE | X.STAMP_TRIGGER)
        dl = torch.from_numpy(picks).cuda()
        db.tag_list(dl.data_ptr(), note_tags[:len(picks)])

    def line(label, call, words, res=None):
        ms, held = _fx_timed(call)
        res = dr if res is None else res
        print(f"  {label}: host held {_fx_stats(held)}; stream time between events {_fx_stats(ms)}; result words = {res.cpu().numpy().tolist()[:words]}")

    print(f"fx {n} voices all sounding, tagged over {CHANNELS} channels ({per_channel} notes each)")
    burst = lambda: db.note_on_channel(notes, iq, sq, value, mask, per_channel, note_tags, da.data_ptr(), dr.data_ptr())   # noqa: E731
    line(f"(a) {NOTES} notes on one channel at its cap, note_on_channel", burst, 4)
    line("(a) the same, download_owners + download + numpy pick and order + update + tag_list", parent_route, 0)
    for mo in (0, 16):
        q = X.fx_steal_query(0, n, X.STEAL_OLDEST, 0, 64, 0, 0, mo)
        line(f"(b) max_out {mo}, find_steal_match on one channel", lambda: db.find_steal_match(q, value, mask, dv.data_ptr(), dc.data_ptr()), 3, dc)
        line(f"(b) max_out {mo}, find_steal on the whole range", lambda: db.find_steal(q, dv.data_ptr(), dc.data_ptr()), 2, dc)

    def block_after(call):
        db.upload(bank); db.set_sample_count(c0)
        db.tag_list(everyone.data_ptr(), tags)
        _fx_block_after(db, out, F, None, 8)
        after = []
        for _ in range(12):
            call()
            after += _fx_block_after(db, out, F, None, 1)
            _fx_block_after(db, out, F, None, 1)
        return after
    steady = _fx_block_after(db, out, F)
    after_chan = block_after(burst)
    after_steal = block_after(lambda: db.note_on_steal(notes, iq, sq, da.data_ptr(), dr.data_ptr()))
    print(f"  (c) the {F}-frame block after the channel burst: {_fx_stats(after_chan)}; after note_on_steal of {NOTES} notes: {_fx_stats(after_steal)}; "
          f"a steady block: {_fx_stats(steady)}")
    db.close()


def pedal():
    """Pedals on bank_patch("3sk", 2**20), every copy sounding and tagged over 16 channels (tag = channel << 24 | slot + 1), 256
    note-offs of one channel held back, then the pedal goes up.  (a) skred_bank_release_tags_pedal beside skred_bank_release_tags of
    the same tags; (b) skred_bank_pedal_up beside skred_bank_stamp_match of the same channel, and beside the only correct route without
    the pedal array -- skred_bank_download_owners and skred_bank_download_env_clocks behind a device wait, the host's pending tags
    mapped to the slots that still carry them, the list uploaded, skred_bank_stamp_slots; (c) the 64-frame block after the pedal-up
    beside the block after stamp_slots of the same slots; (d) skred_bank_tag_slots of 256 slots before the bank has a pedal array and
    after (the clear launch behind the tag kernel).  Medians of 12 with minimum and maximum; host time held, and stream time between
    events."""
    D = device
    n, K, REPS, F, CHANNELS, NOTES = 1 << 20, 4, 12, 64, 16, 256
    VOICES = 0xF
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    v = np.arange(n)
    sel = (v % K) < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 100.0
    e["velocity"][sel], e["is_active"][sel] = 1.0, 1
    e["sample_start"][sel] = np.uint64(now - 40000)
    db = device.DeviceBank(n)
    db.set_tables(tables); db.set_globals(g); db.upload(bank)
    slots = np.arange(0, n, K, dtype=np.int32)
    idx = np.arange(len(slots), dtype=np.uint32)
    tags = (((idx % CHANNELS) + 1) << 24 | (idx // CHANNELS + 1)).astype(np.uint32)
    dl_all = torch.from_numpy(slots).cuda()
    db.tag_slots(dl_all.data_ptr(), tags, K)
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(F, 2, device="cuda")
    m = D.owner_match(3 << 24, 0xFF000000)
    held_at = np.flatnonzero(idx % CHANNELS == 2)[::7][:NOTES]                  # 256 notes of channel 3
    note_tags, note_slots = tags[held_at].copy(), slots[held_at].copy()
    dl_notes = torch.from_numpy(note_slots).cuda()
    torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1)

    def stats(x):
        return f"median {np.median(x):.4f} ms (min {np.min(x):.4f}, max {np.max(x):.4f})"

    def series(call, before=None):
        host, stream = [], []
        for it in range(2 + REPS):
            if before is not None:
                before()
            torch.cuda.synchronize()
            h, s_ms = timed(call)
            if it >= 2:
                host.append(h); stream.append(s_ms)
        return f"host time held {stats(host)}; stream time between events {stats(stream)}"

    retrig = lambda: db.stamp_slots(dl_notes.data_ptr(), NOTES, K, VOICES, D.STAMP_TRIGGER)   # noqa: E731
    hold = lambda: db.release_tags_pedal(0, n, K, VOICES, note_tags, True, res.data_ptr())    # noqa: E731

    def parent_route():
        own = db.download_owners()[::K]                            # the device wait the pedal calls were built to remove
        _, rel = db.download_env_clocks()
        at = {int(t): i for i, t in enumerate(own) if t}           # the host's map: which slot carries which tag now
        lst = np.array([slots[at[int(t)]] for t in note_tags if int(t) in at and rel[slots[at[int(t)]]] == 0], np.int32)
        dl = torch.from_numpy(lst).cuda()
        db.stamp_slots(dl.data_ptr(), len(lst), K, VOICES, D.STAMP_RELEASE)

    print(f"3sk {n} voices = {n // K} slots of {K}, every copy sounding, tagged over {CHANNELS} channels ({n // K // CHANNELS} notes each); "
          f"{NOTES} note-offs of one channel; medians of {REPS}")
    print(f"  (d) tag_slots of {NOTES} slots, no pedal array yet: {series(lambda: db.tag_slots(dl_notes.data_ptr(), note_tags, K))}")
    print(f"  (a) release_tags of {NOTES} tags: {series(lambda: db.release_tags(0, n, K, VOICES, note_tags, D.STAMP_RELEASE, res.data_ptr()), retrig)}; "
          f"d_result = {res.cpu().numpy()[:3].tolist()}")
    print(f"  (a) release_tags_pedal of the same tags, held back: {series(hold, lambda: (retrig(), db.pedal_clear()))}; d_result = {res.cpu().numpy().tolist()}")
    print(f"  (a) release_tags_pedal of the same tags, hold_all 0: {series(lambda: db.release_tags_pedal(0, n, K, VOICES, note_tags, False, res.data_ptr()), lambda: (retrig(), db.pedal_clear()))}; "
          f"d_result = {res.cpu().numpy().tolist()}")
    print(f"  (d) tag_slots of {NOTES} slots with the clear launch behind it: {series(lambda: db.tag_slots(dl_notes.data_ptr(), note_tags, K))}")
    print(f"  (b) pedal_up of the channel: {series(lambda: db.pedal_up(0, n, K, VOICES, m, D.PEDAL_LIFT_SUSTAIN, res.data_ptr()), lambda: (retrig(), hold()))}; "
          f"d_result = {res.cpu().numpy()[:3].tolist()}")
    print(f"  (b) stamp_match of the channel: {series(lambda: db.stamp_match(0, n, K, VOICES, m, D.STAMP_RELEASE, res.data_ptr()), retrig)}; "
          f"d_result = {res.cpu().numpy()[:2].tolist()}")
    print(f"  (b) pedal_latch of the channel: {series(lambda: db.pedal_latch(0, n, K, VOICES, m, res.data_ptr()), lambda: (retrig(), db.pedal_clear()))}; "
          f"d_result = {res.cpu().numpy()[:2].tolist()}")
    db.pedal_clear()
    print(f"  (b) the pedal-up without the array, download_owners + download_env_clocks + host map + list upload + stamp_slots: {series(parent_route, retrig)}")

    def block():
        return timed(lambda: db.render_mix(F, out.data_ptr(), 2, 0, 0))[1]

    def block_after(call, before):
        after = []
        for _ in range(REPS):
            before()
            block()
            call()
            after.append(block())
            block()
        return after
    db.upload(bank)
    for _ in range(8):
        block()
    steady = [block() for _ in range(REPS)]
    after_up = block_after(lambda: db.pedal_up(0, n, K, VOICES, m, D.PEDAL_LIFT_SUSTAIN, res.data_ptr()), lambda: (retrig(), hold()))
    after_slots = block_after(lambda: db.stamp_slots(dl_notes.data_ptr(), NOTES, K, VOICES, D.STAMP_RELEASE), retrig)
    print(f"  (c) the {F}-frame block after pedal_up: {stats(after_up)}; after stamp_slots of the same {NOTES} slots: {stats(after_slots)}; "
          f"a steady block: {stats(steady)}; kernel {db.last_kernel()}, list violations {db.list_violations()}")
    db.close()


def glide():
    """Portamento on bank_patch("3sk", 2**20), every copy sounding and tagged over 16 channels (tag = channel << 24 | slot + 1), 256
    notes of one channel gliding.  (a) skred_bank_glide_tags of the 256 notes and one skred_bank_glide_advance over that channel's
    range (the bank's 16 channels lie interleaved: the range that holds the channel's notes is the whole bank, so the second line is
    the advance over a sixteenth of the bank, the size a channel with a range of its own would have) and over the whole bank, beside
    the parent's route for the same notes: one skred_bank_ctl_tags_each(SKRED_EACH_INC_SCALE) per block; (b) the 64-frame block after
    an advance beside a steady block; (c) skred_bank_tag_slots of 256 slots before the bank has a glide array and after (the clear
    launch behind the tag kernel).  Medians of 12 with minimum and maximum; host time held, and stream time between events."""
    D = device
    n, K, REPS, F, CHANNELS, NOTES = 1 << 20, 4, 12, 64, 16, 256
    VOICES = 0xF
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    v = np.arange(n)
    sel = (v % K) < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 100.0
    e["velocity"][sel], e["is_active"][sel] = 1.0, 1
    e["sample_start"][sel] = np.uint64(now - 40000)
    db = device.DeviceBank(n)
    db.set_tables(tables); db.set_globals(g); db.upload(bank)
    slots = np.arange(0, n, K, dtype=np.int32)
    idx = np.arange(len(slots), dtype=np.uint32)
    tags = (((idx % CHANNELS) + 1) << 24 | (idx // CHANNELS + 1)).astype(np.uint32)
    dl_all = torch.from_numpy(slots).cuda()
    db.tag_slots(dl_all.data_ptr(), tags, K)
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(F, 2, device="cuda")
    at = np.flatnonzero(idx % CHANNELS == 2)[::7][:NOTES]                       # 256 notes of channel 3
    note_tags, note_slots = tags[at].copy(), slots[at].copy()
    dl_notes = torch.from_numpy(note_slots).cuda()
    rate = 2.0 ** (1.0 / 96.0)                                                  # an eighth of a semitone per 64 frames
    slide = D.glide_array([D.glide(D.GLIDE_FROM_SCALE, rate, 1.0 / rate, 2.0 ** (-7.0 / 12.0))] * NOTES)   # a fifth: 56 steps
    bend = D.ctl_each_array([D.ctl_each(D.EACH_INC_SCALE, inc_scale=rate)] * NOTES)
    torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1)

    def stats(x):
        return f"median {np.median(x):.4f} ms (min {np.min(x):.4f}, max {np.max(x):.4f})"

    def series(call, before=None):
        host, stream = [], []
        for it in range(2 + REPS):
            if before is not None:
                before()
            torch.cuda.synchronize()
            h, s_ms = timed(call)
            if it >= 2:
                host.append(h); stream.append(s_ms)
        return f"host time held {stats(host)}; stream time between events {stats(stream)}"

    start = lambda: db.glide_tags(slide, 0, n, K, VOICES, note_tags, res.data_ptr())   # noqa: E731
    land = lambda: db.glide_stop(0, n, True)                                           # noqa: E731

    print(f"3sk {n} voices = {n // K} slots of {K}, every copy sounding, tagged over {CHANNELS} channels ({n // K // CHANNELS} notes each); "
          f"{NOTES} notes of one channel glide; medians of {REPS}")
    print(f"  (c) tag_slots of {NOTES} slots, no glide array yet: {series(lambda: db.tag_slots(dl_notes.data_ptr(), note_tags, K))}")
    print(f"  (a) glide_advance of the whole bank before any glide call (no array: a clear of d_result): {series(lambda: db.glide_advance(0, n, F, res.data_ptr()))}")
    print(f"  (a) the parent's route, ctl_tags_each(INC_SCALE) of {NOTES} tags, once per block: "
          f"{series(lambda: db.ctl_tags_each(None, bend, 0, n, VOICES, note_tags, K, res.data_ptr()))}; d_result = {res.cpu().numpy()[:3].tolist()}")
    db.upload(bank)
    print(f"  (a) glide_tags of {NOTES} tags (FROM_SCALE), once per note: {series(start, land)}; d_result = {res.cpu().numpy()[:3].tolist()}")
    land(); start()
    print(f"  (a) glide_advance by {F} frames over a sixteenth of the bank ({n // CHANNELS} voices): "
          f"{series(lambda: db.glide_advance(0, n // CHANNELS, F, res.data_ptr()))}; d_result = {res.cpu().numpy()[:2].tolist()}")
    land(); start()
    print(f"  (a) glide_advance by {F} frames over the whole bank, {NOTES * K} voices gliding: "
          f"{series(lambda: db.glide_advance(0, n, F, res.data_ptr()))}; d_result = {res.cpu().numpy()[:2].tolist()}")
    land()
    print(f"  (a) glide_advance by {F} frames over the whole bank, nothing gliding: "
          f"{series(lambda: db.glide_advance(0, n, F, res.data_ptr()))}; d_result = {res.cpu().numpy()[:2].tolist()}")
    print(f"  (c) tag_slots of {NOTES} slots with the clear launch behind it: {series(lambda: db.tag_slots(dl_notes.data_ptr(), note_tags, K))}")

    def block():
        return timed(lambda: db.render_mix(F, out.data_ptr(), 2, 0, 0))[1]

    db.upload(bank)
    for _ in range(8):
        block()
    steady = [block() for _ in range(REPS)]
    start()
    after = []
    for _ in range(REPS):                                                       # (56 steps to go: every one of these advances moves 1024 increments)
        block()
        db.glide_advance(0, n, F, res.data_ptr())
        after.append(block())
    moved = res.cpu().numpy()[:2].tolist()
    steady2 = [block() for _ in range(REPS)]
    print(f"  (b) the {F}-frame block after glide_advance (d_result = {moved}): {stats(after)}; a steady block before: {stats(steady)}; "
          f"after: {stats(steady2)}; kernel {db.last_kernel()}, list violations {db.list_violations()}")
    db.close()


def bend():
    """The pitch wheel on bank_patch("3sk", 2**20), every copy sounding and tagged over 16 channels (tag = channel << 24 | slot + 1):
    the `glide` mode's bank.  (a) skred_bank_bend_match of one channel beside skred_bank_ctl_match(SKRED_CTL_INC_SCALE) on the same
    channel, and skred_bank_bend_tags_each of 256 notes beside skred_bank_ctl_tags_each(SKRED_EACH_INC_SCALE); (b) skred_bank_glide_advance
    over the whole bank with 256 notes gliding, before the bank has a bend array and with one (the notes bent); (c) skred_bank_tag_slots
    of 256 slots with the glide clear behind it and with the bend clear as the third; (d) the 64-frame block after a bend beside a
    steady block.  Medians of 12 with minimum and maximum; host time held, and stream time between events."""
    D = device
    n, K, REPS, F, CHANNELS, NOTES = 1 << 20, 4, 12, 64, 16, 256
    VOICES = 0xF
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    v = np.arange(n)
    sel = (v % K) < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 100.0
    e["velocity"][sel], e["is_active"][sel] = 1.0, 1
    e["sample_start"][sel] = np.uint64(now - 40000)
    db = device.DeviceBank(n)
    db.set_tables(tables); db.set_globals(g); db.upload(bank)
    slots = np.arange(0, n, K, dtype=np.int32)
    idx = np.arange(len(slots), dtype=np.uint32)
    tags = (((idx % CHANNELS) + 1) << 24 | (idx // CHANNELS + 1)).astype(np.uint32)
    dl_all = torch.from_numpy(slots).cuda()
    db.tag_slots(dl_all.data_ptr(), tags, K)
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(F, 2, device="cuda")
    at = np.flatnonzero(idx % CHANNELS == 2)[::7][:NOTES]                       # 256 notes of channel 3
    note_tags, note_slots = tags[at].copy(), slots[at].copy()
    dl_notes = torch.from_numpy(note_slots).cuda()
    chan = D.owner_match(3 << 24, 0xFF000000)
    up = 2.0 ** (1.0 / 12.0)
    rate = 2.0 ** (1.0 / 96.0)
    slide = D.glide_array([D.glide(D.GLIDE_FROM_SCALE, rate, 1.0 / rate, 2.0 ** (-7.0 / 12.0))] * NOTES)
    scale_rec = [D.ctl(D.CTL_INC_SCALE, inc_scale=up)] * K
    scale_each = D.ctl_each_array([D.ctl_each(D.EACH_INC_SCALE, inc_scale=up)] * NOTES)
    ratios = np.full(NOTES, up, np.float32)
    torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1)

    def stats(x):
        return f"median {np.median(x):.4f} ms (min {np.min(x):.4f}, max {np.max(x):.4f})"

    def series(call, before=None):
        host, stream = [], []
        for it in range(2 + REPS):
            if before is not None:
                before()
            torch.cuda.synchronize()
            h, s_ms = timed(call)
            if it >= 2:
                host.append(h); stream.append(s_ms)
        return f"host time held {stats(host)}; stream time between events {stats(stream)}"

    start = lambda: db.glide_tags(slide, 0, n, K, VOICES, note_tags, res.data_ptr())   # noqa: E731
    land = lambda: db.glide_stop(0, n, True)                                           # noqa: E731

    print(f"3sk {n} voices = {n // K} slots of {K}, every copy sounding, tagged over {CHANNELS} channels ({n // K // CHANNELS} notes each); "
          f"medians of {REPS}")
    print(f"  (a) ctl_match(INC_SCALE) of one channel over the whole bank: "
          f"{series(lambda: db.ctl_match(scale_rec, 0, n, VOICES, chan, res.data_ptr()))}; d_result = {res.cpu().numpy()[:3].tolist()}")
    print(f"  (a) ctl_tags_each(INC_SCALE) of {NOTES} tags: "
          f"{series(lambda: db.ctl_tags_each(None, scale_each, 0, n, VOICES, note_tags, K, res.data_ptr()))}; d_result = {res.cpu().numpy()[:3].tolist()}")
    db.upload(bank)
    start()
    print(f"  (b) glide_advance by {F} frames over the whole bank, {NOTES * K} voices gliding, no bend array yet: "
          f"{series(lambda: db.glide_advance(0, n, F, res.data_ptr()), lambda: (land(), start()))}; d_result = {res.cpu().numpy()[:2].tolist()}")
    land()
    print(f"  (c) tag_slots of {NOTES} slots with the glide clear behind it: {series(lambda: db.tag_slots(dl_notes.data_ptr(), note_tags, K))}")
    print(f"  (a) bend_match of one channel over the whole bank: "
          f"{series(lambda: db.bend_match(0, n, K, VOICES, chan, up, res.data_ptr()))}; d_result = {res.cpu().numpy()[:3].tolist()}")
    print(f"  (a) bend_match of one channel back to the centre: "
          f"{series(lambda: db.bend_match(0, n, K, VOICES, chan, 1.0, res.data_ptr()), lambda: db.bend_match(0, n, K, VOICES, chan, up))}; "
          f"d_result = {res.cpu().numpy()[:3].tolist()}")
    print(f"  (a) bend_tags_each of {NOTES} tags: "
          f"{series(lambda: db.bend_tags_each(ratios, 0, n, K, VOICES, note_tags, res.data_ptr()))}; d_result = {res.cpu().numpy()[:3].tolist()}")
    land(); start()
    print(f"  (b) glide_advance by {F} frames over the whole bank, {NOTES * K} voices gliding under a bend: "
          f"{series(lambda: db.glide_advance(0, n, F, res.data_ptr()), lambda: (land(), start()))}; d_result = {res.cpu().numpy()[:2].tolist()}")
    land()
    print(f"  (b) glide_advance by {F} frames over the whole bank with a bend array, nothing gliding: "
          f"{series(lambda: db.glide_advance(0, n, F, res.data_ptr()))}; d_result = {res.cpu().numpy()[:2].tolist()}")
    print(f"  (c) tag_slots of {NOTES} slots with the bend clear as the third launch: {series(lambda: db.tag_slots(dl_notes.data_ptr(), note_tags, K))}")

    def block():
        return timed(lambda: db.render_mix(F, out.data_ptr(), 2, 0, 0))[1]

    db.upload(bank)
    db.bend_clear(0, n, False)
    for _ in range(8):
        block()
    steady = [block() for _ in range(REPS)]
    after = []
    for k in range(REPS):
        block()
        db.bend_match(0, n, K, VOICES, chan, 2.0 ** ((k % 5 - 2) / 24.0) if k % 5 != 2 else up, res.data_ptr())
        after.append(block())
    moved = res.cpu().numpy()[:3].tolist()
    db.bend_match(0, n, K, VOICES, chan, 1.0)
    steady2 = [block() for _ in range(REPS)]
    print(f"  (d) the {F}-frame block after bend_match (d_result = {moved}): {stats(after)}; a steady block before: {stats(steady)}; "
          f"after the centre: {stats(steady2)}; kernel {db.last_kernel()}, list violations {db.list_violations()}")
    db.close()


def cutoff():
    """Filter cutoff on the device on bank_patch("3sk", 2**20) with the carriers filtered, every copy sounding and tagged over 16
    channels: the `bend` mode's bank.  (a) skred_bank_cutoff_tags_each(TRACK) of 256 notes beside the parent's route for the same notes
    (skred_filter_coeffs per note on the host, then skred_bank_ctl_tags_each_filter); (b) skred_bank_cutoff_match(TRACK) of one channel
    beside the parent's only route (download_ctl behind a device wait, coefficients per note on the host, ctl_tags_each_filter in
    batches of 1024 tags); (c) skred_bank_cutoff_advance by 64 frames over a sixteenth of the bank, over the whole bank with 1024 voices
    moving and with nothing moving, beside skred_bank_glide_advance on the same ranges and one ctl_tags_each_filter per block; (d)
    skred_bank_tag_slots of 256 slots without and with the cutoff clear behind it; (e) the 64-frame block after an advance beside
    steady blocks.  Medians of 12 with minimum and maximum; host time held, and stream time between events."""
    D = device
    n, K, REPS, F, CHANNELS, NOTES, RATE = 1 << 20, 4, 12, 64, 16, 256, 44100.0
    CARRIERS = 0x7
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    v = np.arange(n)
    sel = (v % K) < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 100.0
    e["velocity"][sel], e["is_active"][sel] = 1.0, 1
    e["sample_start"][sel] = np.uint64(now - 40000)
    bank["voice_filter_mode"][sel] = 1
    for c, x in zip(("b0", "b1", "b2", "a1", "a2"), D.filter_coeffs(1, 2000.0, 0.707, RATE)):
        bank["voice_filter"][c][sel] = x
    size = int(bank["voice_table_size"][0])
    db = device.DeviceBank(n)
    db.set_tables(tables); db.set_globals(g); db.upload(bank)
    slots = np.arange(0, n, K, dtype=np.int32)
    idx = np.arange(len(slots), dtype=np.uint32)
    tags = (((idx % CHANNELS) + 1) << 24 | (idx // CHANNELS + 1)).astype(np.uint32)
    dl_all = torch.from_numpy(slots).cuda()
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(F, 2, device="cuda")
    on3 = np.flatnonzero(idx % CHANNELS == 2)
    at = on3[::7][:NOTES]                                                       # 256 notes of channel 3
    note_tags, note_slots = tags[at].copy(), slots[at].copy()
    dl_notes = torch.from_numpy(note_slots).cuda()
    chan = D.owner_match(3 << 24, 0xFF000000)
    value = 4.0 * 2.0 * np.pi / size
    QM = D.CUTOFF_Q | D.CUTOFF_MODE
    track = D.cutoff(D.CUTOFF_TRACK | QM, value, 0.9, 1)
    track_notes = D.cutoff_array([track] * NOTES)
    sweep = D.cutoff(D.CUTOFF_ABS | D.CUTOFF_GLIDE, 2.5, rate_up=1.0005, rate_down=0.9995)
    slide = D.glide_array([D.glide(D.GLIDE_TO_SCALE, 1.00001, 0.99999, 2.0)] * NOTES)
    torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1)

    def stats(x):
        return f"median {np.median(x):.4f} ms (min {np.min(x):.4f}, max {np.max(x):.4f})"

    def series(call, before=None):
        host, stream = [], []
        for it in range(2 + REPS):
            if before is not None:
                before()
            torch.cuda.synchronize()
            h, s_ms = timed(call)
            if it >= 2:
                host.append(h); stream.append(s_ms)
        return f"host time held {stats(host)}; stream time between events {stats(stream)}"

    def host_coeffs(incs):
        return D.filter_each_array([D.filter_each(*D.filter_coeffs(1, abs(float(i)) * 4.0 * RATE / size, 0.9, RATE)) for i in incs])

    def parent_notes():                                          # the host knows these notes' increments: the note-on's
        filt = host_coeffs(bank["voice_phase_inc"][note_slots])
        db.ctl_tags_each_filter(None, None, filt, 0, n, CARRIERS, 0x1, note_tags, K, res.data_ptr())

    def parent_channel():                                        # after glides and bends the increments are device state
        got = bank.copy()
        db.download_ctl(got)
        filt = host_coeffs(got["voice_phase_inc"][slots[on3]])
        for lo in range(0, len(on3), 1024):
            db.ctl_tags_each_filter(None, None, filt[lo:lo + 1024], 0, n, CARRIERS, 0x1, tags[on3[lo:lo + 1024]], K)

    print(f"3sk {n} voices = {n // K} slots of {K}, carriers filtered, every copy sounding, tagged over {CHANNELS} channels "
          f"({n // K // CHANNELS} notes each); medians of {REPS}")
    print(f"  (d) tag_slots of {NOTES} slots, no cutoff array yet: {series(lambda: db.tag_slots(dl_notes.data_ptr(), note_tags, K))}")
    db.tag_slots(dl_all.data_ptr(), tags, K)
    print(f"  (a) the parent's route for {NOTES} notes (skred_filter_coeffs per note + ctl_tags_each_filter; one set per entry: the first carrier only): {series(parent_notes)}")
    print(f"  (a) cutoff_tags_each(TRACK) of {NOTES} notes: "
          f"{series(lambda: db.cutoff_tags_each(track_notes, 0, n, K, CARRIERS, note_tags, res.data_ptr()))}; d_result = {res.cpu().numpy().tolist()}")
    print(f"  (b) the parent's route for one channel ({len(on3)} notes: download_ctl, coefficients on the host, {-(-len(on3) // 1024)} uploads): "
          f"{series(parent_channel)}")
    print(f"  (b) cutoff_match(TRACK) of one channel over the whole bank: "
          f"{series(lambda: db.cutoff_match(0, n, K, CARRIERS, chan, track, res.data_ptr()))}; d_result = {res.cpu().numpy().tolist()}")
    print(f"  (d) tag_slots of {NOTES} slots with the cutoff clear behind it: {series(lambda: db.tag_slots(dl_notes.data_ptr(), note_tags, K))}")
    db.cutoff_tags_each(track_notes, 0, n, K, 0xF, note_tags)
    print(f"  (c) cutoff_advance by {F} frames over the whole bank, nothing moving: "
          f"{series(lambda: db.cutoff_advance(0, n, F, res.data_ptr()))}; d_result = {res.cpu().numpy()[:2].tolist()}")
    db.cutoff_tags_each(D.cutoff_array([sweep] * NOTES), 0, n, K, 0xF, note_tags, res.data_ptr())
    started = res.cpu().numpy().tolist()
    print(f"  (c) cutoff_advance by {F} frames over the whole bank, {started[0]} voices moving: "
          f"{series(lambda: db.cutoff_advance(0, n, F, res.data_ptr()))}; d_result = {res.cpu().numpy()[:2].tolist()}")
    print(f"  (c) cutoff_advance by {F} frames over a sixteenth of the bank: "
          f"{series(lambda: db.cutoff_advance(0, n // 16, F, res.data_ptr()))}; d_result = {res.cpu().numpy()[:2].tolist()}")
    db.glide_tags(slide, 0, n, K, 0xF, note_tags, res.data_ptr())
    print(f"  (c) glide_advance by {F} frames over the whole bank, {NOTES * K} voices gliding: "
          f"{series(lambda: db.glide_advance(0, n, F, res.data_ptr()))}; d_result = {res.cpu().numpy()[:2].tolist()}")
    print(f"  (c) glide_advance by {F} frames over a sixteenth of the bank: {series(lambda: db.glide_advance(0, n // 16, F, res.data_ptr()))}")
    db.glide_stop(0, n, False)
    print(f"  (c) glide_advance by {F} frames over the whole bank, nothing gliding: {series(lambda: db.glide_advance(0, n, F, res.data_ptr()))}")
    host_filt = host_coeffs(bank["voice_phase_inc"][note_slots])
    print(f"  (c) one ctl_tags_each_filter of {NOTES} notes per block (coefficients given, first carrier only): "
          f"{series(lambda: db.ctl_tags_each_filter(None, None, host_filt, 0, n, CARRIERS, 0x1, note_tags, K, res.data_ptr()))}")

    def block():
        return timed(lambda: db.render_mix(F, out.data_ptr(), 2, 0, 0))[1]

    for _ in range(8):
        block()
    steady = [block() for _ in range(REPS)]
    after = []
    for k in range(REPS):
        block()
        db.cutoff_advance(0, n, F, res.data_ptr())
        after.append(block())
    moved = res.cpu().numpy()[:2].tolist()
    db.cutoff_stop(0, n, False)
    steady2 = [block() for _ in range(REPS)]
    print(f"  (e) the {F}-frame block after cutoff_advance (d_result = {moved}): {stats(after)}; a steady block before: {stats(steady)}; "
          f"after the stop: {stats(steady2)}; kernel {db.last_kernel()}, list violations {db.list_violations()}")
    db.close()


def fenv():
    """The filter envelope on the `cutoff` mode's bank: bank_patch("3sk", 2**20) with the carriers filtered, every copy sounding and
    tagged over 16 channels.  (a) skred_bank_fenv_tags_each of 256 notes beside the parent's route for ONE contour: three
    skred_bank_cutoff_tags_each(GLIDE) calls and, between the first two, the read of cutoff_advance's arrival count behind a device
    wait that times the decay (the third call the parent cannot time at all under a pedal; it is counted as if it could); (b)
    skred_bank_cutoff_advance by 64 frames over the whole bank WITHOUT the array (the plain instantiation: the parent commit's kernel,
    the same code and register figures) and with it: nothing enveloped, 1 024 voices moving, the whole bank resting in sustain;
    (c) the 64-frame block after an advance beside steady blocks.  Medians of 12 with minimum and maximum; host time held, and
    stream time between events."""
    D = device
    n, K, REPS, F, CHANNELS, NOTES, RATE = 1 << 20, 4, 12, 64, 16, 256, 44100.0
    CARRIERS = 0x7
    bank, tables, g = banks.bank_patch("3sk", n)
    now = int(g.synth_sample_count)
    v = np.arange(n)
    sel = (v % K) < 3
    e = bank["voice_amp_envelope"]
    bank["voice_use_amp_envelope"][sel] = 1
    e["attack_time"][sel], e["decay_time"][sel], e["sustain_level"][sel], e["release_time"][sel] = 20.0, 50.0, 0.6, 100.0
    e["velocity"][sel], e["is_active"][sel] = 1.0, 1
    e["sample_start"][sel] = np.uint64(now - 40000)
    bank["voice_filter_mode"][sel] = 1
    for c, x in zip(("b0", "b1", "b2", "a1", "a2"), D.filter_coeffs(1, 2000.0, 0.707, RATE)):
        bank["voice_filter"][c][sel] = x
    size = int(bank["voice_table_size"][0])
    db = device.DeviceBank(n)
    db.set_tables(tables); db.set_globals(g); db.upload(bank)
    slots = np.arange(0, n, K, dtype=np.int32)
    idx = np.arange(len(slots), dtype=np.uint32)
    tags = (((idx % CHANNELS) + 1) << 24 | (idx // CHANNELS + 1)).astype(np.uint32)
    dl_all = torch.from_numpy(slots).cuda()
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(F, 2, device="cuda")
    on3 = np.flatnonzero(idx % CHANNELS == 2)
    note_tags = tags[on3[::7][:NOTES]].copy()                                   # 256 notes of channel 3
    anybody = D.owner_match(0, 0)
    QM = D.CUTOFF_Q | D.CUTOFF_MODE
    track = D.cutoff(D.CUTOFF_TRACK | QM, 4.0 * 2.0 * np.pi / size, 0.9, 1)
    glides = [D.cutoff_array([D.cutoff(D.CUTOFF_TRACK | D.CUTOFF_GLIDE, h * 2.0 * np.pi / size, rate_up=1.5, rate_down=0.9)] * NOTES) for h in (16.0, 8.0, 4.0)]
    contour = D.fenv_array([D.fenv(D.FENV_REL, 4.0, 2.0, 1.0, 1.5, 0.9, 0.8)] * NOTES)
    slow = D.fenv(D.FENV_REL, 4.0, 2.0, 1.0, 1.0005, 0.9995, 0.9995)
    rest = D.fenv(D.FENV_REL, 1.0, 1.0, 1.0, 1.5, 0.9, 0.8)                     # every level is the base: sustain at once
    torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host * 1e3, e0.elapsed_time(e1)

    def stats(x):
        return f"median {np.median(x):.4f} ms (min {np.min(x):.4f}, max {np.max(x):.4f})"

    def series(call, before=None):
        host, stream = [], []
        for it in range(2 + REPS):
            if before is not None:
                before()
            torch.cuda.synchronize()
            h, s_ms = timed(call)
            if it >= 2:
                host.append(h); stream.append(s_ms)
        return f"host time held {stats(host)}; stream time between events {stats(stream)}"

    def parent_contour():
        db.cutoff_tags_each(glides[0], 0, n, K, CARRIERS, note_tags)
        db.cutoff_advance(0, n, F, res.data_ptr())
        res.cpu()                                                # the wait: has the attack landed?
        db.cutoff_tags_each(glides[1], 0, n, K, CARRIERS, note_tags)
        db.cutoff_tags_each(glides[2], 0, n, K, CARRIERS, note_tags)

    def adv():
        db.cutoff_advance(0, n, F, res.data_ptr())

    print(f"3sk {n} voices = {n // K} slots of {K}, carriers filtered, every copy sounding, tagged over {CHANNELS} channels; medians of {REPS}")
    db.tag_slots(dl_all.data_ptr(), tags, K)
    db.cutoff_match(0, n, K, CARRIERS, anybody, track, res.data_ptr())
    print(f"  the base: cutoff_match(TRACK) on every copy: d_result = {res.cpu().numpy().tolist()}")
    print(f"  (b) cutoff_advance by {F} frames over the whole bank, NO fenv array (the parent's kernel), nothing moving: {series(adv)}; d_result = {res.cpu().numpy()[:2].tolist()}")
    print(f"  (a) the parent's route for one contour of {NOTES} notes (three cutoff_tags_each(GLIDE), one advance count read behind a wait): {series(parent_contour)}")
    db.cutoff_stop(0, n, True)
    print(f"  (a) fenv_tags_each of {NOTES} notes: {series(lambda: db.fenv_tags_each(contour, 0, n, K, CARRIERS, note_tags, res.data_ptr()))}; d_result = {res.cpu().numpy().tolist()}")
    db.cutoff_stop(0, n, True)
    print(f"  (b) cutoff_advance by {F} frames over the whole bank, the array present, nothing enveloped: {series(adv)}; d_result = {res.cpu().numpy()[:2].tolist()}")
    db.cutoff_tags_each(D.cutoff_array([track] * NOTES), 0, n, K, 0xF, note_tags)      # all four voices of the notes get a base: 1 024 voices
    db.fenv_tags_each(D.fenv_array([slow] * NOTES), 0, n, K, 0xF, note_tags, res.data_ptr())
    started = res.cpu().numpy().tolist()
    print(f"  (b) cutoff_advance by {F} frames over the whole bank, {started[0]} voices moving in their contours: {series(adv)}; d_result = {res.cpu().numpy()[:2].tolist()}")

    def block():
        return timed(lambda: db.render_mix(F, out.data_ptr(), 2, 0, 0))[1]

    for _ in range(8):
        block()
    steady = [block() for _ in range(REPS)]
    after = []
    for k in range(REPS):
        block()
        adv()
        after.append(block())
    moved = res.cpu().numpy()[:2].tolist()
    print(f"  (c) the {F}-frame block after cutoff_advance (d_result = {moved}): {stats(after)}; a steady block before: {stats(steady)}; "
          f"kernel {db.last_kernel()}, list violations {db.list_violations()}")
    db.fenv_match(0, n, K, CARRIERS, anybody, rest, res.data_ptr())
    started = res.cpu().numpy().tolist()
    stages = db.download_fenv(0, 4096)[:, 0]
    print(f"  (b) cutoff_advance by {F} frames over the whole bank, {started[0]} voices resting in sustain (stages of the first 4096 voices: "
          f"{sorted(set(stages.tolist()))}): {series(adv)}; d_result = {res.cpu().numpy()[:2].tolist()}")
    db.close()


def fxpedal():
    """Pedals on bank_fx(2**20), every voice sounding and tagged over 16 channels (tag = channel << 24 | voice // 16 + 1), 256
    note-offs of one channel held back, then the pedal goes up: the `pedal` mode on the fixed-point bank.  (a) each new call beside
    the only correct route without the pedal array -- skred_fxbank_download_owners and skred_fxbank_download behind a device wait, the
    host's pending tags mapped (numpy: one sort, one search) to the voices that still carry them, the list uploaded,
    skred_fxbank_stamp; (b) skred_fxbank_release_tags_pedal with hold_all 1 and 0 beside skred_fxbank_release_tags of the same tags,
    skred_fxbank_pedal_up and _pedal_latch beside skred_fxbank_stamp_match of the same channel; (c) the 64-frame block after the
    pedal-up beside the block after skred_fxbank_stamp_list of the same voices; (d) skred_fxbank_tag_list of 256 voices before the
    bank has a pedal array and after (the clear launch behind the tag kernel).  Medians of 12 with minimum and maximum; host time
    held, and stream time between events."""
    from skred_amd import fxbank as X
    n, F, CHANNELS, NOTES = 1 << 20, 64, 16, 256
    bank, pool, c0 = X.bank_fx(n)
    db = X.DeviceFxBank(n)
    db.set_tables(pool); db.upload(bank); db.set_sample_count(c0)
    out = torch.zeros(F, 2, dtype=torch.int64, device="cuda")
    v = np.arange(n, dtype=np.int64)
    tags = (((v % CHANNELS) + 1) << 24 | (v // CHANNELS + 1)).astype(np.uint32)
    everyone = torch.arange(n, dtype=torch.int32, device="cuda")
    db.tag_list(everyone.data_ptr(), tags)
    value, mask = 3 << 24, 0xFF000000
    held_at = np.flatnonzero(v % CHANNELS == 2)[::7][:NOTES]                     # 256 notes of channel 3
    note_tags, note_voices = tags[held_at].copy(), held_at.astype(np.int32)
    dl_notes = torch.from_numpy(note_voices).cuda()
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    state = bank.copy()
    torch.cuda.synchronize()

    retrig = lambda: db.stamp_list(dl_notes.data_ptr(), NOTES, X.STAMP_TRIGGER)   # noqa: E731
    hold = lambda: db.release_tags_pedal(0, n, note_tags, True, res.data_ptr())   # noqa: E731
    reset = lambda: (retrig(), db.pedal_clear())                                  # noqa: E731
    pend = lambda: (retrig(), hold())                                             # noqa: E731

    def parent_route():
        own = db.download_owners()                                                # the device waits the pedal calls were built to remove
        db.download(state)
        order = np.argsort(own, kind="stable")                                    # the host's map: which voice carries which tag now
        at = np.minimum(np.searchsorted(own[order], note_tags), n - 1)
        voices = order[at]
        lst = voices[(own[voices] == note_tags) & (state["is_active"][voices] != 0)].astype(np.int32)
        db.stamp(lst, X.FX_STAMP_RELEASE)

    def line(label, call, words, before=None):
        ms, held = _fx_timed(call, before)
        print(f"  {label}: host held {_fx_stats(held)}; stream time between events {_fx_stats(ms)}; d_result = {res.cpu().numpy().tolist()[:words]}")

    print(f"fx {n} voices all sounding, tagged over {CHANNELS} channels ({n // CHANNELS} notes each); {NOTES} note-offs of one channel")
    line(f"(d) tag_list of {NOTES} voices, no pedal array yet", lambda: db.tag_list(dl_notes.data_ptr(), note_tags), 0)
    line(f"(b) release_tags of {NOTES} tags", lambda: db.release_tags(0, n, note_tags, X.STAMP_RELEASE, res.data_ptr()), 3, retrig)
    line("(b) release_tags_pedal of the same tags, held back (hold_all 1)", hold, 4, reset)
    line("(b) release_tags_pedal of the same tags, hold_all 0", lambda: db.release_tags_pedal(0, n, note_tags, False, res.data_ptr()), 4, reset)
    line(f"(a) stamp_owned_pedal of the same {NOTES} voices, held back",
         lambda: db.stamp_owned_pedal(dl_notes.data_ptr(), note_tags, True, res.data_ptr()), 4, reset)
    line(f"(d) tag_list of {NOTES} voices with the clear launch behind it", lambda: db.tag_list(dl_notes.data_ptr(), note_tags), 0)
    line("(a) pedal_up of the channel", lambda: db.pedal_up(0, n, value, mask, X.PEDAL_LIFT_SUSTAIN, res.data_ptr()), 3, pend)
    line("(b) stamp_match of the channel", lambda: db.stamp_match(0, n, value, mask, X.STAMP_RELEASE, res.data_ptr()), 2, retrig)
    line("(a) pedal_latch of the channel", lambda: db.pedal_latch(0, n, value, mask, res.data_ptr()), 2, reset)
    db.pedal_clear()
    line("(a) the pedal-up without the array, download_owners + download + host map + list upload + stamp", parent_route, 0, retrig)

    def block_after(call, before):
        after = []
        for _ in range(12):
            before()
            _fx_block_after(db, out, F, None, 1)
            call()
            after += _fx_block_after(db, out, F, None, 1)
            _fx_block_after(db, out, F, None, 1)
        return after
    db.upload(bank); db.set_sample_count(c0)
    _fx_block_after(db, out, F, None, 8)
    steady = _fx_block_after(db, out, F)
    after_up = block_after(lambda: db.pedal_up(0, n, value, mask, X.PEDAL_LIFT_SUSTAIN, res.data_ptr()), pend)
    after_list = block_after(lambda: db.stamp_list(dl_notes.data_ptr(), NOTES, X.STAMP_RELEASE), retrig)
    print(f"  (c) the {F}-frame block after pedal_up: {_fx_stats(after_up)}; after stamp_list of the same {NOTES} voices: {_fx_stats(after_list)}; "
          f"a steady block: {_fx_stats(steady)}")
    db.close()


def fxglide():
    """Portamento on bank_fx(2**20), every voice sounding and tagged over 16 channels (tag = channel << 24 | voice // 16 + 1), 256
    notes of one channel gliding: the `glide` mode on the fixed-point bank.  (a) skred_fxbank_glide_tags of the 256 tags, and
    skred_fxbank_glide_advance by 64 frames over one channel's range (a sixteenth of the bank), over the whole bank with the 256
    voices gliding, over the whole bank with nothing gliding and on a bank without the array, beside the route the bank had before:
    one skred_fxbank_ctl_tags_each(SKRED_EACH_INC_SCALE) of the 256 tags per block; (b) the 64-frame block after an advance beside a
    steady block before and after it; (c) skred_fxbank_tag_list of 256 voices before the bank has a glide array and with the clear
    launch behind it.  Medians of 12 with minimum and maximum; host time held, and stream time between events."""
    from skred_amd import fxbank as X
    n, F, CHANNELS, NOTES = 1 << 20, 64, 16, 256
    bank, pool, c0 = X.bank_fx(n)
    db, bare = X.DeviceFxBank(n), X.DeviceFxBank(n)
    for d in (db, bare):
        d.set_tables(pool); d.upload(bank); d.set_sample_count(c0)
    out = torch.zeros(F, 2, dtype=torch.int64, device="cuda")
    v = np.arange(n, dtype=np.int64)
    tags = (((v % CHANNELS) + 1) << 24 | (v // CHANNELS + 1)).astype(np.uint32)
    everyone = torch.arange(n, dtype=torch.int32, device="cuda")
    db.tag_list(everyone.data_ptr(), tags)
    at = np.flatnonzero(v % CHANNELS == 2)[::7][:NOTES]                          # 256 notes of channel 3
    note_tags, note_voices = tags[at].copy(), at.astype(np.int32)
    dl_notes = torch.from_numpy(note_voices).cuda()
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    # a slow slide into each note from a fifth below: a third of a semitone per second, so that nobody arrives while the lines are timed
    r = 2.0 ** (0.33 / 12.0 * 64.0 / 48000.0)
    up, down = max(1, int((r - 1.0) * 2.0 ** 32)), max(1, int((1.0 - 1.0 / r) * 2.0 ** 32))
    glides = X.glide_array([X.glide(X.FX_GLIDE_FROM_SCALE, up, down, int(2.0 ** (-7.0 / 12.0) * 65536.0)) for _ in range(NOTES)])
    each = X.fx_each_array([X.fx_each(X.EACH_INC_SCALE, inc_scale_q16=65542) for _ in range(NOTES)])
    torch.cuda.synchronize()

    restore = lambda: db.upload(bank)                                             # noqa: E731 (the struck increments back)
    start = lambda: db.glide_tags(glides, 0, n, note_tags, res.data_ptr())        # noqa: E731
    armed = lambda: (restore(), start())                                          # noqa: E731

    def line(label, call, words, before=None):
        ms, held = _fx_timed(call, before)
        print(f"  {label}: host held {_fx_stats(held)}; stream time between events {_fx_stats(ms)}; d_result = {res.cpu().numpy().tolist()[:words]}")

    print(f"fx {n} voices all sounding, tagged over {CHANNELS} channels ({n // CHANNELS} notes each); {NOTES} notes of one channel glide")
    line(f"(c) tag_list of {NOTES} voices, no glide array yet", lambda: db.tag_list(dl_notes.data_ptr(), note_tags), 0)
    line("(a) glide_advance by 64 frames on a bank without the array (a clear of d_result)", lambda: bare.glide_advance(0, n, F, res.data_ptr()), 2)
    line(f"(a) glide_tags of {NOTES} tags", start, 3, restore)
    line(f"(c) tag_list of {NOTES} voices with the clear launch behind it", lambda: db.tag_list(dl_notes.data_ptr(), note_tags), 0)
    armed()
    line(f"(a) glide_advance by 64 frames over a sixteenth of the bank ({n // CHANNELS} voices)",
         lambda: db.glide_advance(int(note_voices[0]), n // CHANNELS, F, res.data_ptr()), 2)
    armed()
    line(f"(a) glide_advance by 64 frames over the whole bank, {NOTES} voices gliding", lambda: db.glide_advance(0, n, F, res.data_ptr()), 2)
    db.glide_stop(0, n, True)
    line("(a) glide_advance by 64 frames over the whole bank, nothing gliding", lambda: db.glide_advance(0, n, F, res.data_ptr()), 2)
    restore()
    line(f"(a) the route before: ctl_tags_each(INC_SCALE) of the {NOTES} tags, once per block",
         lambda: db.ctl_tags_each(None, each, 0, n, note_tags, res.data_ptr()), 3)

    db.upload(bank); db.set_sample_count(c0)
    start()
    _fx_block_after(db, out, F, None, 8)
    before = _fx_block_after(db, out, F)
    after = _fx_block_after(db, out, F, lambda: db.glide_advance(0, n, F, res.data_ptr()))
    later = _fx_block_after(db, out, F)
    print(f"  (b) the {F}-frame block after an advance ({NOTES} increments moved): {_fx_stats(after)}; a steady block before it: "
          f"{_fx_stats(before)}; after it: {_fx_stats(later)}")
    db.close(); bare.close()


def fxbend():
    """The pitch wheel on bank_fx(2**20), every voice sounding and tagged over 16 channels as in `fxexpr` / `fxglide`: the `bend` mode
    on the fixed-point bank.  Each new call beside its INC_SCALE counterpart in the same run: (a) skred_fxbank_bend_match of one
    channel over the whole bank against skred_fxbank_ctl_match(SKRED_CTL_INC_SCALE) of the same channel; (b)
    skred_fxbank_bend_tags_each of 256 notes against skred_fxbank_ctl_tags_each(SKRED_EACH_INC_SCALE) of the same tags; (c)
    skred_fxbank_glide_advance by 64 frames over the whole bank, 256 voices gliding, on a bank with a bend array (the BEND
    instantiation) and on one without; (d) skred_fxbank_tag_list of 256 voices with the glide clear behind it, and with the bend clear
    as the third launch; (e) the 64-frame block after a bend_match beside a steady block before and after it.  Medians of 12 with
    minimum and maximum; host time held, and stream time between events."""
    from skred_amd import fxbank as X
    n, F, CHANNELS, NOTES = 1 << 20, 64, 16, 256
    bank, pool, c0 = X.bank_fx(n)
    db, plain = X.DeviceFxBank(n), X.DeviceFxBank(n)                              # plain: glides, never a bend
    for d in (db, plain):
        d.set_tables(pool); d.upload(bank); d.set_sample_count(c0)
    out = torch.zeros(F, 2, dtype=torch.int64, device="cuda")
    v = np.arange(n, dtype=np.int64)
    tags = (((v % CHANNELS) + 1) << 24 | (v // CHANNELS + 1)).astype(np.uint32)
    everyone = torch.arange(n, dtype=torch.int32, device="cuda")
    for d in (db, plain):
        d.tag_list(everyone.data_ptr(), tags)
    at = np.flatnonzero(v % CHANNELS == 2)[::7][:NOTES]                          # 256 notes of channel 3
    note_tags, note_voices = tags[at].copy(), at.astype(np.int32)
    dl_notes = torch.from_numpy(note_voices).cuda()
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    value, mask = 3 << 24, 0xFF000000
    r = 2.0 ** (0.33 / 12.0 * 64.0 / 48000.0)
    up, down = max(1, int((r - 1.0) * 2.0 ** 32)), max(1, int((1.0 - 1.0 / r) * 2.0 ** 32))
    glides = X.glide_array([X.glide(X.FX_GLIDE_FROM_SCALE, up, down, int(2.0 ** (-7.0 / 12.0) * 65536.0)) for _ in range(NOTES)])
    each = X.fx_each_array([X.fx_each(X.EACH_INC_SCALE, inc_scale_q16=65542) for _ in range(NOTES)])
    ratios = np.full(NOTES, X.bend_ratio_q24(0.5), np.uint32)
    scale = X.fx_ctl(X.CTL_INC_SCALE, inc_scale_q16=65542)
    torch.cuda.synchronize()

    def line(label, call, words, before=None):
        ms, held = _fx_timed(call, before)
        print(f"  {label}: host held {_fx_stats(held)}; stream time between events {_fx_stats(ms)}; d_result = {res.cpu().numpy().tolist()[:words]}")

    print(f"fx {n} voices all sounding, tagged over {CHANNELS} channels ({n // CHANNELS} notes each)")
    for d in (db, plain):
        d.glide_tags(glides, 0, n, note_tags, res.data_ptr())                      # both banks hold a glide array, 256 voices gliding
    line(f"(d) tag_list of {NOTES} voices, the glide clear behind it", lambda: plain.tag_list(dl_notes.data_ptr(), note_tags), 0)
    line("(a) ctl_match(INC_SCALE) of one channel over the whole bank", lambda: db.ctl_match(scale, 0, n, value, mask, res.data_ptr()), 3,
         lambda: db.upload(bank))
    db.upload(bank)
    line("(a) bend_match of one channel over the whole bank", lambda: db.bend_match(0, n, value, mask, X.bend_ratio_q24(1.0), res.data_ptr()), 3)
    db.bend_match(0, n, value, mask, X.FX_BEND_ONE)
    line(f"(b) ctl_tags_each(INC_SCALE) of {NOTES} tags", lambda: db.ctl_tags_each(None, each, 0, n, note_tags, res.data_ptr()), 3,
         lambda: db.upload(bank))
    db.upload(bank)
    line(f"(b) bend_tags_each of {NOTES} tags", lambda: db.bend_tags_each(ratios, 0, n, note_tags, res.data_ptr()), 3)
    line(f"(d) tag_list of {NOTES} voices, the glide and the bend clear behind it", lambda: db.tag_list(dl_notes.data_ptr(), note_tags), 0)
    for d in (db, plain):
        d.upload(bank)
        d.glide_tags(glides, 0, n, note_tags, res.data_ptr())
    db.bend_tags_each(ratios, 0, n, note_tags, res.data_ptr())                     # the gliding voices are bent: the re-derived store runs
    line(f"(c) glide_advance by 64 frames over the whole bank, {NOTES} voices gliding, no bend array",
         lambda: plain.glide_advance(0, n, F, res.data_ptr()), 2)
    line(f"(c) glide_advance by 64 frames over the whole bank, {NOTES} voices gliding under a bend",
         lambda: db.glide_advance(0, n, F, res.data_ptr()), 2)

    db.glide_stop(0, n, True); db.bend_clear(0, n, True)
    db.upload(bank); db.set_sample_count(c0)
    _fx_block_after(db, out, F, None, 8)
    before = _fx_block_after(db, out, F)
    pos = [0]

    def wheel():
        pos[0] += 1
        db.bend_match(0, n, value, mask, X.bend_ratio_q24(0.01 * (pos[0] % 100) + 0.01), res.data_ptr())

    after = _fx_block_after(db, out, F, wheel)
    later = _fx_block_after(db, out, F)
    print(f"  (e) the {F}-frame block after a bend_match ({n // CHANNELS} increments moved): {_fx_stats(after)}; a steady block before it: "
          f"{_fx_stats(before)}; after it: {_fx_stats(later)}")
    db.close(); plain.close()


def fxcutoff():
    """Filter cutoff on bank_fx(2**20) with filters, every voice sounding and tagged over 16 channels as in `fxglide` / `fxbend`: the
    `cutoff` mode on the fixed-point bank.  (a) skred_fxbank_cutoff_tags_each(TRACK) of 256 notes beside the route the bank had
    before: 256 coefficient sets on the host (fxbank.q30_coeffs at 4 x each note's frequency) and skred_fxbank_ctl_tags_each_filter;
    (b) skred_fxbank_cutoff_match(TRACK) of one channel beside a download of the parameters, the channel's coefficients on the host
    and an update of its voices; (c) skred_fxbank_cutoff_advance by 64 frames over the whole bank with nothing moving, 1 024 voices
    moving and a sixteenth of the bank moving, skred_fxbank_glide_advance beside it in the same states; (d) the 64-frame block after
    an advance beside steady blocks before and after it.  Medians of 12 with minimum and maximum; host time held, and stream time
    between events."""
    from skred_amd import fxbank as X
    n, F, CHANNELS, NOTES, SR = 1 << 20, 64, 16, 256, 48000
    bank, pool, c0 = X.bank_fx(n)
    db = X.DeviceFxBank(n)
    db.set_tables(pool); db.upload(bank); db.set_sample_count(c0)
    out = torch.zeros(F, 2, dtype=torch.int64, device="cuda")
    v = np.arange(n, dtype=np.int64)
    tags = (((v % CHANNELS) + 1) << 24 | (v // CHANNELS + 1)).astype(np.uint32)
    everyone = torch.arange(n, dtype=torch.int32, device="cuda")
    db.tag_list(everyone.data_ptr(), tags)
    chan = np.flatnonzero(v % CHANNELS == 2)                                     # channel 3
    at = chan[::7][:NOTES]
    note_tags = tags[at].copy()
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    value, mask = 3 << 24, 0xFF000000
    track4 = int(round(4.0 * 2.0 * np.pi * (1 << 24)))
    both = X.FX_CUTOFF_Q | X.FX_CUTOFF_MODE
    first = X.fx_cutoff(X.FX_CUTOFF_TRACK | both, track4, 2 << 16, 1)
    recs = X.fx_cutoff_array([first] * NOTES)
    r = 2.0 ** (0.33 / 12.0 * 64.0 / SR)                                         # a third of a semitone per second: nobody arrives while timed
    up, down = max(1, int((r - 1.0) * 2.0 ** 32)), max(1, int((1.0 - 1.0 / r) * 2.0 ** 32))
    sweep = X.fx_cutoff(X.FX_CUTOFF_TRACK | X.FX_CUTOFF_GLIDE, 2 * track4, 0, 0, up, down)
    glides = X.glide_array([X.glide(X.FX_GLIDE_FROM_SCALE, up, down, int(2.0 ** (-7.0 / 12.0) * 65536.0)) for _ in range(1024)])
    view = bank.copy()
    torch.cuda.synchronize()

    def host_coeffs(idx):
        freq = 4.0 * view["phase_inc"][idx].astype(np.float64) / 4294967296.0 * SR
        return X.q30_coeffs(np.ones(len(idx), np.int32), np.minimum(freq, 0.45 * SR).astype(np.float32), np.full(len(idx), 2.0, np.float32), SR)

    def parent_notes():                                                          # the host knows these notes' increments: the note-on's
        c = host_coeffs(at)
        filt = X.fx_filter_each_array([X.fx_filter_each(*(int(c[k][i]) for k in ("b0_q30", "b1_q30", "b2_q30", "a1_q30", "a2_q30"))) for i in range(NOTES)])
        db.ctl_tags_each_filter(None, None, filt, 0, n, note_tags, res.data_ptr())

    def parent_channel():                                                        # after glides and bends the increments are device state
        db.download_params(view)
        c = host_coeffs(chan)
        for k in c:
            view[k][chan] = c[k]
        db.update(view, chan.astype(np.int32), X.DIRTY_PARAMS)

    def line(label, call, words, before=None):
        ms, held = _fx_timed(call, before)
        print(f"  {label}: host held {_fx_stats(held)}; stream time between events {_fx_stats(ms)}; d_result = {res.cpu().numpy().tolist()[:words]}")

    print(f"fx {n} voices with filters, all sounding, tagged over {CHANNELS} channels ({n // CHANNELS} notes each)")
    line(f"(a) the route before: {NOTES} coefficient sets on the host + ctl_tags_each_filter", parent_notes, 3)
    line(f"(a) cutoff_tags_each(TRACK) of {NOTES} tags", lambda: db.cutoff_tags_each(recs, 0, n, note_tags, res.data_ptr()), 4)
    line(f"(b) the route before: download_params, {len(chan)} coefficient sets on the host, update of the channel", parent_channel, 0)
    line("(b) cutoff_match(TRACK) of one channel over the whole bank", lambda: db.cutoff_match(0, n, value, mask, first, res.data_ptr()), 4)
    db.glide_tags(glides[:NOTES], 0, n, note_tags, res.data_ptr()); db.glide_stop(0, n, True)     # the glide array exists, nothing glides
    line("(c) cutoff_advance by 64 frames over the whole bank, nothing moving", lambda: db.cutoff_advance(0, n, F, res.data_ptr()), 2)
    line("(c) glide_advance by 64 frames over the whole bank, nothing gliding", lambda: db.glide_advance(0, n, F, res.data_ptr()), 2)
    many = chan[:1024]
    db.cutoff_tags_each(X.fx_cutoff_array([sweep] * 1024), 0, n, tags[many], res.data_ptr())
    db.glide_tags(glides, 0, n, tags[many], res.data_ptr())
    line("(c) cutoff_advance by 64 frames over the whole bank, 1024 voices moving", lambda: db.cutoff_advance(0, n, F, res.data_ptr()), 2)
    line("(c) glide_advance by 64 frames over the whole bank, 1024 voices gliding", lambda: db.glide_advance(0, n, F, res.data_ptr()), 2)
    db.cutoff_match(0, n, value, mask, sweep, res.data_ptr())
    for k in range(0, len(chan), 1024):
        db.glide_tags(glides, 0, n, tags[chan[k:k + 1024]], res.data_ptr())
    line(f"(c) cutoff_advance by 64 frames over the whole bank, a sixteenth of it ({len(chan)} voices) moving", lambda: db.cutoff_advance(0, n, F, res.data_ptr()), 2)
    line(f"(c) glide_advance by 64 frames over the whole bank, a sixteenth of it ({len(chan)} voices) gliding", lambda: db.glide_advance(0, n, F, res.data_ptr()), 2)

    db.glide_stop(0, n, True); db.cutoff_stop(0, n, False)
    db.upload(bank); db.set_sample_count(c0)
    db.cutoff_tags_each(X.fx_cutoff_array([sweep] * 1024), 0, n, tags[many], res.data_ptr())
    _fx_block_after(db, out, F, None, 8)
    before = _fx_block_after(db, out, F)
    after = _fx_block_after(db, out, F, lambda: db.cutoff_advance(0, n, F, res.data_ptr()))
    later = _fx_block_after(db, out, F)
    print(f"  (d) the {F}-frame block after an advance (1024 voices' coefficients moved): {_fx_stats(after)}; a steady block before it: "
          f"{_fx_stats(before)}; after it: {_fx_stats(later)}")
    db.close()


def fxfenv():
    """The filter envelope on the fixed-point bank: the time of skred_fxbank_cutoff_advance by 64 frames over bank_fx(2**20), every
    voice tagged and holding a cutoff word, as in `fxcutoff`.  (a) a bank without an fenv array: the ENV = false kernel, the one the
    bank had before the envelope; (b) a bank with the array and no contour: the ENV = true kernel, one more 4-byte load per voice; (c)
    every voice of that bank in a moving stage (an attack that crawls: nobody arrives while timed), and beside it every voice of the
    plain bank moving by a cutoff glide of the same rate -- the same steps and coefficient stores without the envelope's loads; (d)
    skred_fxbank_fenv_match of the whole bank and skred_fxbank_fenv_tags_each of 256 notes.  (a) and (b) alternate in one session.
    Medians of 12 with minimum and maximum; host time held, and stream time between events."""
    from skred_amd import fxbank as X
    n, F, CHANNELS, NOTES = 1 << 20, 64, 16, 256
    bank, pool, c0 = X.bank_fx(n)
    v = np.arange(n, dtype=np.int64)
    tags = (((v % CHANNELS) + 1) << 24 | (v // CHANNELS + 1)).astype(np.uint32)
    everyone = torch.arange(n, dtype=torch.int32, device="cuda")
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    base = X.fx_cutoff(X.FX_CUTOFF_ABS | X.FX_CUTOFF_Q | X.FX_CUTOFF_MODE, 1 << 24, 2 << 16, 1)
    crawl = X.fx_fenv(X.FX_FENV_ABS, 1 << 28, 1 << 26, 1 << 22, 1, 1, 1)          # one unit of w per 64 frames: 2^28 - 2^24 steps away
    glide = X.fx_cutoff(X.FX_CUTOFF_ABS | X.FX_CUTOFF_GLIDE, 1 << 28, 0, 0, 1, 1)
    banks = []
    for _ in range(2):
        db = X.DeviceFxBank(n)
        db.set_tables(pool); db.upload(bank); db.set_sample_count(c0)
        db.tag_list(everyone.data_ptr(), tags)
        db.cutoff_match(0, n, 0, 0, base, res.data_ptr())
        banks.append(db)
    plain, env = banks
    env.fenv_match(0, n, 0x7F000000, 0xFF000000, crawl, res.data_ptr())            # a channel nobody is on: the array exists, no contour
    torch.cuda.synchronize()
    assert not env.download_fenv(0, 4096).any() and res.cpu().numpy().tolist()[:3] == [0, 0, n]
    at = np.flatnonzero(v % CHANNELS == 2)[::7][:NOTES]

    def line(label, call, words):
        ms, held = _fx_timed(call, None)
        print(f"  {label}: host held {_fx_stats(held)}; stream time between events {_fx_stats(ms)}; d_result = {res.cpu().numpy().tolist()[:words]}")
        return float(np.median(ms))

    print(f"fx {n} voices, all tagged, every voice with a cutoff word; cutoff_advance by {F} frames over the whole bank")
    a, b = [], []
    for k in range(3):                                                           # alternating: the same session, the same clocks
        a.append(line(f"(a) no fenv array (ENV = false), nothing moving, round {k}", lambda: plain.cutoff_advance(0, n, F, res.data_ptr()), 2))
        b.append(line(f"(b) fenv array, no contour (ENV = true), nothing moving, round {k}", lambda: env.cutoff_advance(0, n, F, res.data_ptr()), 2))
    print(f"  (b) / (a), medians of the three rounds: {np.median(b):.4f} ms / {np.median(a):.4f} ms = {np.median(b) / np.median(a):.3f}")
    line("(d) fenv_match of the whole bank (every voice enters the attack)", lambda: env.fenv_match(0, n, 0, 0, crawl, res.data_ptr()), 4)
    plain.cutoff_match(0, n, 0, 0, glide, res.data_ptr())
    line("(c) fenv array, every voice in the attack", lambda: env.cutoff_advance(0, n, F, res.data_ptr()), 2)
    line("(c) no fenv array, every voice moving by a cutoff glide of the same rate", lambda: plain.cutoff_advance(0, n, F, res.data_ptr()), 2)
    line(f"(d) fenv_tags_each of {NOTES} tags", lambda: env.fenv_tags_each(X.fx_fenv_array([crawl] * NOTES), 0, n, tags[at], res.data_ptr()), 4)
    plain.close(); env.close()


SCENARIOS = {"kernels": kernels, "crossover": crossover, "overhead": overhead, "frames": frames, "fm": fm,
             "noise": noise, "live": live, "patches": patches, "linear": linear, "mid": mid, "cross": cross, "taps": taps, "idle": idle, "steal": steal, "cz": cz, "fxlive": fxlive, "fxsteal": fxsteal, "slots": slots, "slotsteal": slotsteal, "ctl": ctl, "owners": owners, "fxowners": fxowners, "fxctl": fxctl, "expr": expr, "fxexpr": fxexpr, "timbre": timbre, "fxtimbre": fxtimbre, "chan": chan, "fxchan": fxchan, "pedal": pedal, "fxpedal": fxpedal, "glide": glide, "fxglide": fxglide, "bend": bend, "cutoff": cutoff, "fenv": fenv, "fxbend": fxbend, "fxcutoff": fxcutoff, "fxfenv": fxfenv}

if __name__ == "__main__":
    names = sys.argv[1:] or list(SCENARIOS)
    for nm in names:
        if nm not in SCENARIOS:
            sys.exit(f"unknown scenario {nm!r}; one of: {', '.join(SCENARIOS)}")
    for nm in names:
        print(f"== {nm}")
        SCENARIOS[nm]()
