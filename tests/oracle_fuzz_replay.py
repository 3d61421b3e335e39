"""Differential fuzz of oracle/cpu_ref.c against the compiled reference (oracle/_ref/libskred_ref.so), in one process.

For every seed a random 64-voice bank of tests/fuzz_banks.py (modulators anywhere in the bank) is written into the reference's own
arrays (tests/golden/gen_golden.py: inject_bank), rendered in four to six segments of odd callback sizes with control actions
between them, and the same segments are replayed through oracle.cpuref.synth from the state the reference started with.  Nothing
is masked: every stem, the mix, every per-voice field and the globals are compared bit for bit after every segment.  The noise
LCG lives in a function-static of synth(); its state follows from the number of frames rendered so far (Ref.noise_rng).
Prints one JSON line.  usage: oracle_fuzz_replay.py N_SEEDS
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import cpuref  # noqa: E402
from skred_amd.bank import FIELD_NAMES  # noqa: E402

LIB = os.path.join(ROOT, "oracle", "_ref", "libskred_ref.so")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def field_mismatches(a, b):
    """{field: voices that differ} over EVERY field of the two banks, whole structs included (the table binding aside: both banks
    come from the same snapshot)."""
    bad = {}
    for k in FIELD_NAMES:
        if k == "voice_table_offset":
            continue
        x, y = a.a[k], b.a[k]
        m = int((bits(x).reshape(a.n, -1) != bits(y).reshape(b.n, -1)).any(axis=1).sum())
        if m:
            bad[k] = m
    return bad


def main():
    n_seeds = int(sys.argv[1])
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "golden", "gen_golden.py"))
    gg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gg)
    ref = gg.Ref(LIB)
    cat = gg.fuzz_setup(ref)
    res = []
    for seed in range(n_seeds):
        bank, segs, count0 = gg.fuzz_plan(seed, cat)
        gg.inject_bank(ref, bank, cat, count0)
        ob, tables = ref.snapshot()
        og = ref.globals()
        r = {"seed": seed, "segments": len(segs), "frames": 0, "bad": [], "kinds": []}
        for k, (frames, block, acts) in enumerate(segs):
            for a in acts:
                gg.apply_action(ref, a)
                a.apply(ob, og.synth_sample_count)
                r["kinds"].append(a.kind)
            mix, stems = ref.render(frames, block)
            want_bank, _ = ref.snapshot()
            want_g = ref.globals()
            got_mix = np.zeros_like(mix)
            got_stems = np.zeros_like(stems)
            p = 0
            while p < frames:
                n = min(block, frames - p)
                got_mix[p:p + n], got_stems[p:p + n] = cpuref.synth(ob, og, tables, n, 2, 0, want_stems=True)
                p += n
            bad = {}
            if not (np.isfinite(mix).all() and np.isfinite(stems).all()):
                bad["reference_not_finite"] = True
            if not (bits(got_stems) == bits(stems)).all():
                bad["stems"] = int((bits(got_stems).reshape(frames, ref.V, -1) != bits(stems).reshape(frames, ref.V, -1)).any(axis=(0, 2)).sum())
            if not (bits(got_mix) == bits(mix)).all():
                bad["mix"] = int((got_mix != mix).any(axis=1).sum())
            state = field_mismatches(ob, want_bank)
            if state:
                bad["state"] = state
            if og.synth_sample_count != want_g.synth_sample_count:
                bad["synth_sample_count"] = [int(og.synth_sample_count), int(want_g.synth_sample_count)]
            if og.noise_rng != want_g.noise_rng:
                bad["noise_rng"] = [int(og.noise_rng), int(want_g.noise_rng)]
            for f in ("volume_final", "volume_smoother_gain", "volume_smoother_smoothing"):
                if np.float32(getattr(og, f)).tobytes() != np.float32(getattr(want_g, f)).tobytes():
                    bad[f] = [float(getattr(og, f)), float(getattr(want_g, f))]
            if bad:
                r["bad"].append({"segment": k, "frames": frames, "block": block, **bad})
            r["frames"] += frames
            r["mix_rms"] = float(np.sqrt(np.mean(mix.astype(np.float64) ** 2)))
        res.append(r)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
