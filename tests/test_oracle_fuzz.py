"""Pins oracle/cpu_ref.c to the compiled reference on FUZZED banks (tests/oracle_fuzz_replay.py).

The ten hand-written fixtures of test_oracle_vs_golden.py hold one modulation case; the GPU fuzz tests build banks far outside
them (CZ modes with CZ modulators of any kind, modulation by one-shots that stop, by reversed / noise / held / crushed voices,
envelopes in every stage, self references).  Here such banks meet the reference itself, live, wherever its library is built
(__graft_entry__.build() makes it where the reference tree is mounted; it then travels with the tree).
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libskred_ref.so")
REFERENCE = os.environ.get("SKRED_REFERENCE", "/root/reference")
SEEDS = max(24, int(os.environ.get("SKRED_FUZZ_SEEDS", "24")))


def ensure_ref_lib():
    if os.path.isdir(REFERENCE):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    # build() makes the library and it travels with the tree: without it this tier has not run, which is a failure, not a skip
    assert os.path.exists(REF_SO), "oracle/_ref/libskred_ref.so not built (__graft_entry__.build() makes it from the reference tree)"


def test_oracle_equals_reference_on_fuzzed_banks():
    ensure_ref_lib()
    out = subprocess.run([sys.executable, os.path.join(HERE, "oracle_fuzz_replay.py"), str(SEEDS)],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert len(res) == SEEDS
    kinds = set()
    for r in res:
        assert 4 <= r["segments"] <= 6
        assert r["bad"] == [], f"seed {r['seed']}: the oracle differs from the reference: {r['bad']}"
        kinds |= set(r["kinds"])
    assert kinds >= {"mute", "unmute", "note_off", "retrigger", "repoint_own", "unplug", "depth", "phase_inc", "cz_on", "cz_off"}
