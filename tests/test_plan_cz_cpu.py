"""SKRED_OPT_CZ_FAST in the block planner, on the CPU: tests/c_plan_cz_cases.c includes skred_amd/csrc/skred_bank_plan.h (the real
structs), links libskred_amd.so the way tests/test_plan_cpu.py builds its cases and runs without a bank or a GPU.  Its expected
values are written into the C file, derived by hand from the rule; it prints one line per case."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_cz") / "c_plan_cz_cases")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(HERE, "c_plan_cz_cases.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"), "-lskred_amd", "-lm", "-lpthread",
           "-Wl,-rpath," + os.path.join(ROOT, "skred_amd")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return out.stdout.strip().splitlines()


def test_cz_plan_cases(lines):
    cases = [l for l in lines if l.startswith("cz/")]
    assert len(cases) >= 20, "\n".join(lines)
    bad = [l for l in cases if not l.endswith(" ok")]
    assert not bad, "\n".join(bad)
    assert lines[-1] == "OK"


@pytest.mark.parametrize("what", ["option off", "option on", "2^20", "1048576", "global-table", "SKB_ANY_MOD", "packed", "skew", "taps"])
def test_cz_plan_covers(lines, what):
    """the cases the planner's rule is made of each ran (and passed: test_cz_plan_cases)"""
    words = {"2^20": "2^20-voice", "packed": "packed lanes", "skew": "fm_skew 1"}
    assert any(words.get(what, what) in l for l in lines), what


def test_option_and_query_are_exported():
    """SKRED_OPT_CZ_FAST = 12 and skred_bank_last_cz in the public header; the symbol in the library (no bank is created)."""
    import ctypes
    with open(os.path.join(ROOT, "include", "skred_amd.h")) as f:
        text = f.read()
    assert "SKRED_OPT_CZ_FAST = 12" in text
    assert "skred_bank_last_cz(const skred_bank_t *" in text
    lib = ctypes.CDLL(os.path.join(ROOT, "skred_amd", "libskred_amd.so"))
    assert hasattr(lib, "skred_bank_last_cz")
    lib.skred_bank_last_cz.argtypes = [ctypes.c_void_p]
    assert lib.skred_bank_last_cz(None) == 0
