"""The block planner on the CPU: tests/c_plan_cases.c includes skred_amd/csrc/skred_bank_plan.h (the real structs), links
libskred_amd.so the way tests/test_c_abi.py builds its programs and runs without a bank or a GPU.  Its expected values are
written into the C file, derived by hand from the selection rules; it prints one line per case.  The planner's own sources
must also compile as plain C with no ROCm include path."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")

GROUPS = ["family", "stems", "fast2_min_user", "fm_pair", "guard", "pack", "probe", "split", "inplace", "class", "levels", "tape"]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "c_plan_cases")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(HERE, "c_plan_cases.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"), "-lskred_amd", "-lm", "-lpthread",
           "-Wl,-rpath," + os.path.join(ROOT, "skred_amd")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return out.stdout.strip().splitlines()


@pytest.mark.parametrize("group", GROUPS)
def test_plan_cases(lines, group):
    mine = [l for l in lines if l.startswith(group + "/")]
    assert mine, f"no case of group {group} ran"
    bad = [l for l in mine if not l.endswith(" ok")]
    assert not bad, "\n".join(bad)


def test_every_case_passed(lines):
    assert lines[-1] == "OK", "\n".join(l for l in lines if not l.endswith(" ok"))
    assert all(l.split("/")[0] in GROUPS for l in lines[:-1])


def test_planner_is_plain_c(tmp_path):
    """No HIP header, no bank: gcc alone, warnings as errors, only the public header and the layout beside it."""
    out = subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c",
                          os.path.join(CSRC, "skred_bank_plan.c"), "-o", str(tmp_path / "plan.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    for name in ("skred_bank_plan.c", "skred_bank_plan.h"):
        with open(os.path.join(CSRC, name)) as f:
            includes = [l for l in f if l.lstrip().startswith("#include")]
        assert not [l for l in includes if "hip" in l or "skred_bank_priv.h" in l or "skred_launch.h" in l], includes
