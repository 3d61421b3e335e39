"""Builds and runs tests/c_fx_ctl_host.c once for tests/test_fx_owner_cpu.py and tests/test_fx_ctl_cpu.py: the host side of the
fixed-point bank's note owners and controllers on a bank that is nothing but its size.  Returns the program's lines."""
import functools
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "skred_amd", "csrc")


@functools.lru_cache(maxsize=1)
def lines():
    exe = os.path.join(tempfile.mkdtemp(prefix="fx_ctl_host"), "c_fx_ctl_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
           os.path.join(HERE, "c_fx_ctl_host.c"), "-o", exe, "-L" + os.path.join(ROOT, "skred_amd"), "-lskred_amd", "-lm", "-lpthread",
           "-Wl,-rpath," + os.path.join(ROOT, "skred_amd")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode in (0, 1), (out.stdout[-500:], out.stderr[-1500:])
    return tuple(out.stdout.strip().splitlines())


def group(name):
    mine = [l for l in lines() if l.startswith(name + "/")]
    assert mine, f"no case of group {name} ran"
    bad = [l for l in mine if not l.endswith(" ok")]
    assert not bad, "\n".join(bad)
    return mine
