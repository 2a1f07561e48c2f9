"""A walk's result depends only on its id, and the id enters the walk kernels at one place:
the refill of walk_body turns a launch's local index into a global walk id and a point index
(wost_walk.h WOST_WALK_OF_LOCAL), by a double-precision quotient estimate and one correction,
on three paths (walk-range batches, 32-bit offsets, 64 bits). tests/native/walk_ids_check.cpp
compiles that very text for the host, fills the kernel's arguments from the real launch plan
(wost_launch.cpp) and compares every local index with exact integer division: every W in
[1, 8192], 49 * 2^k and 98 * 2^k (whose estimates need the ++q correction), walk counts around
2^31 and up to 2^53 / 3, both sides of the 32-bit switch. The ++q correction must fire on
all three paths; the per-path counts are printed (pytest -s).
tests/test_gpu_walk_ids.py runs the same ids on the device."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "dcrmontecarlo_amd", "csrc")


def test_walk_ids_on_the_host(tmp_path):
    exe = str(tmp_path / "walk_ids_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-host-only", "-I" + os.path.join(REPO, "include"),
                    "-x", "hip", os.path.join(HERE, "native", "walk_ids_check.cpp"),
                    "-x", "c++", os.path.join(CSRC, "wost_launch.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "walk_ids_check: 0 failed checks" in r.stdout
    up = {m.group(1): int(m.group(2)) for m in re.finditer(r"path (\S+) .* \+\+q +(\d+),", r.stdout)}
    assert set(up) == {"range", "small32", "64-bit"} and all(v > 0 for v in up.values()), r.stdout
