"""The launch plan and the kernels' id arithmetic with a point list (wost_solve_range_points,
DESIGN.md 7d), on the host. tests/native/point_list_check.cpp compiles wost_walk.h's
WOST_WALK_OF_LOCAL with WOST_POINT_LIST, fills the kernel's arguments from the real launch
plan (wost_launch.cpp plan_ranges / next_batch with a list) and compares every (walk id, point)
with plain integer arithmetic: the list of all points, of the last point alone and one with
gaps; more walks than a batch holds (range_point0 > 0); Wr = 49 at walk_begin = 4096, where
the quotient's ++q correction must fire; W = 2^40 + 1000. It also checks the lists that
plan_ranges refuses. tests/test_gpu_point_list.py runs the same ids on the device."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "dcrmontecarlo_amd", "csrc")


def test_point_list_plan_and_ids_on_the_host(tmp_path):
    exe = str(tmp_path / "point_list_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-host-only", "-I" + os.path.join(REPO, "include"),
                    "-x", "hip", os.path.join(HERE, "native", "point_list_check.cpp"),
                    "-x", "c++", os.path.join(CSRC, "wost_launch.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "point_list_check: 0 failed checks" in r.stdout
    m = re.search(r"(\d+) indices in (\d+) batches \((\d+) with range_point0 > 0\), \+\+q (\d+),", r.stdout)
    assert m and all(int(g) > 0 for g in m.groups()), r.stdout
