"""The launch plan of a solve (dcrmontecarlo_amd/csrc/wost_launch.cpp: SolveRanges,
next_batch, launch_shape) is HIP-free, so its arithmetic is checked on the host:
tests/native/launch_check.cpp plans solves with a batch limit of three blocks (the
multi-batch paths a solve reaches only above 2^26 walks), maps every local walk of every
batch back to its (point, walk), matches the range validation's messages and compares
launch_shape with shapes worked by hand."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "dcrmontecarlo_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_launch_plan_on_the_host(tmp_path):
    exe = str(tmp_path / "launch_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(REPO, "include"),
                    os.path.join(HERE, "native", "launch_check.cpp"), os.path.join(CSRC, "wost_launch.cpp"),
                    os.path.join(CSRC, "wost_options.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "launch_check: 0 failed checks" in r.stdout
