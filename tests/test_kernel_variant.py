"""Which walk kernel a solve runs is named by plain structs (dcrmontecarlo_amd/csrc/
wost_variant.h: WalkTraits, KernelVariant), so the naming is checked on the host:
tests/native/variant_check.cpp goes through all 32 trait combinations (18 valid, every
spelling distinct), changes every field of a KernelVariant one at a time (the handle's kernel
cache compares variants), and compares the walk kernels' LDS size (wost_walk.h
walk_lds_bytes) with the values of the two-level function it replaced. The first two parts
build with g++ from the header alone; the LDS size's constants live in the device headers,
so that part builds as HIP for the host."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "variant_check.cpp")


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "variant_check: 0 failed checks" in r.stdout
    return r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_variant_header_is_hip_free(tmp_path):
    exe = str(tmp_path / "variant_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", SRC, "-o", exe], check=True)
    assert "LDS" not in _run(exe)


def test_walk_lds_bytes_on_the_host(tmp_path):
    exe = str(tmp_path / "variant_check_hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-Wall", "--offload-host-only",
                    "-I" + os.path.join(REPO, "include"), "-x", "hip", SRC, "-o", exe], check=True)
    assert "variant_check (with the LDS size): 0 failed checks" in _run(exe)
