"""The source sample's clip comparison (wost_device.h norm_greater) is bit for bit the
reference's sqrtf(a2) > sqrtf(b2) (solvers/WoStSolver.py:248): every mantissa of b2 in
six binades (subnormal, smallest normal, around the 2^-100 floor, 1, the last one), a2
ulp by ulp across the band above b2 and octaves beyond, and the special values."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def test_norm_greater_is_the_sqrt_comparison(tmp_path):
    out = str(tmp_path / "libclip_compare_check.so")
    # host build of the __host__ __device__ header; -ffp-contract=off like the kernels' geometry
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950",
                    "-ffp-contract=off", "-pthread", "-I" + os.path.join(REPO, "include"), "-x", "hip",
                    os.path.join(HERE, "native", "clip_compare_check.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    c = (ctypes.c_long * 7)()
    assert lib.clip_compare_check(c) == 0
    bad, n_b2, swept, special, sure, band, not_greater = list(c)
    print(f"b2 values {n_b2}, swept pairs {swept}, special pairs {special}: "
          f"ratio-decided {sure}, band {band}, not greater {not_greater}, mismatches {bad}")
    assert n_b2 == 6 * (1 << 23)
    # per b2: 8 below, b2 itself, 8 above the rounded product, 4 octaves (the first 8
    # subnormals have fewer floats below them), and the >= 16 ulps up to the product in
    # the four normal binades whose product neither overflows nor rounds in subnormal steps
    assert swept >= n_b2 * (8 + 1 + 8 + 4) - 36 + 16 * 4 * (1 << 23)
    assert special == 24 * 24
    assert sure + band + not_greater == swept + special   # no pair skipped
    assert sure > 0 and band > 0
    assert bad == 0
