"""The point-list walk kernels, the parts that need no device: without a list
the generated kernel sources are byte for byte what they were before the list existed
(tests/golden/kernel_source_parent.json: SHA-256 of every case below, recorded with the
parent commit's library by `python tests/test_point_list_source.py --record`); with one they
define WOST_POINT_LIST, name the list in their header line and compile for gfx950; and
KernelVariant::point_list takes part in the kernel cache's comparison."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "kernel_source_parent.json")
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

from dcrmontecarlo_amd import _lib  # noqa: E402
from dcrmontecarlo_amd import fields as F  # noqa: E402
from dcrmontecarlo_amd import scenarios as S  # noqa: E402

SCENARIOS = ("dcr_dipole", "variable_coefficients", "wenner_topography")
KINDS = ("plain", "sources3", "wavenumbers2", "models2")


def _scenario(name):
    if name == "wenner_topography":
        return S.wenner_topography(n_electrodes=4, n_walks=1, n_segments=200)
    return S.ALL[name](6)


def _kwargs(sc, kind):
    if kind == "sources3":
        return {"sources": [sc.f, 2.0 * sc.f, 3.0 * sc.f]}
    if kind == "wavenumbers2":
        return {"n_wavenumbers": 2}
    if kind == "models2":
        return {"models": [(sc.sigma, sc.alpha), (sc.sigma, F.const(0.01))]}
    return {}


def _sha(text: str) -> str:
    return hashlib.sha256(text.encode()).hexdigest()


def _head(src: str) -> str:
    return [l for l in src.splitlines() if l.startswith("// generated")][0]


@pytest.mark.parametrize("name", SCENARIOS)
def test_sources_without_a_list_are_the_parents(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    sc = _scenario(name)
    for kind in KINDS:
        src = sc.kernel_source(**_kwargs(sc, kind))
        assert "WOST_POINT_LIST" not in src and "point list" not in _head(src)
        assert _sha(src) == golden[f"{name}/{kind}"], f"{name}/{kind}: the generated source changed"
        assert sc.kernel_source(point_list=False, **_kwargs(sc, kind)) == src


@pytest.mark.parametrize("name", SCENARIOS)
def test_sources_with_a_list_name_it_and_compile(name):
    sc = _scenario(name)
    for kind in KINDS:
        plain = sc.kernel_source(**_kwargs(sc, kind))
        src = sc.kernel_source(point_list=True, **_kwargs(sc, kind))
        assert src.count("#define WOST_POINT_LIST 1\n") == 1
        assert _head(src) == _head(plain) + ", point list"
        # nothing else differs
        assert src.replace("#define WOST_POINT_LIST 1\n", "").replace(", point list\n", "\n", 1) == plain
        n, used = ctypes.c_int64(), ctypes.c_int32(-1)
        rc = _lib.lib.wost_jit_compile(src.encode(), b"gfx950", 0, None, 0, ctypes.byref(n), ctypes.byref(used))
        assert rc == 0, _lib.lib.wost_last_error().decode()
        assert n.value > 1000


def test_new_entry_points_are_declared_and_exported():
    names = _lib.declared_symbols()
    for n in ("wost_solve_range_points", "wost_kernel_source_point_list"):
        assert n in names
        assert hasattr(_lib.lib, n), f"libwost.so does not export {n}"
    assert _lib.lib.wost_version() == 6   # additive: the ABI version stays


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_variants_that_differ_in_point_list_compare_unequal(tmp_path):
    """tests/native/variant_point_list_check.cpp, built stand-alone with the address and
    undefined-behaviour sanitizers when the compiler has them (host code only)."""
    src = os.path.join(HERE, "native", "variant_point_list_check.cpp")
    exe = str(tmp_path / "variant_point_list_check")
    san = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", src, "-o", exe])
    if san.returncode != 0:
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "variant_point_list_check: 0 failed checks" in r.stdout


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    out = {}
    for name in SCENARIOS:
        sc = _scenario(name)
        for kind in KINDS:
            out[f"{name}/{kind}"] = _sha(sc.kernel_source(**_kwargs(sc, kind)))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(out)} hashes")
