"""The Dirichlet distance through the segment tree (wost_device.h poly_distance_tree)
returns the bits of the full scan (poly_distance) that it replaces.

Host only: the device geometry (__host__ __device__) and the tree builder are compiled for
the host (tests/native/dtree_check.cpp) and fuzzed; the generated kernel source is inspected
and compiled for gfx950 without a device. The walks themselves: tests/test_gpu_dirichlet_tree.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dtree_shapes as SH
from dcrmontecarlo_amd import _lib
from dcrmontecarlo_amd import fields as F
from dcrmontecarlo_amd import scenarios as S
from dcrmontecarlo_amd.geometry import PolyLinesSimple
from dcrmontecarlo_amd.solvers.WoStSolver import kernel_source, kernel_source_points

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LEAVES = (1, 10, 32)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dtree") / "libdtree_check.so")
    src = [os.path.join(HERE, "native", "dtree_check.cpp"), os.path.join(REPO, "dcrmontecarlo_amd", "csrc", "wost_tree.cpp")]
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950",
                    "-I" + os.path.join(REPO, "include"), "-x", "hip", src[0], "-x", "c++", src[1], "-o", out],
                   check=True)
    lib = ctypes.CDLL(out)
    fp, lp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_long)
    lib.dtree_check.argtypes = [fp, ctypes.c_int, ctypes.c_int, fp, ctypes.c_long, lp, lp]
    lib.dtree_check.restype = ctypes.c_int
    lib.dtree_usable.argtypes = [fp, ctypes.c_int]
    lib.dtree_usable.restype = ctypes.c_int
    lib.dtree_variant_differs.restype = ctypes.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def check(lib, verts, pts, leaf):
    """(mismatches, record visits, leaf visits, leaves) of the tree against the scan."""
    verts = np.ascontiguousarray(verts, np.float32)
    pts = np.ascontiguousarray(pts, np.float32)
    out = (ctypes.c_long * 4)()
    bad = ctypes.c_long(-1)
    assert lib.dtree_check(_p(verts), verts.shape[0], leaf, _p(pts), pts.shape[0], out, ctypes.byref(bad)) == 0
    assert out[0] == 0, (f"{out[0]} of {pts.shape[0]} queries differ from the scan (leaf {leaf}); first: "
                         f"point {pts[bad.value].tolist()}")
    return list(out)


def usable(lib, verts):
    verts = np.ascontiguousarray(verts, np.float32)
    return bool(lib.dtree_usable(_p(verts), verts.shape[0]))


NGONS = [(nv, r, c) for nv in (3, 11, 64, 65, 641, 6001) for r, c in ((1.0, (0.0, 0.0)), (300.0, (1000.0, -2000.0)))]


@pytest.mark.parametrize("nv,r,c", NGONS)
def test_tree_equals_scan_on_ngons(harness, nv, r, c):
    verts = SH.ngon(nv, r, c)
    assert usable(harness, verts)
    pts = SH.query_points(verts, np.random.default_rng(nv))
    pts = np.concatenate([pts, np.array([c], np.float32)])   # the centre: every segment ties
    for leaf in LEAVES:
        check(harness, verts, pts, leaf)


@pytest.mark.parametrize("name", ["zigzag", "sine", "thin_rectangle"])
def test_tree_equals_scan_on_open_and_thin_polylines(harness, name):
    verts = getattr(SH, name)()
    assert {"zigzag": 257, "sine": 1001, "thin_rectangle": 2049}[name] == len(verts)
    assert usable(harness, verts)
    pts = SH.query_points(verts, np.random.default_rng(len(verts)))
    for leaf in LEAVES:
        check(harness, verts, pts, leaf)


def test_tree_equals_scan_on_random_polylines(harness):
    """60 random polylines of 5-400 vertices with coordinates 0.1..16."""
    rng = np.random.default_rng(21)
    for verts in SH.random_polylines():
        assert usable(harness, verts)
        pts = SH.query_points(verts, rng)
        for leaf in LEAVES:
            check(harness, verts, pts, leaf)


def test_usability(harness):
    sq = SH.resample([[0, 0], [1, 0], [1, 1], [0, 1], [0, 0]], 64)
    assert usable(harness, sq)
    rep = np.insert(sq, 7, sq[7], axis=0)                     # a repeated vertex: a zero-length segment
    assert not usable(harness, rep)
    bad = sq.copy()
    bad[5, 0] = np.inf
    assert not usable(harness, bad)
    bad[5, 0] = np.nan
    assert not usable(harness, bad)
    big = sq.copy()
    big[5, 1] = 2.0 ** 61
    assert not usable(harness, big)
    big[5, 1] = 2.0 ** 60
    assert usable(harness, big)
    tiny = (sq * np.float32(1e-30)).astype(np.float32)       # squared lengths underflow to 0
    assert not usable(harness, tiny)


def test_the_tree_is_a_tree(harness):
    """A guard against a bound that never prunes, not a performance figure: on the
    6001-vertex circle with 10 segments per leaf (600 leaves) the mean number of leaves a
    query visits, over points with 0.5 <= |p| <= 0.99 or |p| >= 1.01, is at most a quarter
    of the leaves. Measured: 2.09 leaves (and 8.3 record visits) per query."""
    verts = SH.ngon(6001)
    rng = np.random.default_rng(3)
    r = np.concatenate([rng.uniform(0.5, 0.99, 20000), rng.uniform(1.01, 3.0, 20000)])
    th = rng.uniform(0, 2 * np.pi, r.size)
    pts = np.stack([r * np.cos(th), r * np.sin(th)], 1).astype(np.float32)
    rr = np.hypot(pts[:, 0].astype(np.float64), pts[:, 1])
    pts = pts[((rr >= 0.5) & (rr <= 0.99)) | (rr >= 1.01)]
    _, recs, leaves, nleaves = check(harness, verts, pts, 10)
    assert nleaves == 600
    mean = leaves / len(pts)
    print(f"leaves visited per query: {mean:.3f}; record visits per query: {recs / len(pts):.3f}")
    assert mean <= 150.0, mean


def test_default_threshold_is_the_headers():
    """_lib's copy of WOST_DTREE_MIN_SEGMENTS_DEFAULT / WOST_DTREE_LEAF_DEFAULT against include/wost.h."""
    import re

    text = open(os.path.join(REPO, "include", "wost.h")).read()
    val = lambda name: int(re.search(rf"#define {name}\s+\(?(-?\d+)\)?", text).group(1))
    assert val("WOST_DTREE_MIN_SEGMENTS_DEFAULT") == _lib.WOST_DTREE_MIN_SEGMENTS_DEFAULT
    assert val("WOST_DTREE_LEAF_DEFAULT") == _lib.WOST_DTREE_LEAF_DEFAULT


def test_kernel_variant_compares_dirichlet_tree(harness):
    assert harness.dtree_variant_differs() == 1


# ---- generated source (wost_kernel_source*, no device) ----------------------------------

def _ngon_source(nv, **kw):
    return kernel_source(PolyLinesSimple(SH.ngon(nv)), F.X**2 - F.Y**2, **kw)


def test_source_is_unchanged_without_the_tree():
    """Below the threshold, and with the tree forbidden, the source is byte for byte the one
    generated without the feature's option."""
    for name in ("laplace_square", "dcr_dipole", "variable_coefficients"):
        sc = S.ALL[name]()
        base = sc.kernel_source()
        assert "dirichlet tree" not in base and "poly_distance_tree" not in base and "DIRICHLET_TREE" not in base
        assert sc.kernel_source(dirichlet_tree=-1) == base
        assert sc.kernel_source(dirichlet_tree=_lib.WOST_DTREE_MIN_SEGMENTS_DEFAULT) == base
        # compiled-in polylines keep poly_distance_const even when the tree is forced
        assert sc.kernel_source(dirichlet_tree=0) == base
    off = _ngon_source(641, dirichlet_tree=-1)
    assert "dirichlet tree" not in off and "poly_distance_tree" not in off and "DIRICHLET_TREE" not in off
    assert _ngon_source(641, dirichlet_tree=100_000) == off
    assert "wost::poly_distance(sD, nd, x, y)" in off
    dflt = _lib.WOST_DTREE_MIN_SEGMENTS_DEFAULT
    assert dflt < 0 or dflt >= 128
    if dflt < 0 or dflt > 640:
        assert _ngon_source(641) == off
    small = _ngon_source(65)                                  # the 64-gons of the staged-scan tests
    assert small == _ngon_source(65, dirichlet_tree=-1)


def test_source_names_the_tree_when_forced():
    on = _ngon_source(641, dirichlet_tree=0)
    head = [ln for ln in on.splitlines() if ln.startswith("// generated by libwost")]
    assert len(head) == 1 and head[0].endswith(", dirichlet tree"), head
    assert "#define WOST_DIRICHLET_TREE 1" in on
    assert "wost::poly_distance_tree(" in on and "wost::poly_distance(sD" not in on
    assert on != _ngon_source(641, dirichlet_tree=-1)
    assert _ngon_source(641, dirichlet_tree=0, dirichlet_tree_leaf=32) == on   # the leaf size is run-time data


def test_repeated_vertex_keeps_the_scan_even_when_forced():
    verts = SH.ngon(641)
    rep = np.insert(verts, 100, verts[100], axis=0)
    src = kernel_source(PolyLinesSimple(rep), F.X**2 - F.Y**2, dirichlet_tree=0)
    assert "poly_distance_tree" not in src and "dirichlet tree" not in src
    assert src == kernel_source(PolyLinesSimple(rep), F.X**2 - F.Y**2, dirichlet_tree=-1)


def _compiles(src: str):
    n, used = ctypes.c_int64(), ctypes.c_int32(-1)
    rc = _lib.lib.wost_jit_compile(src.encode(), b"gfx950", 0, None, 0, ctypes.byref(n), ctypes.byref(used))
    assert rc == 0, _lib.lib.wost_last_error().decode()
    assert n.value > 1000


def _rect_with_line(nd_seg=600, nn_seg=600):
    """The rectangle [0,1] x [-0.5,1] with the zero-flux line y = 0 across it
    (tests/test_gpu_long_polylines.py), both resampled."""
    D = SH.resample([[0, -0.5], [1, -0.5], [1, 1], [0, 1], [0, -0.5]], nd_seg)
    xs = np.linspace(1.0, 0.0, nn_seg + 1, dtype=np.float32)
    N = np.stack([xs, np.zeros(nn_seg + 1, np.float32)], axis=1)
    return D, N


def test_forced_sources_compile_for_gfx950():
    _compiles(_ngon_source(641, dirichlet_tree=0))
    D, N = _rect_with_line()
    both = kernel_source(PolyLinesSimple(D), F.X, PolyLinesSimple(N), dirichlet_tree=0)
    assert "+tree" in both and "dirichlet tree" in both          # both trees in one kernel
    _compiles(both)
    pc = kernel_source_points(PolyLinesSimple(D), None, PolyLinesSimple(N), n_charges=2, n_sources=1,
                              compat="fixed", dirichlet_tree=0)
    assert "+fixed" in pc and "dirichlet tree" in pc
    _compiles(pc)
