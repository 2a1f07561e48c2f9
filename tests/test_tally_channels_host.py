"""Channel maps (DESIGN.md 7f "Channel maps"), the parts that need no device: the kernel's
combination rule as the library restates it for the host (wost_device.h tally_weighted, the
kernels' own text) against numpy float32 evaluated term by term; the weight refusals; the
generated sources with WOST_TALLY_MAPS; KernelVariant::tally_maps in the kernel cache's
comparison; the row base of the [p][r][t] layout; the exports; and the facade's chunking on a
stubbed launch. tests/test_gpu_tally_channels.py runs the kernels."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from dcrmontecarlo_amd import _lib
from dcrmontecarlo_amd import greens_map as G
from dcrmontecarlo_amd import scenarios as S
from dcrmontecarlo_amd.solvers.WoStSolver import WostSolver_2D

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = ctypes.POINTER(ctypes.c_float)


def _weighted(d, w):
    d = np.ascontiguousarray(d, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    n, C = d.shape
    T = w.shape[0]
    out = np.empty((n, T), np.float32)
    rc = _lib.lib.wost_tally_weighted(d.ctypes.data_as(F32), n, C, w.ctypes.data_as(F32), T, out.ctypes.data_as(F32))
    assert rc == 0, _lib.lib.wost_last_error().decode()
    return out


def _numpy_weighted(d, w):
    """v = 0; for c ascending: if w[c] != 0: v = fl(v + fl(w[c] * d[c])), all float32."""
    d, w = d.astype(np.float32), w.astype(np.float32)
    out = np.zeros((d.shape[0], w.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for t in range(w.shape[0]):
            v = np.zeros(d.shape[0], np.float32)
            for c in range(d.shape[1]):
                if w[t, c] != 0:
                    p = (w[t, c] * d[:, c]).astype(np.float32)
                    v = (v + p).astype(np.float32)
            out[:, t] = v
    return out


# ---- 1. the combination ---------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 2, 6, 16])
@pytest.mark.parametrize("T", [1, 4])
def test_combination_matches_numpy_term_by_term(C, T):
    rng = np.random.default_rng(100 * C + T)
    n = 4096
    # deposits over many binades, weights of both signs; some weights exactly zero
    d = (rng.standard_normal((n, C)) * 10.0 ** rng.uniform(-6, 3, (n, C))).astype(np.float32)
    w = (rng.standard_normal((T, C)) * 10.0 ** rng.uniform(-2, 2, (T, C))).astype(np.float32)
    if C > 2:
        w[rng.random((T, C)) < 0.25] = 0.0
        w[:, 0] = np.where((w != 0).any(axis=1), w[:, 0], 1.0)
    got, want = _weighted(d, w), _numpy_weighted(d, w)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    # the sum is not fused: where a fused multiply-add would differ, the result is the unfused one
    if C >= 2:
        fused = np.zeros((n, T), np.float64)
        for c in range(C):
            fused = (fused + w[None, :, c].astype(np.float64) * d[:, c, None].astype(np.float64)).astype(np.float32)
        assert (fused.astype(np.float32) != want).any()   # (the data do tell the two apart)


def test_unit_rows_return_the_channels_bits_and_zero_weights_skip():
    rng = np.random.default_rng(7)
    C = 6
    d = (rng.standard_normal((512, C)) * 10.0 ** rng.uniform(-8, 4, (512, C))).astype(np.float32)
    d[:, 1] = np.nan
    d[:, 3] = np.inf
    d[::2, 4] = -np.inf
    for c in (0, 2, 5):
        got = _weighted(d, np.eye(C, dtype=np.float32)[c:c + 1])
        assert got[:, 0].view(np.uint32).tolist() == d[:, c].view(np.uint32).tolist()
    # a zero weight skips a NaN; a non-zero one does not
    w = np.zeros((2, C), np.float32)
    w[0, [0, 2]] = 0.5, -2.0
    w[1, [0, 1]] = 0.5, 1.0
    got = _weighted(d, w)
    assert np.isfinite(got[:, 0]).all() and np.isnan(got[:, 1]).all()
    assert got[:, 0].view(np.uint32).tolist() == _numpy_weighted(d, w)[:, 0].view(np.uint32).tolist()


# ---- 2. weight refusals ---------------------------------------------------------------------

def _check(w, T, C):
    a = None if w is None else np.ascontiguousarray(w, np.float32)
    rc = _lib.lib.wost_tally_check_weights(None if a is None else a.ctypes.data_as(F32), T, C)
    return rc, _lib.lib.wost_last_error().decode()


def test_weight_refusals():
    good = np.array([[1.0, 0.0, -2.0], [0.0, 0.0, 1e-30]], np.float32)
    assert _check(good, 2, 3)[0] == 0
    assert _check(np.ones((_lib.WOST_TALLY_MAX_MAPS, 16)), _lib.WOST_TALLY_MAX_MAPS, 16)[0] == 0
    for T in (0, -1, _lib.WOST_TALLY_MAX_MAPS + 1):
        rc, msg = _check(np.ones((8, 3)), T, 3)
        assert rc != 0 and "n_maps" in msg
    for C in (0, _lib.WOST_MAX_SOURCES + 1):
        rc, msg = _check(np.ones((2, 32)), 2, C)
        assert rc != 0 and "channels" in msg
    rc, msg = _check(None, 2, 3)
    assert rc != 0 and "NULL" in msg
    for bad in (np.nan, np.inf, -np.inf):
        w = good.copy()
        w[1, 1] = bad
        rc, msg = _check(w, 2, 3)
        assert rc != 0 and "[1][1]" in msg and "finite" in msg
    w = good.copy()
    w[1] = 0.0
    rc, msg = _check(w, 2, 3)
    assert rc != 0 and "row 1" in msg and "zero" in msg
    w[1, 2] = -0.0   # (a negative zero is a zero)
    assert _check(w, 2, 3)[0] != 0


# ---- 3. generated sources -------------------------------------------------------------------

def _head(src: str) -> str:
    return [l for l in src.splitlines() if l.startswith("// generated")][0]


def _compile(src: str):
    n, used = ctypes.c_int64(), ctypes.c_int32(-1)
    rc = _lib.lib.wost_jit_compile(src.encode(), b"gfx950", 0, None, 0, ctypes.byref(n), ctypes.byref(used))
    return rc, n.value, _lib.lib.wost_last_error().decode()


def _scenarios():
    return {"dcr_dipole": S.ALL["dcr_dipole"](6),
            "wenner_topography": S.wenner_topography(n_electrodes=4, n_walks=1, n_segments=200)}


def _two_models(sc):
    return [(sc.sigma, sc.alpha), (sc.sigma, sc.alpha * 1.25)]


@pytest.mark.parametrize("name", ["dcr_dipole", "wenner_topography"])
@pytest.mark.parametrize("K,T,models", [(1, 1, False), (1, 4, False), (3, 1, False), (3, 4, False), (2, 3, True),
                                        (0, 2, True)])
def test_sources_with_maps_differ_by_the_macro_alone_and_compile(name, K, T, models):
    sc = _scenarios()[name]
    kw = {"compat": "fixed", "n_wavenumbers": K, **({"models": _two_models(sc)} if models else {})}
    plain = sc.kernel_source(**kw)
    assert "WOST_TALLY" not in plain and "tally" not in _head(plain)
    assert sc.kernel_source(tally_maps=0, **kw) == plain
    src = sc.kernel_source(tally_maps=T, **kw)
    macro = f"#define WOST_TALLY_MAPS {T}\n"
    suffix = f", {T} tally map" + ("s" if T > 1 else "")
    assert src.count(macro) == 1 and "#define WOST_TALLY 1" not in src
    assert _head(src) == _head(plain) + suffix
    if name == "wenner_topography":
        assert "+tree" in _head(src)
    assert src.replace(macro, "").replace(suffix + "\n", "\n", 1) == plain   # nothing else differs
    rc, size, msg = _compile(src)
    assert rc == 0, msg
    assert size > 1000


def test_refused_map_sources():
    sc = _scenarios()["dcr_dipole"]
    # the kernel refuses several sources: the macro forced into a two-source source
    multi = "#define WOST_TALLY_MAPS 2\n" + sc.kernel_source(compat="fixed", sources=[sc.f, 2.0 * sc.f])
    rc, _, msg = _compile(multi)
    assert rc != 0 and "channel maps need a source mode, one source" in msg
    # ... and both tallies at once
    both = "#define WOST_TALLY 1\n" + sc.kernel_source(compat="fixed", n_wavenumbers=1, tally_maps=1)
    assert _compile(both)[0] != 0
    # the one-channel tally still takes no channels
    with pytest.raises(ValueError, match="tally"):
        sc.kernel_source(compat="fixed", tally=True, n_wavenumbers=2)
    for kw in ({"tally": True}, {"sources": [sc.f, 2.0 * sc.f]}, {"point_list": True}, {"options": {"refill_min": 2}},
               {"dirichlet_tree": 0}):
        with pytest.raises(ValueError, match="tally"):
            sc.kernel_source(compat="fixed", tally_maps=2, **kw)
    with pytest.raises(NotImplementedError, match="fixed"):
        sc.kernel_source(n_wavenumbers=2, tally_maps=2)                       # compat="reference"
    with pytest.raises(ValueError, match="n_maps"):
        sc.kernel_source(compat="fixed", n_wavenumbers=2, tally_maps=_lib.WOST_TALLY_MAX_MAPS + 1)
    with pytest.raises(ValueError, match="source"):
        S.ALL["laplace_square"]().kernel_source(compat="fixed", tally_maps=1)   # no source field


# ---- 4. the kernel cache's comparison -------------------------------------------------------

def test_variants_that_differ_in_tally_maps_compare_unequal(tmp_path):
    """tests/native/variant_tally_maps_check.cpp, built stand-alone with the address and
    undefined-behaviour sanitizers when the compiler has them (host code only)."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    src = os.path.join(HERE, "native", "variant_tally_maps_check.cpp")
    exe = str(tmp_path / "variant_tally_maps_check")
    san = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", src, "-o", exe])
    if san.returncode != 0:
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "variant_tally_maps_check: 0 failed checks" in r.stdout


# ---- 5. the row base ------------------------------------------------------------------------

def _row(n_points, R, T, bins, p, walk, t):
    e = ctypes.c_int64(-1)
    rc = _lib.lib.wost_tally_map_row(n_points, R, T, bins, p, walk, t, ctypes.byref(e))
    return rc, int(e.value)


def test_row_base_of_every_point_row_and_map():
    N, R, T, bins = 3, 4, 3, 17
    seen = set()
    for p in range(N):
        for blk in range(2 * R + 1):
            for t in range(T):
                for walk in (blk * 4096, blk * 4096 + 4095):
                    rc, e = _row(N, R, T, bins, p, walk, t)
                    assert rc == 0
                    assert e == ((p * R + blk % R) * T + t) * bins
                    seen.add(e)
    assert seen == {i * bins for i in range(N * R * T)}   # every sub-row, none twice
    # a walk index beyond 2^32 (walks_per_point < 2^43)
    walk = (1 << 42) + 5 * 4096 + 7
    assert _row(N, R, T, bins, 2, walk, 1) == (0, ((2 * R + ((walk // 4096) % R)) * T + 1) * bins)


def test_row_base_at_the_buffer_limit():
    """2^27 entries (WOST_TALLY_MAX_BYTES / 8): the 32-bit arithmetic reaches the last sub-row."""
    cap = _lib.WOST_TALLY_MAX_BYTES // 8
    N, R, T = 64, 8, 4
    bins = cap // (N * R * T)
    assert N * R * T * bins == cap == 1 << 27
    rc, e = _row(N, R, T, bins, N - 1, (R - 1) * 4096, T - 1)
    assert rc == 0 and e == cap - bins
    rc, e = _row(N, R, T, bins, N // 2, 3 * 4096 + 1, 2)
    assert rc == 0 and e == (((N // 2) * R + 3) * T + 2) * bins
    assert _row(N + 1, R, T, bins, 0, 0, 0)[0] != 0          # one point more: beyond the cap
    assert _row(N, R, T + 1, bins, 0, 0, 0)[0] != 0          # the factor T counts
    assert _row(N, R, T, bins, N, 0, 0)[0] != 0 and _row(N, R, T, bins, 0, 0, T)[0] != 0


# ---- 6. exports -----------------------------------------------------------------------------

def test_new_entry_points_are_declared_and_exported():
    names = _lib.declared_symbols()
    for n in ("wost_solve_range_tally_channels", "wost_kernel_source_tally_channels", "wost_tally_check_weights",
              "wost_tally_weighted", "wost_tally_map_row"):
        assert n in names
        assert hasattr(_lib.lib, n), f"libwost.so does not export {n}"
    assert _lib.lib.wost_version() == 6   # additive: the ABI version stays
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "wost.h")).read()
    assert f"#define WOST_TALLY_MAX_MAPS {_lib.WOST_TALLY_MAX_MAPS}\n" in hdr


# ---- 7. the facade on a stubbed launch ------------------------------------------------------

class _Stub(WostSolver_2D):
    """solve_greens_maps without a handle: the launch records its rows and returns integers
    that name (first weight of the row, point, replica, bin)."""

    def __init__(self, C):
        self.C, self.launches = C, []
        self.compat, self.point_sources, self.source = "fixed", None, object()
        self.wavenumbers = np.arange(C, dtype=np.float64) if C > 1 else None
        self.last_timing = {"total_steps": 11, "walk_kernel_ms": 1.0, "total_ms": 2.0}

    def __del__(self):
        pass

    num_models = property(lambda self: 0)

    def num_channels(self):
        return self.C

    def _default_tally_scale(self, nWalks, w0, w1, R, maxSteps):
        return 20

    def _launch_greens_maps(self, p, grid, w, nWalks, w0, w1, maxSteps, eps, seed, R, s, want_walks):
        self.launches.append((w.copy(), s, seed, want_walks))
        n, (T, C) = p.shape[0], w.shape
        bins = grid.nx * grid.ny + 1
        tally = (np.round(w[:, 0] * 1000).astype(np.int64)[None, None, :, None] * 10 ** 6 +
                 np.arange(n)[:, None, None, None] * 10 ** 4 + np.arange(R)[None, :, None, None] * 100 +
                 np.arange(bins)[None, None, None, :])
        sums = np.tile(np.arange(2 * C + 1, dtype=np.float64), (n, 1)) + 100.0 * len(self.launches)
        nw = w1 - w0
        return (tally.astype(np.int64), np.full((n, R), nw // R, np.int64), sums,
                np.zeros((n, nw, C), np.float32) if want_walks else None,
                np.zeros((n, nw), np.uint32) if want_walks else None)


def test_facade_chunks_rounds_and_shapes():
    s = _Stub(3)
    pts = np.array([[0.0, 0.0], [0.5, 0.25]], np.float32)
    grid = G.TallyGrid(-1.0, -1.0, 0.5, 1.0, 4, 2)
    third = 1.0 / 3.0
    w = np.array([[1.0 + k, third, 0.0] for k in range(6)], np.float64)
    maps, u, st = s.solve_greens_maps(pts, grid, w, nWalks=8192, maxSteps=50, replicas=2, seed=5, return_channels=True)
    # 6 rows: launches of 4 and 2, the same seed, scale and walks
    assert [l[0].shape for l in s.launches] == [(4, 3), (2, 3)]
    assert all(l[1:3] == s.launches[0][1:3] for l in s.launches)
    # rounded to float32 before the launch
    got = np.concatenate([l[0] for l in s.launches])
    assert got.dtype == np.float32 and got.tolist() == w.astype(np.float32).tolist()
    assert float(got[0, 1]) != third and float(got[0, 1]) == float(np.float32(third))
    # default scale: the bound's 20 minus ceil(log2(max row sum 6.33)) = 3
    assert s.launches[0][1] == 17
    assert isinstance(maps, list) and len(maps) == 6
    for k, m in enumerate(maps):
        assert isinstance(m, G.GreensMap)
        assert m.sums.shape == (2, 2, 2, 4) and m.outside.shape == (2, 2) and m.row_walks.shape == (2, 2)
        assert m.sums.dtype == np.int64 and m.quantum == 2.0 ** -17 and m.grid == grid
        assert m.u is None and m.stats is None
        # row k's integers, in (iy, ix) order, the outside bin apart
        assert m.sums[1, 1].ravel().tolist() == [(1 + k) * 10 ** 9 + 10 ** 4 + 100 + b for b in range(8)]
        assert m.outside[1, 1] == (1 + k) * 10 ** 9 + 10 ** 4 + 100 + 8
    # the channels' solve is the first launch's
    assert u.shape == (2, 3) and st.mean.shape == (2, 3) and st.stderr.shape == (2, 3)
    assert np.allclose(st.mean[:, 1], (2.0 + 100.0) / 8192)
    # one row, given flat: one map, one launch; an explicit quantum is rounded down to a power of two
    s = _Stub(3)
    maps = s.solve_greens_maps(pts, grid, [0.5, 0.0, 0.0], nWalks=4096, quantum=3e-4)
    assert len(maps) == 1 and s.launches[0][0].shape == (1, 3) and maps[0].quantum == 2.0 ** -12


def test_facade_refusals_need_no_launch():
    s = _Stub(3)
    pts = np.zeros((1, 2), np.float32)
    grid = G.TallyGrid(-1.0, -1.0, 0.5, 1.0, 4, 2)
    for w, what in (([[1.0, 0.0]], "shape"), ([[0.0, 0.0, 0.0]], "zero"), ([[1.0, np.nan, 0.0]], "finite"),
                    ([[1e39, 0.0, 0.0]], "finite")):
        with pytest.raises(ValueError, match=what):
            s.solve_greens_maps(pts, grid, w)
    with pytest.raises(ValueError, match="replicas"):
        s.solve_greens_maps(pts, grid, [[1.0, 0.0, 0.0]], replicas=0)
    with pytest.raises(ValueError, match="exceeds"):
        s.solve_greens_maps(pts, G.TallyGrid(0.0, 0.0, 1.0, 1.0, 4096, 4096), np.eye(3), replicas=8)
    s.compat = "reference"
    with pytest.raises(NotImplementedError, match="fixed"):
        s.solve_greens_maps(pts, grid, [[1.0, 0.0, 0.0]])
    s.compat, s.point_sources = "fixed", object()
    with pytest.raises(NotImplementedError, match="point sources"):
        s.solve_greens_maps(pts, grid, [[1.0, 0.0, 0.0]])
    s.point_sources, s.wavenumbers = None, None   # 3 channels without wavenumbers or models: extra sources
    with pytest.raises(NotImplementedError, match="one source"):
        s.solve_greens_maps(pts, grid, [[1.0, 0.0, 0.0]])
    assert s.launches == []
