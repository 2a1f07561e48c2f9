"""Green's function maps, the parts that need no device: the cell rule and
the fixed-point conversion as the library restates them for the host (wost_device.h
tally_cell / tally_quantize, the kernels' own text) against numpy; the deposit limit; the
generated sources with a tally; KernelVariant::tally in the kernel cache's comparison; and the
arithmetic of GreensMap. tests/test_gpu_tally.py runs the kernels."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from dcrmontecarlo_amd import _lib
from dcrmontecarlo_amd import greens_map as G
from dcrmontecarlo_amd import scenarios as S

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT_1D = _lib.WOST_TALLY_MAX_CELLS_1D


# ---- 1. the cell rule ---------------------------------------------------------------------

def _axis_points(edges: np.ndarray, rng) -> np.ndarray:
    """Every edge and its two float32 neighbours, points inside the cells, points far
    outside, +-inf and NaN."""
    e = edges.astype(np.float32)
    span = np.float32(e[-1] - e[0])
    inside = rng.uniform(float(e[0]) - 0.3 * float(span), float(e[-1]) + 0.3 * float(span), 4096).astype(np.float32)
    far = np.array([-3.0e38, -1.0e20, -1.0e9, 1.0e9, 1.0e20, 3.0e38, -np.inf, np.inf, np.nan, 0.0, -0.0], np.float32)
    return np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf)), inside, far])


def _expected_axis(edges: np.ndarray, v: np.ndarray) -> np.ndarray:
    """The cell by the definition: [e_i, e_{i+1}), -1 outside or NaN."""
    i = np.searchsorted(edges, v, side="right") - 1
    i = np.where(np.isnan(v) | (i < 0) | (i >= edges.shape[0] - 1), -1, i)
    return i.astype(np.int64)


def _guess_axis(v, o, d):
    """The kernel's float32 first guess, before its correction step."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor((v.astype(np.float32) - np.float32(o)) * (np.float32(1.0) / np.float32(d)))


X_GRIDS = [(-79.3, 7.7, 21), (-79.3, 7.7, 1), (0.1, 0.1, 1000), (-1.0, 2.0 / 3.0, 3), (1.0e-3, 1.0e-7, 4097),
           (-3.7e5, 0.7, LIMIT_1D), (-float(LIMIT_1D) / 2, 1.0, LIMIT_1D), (5.0e5, 1.0, 77), (-100.0, 3.0e-4, 65536)]


def test_cell_rule_matches_the_edges_on_each_axis():
    rng = np.random.default_rng(5)
    erred = 0
    for (o, d, n) in X_GRIDS:
        for axis in (0, 1):
            grid = G.TallyGrid(o, -0.5, d, 1.0, n, 1) if axis == 0 else G.TallyGrid(-0.5, o, 1.0, d, 1, n)
            edges = G.tally_edges(grid)[axis]
            assert edges.dtype == np.float32 and edges.shape == (n + 1,)
            assert np.all(np.diff(edges.astype(np.float64)) > 0), "edges must ascend strictly"
            v = _axis_points(edges, rng)
            pts = np.zeros((v.shape[0], 2), np.float32)
            pts[:, axis] = v
            got = G.tally_cell(grid, pts).astype(np.int64)
            want = _expected_axis(edges, v)
            want = np.where(want < 0, n, want)   # the outside bin of a 1 x n / n x 1 grid
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (f"grid {grid}: {bad.size} mismatches, first at v = {v[bad[0]]!r}: "
                                   f"cell {got[bad[0]]}, edges say {want[bad[0]]}")
            # the guess is within one cell of the answer wherever the answer is a cell, and it
            # does err: the correction step is exercised
            g = _guess_axis(v, grid[axis], grid[2 + axis])
            cell = want < n
            err = np.abs(g[cell] - want[cell])
            assert err.max() <= 1
            erred += int((err == 1).sum())
    assert erred > 0, "no grid's first guess erred: the correction step was never needed"


def test_cell_rule_in_two_dimensions():
    grid = G.TallyGrid(-79.3, -13.1, 7.7, 0.37, 21, 5)
    ex, ey = G.tally_edges(grid)
    rng = np.random.default_rng(6)
    vx, vy = _axis_points(ex, rng), _axis_points(ey, rng)
    xx, yy = np.meshgrid(vx[::7], vy[::5], indexing="ij")
    pts = np.stack([xx.ravel(), yy.ravel()], axis=1).astype(np.float32)
    ix, iy = _expected_axis(ex, pts[:, 0]), _expected_axis(ey, pts[:, 1])
    want = np.where((ix < 0) | (iy < 0), grid.nx * grid.ny, iy * grid.nx + ix)
    got = G.tally_cell(grid, pts)
    assert np.array_equal(got, want)
    assert (want == grid.nx * grid.ny).any() and (want < grid.nx * grid.ny).any()
    assert np.unique(want).size == grid.nx * grid.ny + 1   # every cell and the outside bin


@pytest.mark.parametrize("grid", [
    (0.0, 0.0, 1.0, 1.0, LIMIT_1D + 1, 1),      # more cells than the proof covers
    (0.0, 0.0, 1.0, 1.0, 1, 0),
    (0.0, 0.0, 0.0, 1.0, 4, 4),                 # no width
    (0.0, 0.0, -1.0, 1.0, 4, 4),
    (0.0, 0.0, 1.0, float("nan"), 4, 4),
    (float("inf"), 0.0, 1.0, 1.0, 4, 4),
    (1.0e9, 0.0, 1.0, 1.0, 4, 4),               # edges 1e9 cell widths from 0: float32 cannot tell the cells apart
    (0.0, -3.0e6, 1.0, 1.0, 4, 4),
    (0.0, 0.0, 1.0e-30, 1.0, 4, 4),
    (0.0, 0.0, 1.0, 1.0, 1 << 14, 1 << 14),     # 2^28 cells: beyond the buffer's cap
])
def test_cell_rule_refuses_grids_it_cannot_prove(grid):
    with pytest.raises(ValueError, match="tally grid"):
        G.tally_cell(grid, np.zeros((1, 2), np.float32))


# ---- 2. the fixed-point conversion --------------------------------------------------------

def test_fixed_point_conversion_matches_numpy():
    rng = np.random.default_rng(7)
    for s, L in ((0, 1 << 40), (20, 1 << 41), (37, 1 << 41), (-12, 1 << 10), (60, 1 << 62), (100, 1 << 62), (-100, 2),
                 (5, 1)):
        sc = np.float32(2.0 ** s)
        k = np.arange(-70, 70, dtype=np.float64)
        binades = (np.float32(2.0) ** k.astype(np.float32))[:, None] * (1.0 + np.arange(8, dtype=np.float32) / 8.0)[None]
        n = np.concatenate([np.arange(0, 64, dtype=np.float64), 2.0 ** np.arange(6, 23)])
        ties = ((n + 0.5) * 2.0 ** -s).astype(np.float32)               # exactly between two quanta
        near = np.float32(float(L) * 2.0 ** -s)
        lim = np.array([near, np.nextafter(near, np.float32(0)), np.nextafter(near, np.float32(np.inf)), near / 2, near * 2],
                       np.float32)
        rnd = (rng.standard_normal(4096) * float(near) / 4).astype(np.float32)
        with np.errstate(over="ignore", under="ignore"):
            scaled = binades.ravel() / sc
        d = np.concatenate([scaled, ties, lim, rnd, np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e38, 1.0e-45],
                                                             np.float32)]).astype(np.float32)
        d = np.concatenate([d, -d])
        with np.errstate(over="ignore", invalid="ignore"):
            ref = np.rint(np.float32(d) * sc)
            assert ref.dtype == np.float32
            ok_ref = np.abs(ref) < np.float32(L)
        q, ok = G.tally_quantize(d, s, L)
        assert np.array_equal(ok, ok_ref), f"s = {s}: the limit test differs"
        assert np.array_equal(q[ok], ref[ok_ref].astype(np.int64)), f"s = {s}: quantised values differ"
        assert np.all(q[~ok] == 0)
        assert ok.any() and (~ok).any()
    for bad in ((101, 1 << 10), (-101, 1 << 10), (0, 3), (0, 0), (0, -4)):
        with pytest.raises(ValueError):
            G.tally_quantize(np.ones(1, np.float32), *bad)


def test_deposit_limit_keeps_a_row_below_2_63():
    B = _lib.WOST_BLOCK_WALKS
    for (W, w0, w1, R, steps) in ((16384, 0, 16384, 4, 200), (16384, 0, 16384, 1, 200), (16384, 4096, 12288, 4, 200),
                                  (10000, 0, 10000, 8, 1000), (1 << 30, 0, 1 << 30, 3, 100000), (5, 0, 5, 8, 0)):
        rows = np.bincount((np.arange(w0, w1, dtype=np.int64) // B) % R, minlength=R) if w1 - w0 <= 1 << 20 else None
        most = int(rows.max()) if rows is not None else -(-((w1 - w0) // B) // R) * B
        L = G.tally_limit(W, w0, w1, R, steps)
        assert L & (L - 1) == 0 and 1 <= L <= 1 << 62
        n = max(most, 1) * max(steps, 1)
        assert n * L < 1 << 63
        assert L == 1 << 62 or n * (2 * L) >= 1 << 63, "not the largest power of two"
    with pytest.raises(ValueError):
        G.tally_limit(16384, 0, 16384, 0, 200)


# ---- 3. generated sources -----------------------------------------------------------------

def _head(src: str) -> str:
    return [l for l in src.splitlines() if l.startswith("// generated")][0]


def _tally_scenarios():
    return {"poisson_square": S.ALL["poisson_square"](),
            "dcr_dipole": S.ALL["dcr_dipole"](6),
            "wenner_topography": S.wenner_topography(n_electrodes=4, n_walks=1, n_segments=200)}


@pytest.mark.parametrize("name", ["poisson_square", "dcr_dipole", "wenner_topography"])
def test_sources_with_a_tally_name_it_and_compile(name):
    sc = _tally_scenarios()[name]
    plain = sc.kernel_source(compat="fixed")
    assert "WOST_TALLY" not in plain and "tally" not in _head(plain)
    assert sc.kernel_source(compat="fixed", tally=False) == plain
    src = sc.kernel_source(compat="fixed", tally=True)
    assert src.count("#define WOST_TALLY 1\n") == 1
    assert _head(src) == _head(plain) + ", tally"
    assert "+fixed" in _head(src) and "+source" in _head(src)
    if name == "wenner_topography":
        assert "+tree" in _head(src)
    # nothing else differs
    assert src.replace("#define WOST_TALLY 1\n", "").replace(", tally\n", "\n", 1) == plain
    n, used = ctypes.c_int64(), ctypes.c_int32(-1)
    rc = _lib.lib.wost_jit_compile(src.encode(), b"gfx950", 0, None, 0, ctypes.byref(n), ctypes.byref(used))
    assert rc == 0, _lib.lib.wost_last_error().decode()
    assert n.value > 1000


def test_refused_combinations_get_no_source():
    sc = _tally_scenarios()["dcr_dipole"]
    with pytest.raises(NotImplementedError, match="fixed"):
        sc.kernel_source(tally=True)                              # compat="reference"
    with pytest.raises(ValueError, match="source"):
        S.ALL["laplace_square"]().kernel_source(compat="fixed", tally=True)   # no source field
    for kw in ({"sources": [sc.f, 2.0 * sc.f]}, {"n_wavenumbers": 2}, {"models": [(sc.sigma, sc.alpha)]},
               {"point_list": True}, {"options": {"refill_min": 2}}, {"dirichlet_tree": 0}):
        with pytest.raises(ValueError, match="tally"):
            sc.kernel_source(compat="fixed", tally=True, **kw)
    # ... and the kernel itself refuses channels: a multi-source source with the macro forced
    multi = "#define WOST_TALLY 1\n" + sc.kernel_source(compat="fixed", sources=[sc.f, 2.0 * sc.f])
    n, used = ctypes.c_int64(), ctypes.c_int32(-1)
    rc = _lib.lib.wost_jit_compile(multi.encode(), b"gfx950", 0, None, 0, ctypes.byref(n), ctypes.byref(used))
    assert rc != 0 and "a tally needs" in _lib.lib.wost_last_error().decode()


def test_new_entry_points_are_declared_and_exported():
    names = _lib.declared_symbols()
    for n in ("wost_solve_range_tally", "wost_kernel_source_tally", "wost_tally_cell", "wost_tally_quantize",
              "wost_tally_limit", "wost_tally_default_scale"):
        assert n in names
        assert hasattr(_lib.lib, n), f"libwost.so does not export {n}"
    assert _lib.lib.wost_version() == 6   # additive: the ABI version stays


# ---- 4. the kernel cache's comparison -----------------------------------------------------

def test_variants_that_differ_in_tally_compare_unequal(tmp_path):
    """tests/native/variant_tally_check.cpp, built stand-alone with the address and
    undefined-behaviour sanitizers when the compiler has them (host code only)."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    src = os.path.join(HERE, "native", "variant_tally_check.cpp")
    exe = str(tmp_path / "variant_tally_check")
    san = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", src, "-o", exe])
    if san.returncode != 0:
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "variant_tally_check: 0 failed checks" in r.stdout


# ---- 5. GreensMap ---------------------------------------------------------------------------

def _synthetic(R=4, seed=9):
    rng = np.random.default_rng(seed)
    N, ny, nx = 3, 5, 7
    grid = G.TallyGrid(-1.0, 2.0, 0.5, 0.25, nx, ny)
    sums = rng.integers(-(1 << 40), 1 << 44, size=(N, R, ny, nx), dtype=np.int64)
    outside = rng.integers(0, 1 << 30, size=(N, R), dtype=np.int64)
    walks = np.tile(np.array([4096, 4096, 4096, 1712][:R] if R > 1 else [14000], np.int64), (N, 1))
    return G.GreensMap(sums, outside, walks, 2.0 ** -30, grid), rng


def test_greens_map_arithmetic():
    gm, rng = _synthetic()
    N, R, ny, nx = gm.sums.shape
    area = 0.5 * 0.25
    q = 2.0 ** -30
    W = gm.row_walks.astype(np.float64)
    # mean: the integer rows added exactly, then scaled
    tot = np.zeros((N, ny, nx), dtype=object)
    for r in range(R):
        tot = tot + gm.sums[:, r].astype(object)
    want = np.array(tot, dtype=np.float64) * q / W.sum(axis=1)[:, None, None] / area
    assert np.array_equal(gm.mean, want)
    # stderr: batch means over the rows, weighted by their walks
    rows = gm.sums.astype(np.float64) * q / W[:, :, None, None] / area
    m = (W[:, :, None, None] * rows).sum(axis=1) / W.sum(axis=1)[:, None, None]
    var = (W[:, :, None, None] * (rows - m[:, None]) ** 2).sum(axis=1) / ((R - 1) * W.sum(axis=1)[:, None, None])
    np.testing.assert_allclose(gm.stderr, np.sqrt(var), rtol=1e-12)
    np.testing.assert_allclose(m, gm.mean, rtol=1e-12)   # the weighted row mean is the mean
    # equal rows: the textbook standard error of R batch means
    eq = G.GreensMap(gm.sums, gm.outside, np.full_like(gm.row_walks, 4096), q, gm.grid)
    r_eq = eq.sums.astype(np.float64) * q / 4096 / area
    np.testing.assert_allclose(eq.stderr, r_eq.std(axis=1, ddof=1) / np.sqrt(R), rtol=1e-12)
    # potential: per replica first
    f = rng.standard_normal((ny, nx))
    u, se = gm.potential(f)
    per_row = (gm.sums.astype(np.float64) * q / W[:, :, None, None] * f).sum(axis=(2, 3))
    u_want = (W * per_row).sum(axis=1) / W.sum(axis=1)
    np.testing.assert_allclose(u, u_want, rtol=1e-10, atol=1e-12 * np.abs(per_row).max())
    se_want = np.sqrt((W * (per_row - u_want[:, None]) ** 2).sum(axis=1) / ((R - 1) * W.sum(axis=1)))
    np.testing.assert_allclose(se, se_want, rtol=1e-9)
    # a constant source: the potential is the mean's integral
    u1, _ = gm.potential(np.ones((ny, nx)))
    np.testing.assert_allclose(u1, gm.mean.sum(axis=(1, 2)) * area, rtol=1e-12)
    with pytest.raises(ValueError):
        gm.potential(np.ones((nx, ny)))


def test_greens_map_single_replica_and_merge():
    one, _ = _synthetic(R=1)
    assert np.isnan(one.stderr).all() and np.isnan(one.potential(np.ones(one.sums.shape[2:]))[1]).all()
    assert np.isfinite(one.mean).all()
    a, _ = _synthetic(seed=1)
    b, _ = _synthetic(seed=2)
    c = a + b
    assert np.array_equal(c.sums, a.sums + b.sums) and np.array_equal(c.row_walks, a.row_walks + b.row_walks)
    assert np.array_equal(c.outside, a.outside + b.outside)
    with pytest.raises(ValueError):
        a + G.GreensMap(b.sums, b.outside, b.row_walks, b.quantum * 2, b.grid)
    # a row without walks takes no part
    z = G.GreensMap(a.sums.copy(), a.outside, a.row_walks.copy(), a.quantum, a.grid)
    z.sums[:, 3] = 0
    z.row_walks[:, 3] = 0
    three = G.GreensMap(a.sums[:, :3], a.outside[:, :3], a.row_walks[:, :3], a.quantum, a.grid)
    np.testing.assert_allclose(z.stderr, three.stderr, rtol=1e-12)
    assert np.array_equal(z.mean, three.mean)
