"""Green's function maps on the device (wost_solve_range_tally, WostSolver_2D.solve_greens_map;
DESIGN.md 7f). A tally solve is an ordinary walk-range solve whose walks also add every
unclipped source sample's weight to a grid, in fixed point:

 6. the walks are untouched: values, steps, block and point rows are solve_range's bits;
 7. every cell is its box source: the cell's sum against one multi-source launch of the 16
    half-open box indicators, within a bound derived from float32 accumulation and the
    quantum -- nothing in it is measured;
 8. the integers do not depend on the launch shape, shards add up, R = 1 is the sum of R = 4's
    rows, and row_walks is as stated; the tree kernel's tally is the scan kernel's;
 9. the expectation: the unit disk's Green's function at the centre, by quadrature;
10. the flag and the refusals.

Three problems, 3 points x 16384 walks (4 blocks: R = 4 has one block per row), 200 steps.
tests/test_tally_host.py checks the cell rule and the conversion on the host."""
import ctypes
import dataclasses
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 16384
STEPS = 200
SEED = 20260117
B = 4096


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the three problems ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """(scenario, points, solver keywords, a 4 x 4 grid around the points)."""
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey
    from dcrmontecarlo_amd.greens_map import TallyGrid

    if name == "sq":   # Dirichlet only, no delta tracking: a deposit is r^2 / 4
        sc = dataclasses.replace(S.poisson_square(), max_steps=STEPS)
        pts = np.array([[0.7, 0.1], [-0.4, 0.9], [1.2, -1.1]], np.float32)
        return sc, pts, {}, TallyGrid(-1.3, -1.45, 0.65, 0.7, 4, 4)
    if name == "dd":   # tests/test_gpu_models.py's dcr_dipole: a transmitter dipole, sigma_bar 0.02
        sc = S.dcr_dipole(6, n_walks=W)
        sc = dataclasses.replace(sc, f=survey.dipole_source(sc.points[2], sc.points[3], 0.5), max_steps=STEPS)
        pts = np.ascontiguousarray(sc.points[[1, 3, 4]])
        return sc, pts, {"sigma_bar": 0.02}, TallyGrid(-79.3, -30.1, 7.7, 7.7, 4, 4)
    if name == "tree":   # a 200-segment topographic surface: the segment-tree kernel
        sc = S.wenner_topography(n_electrodes=4, n_walks=W, n_segments=200, physical=True)
        sc = dataclasses.replace(sc, max_steps=STEPS)
        pts = np.ascontiguousarray(sc.points[[0, 1, 3]])
        return sc, pts, {}, TallyGrid(-450.3, -95.7, 225.0, 24.5, 4, 4)
    raise KeyError(name)


# dd runs at sigma_bar = 0.02 and tree at its estimate 5e-6, far below sigma' in the thin
# sigmoid shells of their alpha (in the thousands): there the collision weight 1 - sigma' /
# sigma_bar is signed and huge, and a walk that collides in a shell carries it on. Measured on
# the device, the f = 1 walk values of these shapes span -2.7e15 .. 7e13 (dd; median 12) and
# -9e14 .. 5e10 (tree; median 4e6): far beyond the default quantum's bound 1 / (sigma_bar min
# alpha) and its 2^16 head room, and the solve says so (test 10's flag). These tests are
# about bits and order, not resolution, and pass a quantum of 2^8: deposits up to 2^51.
SCALE = {"sq": None, "dd": -8, "tree": -8}


def _solver(name, scenario=None, tree=None, **kw):
    sc, _, skw, _ = _case(name)
    s = (scenario or sc).solver(compat="fixed", device=0, **{**skw, **kw})
    s.set_fixed_step_check(False)   # (dd, tree: the walks are truncated at 200 steps; fine here)
    if tree is not None:
        s.set_segment_tree(0 if tree else -1)
    return s


def _range(s, pts, w0=0, w1=W, eps=None, steps=STEPS):
    """wost_solve_range's block rows, point rows, values and steps."""
    from dcrmontecarlo_amd import _lib

    p = np.ascontiguousarray(pts, np.float32)
    n, nw = len(p), w1 - w0
    nbr = -(-nw // B)
    blocks, rows = np.zeros((n, nbr, 3)), np.zeros((n, 3))
    wv, ws = np.empty((n, nw), np.float32), np.empty((n, nw), np.uint32)
    _lib.check(_lib.lib.wost_solve_range(s._h, _lib.fptr(p), n, W, w0, w1, steps, float(eps), SEED, _lib.dptr(blocks),
                                         _lib.dptr(rows), _lib.fptr(wv), _lib.u32ptr(ws)), "wost_solve_range")
    return blocks, rows, wv, ws


def _tally(s, pts, grid, R, w0=0, w1=W, eps=None, steps=STEPS, scale=None):
    """wost_solve_range_tally through the C ABI: (block rows, point rows, values, steps, tally
    [n, R, bins], row_walks [n, R], scale_log2)."""
    from dcrmontecarlo_amd import _lib
    from dcrmontecarlo_amd.greens_map import _c_grid

    p = np.ascontiguousarray(pts, np.float32)
    n, nw = len(p), w1 - w0
    nbr = -(-nw // B)
    if scale is None:
        sl = ctypes.c_int32(0)
        _lib.check(_lib.lib.wost_tally_default_scale(s._h, W, w0, w1, R, steps, ctypes.byref(sl)), "default scale")
        scale = int(sl.value)
    cg = _c_grid(grid)
    blocks, rows = np.zeros((n, nbr, 3)), np.zeros((n, 3))
    wv, ws = np.empty((n, nw), np.float32), np.empty((n, nw), np.uint32)
    tally = np.full((n, R, grid.nx * grid.ny + 1), -1, np.int64)
    rw = np.full((n, R), -1, np.int64)
    i64 = ctypes.POINTER(ctypes.c_int64)
    _lib.check(_lib.lib.wost_solve_range_tally(s._h, _lib.fptr(p), n, W, w0, w1, steps, float(eps), SEED, ctypes.byref(cg),
                                               R, scale, _lib.dptr(blocks), _lib.dptr(rows), _lib.fptr(wv),
                                               _lib.u32ptr(ws), tally.ctypes.data_as(i64), rw.ctypes.data_as(i64)),
               "wost_solve_range_tally")
    return blocks, rows, wv, ws, tally, rw, scale


# ---- 6. the walks are untouched -------------------------------------------------------------
@pytest.mark.parametrize("name", ["sq", "dd", "tree"])
def test_a_tally_solve_walks_the_handles_walks(gpu_available, name):
    sc, pts, _, grid = _case(name)
    s = _solver(name)
    plain = _range(s, pts, eps=sc.eps)
    got = _tally(s, pts, grid, 4, eps=sc.eps, scale=SCALE[name])
    t = s.timing()
    assert t["jit"] == 1 and t["tree"] == (1 if name == "tree" else 0)
    np.testing.assert_array_equal(got[3], plain[3], err_msg="step counts")
    np.testing.assert_array_equal(_bits(got[2]), _bits(plain[2]), err_msg="per-walk values")
    np.testing.assert_array_equal(got[0], plain[0], err_msg="block rows")
    np.testing.assert_array_equal(got[1], plain[1], err_msg="point rows")
    assert (got[4] != 0).any() and (got[5] == B).all()
    # ... and the handle's next plain solve is what it was
    again = _range(s, pts, eps=sc.eps)
    np.testing.assert_array_equal(_bits(again[2]), _bits(plain[2]))
    # a shard of the walks: the same walks as solve_range's shard
    shard = _tally(s, pts, grid, 4, B, 3 * B, eps=sc.eps, scale=SCALE[name])
    np.testing.assert_array_equal(_bits(shard[2]), _bits(plain[2][:, B:3 * B]))
    np.testing.assert_array_equal(shard[0], plain[0][:, 1:3])


# ---- 7. every cell is its box source --------------------------------------------------------
def _box_sources(grid):
    """The 16 half-open cells as closed box indicators, cell order (iy * nx + ix)."""
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd.greens_map import tally_edges

    ex, ey = tally_edges(grid)
    lo = np.float32(-np.inf)
    return [F.indicator_box(float(ex[i]), float(np.nextafter(ex[i + 1], lo)), float(ey[j]), float(np.nextafter(ey[j + 1], lo)))
            for j in range(grid.ny) for i in range(grid.nx)]


@pytest.mark.parametrize("name", ["sq", "dd", "tree"])
def test_every_cell_is_its_box_source(gpu_available, name):
    """Per point and cell |tally * quantum - sum_w v_w| <= sum_w (k_w - 1) 2^-24 |v_w| + D *
    quantum / 2: v_w is walk w's value for the cell's box source (a float32 sum of the walk's
    at most k_w non-negative deposits in the cell, each partial sum below v_w: error at most
    (k_w - 1) 2^-24 v_w), D the steps of the walks that scored in the cell (each deposit is
    rounded to the quantum once). The boundary function is 0 (a walk's value is its source
    score alone), and sigma_bar lies above every sigma' the walks meet, so that the collision
    weights, and so the deposits, are non-negative (asserted on the box sources' values):
    alpha's sigmoid shells have sigma' in the thousands (1079 on dcr_dipole's 50 x 50 grid),
    and a sigma_bar above that moves a walk ~2 / sqrt(sigma_bar) per step. So the points and
    the grid are chosen close together here -- dd: three points within 0.7 units of (-60, 0)
    and cells of 0.4 units under sigma_bar = 1.05 x the sampled maximum; tree: three points
    under the surface near x = -400, 200 units from the nearest shell, sigma_bar = 1 (a walk
    covers ~30 units in 200 steps, sigma' is 0 there) and cells of 25 x 16 units."""
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd import survey
    from dcrmontecarlo_amd.greens_map import TallyGrid

    sc, pts, _, grid = _case(name)
    sc0 = dataclasses.replace(sc, g=None)
    kw = {}
    if name == "dd":
        kw["sigma_bar"] = 1.05 * survey.sigma_bar_for_models(sc0.solver(), [(sc.sigma, sc.alpha)])
        pts = np.array([[-60.0, -0.2], [-59.7, 0.1], [-60.3, 0.3]], np.float32)
        grid = TallyGrid(-60.83, -0.79, 0.4, 0.4, 4, 4)
    if name == "tree":
        kw["sigma_bar"] = 1.0
        x = np.array([-400.0, -395.0, -405.0])
        pts = np.stack([x, 1.0 + 2.0 * np.sin(x / 37.0) - np.array([0.1, 2.0, 5.0])], axis=1).astype(np.float32)
        grid = TallyGrid(-450.3, -60.1, 25.0, 16.0, 4, 4)
    s = _solver(name, scenario=sc0, **kw)
    got = _tally(s, pts, grid, 4, eps=sc.eps)
    if name == "tree":
        assert s.timing()["tree"] == 1
    tally, quantum = got[4].sum(axis=1), 2.0 ** -got[6]    # [n, 17]
    vals, steps = s.solve_sources_walks(pts, _box_sources(grid), nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED)
    np.testing.assert_array_equal(steps, got[3], err_msg="the box sources' walks are the tally's walks")
    assert vals.shape == (16, len(pts), W) and (vals >= 0).all(), "the bound assumes non-negative deposits"
    v = vals.astype(np.float64)
    k = steps.astype(np.float64)
    want = v.sum(axis=2).T                                                        # [n, 16]
    bound = ((np.maximum(k - 1, 0) * 2.0 ** -24)[None] * v).sum(axis=2).T + \
        ((v > 0) * k[None]).sum(axis=2).T * quantum / 2
    err = np.abs(tally[:, :16] * quantum - want)
    # an empty comparison passes nothing: every cell and the outside bin receive deposits, and
    # most (point, cell) pairs do
    assert (tally[:, :16].sum(axis=0) > 0).all() and (tally[:, 16] > 0).all() and (tally[:, :16] > 0).mean() >= 0.5
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, 0.0)
    print(f"{name}: cells: largest error / bound {ratio.max():.3g} (quantum 2^{-got[6]}, sigma_bar {s.sigma_bar}, "
          f"{int((tally[:, :16] > 0).sum())} of {tally[:, :16].size} (point, cell) pairs scored, cell sums "
          f"{want[want > 0].min():.3g}..{want.max():.3g})")
    assert (err <= bound).all()
    # all cells and the outside bin: the source f = 1
    one, steps1 = s.solve_sources_walks(pts, [F.const(1.0), F.const(0.0)], nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED)
    np.testing.assert_array_equal(steps1, got[3])
    v1 = one[0].astype(np.float64)
    err1 = np.abs(tally.sum(axis=1) * quantum - v1.sum(axis=1))
    bound1 = (np.maximum(k - 1, 0) * 2.0 ** -24 * v1).sum(axis=1) + k.sum(axis=1) * quantum / 2
    print(f"{name}: all bins: largest error / bound {np.max(err1 / bound1):.3g}")
    assert (v1 >= 0).all() and (err1 <= bound1).all()


# ---- 8. order independence ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sq", "dd"])
def test_the_integers_do_not_depend_on_order(gpu_available, name):
    sc, pts, _, grid = _case(name)
    s = _solver(name)
    full = _tally(s, pts, grid, 4, eps=sc.eps, scale=SCALE[name])
    scale = full[6]
    assert (full[5] == B).all()                                   # 4 blocks, one per row
    for opts in ({"chunk0": 1, "chunk_min": 1, "chunk_max": 1}, {"chunk0": 1024, "chunk_max": 1024, "grid_blocks_per_cu": 1}):
        o = _solver(name)
        for key, val in opts.items():
            o.set_option(key, val)
        other = _tally(o, pts, grid, 4, eps=sc.eps, scale=scale)
        assert o.timing()["chunk0"] == opts["chunk0"]
        np.testing.assert_array_equal(other[4], full[4], err_msg=f"launch shape {opts}")
        np.testing.assert_array_equal(other[5], full[5])
    # two walk-range shards add up
    a = _tally(s, pts, grid, 4, 0, B, eps=sc.eps, scale=scale)
    b = _tally(s, pts, grid, 4, B, W, eps=sc.eps, scale=scale)
    np.testing.assert_array_equal(a[4] + b[4], full[4])
    np.testing.assert_array_equal(a[5], np.tile([B, 0, 0, 0], (len(pts), 1)))
    np.testing.assert_array_equal(b[5], np.tile([0, B, B, B], (len(pts), 1)))
    assert (a[4][:, 1:] == 0).all() and (b[4][:, 0] == 0).all()
    # R = 1 is the sum of R = 4's rows; R = 3 wraps block 3 into row 0
    one = _tally(s, pts, grid, 1, eps=sc.eps, scale=scale)
    np.testing.assert_array_equal(one[4][:, 0], full[4].sum(axis=1))
    assert (one[5] == W).all()
    three = _tally(s, pts, grid, 3, eps=sc.eps, scale=scale)
    np.testing.assert_array_equal(three[4][:, 0], full[4][:, 0] + full[4][:, 3])
    np.testing.assert_array_equal(three[4][:, 1:], full[4][:, 1:3])
    np.testing.assert_array_equal(three[5], np.tile([2 * B, B, B], (len(pts), 1)))
    # a walk count that is no multiple of the block: the last row's count is the remainder
    s2 = _solver(name)
    from dcrmontecarlo_amd.greens_map import GreensMap  # noqa: F401
    gm = s2.solve_greens_map(pts, grid, nWalks=2 * B + 100, maxSteps=STEPS, eps=sc.eps, seed=SEED, replicas=4,
                             quantum=2.0 ** -scale)
    np.testing.assert_array_equal(gm.row_walks, np.tile([B, B, 100, 0], (len(pts), 1)))
    assert (gm.sums[:, 3] == 0).all() and (gm.sums[:, 2] != 0).any()


def test_the_tree_kernels_tally_is_the_scan_kernels(gpu_available):
    sc, pts, _, grid = _case("tree")
    tr, scan = _solver("tree", tree=True), _solver("tree", tree=False)
    a = _tally(tr, pts, grid, 4, eps=sc.eps, scale=SCALE["tree"])
    assert tr.timing()["tree"] == 1
    b = _tally(scan, pts, grid, 4, eps=sc.eps, scale=a[6])
    assert scan.timing()["tree"] == 0
    np.testing.assert_array_equal(_bits(a[2]), _bits(b[2]), err_msg="the two kernels' walks")
    np.testing.assert_array_equal(a[4], b[4])
    assert (a[4].sum(axis=1)[:, :16] != 0).any()


# ---- 9. the expectation -----------------------------------------------------------------------
def test_the_map_of_the_disk_is_its_greens_function(gpu_available):
    """Unit disk through a 64-gon, Laplace, query point at the centre: the polygon lies
    between the disks of the inscribed radius cos(pi / 64) and of radius 1, and the Green's
    function grows with the domain, so every cell average of G(0, .) lies between those of
    ln(rho_b / |y|) / (2 pi) for the two radii (Gauss-Legendre quadrature in double). 4 x 3
    cells inside the inscribed disk; the pole lies on the edge between cells (1, 1) and (2, 1),
    which are left out."""
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd.greens_map import TallyGrid, tally_edges

    sc = S.Scenario("disk64", S._circle(64, 1.0), None, g=None, f=None, points=np.zeros((1, 2), np.float32),
                    n_walks=8 * B, max_steps=STEPS, eps=1e-4)
    s = sc.solver(compat="fixed", device=0)
    grid = TallyGrid(-0.6, -0.6, 0.3, 0.4, 4, 3)
    gm = s.solve_greens_map(sc.points, grid, nWalks=8 * B, maxSteps=STEPS, eps=1e-4, seed=SEED, replicas=8)
    assert s.source is None and gm.sums.shape == (1, 8, 3, 4) and (gm.row_walks == B).all()
    assert float(gm.u[0, 0]) == 0.0   # no source, no boundary function
    ex, ey = (e.astype(np.float64) for e in tally_edges(grid))
    t, wq = np.polynomial.legendre.leggauss(48)

    def cell_average(i, j, rho_b):
        x = 0.5 * (ex[i] + ex[i + 1]) + 0.5 * (ex[i + 1] - ex[i]) * t
        y = 0.5 * (ey[j] + ey[j + 1]) + 0.5 * (ey[j + 1] - ey[j]) * t
        r = np.hypot(x[:, None], y[None, :])
        return float((wq[:, None] * wq[None, :] * np.log(rho_b / r)).sum() / 4.0 / (2.0 * math.pi))

    mean, se = gm.mean[0], gm.stderr[0]
    worst = 0.0
    for j in range(3):
        for i in range(4):
            if j == 1 and i in (1, 2):
                continue
            lo, hi = cell_average(i, j, math.cos(math.pi / 64)), cell_average(i, j, 1.0)
            z = max(lo - mean[j, i], mean[j, i] - hi, 0.0) / se[j, i]
            worst = max(worst, z)
            print(f"cell ({i}, {j}): mean {mean[j, i]:.6f} +- {se[j, i]:.2g}, expected [{lo:.6f}, {hi:.6f}]: {z:.2f} stderr")
            assert se[j, i] > 0 and z <= 4.0
    # the source that is 1 on the grid's cells: the potential is the map's integral
    u, use = gm.potential(np.ones((3, 4)))
    assert abs(u[0] - gm.mean[0].sum() * gm.cell_area) <= 1e-12 and use[0] > 0


# ---- 10. the flag and the refusals --------------------------------------------------------
def test_a_quantum_too_fine_raises_and_returns_nothing(gpu_available):
    sc, pts, _, grid = _case("sq")
    s = _solver("sq")
    with pytest.raises(ValueError, match="quantum"):
        s.solve_greens_map(pts, grid, nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED, replicas=4, quantum=2.0 ** -90)
    # through the C ABI: the caller's arrays are not written, and the quantum the message names fits
    import re
    from dcrmontecarlo_amd import _lib
    from dcrmontecarlo_amd.greens_map import _c_grid
    p = np.ascontiguousarray(pts, np.float32)
    cg = _c_grid(grid)
    tally = np.full((len(p), 4, 17), -1, np.int64)
    rw = np.full((len(p), 4), -1, np.int64)
    i64 = ctypes.POINTER(ctypes.c_int64)
    rc = _lib.lib.wost_solve_range_tally(s._h, _lib.fptr(p), len(p), W, 0, W, STEPS, float(sc.eps), SEED, ctypes.byref(cg),
                                         4, 90, None, None, None, None, tally.ctypes.data_as(i64), rw.ctypes.data_as(i64))
    msg = _lib.lib.wost_last_error().decode()
    assert rc == _lib.WOST_ERR_INVALID_ARG and "quantum" in msg
    assert (tally == -1).all() and (rw == -1).all(), "a refused solve returns no sums"
    named = int(re.search(r"scale_log2 (-?\d+)", msg).group(1))
    # sq's deposits are r^2 / 4 <= 2 (the square +-2): the named quantum is within a few bits of 2^-43 * 2
    assert 35 <= named <= 43, msg
    fits = _tally(s, pts, grid, 4, eps=sc.eps, scale=named)
    assert (fits[4] > 0).any()
    with pytest.raises(ValueError, match="quantum"):   # ... and it is not a wasteful one: 4 bits finer does not fit
        _tally(s, pts, grid, 4, eps=sc.eps, scale=named + 4)
    # the same call with a quantum that fits works, and names itself
    gm = s.solve_greens_map(pts, grid, nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED, replicas=4, quantum=2.0 ** -30)
    assert gm.quantum == 2.0 ** -30 and (gm.sums > 0).any()
    assert _lib.lib.wost_version() == 6


def test_refusals(gpu_available):
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd import survey

    sc, pts, skw, grid = _case("dd")
    kw = dict(nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED, replicas=4, quantum=2.0 ** -SCALE["dd"])
    ref = sc.solver(device=0, **skw)                                   # compat="reference"
    with pytest.raises(NotImplementedError, match="fixed"):
        ref.solve_greens_map(pts, grid, **kw)
    s = _solver("dd")
    s.set_wavenumbers([0.01])
    with pytest.raises(NotImplementedError, match="wavenumbers"):
        s.solve_greens_map(pts, grid, **kw)
    s.set_wavenumbers(None)
    s.set_models([(None, sc.alpha), (None, F.const(100.0))])
    with pytest.raises(NotImplementedError, match="models"):
        s.solve_greens_map(pts, grid, **kw)
    s.set_models(None)
    with pytest.raises(NotImplementedError, match="history"):
        s.solve_greens_map(pts, grid, return_history=True, **kw)
    # extra sources on the handle (wost_set_sources): the library refuses
    with s.sources_installed(s.source_fields([sc.f, 2.0 * sc.f])):
        with pytest.raises(NotImplementedError, match="one channel"):
            s.solve_greens_map(pts, grid, **kw)
    ps = _solver("dd", scenario=dataclasses.replace(sc, f=None))
    # ... also for a solver without a source of its own, whose installed sources stay installed
    with ps.sources_installed(ps.source_fields([sc.f, 2.0 * sc.f])):
        with pytest.raises(NotImplementedError, match="one channel"):
            ps.solve_greens_map(pts, grid, **kw)
        assert ps.num_channels() == 2
    e = np.asarray(sc.points, np.float64)
    ps.set_point_sources([survey.point_dipole(e[2], e[3])])
    with pytest.raises(NotImplementedError, match="point sources"):
        ps.solve_greens_map(pts, grid, **kw)
    # bad grids, too many replicas, an oversized buffer
    for bad in ((0.0, 0.0, 0.0, 1.0, 4, 4), (0.0, 0.0, 1.0, 1.0, 0, 4), (1.0e9, 0.0, 1.0, 1.0, 4, 4),
                (0.0, 0.0, 1.0, 1.0, (1 << 20) + 1, 1)):
        with pytest.raises(ValueError):
            s.solve_greens_map(pts, bad, **kw)
    with pytest.raises(ValueError, match="replicas"):
        s.solve_greens_map(pts, grid, **{**kw, "replicas": 0})
    with pytest.raises(ValueError, match="exceeds"):
        s.solve_greens_map(pts, (-100.0, -100.0, 0.05, 0.05, 4096, 4096), **kw)
    # ... and the library's own check (it refuses before it writes: one entry is enough)
    from dcrmontecarlo_amd import _lib
    from dcrmontecarlo_amd.greens_map import _c_grid
    p = np.ascontiguousarray(pts, np.float32)
    cg = _c_grid((-100.0, -100.0, 0.05, 0.05, 4096, 4096))
    one = np.zeros(1, np.int64)
    rc = _lib.lib.wost_solve_range_tally(s._h, _lib.fptr(p), len(p), W, 0, W, STEPS, float(sc.eps), SEED, ctypes.byref(cg),
                                         4, 0, None, None, None, None, one.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                         None)
    assert rc == _lib.WOST_ERR_INVALID_ARG and b"exceeds" in _lib.lib.wost_last_error()
    # a disabled specialised kernel: refused at the solve
    s.set_jit(False)
    with pytest.raises(NotImplementedError, match="field-specialised"):
        s.solve_greens_map(pts, grid, **kw)
    s.set_jit(True)
    gm = s.solve_greens_map(pts, grid, **kw)
    assert gm.sums.shape == (3, 4, 4, 4) and (gm.sums != 0).any()


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _case.cache_clear()
