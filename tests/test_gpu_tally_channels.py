"""Channel maps on the device (wost_solve_range_tally_channels, WostSolver_2D.solve_greens_maps;
DESIGN.md 7f "Channel maps"): the tally of a handle with wavenumbers and / or models, map t a
weighted combination of the launch's channels formed per deposit in the kernel.

 A. the walks are untouched: values, steps, block and point rows are solve_range's, all C channels;
 B. the link to the one-channel tally: k^2 = 0 with the weight [[1]] gives its integers; on the
    box, k = 1 gives those of a handle with the explicit field sigma = k^2 alpha;
 C. every unit row of a K = 3 launch is the one-map tally of a handle with that wavenumber
    alone; the tree kernel's maps are the scan kernel's;
 D. two models x two wavenumbers: every unit row is that model's own handle; the paired
    difference map is consistent with its two parts;
 E. a weighted row against its unit rows, within a bound derived from the roundings alone;
 F. the integers do not depend on the launch shape, shards add up, R = 1 is the sum of R = 4's
    rows, row_walks is as stated;
 G. six rows through the facade equal the same rows asked for one at a time;
 H. the expectation: the screened Green's function of the unit disk at the centre;
 I. the flag, the refusals, and greens_section_25d against solve_greens_maps.

3 points x 16384 walks (4 blocks: R = 4 has one block per row), 200 steps, 4 x 4 cells.
tests/test_tally_channels_host.py checks the combination rule and the layout on the host."""
import ctypes
import dataclasses
import functools
import math
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 16384
STEPS = 200
SEED = 20260117
B = 4096
K3 = (0.5, 1.0, 2.0)   # k^2 = 0.25, 1, 4: powers of two


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the problems -----------------------------------------------------------------------------
def _box_alpha1():
    from dcrmontecarlo_amd import fields as F

    return 2.0 + 1.0 * F.exp(-0.5 * ((F.X - 2.0) ** 2 + (F.Y + 1.5) ** 2))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(make(**fields) -> solver, points, eps, a 4 x 4 grid around the points, wavenumbers)."""
    from dcrmontecarlo_amd import PolyLinesSimple, WostSolver_2D
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey
    from dcrmontecarlo_amd import wavenumber as WN
    from dcrmontecarlo_amd.greens_map import TallyGrid

    if name == "box":   # DESIGN.md 7a's half-plane box: alpha = 2, sigma_bar = 5, Neumann top; interior points
        D = PolyLinesSimple(np.array([[-10, 0], [-10, -10], [10, -10], [10, 0]], np.float32))
        N = PolyLinesSimple(np.array([[10, 0], [-10, 0]], np.float32))
        src = survey.electrode_source((0.0, 0.0), 0.25, 1.0)

        def make(alpha=2.0, sigma=None, sigma_bar=5.0, tree=None):
            return WostSolver_2D(D, 0.0, N, source=src, sigma=sigma, alpha=alpha, compat="fixed", sigma_bar=sigma_bar,
                                 device=0)

        pts = np.array([[1.0, -1.0], [2.0, -0.5], [3.0, -2.0]], np.float32)
        return make, pts, 1e-3, TallyGrid(-1.0, -4.0, 1.5, 1.0, 4, 4), K3
    if name == "dd":   # dcr_dipole, 6 electrodes, at sigma_bar_for(k_max): collision weights in [0, 1]
        sc = S.dcr_dipole(6, n_walks=W)
        sc = dataclasses.replace(sc, f=survey.dipole_source(sc.points[2], sc.points[3], 0.5), max_steps=STEPS, g=None)
        k = (0.0, 0.5, 1.0)
        sb = WN.sigma_bar_for(sc.solver(device=0), max(k))

        def make(alpha=None, sigma=None, sigma_bar=sb, tree=None):
            scn = dataclasses.replace(sc, sigma=sigma if sigma is not None else sc.sigma)
            return scn.solver(compat="fixed", device=0, sigma_bar=sigma_bar)

        # a walk moves ~2 / sqrt(sigma_bar) = 0.06 per step: points and cells close together
        pts = np.array([[-60.0, -0.2], [-59.7, 0.1], [-60.3, 0.3]], np.float32)
        return make, pts, sc.eps, TallyGrid(-60.83, -0.79, 0.4, 0.4, 4, 4), k
    if name == "tree":   # a 200-segment topographic surface: the segment-tree kernel; sigma' is 0 near the points
        sc = S.wenner_topography(n_electrodes=4, n_walks=W, n_segments=200, physical=True)
        sc = dataclasses.replace(sc, max_steps=STEPS, g=None)

        def make(alpha=None, sigma=None, sigma_bar=1.0, tree=True):
            s = sc.solver(compat="fixed", device=0, sigma_bar=sigma_bar)
            s.set_segment_tree(0 if tree else -1)
            return s

        x = np.array([-400.0, -395.0, -405.0])
        pts = np.stack([x, 1.0 + 2.0 * np.sin(x / 37.0) - np.array([0.1, 2.0, 5.0])], axis=1).astype(np.float32)
        return make, pts, sc.eps, TallyGrid(-450.3, -60.1, 25.0, 16.0, 4, 4), (0.0, 0.25, 0.5)
    raise KeyError(name)


def _solver(name, k=None, **kw):
    s = _case(name)[0](**kw)
    s.set_fixed_step_check(False)   # (the walks are truncated at 200 steps; fine here)
    if k is not None:
        s.set_wavenumbers(k)
    return s


def _range(s, pts, eps, w0=0, w1=W):
    """wost_solve_range's block rows, point rows, values and steps for the handle's C channels."""
    from dcrmontecarlo_amd import _lib

    p = np.ascontiguousarray(pts, np.float32)
    n, nw, C = len(p), w1 - w0, s.num_channels()
    blocks, rows = np.zeros((n, -(-nw // B), 2 * C + 1)), np.zeros((n, 2 * C + 1))
    wv, ws = np.empty((n, nw, C), np.float32), np.empty((n, nw), np.uint32)
    _lib.check(_lib.lib.wost_solve_range(s._h, _lib.fptr(p), n, W, w0, w1, STEPS, float(eps), SEED, _lib.dptr(blocks),
                                         _lib.dptr(rows), _lib.fptr(wv), _lib.u32ptr(ws)), "wost_solve_range")
    return blocks, rows, wv, ws


def _default_scale(s, R, w0=0, w1=W):
    from dcrmontecarlo_amd import _lib

    sl = ctypes.c_int32(0)
    _lib.check(_lib.lib.wost_tally_default_scale(s._h, W, w0, w1, R, STEPS, ctypes.byref(sl)), "default scale")
    return int(sl.value)


def _maps_rc(s, pts, grid, R, weights, eps, w0=0, w1=W, scale=None, fill=-1):
    """wost_solve_range_tally_channels through the C ABI: (rc, (block rows, point rows, values,
    steps, tally [n, R, T, bins], row_walks [n, R], scale_log2))."""
    from dcrmontecarlo_amd import _lib
    from dcrmontecarlo_amd.greens_map import _c_grid

    p = np.ascontiguousarray(pts, np.float32)
    w = np.ascontiguousarray(np.atleast_2d(np.asarray(weights, np.float32)))
    n, nw, C, T = len(p), w1 - w0, s.num_channels(), w.shape[0]
    if scale is None:   # the facade's default: one channel's bound times the largest row sum
        scale = _default_scale(s, R, w0, w1) - int(np.ceil(np.log2(np.abs(w.astype(np.float64)).sum(axis=1).max())))
    cg = _c_grid(grid)
    blocks, rows = np.zeros((n, -(-nw // B), 2 * C + 1)), np.zeros((n, 2 * C + 1))
    wv, ws = np.empty((n, nw, C), np.float32), np.empty((n, nw), np.uint32)
    tally = np.full((n, R, T, grid.nx * grid.ny + 1), fill, np.int64)
    rw = np.full((n, R), fill, np.int64)
    i64 = ctypes.POINTER(ctypes.c_int64)
    rc = _lib.lib.wost_solve_range_tally_channels(
        s._h, _lib.fptr(p), n, W, w0, w1, STEPS, float(eps), SEED, ctypes.byref(cg), R, scale, _lib.fptr(w), T,
        _lib.dptr(blocks), _lib.dptr(rows), _lib.fptr(wv), _lib.u32ptr(ws), tally.ctypes.data_as(i64),
        rw.ctypes.data_as(i64))
    return rc, (blocks, rows, wv, ws, tally, rw, scale)


def _maps(*a, **kw):
    from dcrmontecarlo_amd import _lib

    rc, out = _maps_rc(*a, **kw)
    _lib.check(rc, "wost_solve_range_tally_channels")
    return out


def _one(s, pts, grid, R, eps, scale, w0=0, w1=W):
    """wost_solve_range_tally (the one-channel tally): tally [n, R, bins]."""
    from dcrmontecarlo_amd import _lib
    from dcrmontecarlo_amd.greens_map import _c_grid

    p = np.ascontiguousarray(pts, np.float32)
    cg = _c_grid(grid)
    tally = np.full((len(p), R, grid.nx * grid.ny + 1), -1, np.int64)
    i64 = ctypes.POINTER(ctypes.c_int64)
    _lib.check(_lib.lib.wost_solve_range_tally(s._h, _lib.fptr(p), len(p), W, w0, w1, STEPS, float(eps), SEED,
                                               ctypes.byref(cg), R, scale, None, None, None, None,
                                               tally.ctypes.data_as(i64), None), "wost_solve_range_tally")
    return tally


# ---- A. the walks are untouched ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "dd", "tree"])
def test_a_channel_tally_walks_the_handles_walks(gpu_available, name):
    _, pts, eps, grid, k = _case(name)
    s = _solver(name, k)
    assert s.num_channels() == 3
    plain = _range(s, pts, eps)
    got = _maps(s, pts, grid, 4, [[0.5, -1.0, 0.25], [0.0, 1.0, 0.0]], eps)
    t = s.timing()
    assert t["jit"] == 1 and t["tree"] == (1 if name == "tree" else 0)
    np.testing.assert_array_equal(got[3], plain[3], err_msg="step counts")
    np.testing.assert_array_equal(_bits(got[2]), _bits(plain[2]), err_msg="per-walk values of every channel")
    np.testing.assert_array_equal(got[0], plain[0], err_msg="block rows")
    np.testing.assert_array_equal(got[1], plain[1], err_msg="point rows")
    assert (got[4][:, :, 0] != 0).any() and (got[4][:, :, 1] != 0).any() and (got[5] == B).all()
    # ... and the handle's next plain solve is what it was
    again = _range(s, pts, eps)
    np.testing.assert_array_equal(_bits(again[2]), _bits(plain[2]))
    # a shard of the walks: the same walks as solve_range's shard
    shard = _maps(s, pts, grid, 4, [[0.0, 0.0, 1.0]], eps, B, 3 * B)
    np.testing.assert_array_equal(_bits(shard[2]), _bits(plain[2][:, B:3 * B]))
    np.testing.assert_array_equal(shard[0], plain[0][:, 1:3])


# ---- B. the link to the one-channel tally -----------------------------------------------------
@pytest.mark.parametrize("name", ["dd", "tree"])
def test_k_zero_with_unit_weight_is_the_one_channel_tally(gpu_available, name):
    _, pts, eps, grid, _ = _case(name)
    plain = _solver(name)
    scale = _default_scale(plain, 4)
    want = _one(plain, pts, grid, 4, eps, scale)
    got = _maps(_solver(name, [0.0]), pts, grid, 4, [[1.0]], eps, scale=scale)
    assert got[4].shape == (3, 4, 1, 17)
    np.testing.assert_array_equal(got[4][:, :, 0], want)
    assert (want[:, :, :16] > 0).any()
    # a handle without wavenumbers or models has one channel too
    np.testing.assert_array_equal(_maps(plain, pts, grid, 4, [[1.0]], eps, scale=scale)[4][:, :, 0], want)


def test_one_wavenumber_is_the_explicit_sigma_field(gpu_available):
    """Box, alpha = 2: k = 1 against the one-channel tally of sigma = k^2 alpha = 2 (exact)."""
    _, pts, eps, grid, _ = _case("box")
    explicit = _solver("box", sigma=2.0)
    scale = _default_scale(explicit, 4)
    want = _one(explicit, pts, grid, 4, eps, scale)
    got = _maps(_solver("box", [1.0]), pts, grid, 4, [[1.0]], eps, scale=scale)
    np.testing.assert_array_equal(got[4][:, :, 0], want)
    assert (want[:, :, :16] > 0).mean() >= 0.5


# ---- C. unit rows -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "dd", "tree"])
def test_unit_rows_are_the_single_wavenumber_tallies(gpu_available, name):
    _, pts, eps, grid, k = _case(name)
    s = _solver(name, k)
    scale = _default_scale(s, 4)
    got = _maps(s, pts, grid, 4, np.eye(3), eps, scale=scale)
    for j, kj in enumerate(k):
        alone = _maps(_solver(name, [kj]), pts, grid, 4, [[1.0]], eps, scale=scale)
        np.testing.assert_array_equal(got[4][:, :, j], alone[4][:, :, 0], err_msg=f"wavenumber {kj}")
    assert (got[4][:, :, 0] != got[4][:, :, 2]).any()   # (the wavenumbers do differ)
    if name == "tree":   # the tree kernel's maps are the scan kernel's
        assert s.timing()["tree"] == 1
        scan = _solver(name, k, tree=False)
        other = _maps(scan, pts, grid, 4, np.eye(3), eps, scale=scale)
        assert scan.timing()["tree"] == 0
        np.testing.assert_array_equal(other[4], got[4])


# ---- D. models ----------------------------------------------------------------------------------
def _box_models():
    from dcrmontecarlo_amd import survey

    models = [(None, 2.0), (None, _box_alpha1())]
    sb = 1.05 * survey.sigma_bar_for_models(_case("box")[0](), models, 1.0)
    return models, sb


def test_unit_rows_of_two_models_are_each_models_own_handle(gpu_available):
    _, pts, eps, grid, _ = _case("box")
    models, sb = _box_models()
    k = [0.5, 1.0]
    s = _solver("box", k, sigma_bar=sb)
    s.set_models(models)
    assert s.num_channels() == 4
    scale = _default_scale(s, 4)
    got = _maps(s, pts, grid, 4, np.eye(4), eps, scale=scale)
    plain = _range(s, pts, eps)
    np.testing.assert_array_equal(_bits(got[2]), _bits(plain[2]))
    for m, (_, alpha) in enumerate(models):
        for j, kj in enumerate(k):   # channel m * NK + j
            own = _maps(_solver("box", [kj], alpha=alpha, sigma_bar=sb), pts, grid, 4, [[1.0]], eps, scale=scale)
            np.testing.assert_array_equal(got[4][:, :, m * 2 + j], own[4][:, :, 0], err_msg=f"model {m}, k {kj}")
    assert (got[4][:, :, 0] != got[4][:, :, 2]).any(), "the two models differ"


def _row_bound(Q, w, D, C):
    """E's bound in quanta: (D / 2)(1 + sum |w_c|) + gamma_C sum_c |w_c| (Q_c + D / 2)."""
    g = C * 2.0 ** -24 / (1.0 - C * 2.0 ** -24)
    aw = np.abs(np.asarray(w, np.float64))
    return D / 2.0 * (1.0 + aw.sum()) + g * sum(aw[c] * (Q[c] + D / 2.0) for c in range(len(aw)))


def test_the_paired_difference_map_is_consistent(gpu_available):
    from dcrmontecarlo_amd import survey

    _, pts, eps, grid, _ = _case("box")
    models, sb = _box_models()
    s = _solver("box", sigma_bar=sb)
    diff, bg, md = survey.paired_difference_map(s, models[1], models[0], pts, grid, nWalks=W, maxSteps=STEPS, eps=eps,
                                                seed=SEED, replicas=4)
    ws = _range(s, pts, eps)[3]   # (the paths depend on sigma_bar alone: the models' walks are the handle's)
    assert s.models is None and s.num_channels() == 1   # restored
    assert diff.quantum == bg.quantum == md.quantum and (bg.sums >= 0).all() and (md.sums >= 0).all()
    D = ws.astype(np.float64).reshape(len(pts), 4, B).sum(axis=2)[:, :, None, None]   # steps per (point, row)
    Q = [bg.sums.astype(np.float64), md.sums.astype(np.float64)]
    err = np.abs(diff.sums.astype(np.float64) - (Q[1] - Q[0]))
    bound = _row_bound(Q, [-1.0, 1.0], D, 2)
    print(f"paired difference: largest error / bound {np.max(err / bound):.3g}; |difference| up to "
          f"{np.abs(diff.sums).max()} quanta of {np.abs(md.sums).max()}")
    assert (err <= bound).all() and (diff.sums != 0).any()
    # the unit rows are the two models' own maps
    own = _solver("box", alpha=models[1][1], sigma_bar=sb).solve_greens_maps(
        pts, grid, [[1.0]], nWalks=W, maxSteps=STEPS, eps=eps, seed=SEED, replicas=4, quantum=md.quantum)[0]
    np.testing.assert_array_equal(own.sums, md.sums)


# ---- E. a weighted row against its unit rows ----------------------------------------------------
@pytest.mark.parametrize("name", ["box", "dd"])
def test_a_weighted_row_against_its_unit_rows(gpu_available, name):
    """Per point, replica row and cell (so also per point and cell): |Q_t - sum_c w_c Q_c| <=
    (D / 2)(1 + sum |w_c|) + gamma_C sum_c |w_c| (Q_c + D / 2) quanta, gamma_C = C 2^-24 / (1 -
    C 2^-24), D the row's walk steps. Every deposit is rounded to the quantum once (1/2 each:
    D / 2 for the row's own sum, |w_c| D / 2 for the unit rows'), and v_t is C float32
    products and sums of terms |w_c| d_c, d_c >= 0: relative error gamma_C of sum_c |w_c| d_c,
    whose exact sum over the row's deposits is at most sum_c |w_c| (Q_c + D / 2) quanta.
    Nothing in the bound is measured. The collision weights lie in [0, 1] (sigma_bar covers
    sigma' + k^2), so the deposits are non-negative."""
    _, pts, eps, grid, k = _case(name)
    s = _solver(name, k)
    scale = _default_scale(s, 4) - 2
    worst = 0.0
    for w in ([0.75, -1.5, 0.3], [-0.2, 0.6, -1.0 / 3.0]):
        w32 = np.asarray(w, np.float32)
        got = _maps(s, pts, grid, 4, np.vstack([w32[None], np.eye(3, dtype=np.float32)]), eps, scale=scale)
        tally = got[4].astype(np.float64)[..., :16]                   # [n, R, 4, 16]
        assert (got[4][:, :, 1:] >= 0).all() and (got[4][:, :, 1:, :16] > 0).mean() >= 0.5
        D = got[3].astype(np.float64).reshape(len(pts), 4, B).sum(axis=2)[:, :, None]
        Q = [tally[:, :, 1 + c] for c in range(3)]
        err = np.abs(tally[:, :, 0] - sum(float(w32[c]) * Q[c] for c in range(3)))
        bound = _row_bound(Q, w32, D, 3)
        worst = max(worst, float(np.max(err / bound)))
        assert (err <= bound).all()
        assert (w32 < 0).any() and (w32 > 0).any() and (tally[:, :, 0] != 0).any()   # a row of mixed signs
    print(f"{name}: weighted row: largest error / bound {worst:.3g} (quantum 2^{-scale})")


# ---- F. order independence ----------------------------------------------------------------------
def test_the_integers_do_not_depend_on_order(gpu_available):
    _, pts, eps, grid, k = _case("box")
    wts = [[0.5, 0.25, -0.125], [0.0, 1.0, 0.0]]
    s = _solver("box", k)
    scale = _default_scale(s, 4)
    full = _maps(s, pts, grid, 4, wts, eps, scale=scale)
    assert (full[5] == B).all()                                   # 4 blocks, one per row
    for opts in ({"chunk0": 1, "chunk_min": 1, "chunk_max": 1}, {"chunk0": 1024, "chunk_max": 1024, "grid_blocks_per_cu": 1}):
        o = _solver("box", k)
        for key, val in opts.items():
            o.set_option(key, val)
        other = _maps(o, pts, grid, 4, wts, eps, scale=scale)
        assert o.timing()["chunk0"] == opts["chunk0"]
        np.testing.assert_array_equal(other[4], full[4], err_msg=f"launch shape {opts}")
        np.testing.assert_array_equal(other[5], full[5])
    # two walk-range shards add up
    a = _maps(s, pts, grid, 4, wts, eps, 0, B, scale=scale)
    b = _maps(s, pts, grid, 4, wts, eps, B, W, scale=scale)
    np.testing.assert_array_equal(a[4] + b[4], full[4])
    np.testing.assert_array_equal(a[5], np.tile([B, 0, 0, 0], (len(pts), 1)))
    np.testing.assert_array_equal(b[5], np.tile([0, B, B, B], (len(pts), 1)))
    assert (a[4][:, 1:] == 0).all() and (b[4][:, 0] == 0).all()
    # R = 1 is the sum of R = 4's rows; R = 3 wraps block 3 into row 0
    one = _maps(s, pts, grid, 1, wts, eps, scale=scale)
    np.testing.assert_array_equal(one[4][:, 0], full[4].sum(axis=1))
    assert (one[5] == W).all()
    three = _maps(s, pts, grid, 3, wts, eps, scale=scale)
    np.testing.assert_array_equal(three[4][:, 0], full[4][:, 0] + full[4][:, 3])
    np.testing.assert_array_equal(three[4][:, 1:], full[4][:, 1:3])
    np.testing.assert_array_equal(three[5], np.tile([2 * B, B, B], (len(pts), 1)))


# ---- G. chunking ----------------------------------------------------------------------------------
def test_six_rows_equal_the_rows_one_at_a_time(gpu_available):
    _, pts, eps, grid, k = _case("box")
    s = _solver("box", k)
    rows = np.array([[1, 0, 0], [0.5, 0.5, 0], [0, 1, 0], [0.1, -0.2, 0.3], [0, 0, 1], [1.0 / 3.0, 1.0 / 7.0, -1.0]])
    kw = dict(nWalks=W, maxSteps=STEPS, eps=eps, seed=SEED, replicas=4, quantum=2.0 ** -30)
    maps, u, st = s.solve_greens_maps(pts, grid, rows, return_channels=True, **kw)
    assert len(maps) == 6 and u.shape == (3, 3) and st.stderr.shape == (3, 3)
    plain = _range(s, pts, eps)
    np.testing.assert_array_equal(_bits(u), _bits((plain[1][:, 0:6:2] / W).astype(np.float32)))
    for t, row in enumerate(rows):
        alone = s.solve_greens_maps(pts, grid, row, **kw)
        assert len(alone) == 1
        np.testing.assert_array_equal(alone[0].sums, maps[t].sums, err_msg=f"row {t}")
        np.testing.assert_array_equal(alone[0].outside, maps[t].outside)
        np.testing.assert_array_equal(alone[0].row_walks, maps[t].row_walks)
    assert (maps[3].sums != 0).any() and maps[0].quantum == 2.0 ** -30


# ---- H. the expectation ---------------------------------------------------------------------------
def _disk_cell_average(ex, ey, i, j, k, rho_b, nodes=48):
    """Cell average of G_k(0, y) = [K0(k r) - I0(k r) K0(k rho) / I0(k rho)] / (2 pi), the
    Green's function of Laplace(u) - k^2 u = -delta on the disk of radius rho with u = 0 on
    its boundary, pole at the centre, by Gauss-Legendre quadrature in double."""
    from scipy.special import i0, k0

    t, wq = np.polynomial.legendre.leggauss(nodes)
    x = 0.5 * (ex[i] + ex[i + 1]) + 0.5 * (ex[i + 1] - ex[i]) * t
    y = 0.5 * (ey[j] + ey[j + 1]) + 0.5 * (ey[j + 1] - ey[j]) * t
    r = np.hypot(x[:, None], y[None, :])
    g = (k0(k * r) - i0(k * r) * k0(k * rho_b) / i0(k * rho_b)) / (2.0 * math.pi)
    return float((wq[:, None] * wq[None, :] * g).sum() / 4.0)


def test_the_maps_of_the_disk_are_its_screened_greens_functions(gpu_available):
    """Unit disk through a 64-gon, alpha = 1, sigma_bar = 5, k in {1, 2}, query point at the
    centre, R = 32 rows of one block each; rows e_0, e_1 and (0.5, 0.25). The polygon lies
    between the disks of radius cos(pi / 64) and 1 and the screened Green's function grows
    with the domain too, so every cell average lies between those of the two disks; the
    weighted row's weights are positive, so its bracket follows by linearity. Every cell of
    the 4 x 3 grid except the two that share the pole must lie within 4 of its own standard
    errors of that interval. R = 32 rather than 8: the 30 checks against a t-distribution
    with 7 degrees of freedom would fail by chance about one time in eight. DESIGN.md 9 item
    0's bias of the compat="fixed" screened estimator, a few 1e-3 relative, is far below this
    test's resolution (a cell's relative standard error is a few per cent here) and is not
    what it checks. There is no CPU oracle for this expectation (compat="fixed" has none)."""
    from dcrmontecarlo_amd import PolyLinesSimple, WostSolver_2D
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd.greens_map import TallyGrid, tally_edges

    s = WostSolver_2D(PolyLinesSimple(S._circle(64, 1.0)), None, None, alpha=1.0, compat="fixed", sigma_bar=5.0, device=0)
    k = [1.0, 2.0]
    s.set_wavenumbers(k)
    grid = TallyGrid(-0.6, -0.6, 0.3, 0.4, 4, 3)
    R = 32
    rows = np.array([[1.0, 0.0], [0.0, 1.0], [0.5, 0.25]])
    maps = s.solve_greens_maps(np.zeros((1, 2), np.float32), grid, rows, nWalks=R * B, maxSteps=STEPS, eps=1e-4,
                               seed=SEED, replicas=R)
    assert s.source is None and len(maps) == 3 and maps[0].sums.shape == (1, R, 3, 4) and (maps[0].row_walks == B).all()
    ex, ey = (e.astype(np.float64) for e in tally_edges(grid))
    worst = 0.0
    for t, gm in enumerate(maps):
        mean, se = gm.mean[0], gm.stderr[0]
        for j in range(3):
            for i in range(4):
                if j == 1 and i in (1, 2):
                    continue
                lo = sum(rows[t, c] * _disk_cell_average(ex, ey, i, j, k[c], math.cos(math.pi / 64)) for c in range(2))
                hi = sum(rows[t, c] * _disk_cell_average(ex, ey, i, j, k[c], 1.0) for c in range(2))
                z = max(lo - mean[j, i], mean[j, i] - hi, 0.0) / se[j, i]
                worst = max(worst, z)
                print(f"row {t} cell ({i}, {j}): mean {mean[j, i]:.6f} +- {se[j, i]:.2g}, expected [{lo:.6f}, {hi:.6f}]: "
                      f"{z:.2f} stderr")
                assert se[j, i] > 0 and lo < hi and z <= 4.0
    print(f"disk: worst cell {worst:.2f} stderr outside its interval")


# ---- I. the flag and the refusals -------------------------------------------------------------
def test_a_quantum_too_fine_for_a_weighted_row_raises_and_writes_nothing(gpu_available):
    from dcrmontecarlo_amd import _lib

    _, pts, eps, grid, k = _case("box")
    s = _solver("box", k)
    wts = [[1.0, 0.0, 0.0], [4096.0, 4096.0, 0.0]]
    with pytest.raises(ValueError, match="quantum"):
        s.solve_greens_maps(pts, grid, wts, nWalks=W, maxSteps=STEPS, eps=eps, seed=SEED, replicas=4, quantum=2.0 ** -90)
    # a quantum at which the unit row fits and the weighted row does not
    fine = _default_scale(s, 4) + 14
    assert (_maps(s, pts, grid, 4, wts[:1], eps, scale=fine)[4] > 0).any()
    rc, out = _maps_rc(s, pts, grid, 4, wts, eps, scale=fine)
    msg = _lib.lib.wost_last_error().decode()
    assert rc == _lib.WOST_ERR_INVALID_ARG and "quantum" in msg
    assert (out[4] == -1).all() and (out[5] == -1).all(), "a refused solve returns no sums"
    named = int(re.search(r"scale_log2 (-?\d+)", msg).group(1))
    assert named < fine
    fits = _maps(s, pts, grid, 4, wts, eps, scale=named)
    assert (fits[4][:, :, 1] > 0).any()
    assert _lib.lib.wost_version() == 6


def test_refusals(gpu_available):
    from dcrmontecarlo_amd import _lib
    from dcrmontecarlo_amd import survey
    from dcrmontecarlo_amd.greens_map import _c_grid

    make, pts, eps, grid, k = _case("dd")
    kw = dict(nWalks=W, maxSteps=STEPS, eps=eps, seed=SEED, replicas=4)
    s = _solver("dd", k)

    def refused(solver, weights=np.eye(3), g=grid, R=4, n_maps=None, scale=0, null_weights=False, null_tally=False):
        w = np.ascontiguousarray(np.atleast_2d(np.asarray(weights, np.float32)))
        T = w.shape[0] if n_maps is None else n_maps
        p = np.ascontiguousarray(pts, np.float32)
        cg = _c_grid(g)
        one = np.full(1, -1, np.int64)   # (the library refuses before it writes: one entry is enough)
        rc = _lib.lib.wost_solve_range_tally_channels(
            solver._h, _lib.fptr(p), len(p), W, 0, W, STEPS, float(eps), SEED, ctypes.byref(cg), R, scale,
            None if null_weights else _lib.fptr(w), T, None, None, None, None,
            None if null_tally else one.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None)
        assert one[0] == -1
        return rc, _lib.lib.wost_last_error().decode()

    # compat="reference"
    from dcrmontecarlo_amd import scenarios as S
    sc = S.dcr_dipole(6, n_walks=W)
    r = sc.solver(device=0, sigma_bar=s.sigma_bar)
    r.set_wavenumbers(k)
    rc, msg = refused(r)
    assert rc == _lib.WOST_ERR_UNSUPPORTED and "fixed" in msg
    with pytest.raises(NotImplementedError, match="fixed"):
        r.solve_greens_maps(pts, grid, np.eye(3), **kw)
    # more than one source
    with s.sources_installed(s.source_fields([sc.f, 2.0 * sc.f])):
        rc, msg = refused(s, np.eye(6))
        assert rc == _lib.WOST_ERR_UNSUPPORTED and "one source" in msg
        with pytest.raises(NotImplementedError, match="one source"):
            s.solve_greens_maps(pts, grid, np.eye(6), **kw)
    # point charges; no source field
    ps = dataclasses.replace(sc, f=None).solver(compat="fixed", device=0, sigma_bar=s.sigma_bar)
    rc, msg = refused(ps, [[1.0]])
    assert rc == _lib.WOST_ERR_INVALID_ARG and "source field" in msg
    e = np.asarray(sc.points, np.float64)
    ps.set_point_sources([survey.point_dipole(e[2], e[3])])
    rc, msg = refused(ps, [[1.0]])
    assert rc == _lib.WOST_ERR_UNSUPPORTED and "point sources" in msg
    with pytest.raises(NotImplementedError, match="point sources"):
        ps.solve_greens_maps(pts, grid, [[1.0]], **kw)
    # the maps and their weights
    for n_maps in (0, -1, 5):
        rc, msg = refused(s, np.ones((5, 3)), n_maps=n_maps)
        assert rc == _lib.WOST_ERR_INVALID_ARG and "n_maps" in msg
    assert "NULL" in refused(s, null_weights=True)[1]
    assert "finite" in refused(s, [[1.0, np.nan, 0.0]])[1] and "finite" in refused(s, [[np.inf, 0.0, 0.0]])[1]
    assert "zero" in refused(s, [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])[1]
    with pytest.raises(ValueError, match="shape"):
        s.solve_greens_maps(pts, grid, np.eye(2), **kw)
    with pytest.raises(ValueError, match="zero"):
        s.solve_greens_maps(pts, grid, [[0.0, 0.0, 0.0]], **kw)
    # grids, replicas, scales, the buffer (with its factor T)
    assert "NULL tally" in refused(s, null_tally=True)[1]
    for bad in ((0.0, 0.0, 0.0, 1.0, 4, 4), (0.0, 0.0, 1.0, 1.0, 0, 4), (1.0e9, 0.0, 1.0, 1.0, 4, 4)):
        assert refused(s, g=bad)[0] == _lib.WOST_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            s.solve_greens_maps(pts, bad, np.eye(3), **kw)
    assert "replicas" in refused(s, R=0)[1] and "scale_log2" in refused(s, scale=101)[1]
    big = (-100.0, -100.0, 0.05, 0.05, 2048, 2048)   # 3 points x 4 rows x 2^22 bins x 8 bytes: one map would fit
    rc, msg = refused(s, np.eye(3), g=big)
    assert rc == _lib.WOST_ERR_INVALID_ARG and "exceeds" in msg and "3 maps" in msg
    with pytest.raises(ValueError, match="exceeds"):
        s.solve_greens_maps(pts, big, np.eye(3), **kw)
    # a disabled specialised kernel: refused at the solve
    s.set_jit(False)
    rc, msg = refused(s)
    assert rc == _lib.WOST_ERR_UNSUPPORTED and "field-specialised" in msg
    with pytest.raises(NotImplementedError, match="field-specialised"):
        s.solve_greens_maps(pts, grid, np.eye(3), **kw)
    s.set_jit(True)
    maps = s.solve_greens_maps(pts, grid, np.eye(3), **kw)
    assert len(maps) == 3 and maps[0].sums.shape == (3, 4, 4, 4) and (maps[0].sums != 0).any()
    np.testing.assert_array_equal(s.wavenumbers, k)


def test_the_25d_section_is_the_row_of_half_weights(gpu_available):
    from dcrmontecarlo_amd import wavenumber as WN

    _, pts, eps, grid, _ = _case("box")
    s = _solver("box")
    kw = dict(nWalks=W, maxSteps=STEPS, eps=eps, seed=SEED, replicas=4, quantum=2.0 ** -32)
    gm, units, k, w = WN.greens_section_25d(s, pts, grid, 2.0, 6.0, per_wavenumber=True, **kw)
    assert s.wavenumbers is None and k.size == 4 and len(units) == 4   # restored; r_max / r_min = 3: four wavenumbers
    assert float(k.max()) ** 2 < 5.0   # (sigma_bar covers k_max^2 = 4)
    s.set_wavenumbers(k)
    want = s.solve_greens_maps(pts, grid, [w / 2.0] + list(np.eye(4)), **kw)
    np.testing.assert_array_equal(gm.sums, want[0].sums)
    np.testing.assert_array_equal(gm.outside, want[0].outside)
    for j in range(4):
        np.testing.assert_array_equal(units[j].sums, want[1 + j].sums)
    s.set_wavenumbers(None)
    gm2, k2, w2 = WN.greens_section_25d(s, pts, grid, 2.0, 6.0, **kw)
    np.testing.assert_array_equal(gm2.sums, gm.sums)


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _case.cache_clear()
