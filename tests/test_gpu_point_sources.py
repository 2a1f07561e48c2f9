"""Point sources on the device (WostSolver_2D.set_point_sources, wost_set_point_sources;
DESIGN.md 7b): a walk scores every charge inside a step's ball and visible from its point
with the ball's Green's function, exactly, instead of sampling a source field.

All cases run compat="fixed" with eps = 1e-4 and 16 blocks (65,536 walks) per point unless
said otherwise.

The statistical rule. Polygonal Dirichlet arcs are regular with circumradius 1, so domain
monotonicity of the Green's function brackets the polygon's solution between the closed
forms of the inscribed disk (radius cos(pi / n) for an n-gon) and of the unit disk:
    G_in - 4 se <= mean <= G_out + 4 se    and    se <= 0.02 G_out,
se being the solve's own standard error. The 2% cap is a sizing condition.

What this file pins, and what it does not. These cases are statistical: they check the
multi-step walk -- the estimator's expectation, the weights carried from step to step, the
boundary codes after Neumann hits -- to a few standard errors, i.e. to about 1%. The score of a
single step is pinned deterministically elsewhere, in tests/test_gpu_point_sources_step.py:
one-step solves against the double closed form, to a bound of a few float32 ulps derived from
the device's operations -- ball_greens and the three ranges of ball_greens_screened on the
device's own arithmetic, the in-ball edge, the rmin clamp, the t = 88 cut-off, alpha(z_p),
the factor 2 and the corner radius of a surface point, point_code, visibility through the scan
and the tree kernel, and the source and wavenumber channel mapping. The bit-equalities below
(channel against single solve, tree against scan, shards) say nothing about the value itself."""
import dataclasses
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 1e-4
W16 = 16 * 4096
SEED = 17
TWO_PI = 2.0 * math.pi


# ---- geometry and closed forms ----------------------------------------------------------------
def _arc(n_seg, a0, a1):
    """Regular polyline of n_seg segments on the unit circle from angle a0 to a1, its ends exact."""
    th = np.linspace(a0, a1, n_seg + 1)
    v = np.stack([np.cos(th), np.sin(th)], axis=1)
    v[np.abs(v) < 1e-15] = 0.0
    return v.astype(np.float32)


def _inradius(n_seg, a0, a1):
    return math.cos(0.5 * (a1 - a0) / n_seg)


def g_disk(x, z, a=1.0):
    """Green's function of the disk of radius a (Dirichlet 0) by the image charge."""
    X, Z = complex(*x) / a, complex(*z) / a
    return math.log(abs(1.0 - X * Z.conjugate()) / abs(X - Z)) / TWO_PI


def g_screened_disk(rho, kappa, a=1.0):
    """[K0(kappa rho) - K0(kappa a) I0(kappa rho) / I0(kappa a)] / 2 pi: a unit charge at the centre."""
    from scipy.special import i0, k0

    return (k0(kappa * rho) - k0(kappa * a) * i0(kappa * rho) / i0(kappa * a)) / TWO_PI


def g_wedge(x, z, a=1.0):
    """The sector 0 < phi < 3 pi / 2 of the disk of radius a, Neumann on its two straight
    edges, Dirichlet 0 on the arc: zeta = rho^(2/3) exp(2 i phi / 3) maps it onto the upper
    half disk, where the Neumann diameter is an even reflection."""
    def zeta(p):
        rho = math.hypot(p[0], p[1]) / a
        phi = math.atan2(p[1], p[0]) % TWO_PI
        return rho ** (2.0 / 3.0) * complex(math.cos(2.0 * phi / 3.0), math.sin(2.0 * phi / 3.0))

    def gd(A, B):
        return math.log(abs(1.0 - A * B.conjugate()) / abs(A - B)) / TWO_PI

    Z, Z0 = zeta(x), zeta(z)
    return gd(Z, Z0) + gd(Z, Z0.conjugate())


def _polar(rho, deg):
    return (rho * math.cos(math.radians(deg)), rho * math.sin(math.radians(deg)))


def _solver(D, N=None, **kw):
    from dcrmontecarlo_amd import PolyLinesSimple, WostSolver_2D

    return WostSolver_2D(PolyLinesSimple(np.asarray(D, np.float32)), 0.0,
                         None if N is None else PolyLinesSimple(np.asarray(N, np.float32)), compat="fixed", **kw)


def _check(name, st, lo, hi, idx=None):
    """The statistical rule, printing each figure first."""
    mean, se = np.atleast_1d(st.mean if idx is None else st.mean[idx]), np.atleast_1d(st.stderr if idx is None else st.stderr[idx])
    lo, hi = np.atleast_1d(np.asarray(lo, np.float64)), np.atleast_1d(np.asarray(hi, np.float64))
    print(f"{name}: bracket [{lo}, {hi}] mean {mean} se {se} se/G_out {se / hi} "
          f"z_in {(mean - lo) / se} z_out {(mean - hi) / se}")
    assert np.all(se <= 0.02 * hi)
    assert np.all(lo - 4.0 * se <= mean) and np.all(mean <= hi + 4.0 * se)


# ---- 1. Laplace disk --------------------------------------------------------------------------
@pytest.mark.parametrize("n_gon", [64, 32])
def test_laplace_disk(gpu_available, n_gon):
    """A 64-gon (g = 0), q = 1 at (0.3, 0): the unit disk's Green's function by the image
    charge, 0.08124 at (-0.2, 0.4). The 32-gon (33 vertices) takes the compiled-in polyline
    path, with its own wider bracket. (A CPU walk of this estimator: 0.08121 +- 0.00029 at
    200k walks, per-walk std / mean 1.6, i.e. a relative se of 0.6% at 65,536 walks.)"""
    z = (0.3, 0.0)
    pts = np.array([[-0.2, 0.4], [0.1, -0.7]], np.float32)
    s = _solver(_arc(n_gon, 0.0, TWO_PI))
    s.set_point_sources([[(z, 1.0)]])
    u, st = s.solve(pts, nWalks=W16, maxSteps=1000, eps=EPS, seed=SEED, return_stats=True)
    assert s.last_timing["jit"] == 1
    a = _inradius(n_gon, 0.0, TWO_PI)
    _check(f"laplace {n_gon}-gon", st, [g_disk(p, z, a) for p in pts], [g_disk(p, z) for p in pts])
    assert abs(g_disk(pts[0], z) - 0.08124) < 1e-5
    # positions are data, not code: another electrode set runs the kernel this handle has
    z2 = (-0.1, 0.25)
    s.set_point_sources([[(z2, 2.0)]])
    _, st2 = s.solve(pts, nWalks=W16, maxSteps=1000, eps=EPS, seed=SEED, return_stats=True)
    assert s.last_timing["jit"] == 1 and s.last_timing["jit_ms"] == 0.0
    _check(f"laplace {n_gon}-gon, moved charge", st2, [2.0 * g_disk(p, z2, a) for p in pts],
           [2.0 * g_disk(p, z2) for p in pts])


# ---- 2. screened disk -------------------------------------------------------------------------
def test_screened_disk(gpu_available):
    """64-gon, alpha = 1, sigma = 4 (kappa = 2), sigma_bar = 6, a unit charge at the centre,
    the query at (0.3, 0.2): [K0(2 rho) - K0(2) I0(2 rho) / I0(2)] / 2 pi = 0.09265. (A CPU walk:
    0.09297 +- 0.00039 at 20k walks, per-walk std / mean 0.6.) Then the same through
    wavenumbers (sigma = 0, k = 1 and 2), and with alpha = 2, which divides the values by 2."""
    D = _arc(64, 0.0, TWO_PI)
    a = _inradius(64, 0.0, TWO_PI)
    pts = np.array([[0.3, 0.2]], np.float32)
    rho = math.hypot(0.3, 0.2)
    s = _solver(D, sigma=4.0, alpha=1.0, sigma_bar=6.0)
    s.set_point_sources([[((0.0, 0.0), 1.0)]])
    _, st = s.solve(pts, nWalks=W16, maxSteps=1000, eps=EPS, seed=SEED, return_stats=True)
    _check("screened disk", st, g_screened_disk(rho, 2.0, a), g_screened_disk(rho, 2.0))
    assert abs(g_screened_disk(rho, 2.0) - 0.09265) < 1e-5
    for alpha in (1.0, 2.0):
        s = _solver(D, alpha=alpha, sigma_bar=6.0)
        s.set_point_sources([[((0.0, 0.0), 1.0)]])
        _, st = s.solve_wavenumbers(pts, [1.0, 2.0], nWalks=W16, maxSteps=1000, eps=EPS, seed=SEED, return_stats=True)
        for j, k in enumerate((1.0, 2.0)):
            _check(f"screened disk alpha {alpha} k {k}", st, g_screened_disk(rho, k, a) / alpha,
                   g_screened_disk(rho, k) / alpha, idx=(j, 0))


# ---- 3. half disk, surface electrode ----------------------------------------------------------
def test_half_disk_surface_electrode(gpu_available):
    """Neumann segment (1, 0) -> (-1, 0), Dirichlet half 64-gon below it, strength 1 entering at
    the origin: (1 / pi) ln(1 / rho) by reflection, 0.22064 at (0.3, -0.4) and at (0.5, 0) --
    the second query lies on the surface, the survey's case: its walks start as boundary
    points. The grazing-ray rule and the half-ball's factor 2 exist for this case. (CPU walks,
    200k: 0.22215 +- 0.00089 and 0.22135 +- 0.00097, per-walk std / mean 1.8 and 2.0.)
    Then the Neumann line split into 8 segments, the electrode at its middle vertex and the
    query one segment length away."""
    from dcrmontecarlo_amd import survey

    D = _arc(32, math.pi, TWO_PI)
    a = _inradius(32, math.pi, TWO_PI)
    exact = lambda rho, rad=1.0: math.log(rad / rho) / math.pi
    pts = np.array([[0.3, -0.4], [0.5, 0.0]], np.float32)
    s = _solver(D, [[1, 0], [-1, 0]])
    s.set_point_sources([survey.point_electrode((0.0, 0.0), 1.0, surface=False)])
    _, st = s.solve(pts, nWalks=W16, maxSteps=1000, eps=EPS, seed=SEED, return_stats=True)
    _check("half disk", st, [exact(0.5, a)] * 2, [exact(0.5)] * 2)
    assert abs(exact(0.5) - 0.22064) < 1e-5
    s = _solver(D, np.stack([np.linspace(1, -1, 9), np.zeros(9)], axis=1))
    s.set_point_sources([survey.point_electrode((0.0, 0.0), 1.0, surface=False)])
    _, st = s.solve(np.array([[0.25, 0.0]], np.float32), nWalks=W16, maxSteps=1000, eps=EPS, seed=SEED, return_stats=True)
    _check("half disk, 8 segments", st, exact(0.25, a), exact(0.25))


# ---- 4. re-entrant wedge ----------------------------------------------------------------------
def test_wedge_formula_on_the_cpu():
    """The closed form used below, checked before it is used (no device needed): zero on the
    arc, symmetric in x and z, and the logarithmic pole's strength 1 / 2 pi."""
    z = _polar(0.6, 18)
    for deg in (1, 77, 135, 200, 269):
        assert abs(g_wedge(_polar(1.0, deg), z)) < 1e-12
    for x in (_polar(0.6, 252), _polar(0.5, 108), _polar(0.2, 30)):
        assert abs(g_wedge(x, z) - g_wedge(z, x)) < 1e-12
        assert g_wedge(x, z) > 0
    near = (z[0] + 1e-6, z[1])
    assert abs(g_wedge(near, z) / (-math.log(1e-6) / TWO_PI) - 1.0) < 0.1


def test_reentrant_wedge(gpu_available):
    """The sector 0 < phi < 3 pi / 2 of the unit disk: Neumann (1, 0) -> (0, 0) -> (0, -1), a
    96-segment Dirichlet arc, a unit charge at 0.6 e^(i 18 deg). The query at 0.6 e^(i 252 deg)
    does not see the charge (the corner is in the way), the one at 0.5 e^(i 108 deg) does: the
    visibility test. The bracket scales rho by the arc's inradius. Measured: 0.01869 +- 0.00030 in
    [0.018476, 0.018498] (1.6% relative: the 2% sizing holds at 16 blocks) and 0.06458 +- 0.00060
    in [0.06498, 0.06504]."""
    z = _polar(0.6, 18)
    a0, a1 = 0.0, 1.5 * math.pi
    pts = np.array([_polar(0.6, 252), _polar(0.5, 108)], np.float32)
    s = _solver(_arc(96, a0, a1), [[1, 0], [0, 0], [0, -1]])
    s.set_point_sources([[(z, 1.0)]])
    _, st = s.solve(pts, nWalks=W16, maxSteps=1000, eps=EPS, seed=SEED, return_stats=True)
    a = _inradius(96, a0, a1)
    _check("wedge", st, [g_wedge(p, z, a) for p in pts], [g_wedge(p, z) for p in pts])


# ---- 5. channels are independent --------------------------------------------------------------
W5 = 4096 + 1000


@functools.lru_cache(maxsize=None)
def _scenario(name):
    from dcrmontecarlo_amd import scenarios as S

    if name == "dd":
        sc = S.dcr_dipole(n_electrodes=8)
        return dataclasses.replace(sc, f=None), sc.points[[2, 3, 4]]
    sc = S.variable_coefficients()
    return dataclasses.replace(sc, f=None), sc.points[[0, 7, 40]]


def _fixed_solver(name, sigma_bar, tree=None):
    from dcrmontecarlo_amd.wavenumber import sigma_bar_for

    sc, pts = _scenario(name)
    sb = sigma_bar_for(sc.solver(), 0.0) + sigma_bar
    s = sc.solver(compat="fixed", sigma_bar=sb)
    s.set_fixed_step_check(False)
    if tree is not None:
        s.set_segment_tree(0 if tree else -1)
    return sc, pts, s


def test_every_channel_equals_its_single_solve(gpu_available):
    """2 wavenumbers x 3 point dipoles on dcr_dipole's electrodes: every channel's per-walk
    values, sums and steps are bit for bit those of its own single-channel solve."""
    from dcrmontecarlo_amd import survey

    sc, pts, s = _fixed_solver("dd", 2.5)
    e = np.asarray(sc.points, np.float64)
    # (dipoles among the query points: 60 units away every screened solve is exactly 0)
    dip = [survey.point_dipole(e[2], e[3]), survey.point_dipole(e[3], e[4], 2.0), survey.point_dipole(e[4], e[2])]
    k = np.array([0.5, 1.5])
    kw = dict(nWalks=W5, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    vals, steps = s.solve_wavenumbers_walks(pts, k, sources=dip, **kw)
    u, st = s.solve_wavenumbers(pts, k, sources=dip, return_stats=True, **kw)
    assert vals.shape == (2, 3, 3, W5) and u.shape == (2, 3, 3) and s.last_timing["jit"] == 1
    assert s.point_sources is None and s.num_channels() == 1   # restored
    assert len({vals[j, i].tobytes() for j in range(2) for i in range(3)}) == 6 and np.any(vals != 0)
    for i, d in enumerate(dip):
        s.set_point_sources([d])
        for j in range(2):
            s.set_wavenumbers([k[j]])
            v1, s1 = s.solve_walks(pts, **kw)
            _, st1 = s.solve(pts, return_stats=True, **kw)
            np.testing.assert_array_equal(steps, s1)
            np.testing.assert_array_equal(vals[j, i].view(np.uint32), v1.view(np.uint32))
            np.testing.assert_array_equal(st.mean[j, i], st1.mean)
            np.testing.assert_array_equal(st.stderr[j, i], st1.stderr)
        s.set_wavenumbers(None)
    s.set_point_sources(None)


def test_point_sources_over_two_launches_equal_their_single_solves(gpu_available):
    """17 point dipoles between neighbouring electrodes, each with a charge on a query point:
    34 charges (> WOST_MAX_POINT_CHARGES) in 17 sources (> WOST_MAX_SOURCES), so
    solve_point_sources scores 16 + 1 sources in two launches. Every source's per-walk values,
    steps, mean and standard error are bit for bit those of its own single solve."""
    from dcrmontecarlo_amd import survey

    sc, pts, s = _fixed_solver("dd", 2.5)
    e = np.asarray(sc.points, np.float64)
    dip = [survey.point_dipole(e[2 + i % 2], e[3 + i % 2], 1.0 + 0.25 * i) for i in range(17)]
    kw = dict(nWalks=W5, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    vals, steps = s.solve_point_sources_walks(pts, dip, **kw)
    u, st = s.solve_point_sources(pts, dip, return_stats=True, **kw)
    assert vals.shape == (17, 3, W5) and steps.shape == (3, W5) and s.last_timing["jit"] == 1
    assert u.shape == (17, 3) and st.mean.shape == (17, 3) and st.stderr.shape == (17, 3)
    assert s.point_sources is None and s.num_channels() == 1   # restored
    assert np.any(vals[:16] != 0) and np.any(vals[16] != 0)    # both launches scored something
    for i, d in enumerate(dip):
        s.set_point_sources([d])
        v1, s1 = s.solve_walks(pts, **kw)
        _, st1 = s.solve(pts, return_stats=True, **kw)
        np.testing.assert_array_equal(steps, s1)
        np.testing.assert_array_equal(vals[i].view(np.uint32), v1.view(np.uint32))
        np.testing.assert_array_equal(st.mean[i], st1.mean)
        np.testing.assert_array_equal(st.stderr[i], st1.stderr)
        np.testing.assert_array_equal(u[i], st1.mean.astype(np.float32))
    s.set_point_sources(None)


def test_tree_kernel_equals_scan_kernel_with_point_sources(gpu_available):
    """variable_coefficients (a Neumann circle) at 3 wavenumbers, two sources of point charges
    near the circle: the segment-tree kernel's values, sums and steps equal the scan kernel's."""
    res = []
    for tree in (True, False):
        sc, pts, s = _fixed_solver("vc", 2.0, tree=tree)
        src = [[((0.7, 0.1), 1.0), ((-0.45, 0.3), -0.5)], [((0.0, -0.62), 2.0)]]
        vals, steps = s.solve_wavenumbers_walks(pts, np.sqrt([0.0, 0.4, 1.9]), nWalks=W5, maxSteps=sc.max_steps,
                                                eps=sc.eps, sources=src, seed=SEED)
        assert s.last_timing["tree"] == (1 if tree else 0) and s.last_timing["jit"] == 1
        res.append((vals, steps))
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[0][0].view(np.uint32), res[1][0].view(np.uint32))
    assert len({res[0][0][j, i].tobytes() for j in range(3) for i in range(2)}) == 6 and np.any(res[0][0] != 0)


def test_walk_range_shards_merge_and_the_gaussian_source_comes_back(gpu_available):
    """Two walk-range shards of a two-source point solve merge to the full solve; and clearing
    the charges and setting the Gaussian source back gives the bits the handle gave before."""
    from dcrmontecarlo_amd import _lib
    from dcrmontecarlo_amd import survey

    sc, pts, s = _fixed_solver("vc", 0.0)
    kw = dict(maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    gauss = survey.electrode_source((0.7, 0.1), 0.15)
    s.setSourceTerm(gauss)
    before = s.solve_walks(pts, nWalks=W5, **kw)
    s.setSourceTerm(None)
    s.set_point_sources([[((0.7, 0.1), 1.0)], [((0.0, -0.62), 2.0), ((-0.45, 0.3), -0.5)]])
    assert s.num_channels() == 2
    with pytest.raises(ValueError, match="point sources"):
        s.setSourceTerm(gauss)                      # no source field beside the charges
    p = np.ascontiguousarray(pts, np.float32)
    rows = np.zeros((3, 5))
    rc = _lib.lib.wost_solve_multi(s._h, _lib.fptr(p), 3, W5, 0, s.num_blocks(3, W5), sc.max_steps, sc.eps, SEED, None,
                                   _lib.dptr(rows), None, None)
    assert rc == 0
    a = s.solve_range(pts, W5, 0, 4096, **kw)
    b = s.solve_range(pts, W5, 4096, W5, **kw)
    assert a.shape == (3, 1, 5) and b.shape == (3, 1, 5)
    np.testing.assert_array_equal((np.zeros((3, 5)) + a[:, 0]) + b[:, 0], rows)
    assert np.all(rows[:, 1] > 0)
    s.set_point_sources(None)
    assert s.num_channels() == 1
    s.setSourceTerm(gauss)
    after = s.solve_walks(pts, nWalks=W5, **kw)
    np.testing.assert_array_equal(before[1], after[1])
    np.testing.assert_array_equal(before[0].view(np.uint32), after[0].view(np.uint32))


# ---- 6. half plane, point electrode -----------------------------------------------------------
HALF_PLANE_BLOCKS = 640


def test_half_plane_point_electrode(gpu_available):
    """tests/test_gpu_wavenumber.py::test_half_plane_k0's box, points and wavenumbers with
    survey.point_electrode((0, 0), Q, surface=True) in place of the Gaussian: u_k(r) =
    Q / (2 pi a0) K0(k r), no width factor. Each estimate within 4 of its own standard errors,
    each standard error <= 2% of the expected value. At that test's 640 blocks: measured
    relative standard errors 0.08%, 0.15%, 0.24% (k = 1) and 0.04%, 0.13%, 0.37% (k = 2), the
    means +0.14%, +0.05%, +0.05% and +0.05%, +0.06%, -0.08% from the closed form (at most 1.8
    standard errors): the same-signed bias DESIGN.md section 9 item 0 records for the Gaussian
    electrode is not seen here. 37 ms of kernel time."""
    from scipy.special import k0

    from dcrmontecarlo_amd import survey

    a0, Q = 2.0, 1.0
    D = np.array([[-10, 0], [-10, -10], [10, -10], [10, 0]], np.float32)
    s = _solver(D, [[10, 0], [-10, 0]], alpha=a0, sigma_bar=5.0)
    pts = np.array([[1, 0], [2, 0], [3, 0]], np.float32)
    k = np.array([1.0, 2.0])
    u, st = s.solve_wavenumbers(pts, k, nWalks=HALF_PLANE_BLOCKS * 4096, maxSteps=2000, eps=1e-3, seed=31,
                                sources=[survey.point_electrode((0.0, 0.0), Q, surface=True)], return_stats=True)
    want = Q / (2 * math.pi * a0) * k0(np.outer(k, np.array([1.0, 2.0, 3.0])))
    mean, se = st.mean[:, 0], st.stderr[:, 0]
    print("expected", want, "\nmean", mean, "\nstderr / expected", se / want, "\nz", (mean - want) / se,
          "\nkernel ms", st.kernel_ms, "mean steps", st.mean_steps)
    assert np.all(se <= 0.02 * want)
    assert np.all(np.abs(mean - want) <= 4.0 * se)


# ---- 7. 2.5-D Wenner with point electrodes ----------------------------------------------------
def test_wenner_25d_point_electrodes_on_the_homogeneous_box(gpu_available):
    """DESIGN.md 7a's end-to-end case (box [-10, 10] x [-10, 0], alpha = 2, six electrodes 0.1
    apart, n = 4 wavenumbers k = 0.5 .. 40) with electrodes="point" at 4 * 4096 walks: rho_a a0
    within 4 of its standard errors of 1 for each quadripole (measured: 0.999, 0.992, 0.992,
    each +- 0.017). The finite box's effect on the lowest wavenumber is printed: the walls'
    nearest image, K0(k_min 2 depth), is 2.6e-5 of the receivers' difference at k_min = 0.5, far
    below the standard error, so every channel is asserted."""
    from scipy.special import k0

    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import wavenumber as WN

    a0, dx, n_el = 2.0, 0.1, 6
    D = np.array([[-10, 0], [-10, -10], [10, -10], [10, 0]], np.float32)
    N = np.array([[10, 0], [-10, 0]], np.float32)
    x = (np.arange(n_el) - 0.5 * (n_el - 1)) * dx
    pts = np.stack([x, np.zeros_like(x)], axis=1).astype(np.float32)
    sc = S.Scenario("halfspace_box", D, N, g=F.const(0.0), f=F.const(0.0), alpha=F.const(a0), points=pts,
                    max_steps=100_000, eps=1e-4)
    r = WN.run_wenner_survey_25d(sc, 4 * 4096, a=1, seed=3, electrodes="point")
    ratio, se = r.rho_a * a0, r.rho_a_se * a0
    # the lowest wavenumber's box effect: the Dirichlet walls' nearest image, relative to the
    # receivers' potential difference at that wavenumber
    kmin = float(r.k.min())
    print("k", r.k, "w", r.w, "sigma_bar", r.sigma_bar, "\nrho_a / rho", ratio, "+-", se, "z", (ratio - 1.0) / se,
          "\nkernel ms", r.kernel_ms, "walk steps", r.walk_steps,
          f"\nlowest wavenumber k = {kmin}: K0(k 2 depth) / (K0(k a) - K0(2 k a)) =",
          float(k0(kmin * 20.0) / (k0(kmin * dx) - k0(2 * kmin * dx))))
    assert r.launches == 1
    assert np.all(np.abs(ratio - 1.0) <= 4.0 * se)


# ---- 8. errors on the device ------------------------------------------------------------------
def test_errors_and_a_query_point_on_a_charge(gpu_available):
    from dcrmontecarlo_amd import PolyLinesSimple, WostSolver_2D
    from dcrmontecarlo_amd import _lib
    from dcrmontecarlo_amd import survey

    D = _arc(32, math.pi, TWO_PI)
    N = [[1, 0], [-1, 0]]
    s = _solver(D, N)
    z = (0.25, 0.0)
    s.set_point_sources([survey.point_electrode(z, 1.0, surface=False)])
    pts = np.array([z, (0.25, -0.3)], np.float32)
    _, st = s.solve(pts, nWalks=4096, maxSteps=1000, eps=EPS, seed=SEED, return_stats=True)
    # a walk that starts on the charge scores it at r = eps / 2, with the surface's factor 2
    assert np.all(np.isfinite(st.mean)) and st.mean[0] > st.mean[1] > 0
    assert st.mean[0] < 10.0                        # (2 ln(R / (eps / 2)) / 2 pi = 3.1 at R = 0.75, and the later steps)
    s.set_jit(False)
    with pytest.raises(NotImplementedError, match="field-specialised"):
        s.solve(pts, nWalks=64, maxSteps=100, eps=EPS)
    s.set_jit(True)
    with pytest.raises(NotImplementedError, match="wost_solve_history"):
        s.solve(pts[:1], nWalks=8, maxSteps=50, eps=EPS, return_history=True)
    two = (_lib.WostPointCharge * 2)(_lib.WostPointCharge(0.1, -0.2, 1.0, 0), _lib.WostPointCharge(0.1, -0.3, 1.0, 0))
    with pytest.raises(ValueError, match="source 1 has no point charge"):
        _lib.check(_lib.lib.wost_set_point_sources(s._h, two, 2, 2))
    assert s.num_channels() == 1                    # a refused set changes nothing
    # reference mode; a handle with a source field; more charges than a launch takes
    ref = WostSolver_2D(PolyLinesSimple(D), 0.0, PolyLinesSimple(np.asarray(N, np.float32)))
    with pytest.raises(NotImplementedError, match="fixed"):
        ref.set_point_sources([[(z, 1.0)]])
    withf = _solver(D, N, source=survey.electrode_source(z, 0.1))
    with pytest.raises(ValueError, match="source field"):
        withf.set_point_sources([[(z, 1.0)]])
    arr = (_lib.WostPointCharge * 33)(*[_lib.WostPointCharge(0.01 * i, -0.2, 1.0, 0) for i in range(33)])
    assert _lib.lib.wost_set_point_sources(s._h, arr, 33, 1) == _lib.WOST_ERR_INVALID_ARG
    arr[3].strength = float("inf")
    assert _lib.lib.wost_set_point_sources(s._h, arr, 32, 1) == _lib.WOST_ERR_INVALID_ARG
    n, chk = _lib.ctypes.c_int32(0), _lib.ctypes.c_uint64(0)
    assert _lib.lib.wost_point_sources_info(s._h, _lib.ctypes.byref(n), _lib.ctypes.byref(chk)) == 0
    assert n.value == 1 and chk.value != 0
