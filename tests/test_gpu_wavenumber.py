"""2.5-D wavenumber batching on the device (wost_set_wavenumbers, WostSolver_2D.
solve_wavenumbers; DESIGN.md "2.5-D wavenumber batching").

Under delta tracking a walk's path depends only on sigma_bar; the wavenumber k enters
through the collision weight 1 - (sigma' + k^2) / sigma_bar alone. One walk therefore
scores K wavenumbers (and S sources): channel c = j * S + s. These tests pin that every
channel is bit for bit the single solve of (k_j, source_s), that k^2 = 0 is today's path,
that the segment-tree kernels, walk-range shards and the facade's chunking agree, the
error returns, and the estimator against the closed form K0(k r) on a half-plane.

Shapes: 3 points, W = 4096 + 1000 walks (one full and one partial reduction block).
"""
import ctypes
import dataclasses
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 4096 + 1000
SEED = 31
COMPATS = ["reference", "fixed"]


@functools.lru_cache(maxsize=None)
def _scenario(name):
    from dcrmontecarlo_amd import scenarios as S

    if name == "dd":   # a small dcr_dipole: variable, differentiable alpha, one Neumann segment
        from dcrmontecarlo_amd import survey

        sc = S.dcr_dipole(n_electrodes=8)
        # its own electrodes are 60 units from the scenario's source, where every screened
        # solve is exactly 0: a source at the middle one of three adjacent electrodes instead
        sc = dataclasses.replace(sc, f=survey.electrode_source(sc.points[3], 1.5))
        return sc, sc.points[[2, 3, 4]]
    sc = S.variable_coefficients()   # Neumann circle, variable sigma, variable detached alpha
    return sc, sc.points[[0, 7, 40]]


def _solver(name, compat, sc=None, **kw):
    """name: "vc", "dd", or "tree" (vc with its Neumann queries through the segment tree)."""
    base, pts = _scenario("dd" if name == "dd" else "vc")
    s = (sc or base).solver(compat=compat, **kw)
    if compat == "fixed":
        s.set_fixed_step_check(False)   # (dd: sigma_bar 10 on a +-100 box truncates every walk; fine here)
    if name == "tree":
        s.set_segment_tree(0)
    return base, pts, s


@functools.lru_cache(maxsize=None)
def _max_sigma_prime(name):
    """max sigma' on the reference's grid (wavenumber.sigma_bar_for with k = 0)."""
    from dcrmontecarlo_amd.wavenumber import sigma_bar_for

    return sigma_bar_for(_scenario(name)[0].solver(), 0.0)


def _set_k2(s, k2):
    """wost_set_wavenumbers with the exact k^2 values (the facade takes k)."""
    from dcrmontecarlo_amd import _lib

    a = np.ascontiguousarray(k2, np.float64)
    return _lib.lib.wost_set_wavenumbers(s._h, _lib.dptr(a) if a.size else None, int(a.size))


def _multi(s, pts, n_walks, max_steps, eps, seed=SEED, walks=True):
    """wost_solve_multi with the handle's channels: (point rows [N, 2C+1], values [N, W, C], steps)."""
    from dcrmontecarlo_amd import _lib

    p = np.ascontiguousarray(pts, np.float32)
    n, C = len(p), s.num_channels()
    rows = np.zeros((n, 2 * C + 1))
    wv = np.empty((n, n_walks, C), np.float32) if walks else None
    ws = np.empty((n, n_walks), np.uint32) if walks else None
    rc = _lib.lib.wost_solve_multi(s._h, _lib.fptr(p), n, n_walks, 0, s.num_blocks(n, n_walks), int(max_steps),
                                   float(eps), seed, None, _lib.dptr(rows), _lib.fptr(wv), _lib.u32ptr(ws))
    return rc, rows, wv, ws


def _sources(sc, pts, n):
    from dcrmontecarlo_amd import survey

    c = np.asarray(pts, np.float64)
    w = 0.1 * float(np.ptp(np.asarray(sc.dirichlet, np.float64)[:, 0]))
    return [survey.electrode_source(c[k % len(c)] * (1.0 - 0.1 * k), w, current=1.0 + k) for k in range(n)]


# ---- 1. k^2 = 0 is today's path ---------------------------------------------------------
@pytest.mark.parametrize("compat", COMPATS)
@pytest.mark.parametrize("name", ["vc", "dd", "tree"])
def test_zero_wavenumber_keeps_every_bit(gpu_available, name, compat):
    sc, pts, s = _solver(name, compat)
    kw = dict(nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    v0, s0 = s.solve_walks(pts, **kw)
    s.solve(pts, **kw)
    sums0 = s.last_point_sums.copy()
    assert s.last_timing["tree"] == (1 if name == "tree" else 0)
    s.set_wavenumbers([0.0])
    assert s.num_channels() == 1
    v1, s1 = s.solve_walks(pts, **kw)
    s.solve(pts, **kw)
    np.testing.assert_array_equal(s0, s1)
    np.testing.assert_array_equal(v0.view(np.uint32), v1.view(np.uint32))
    np.testing.assert_array_equal(sums0, s.last_point_sums)
    s.set_wavenumbers(None)
    v2, s2 = s.solve_walks(pts, **kw)
    np.testing.assert_array_equal(v0.view(np.uint32), v2.view(np.uint32))


# ---- 2. bitwise anchor to today's path --------------------------------------------------
def _square_solver(sigma, compat):
    from dcrmontecarlo_amd import WostSolver_2D, PolyLinesSimple
    from dcrmontecarlo_amd import fields as F

    D = PolyLinesSimple(np.array([[-1, -1], [1, -1], [1, 1], [-1, 1], [-1, -1]], np.float32))
    f = 1.0 + 0.5 * F.X * F.Y + F.gaussian((0.2, -0.1), 0.3)
    return WostSolver_2D(D, F.X, None, source=f, sigma=sigma, compat=compat, sigma_bar=4.0)


@pytest.mark.parametrize("compat", COMPATS)
def test_channels_equal_todays_solves_of_shifted_sigma(gpu_available, compat):
    """sigma = 0.5, alpha = 1 (detached), k^2 = 0, 0.25, 1.5: sigma' + k^2 = 0.5, 0.75, 2.0
    and every product with 1 / sigma_bar = 0.25 are exact in float32, so channel j is bit for
    bit today's solve_walks with sigma = 0.5 + k^2 -- one launch with the specialised
    kernel, and one k^2 at a time with the precompiled (NK = 1) kernel."""
    pts = np.array([[0.3, 0.2], [-0.7, 0.5], [0.0, -0.9]], np.float32)
    k2 = [0.0, 0.25, 1.5]
    kw = dict(nWalks=W, maxSteps=400, eps=1e-3, seed=SEED)
    want = [_square_solver(0.5 + q, compat).solve_walks(pts, **kw) for q in k2]
    s = _square_solver(0.5, compat)
    assert _set_k2(s, k2) == 0 and s.num_channels() == 3
    rc, _, vals, steps = _multi(s, pts, W, 400, 1e-3)
    assert rc == 0 and s.timing()["jit"] == 1
    off = _square_solver(0.5, compat)
    off.set_jit(False)
    for j, (v, st) in enumerate(want):
        np.testing.assert_array_equal(steps, st)
        np.testing.assert_array_equal(vals[:, :, j].view(np.uint32), v.view(np.uint32))
        assert _set_k2(off, [k2[j]]) == 0
        v1, s1 = off.solve_walks(pts, **kw)
        assert off.last_timing["jit"] == 0
        np.testing.assert_array_equal(s1, st)
        np.testing.assert_array_equal(v1.view(np.uint32), v.view(np.uint32))
    assert len({w[0].tobytes() for w in want}) == 3   # (the three solves do differ)


# ---- 3. variable alpha ------------------------------------------------------------------
@pytest.mark.parametrize("compat", COMPATS)
@pytest.mark.parametrize("name", ["vc", "dd"])
def test_variable_alpha_matches_sigma_plus_k2_alpha(gpu_available, name, compat):
    """k^2 = 0.3, 2.0 against two single solves with sigma + k^2 alpha as the sigma field and
    the same sigma_bar: identical steps (paths do not depend on sigma'), and each point mean
    within 0.01 of the single solve's standard error -- the sides differ by the fp32 rounding
    of sigma' (~1e-6 relative per walk) while a wrong or swapped k^2 moves the mean by many
    standard errors."""
    k2 = [0.3, 2.0]
    sb = _max_sigma_prime("dd" if name == "dd" else "vc") + max(k2)
    sc, pts, s = _solver(name, compat, sigma_bar=sb)
    kw = dict(nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    assert _set_k2(s, k2) == 0
    rc, rows, vals, steps = _multi(s, pts, W, sc.max_steps, sc.eps)
    assert rc == 0
    means = []
    for j, q in enumerate(k2):
        sig = q * sc.alpha if sc.sigma is None else sc.sigma + q * sc.alpha
        _, _, one = _solver(name, compat, sc=dataclasses.replace(sc, sigma=sig), sigma_bar=sb)
        v, st = one.solve_walks(pts, **kw)
        np.testing.assert_array_equal(steps, st)
        m1 = v.astype(np.float64).mean(axis=1)
        se1 = v.astype(np.float64).std(axis=1, ddof=1) / math.sqrt(W)
        mj = vals[:, :, j].astype(np.float64).mean(axis=1)
        print(name, compat, "k2", q, "mean", mj, "single", m1, "stderr", se1, "diff/se", (mj - m1) / se1)
        assert np.all(se1 > 0)
        assert np.all(np.abs(mj - m1) <= 0.01 * se1)
        means.append(mj)
    assert np.all(np.abs(means[0] - means[1]) > 0)


# ---- 4. channel independence, chunking --------------------------------------------------
@pytest.mark.parametrize("compat", COMPATS)
def test_every_channel_equals_its_single_solve(gpu_available, compat):
    k = np.sqrt(np.array([0.0, 0.2, 0.7, 1.3, 2.4]))
    sb = _max_sigma_prime("vc") + 2.5
    sc, pts, s = _solver("vc", compat, sigma_bar=sb)
    srcs = _sources(sc, pts, 3)
    kw = dict(nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    out = {}
    for nk in (2, 5):   # 6 and 15 channels
        vals, steps = s.solve_wavenumbers_walks(pts, k[:nk], sources=srcs, **kw)
        u, st = s.solve_wavenumbers(pts, k[:nk], sources=srcs, return_stats=True, **kw)
        assert vals.shape == (nk, 3, 3, W) and u.shape == (nk, 3, 3) and steps.shape == (3, W)
        out[nk] = (vals, steps, st)
    assert s.wavenumbers is None and s.num_channels() == 1   # restored
    for si, f in enumerate(srcs):
        s.setSourceTerm(f)
        for j in range(5):
            s.set_wavenumbers([k[j]])
            v1, s1 = s.solve_walks(pts, **kw)
            _, st1 = s.solve(pts, return_stats=True, **kw)
            for nk in (2, 5):
                if j >= nk:
                    continue
                vals, steps, st = out[nk]
                np.testing.assert_array_equal(steps, s1)
                np.testing.assert_array_equal(vals[j, si].view(np.uint32), v1.view(np.uint32))
                np.testing.assert_array_equal(st.mean[j, si], st1.mean)
                np.testing.assert_array_equal(st.stderr[j, si], st1.stderr)


def test_seventeen_channels_are_chunked_by_the_facade_and_refused_by_the_library(gpu_available):
    from dcrmontecarlo_amd import _lib

    k = np.sqrt(np.linspace(0.0, 2.4, 17))
    sc, pts, s = _solver("vc", "reference", sigma_bar=_max_sigma_prime("vc") + 2.5)
    kw = dict(nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    vals, steps = s.solve_wavenumbers_walks(pts, k, **kw)
    assert vals.shape == (17, 3, W)
    for j in (0, 15, 16):   # the first launch's ends and the second launch's only channel
        s.set_wavenumbers([k[j]])
        v1, s1 = s.solve_walks(pts, **kw)
        np.testing.assert_array_equal(steps, s1)
        np.testing.assert_array_equal(vals[j].view(np.uint32), v1.view(np.uint32))
    s.set_wavenumbers(None)
    assert _set_k2(s, np.linspace(0.0, 1.0, 17)) == _lib.WOST_ERR_INVALID_ARG
    assert b"channels" in _lib.lib.wost_last_error()
    # the same product from the other side: 9 wavenumbers, then 2 sources
    assert _set_k2(s, np.linspace(0.0, 1.0, 9)) == 0
    with pytest.raises(ValueError, match="channels"):
        with s.sources_installed(s.source_fields(_sources(sc, pts, 2))):
            pass
    assert s.num_channels() == 9


# ---- 5. tree kernel == scan kernel ------------------------------------------------------
@pytest.mark.parametrize("compat", COMPATS)
def test_tree_kernel_equals_scan_kernel_at_three_wavenumbers(gpu_available, compat):
    k2 = [0.0, 0.4, 1.9]
    sb = _max_sigma_prime("vc") + 2.0
    res = []
    for name in ("tree", "vc"):
        sc, pts, s = _solver(name, compat, sigma_bar=sb)
        if name == "vc":
            s.set_segment_tree(-1)
        assert _set_k2(s, k2) == 0
        rc, rows, vals, steps = _multi(s, pts, W, sc.max_steps, sc.eps)
        assert rc == 0 and s.timing()["tree"] == (1 if name == "tree" else 0) and s.timing()["jit"] == 1
        res.append((rows, vals, steps))
    np.testing.assert_array_equal(res[0][2], res[1][2])
    np.testing.assert_array_equal(res[0][1].view(np.uint32), res[1][1].view(np.uint32))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    assert len({res[0][1][:, :, j].tobytes() for j in range(3)}) == 3


# ---- 6. walk-range shards ---------------------------------------------------------------
def test_walk_range_shards_merge_to_the_full_solve(gpu_available):
    sc, pts, s = _solver("vc", "reference", sigma_bar=_max_sigma_prime("vc") + 1.0)
    with s.sources_installed(s.source_fields(_sources(sc, pts, 2))):
        assert _set_k2(s, [0.1, 0.9]) == 0 and s.num_channels() == 4
        rc, rows, _, _ = _multi(s, pts, W, sc.max_steps, sc.eps, walks=False)
        assert rc == 0 and rows.shape == (3, 9)
        a = s.solve_range(pts, W, 0, 4096, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
        b = s.solve_range(pts, W, 4096, W, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
        assert a.shape == (3, 1, 9) and b.shape == (3, 1, 9)
        merged = (np.zeros((3, 9)) + a[:, 0]) + b[:, 0]   # block order, added to 0.0 one block at a time
        np.testing.assert_array_equal(merged, rows)
        _set_k2(s, [])


# ---- 7. errors --------------------------------------------------------------------------
def test_error_returns(gpu_available):
    from dcrmontecarlo_amd import _lib
    from dcrmontecarlo_amd import scenarios as S

    plain = S.poisson_square().solver()   # neither sigma nor alpha: no delta tracking
    assert _set_k2(plain, [1.0]) == _lib.WOST_ERR_UNSUPPORTED
    assert b"constant alpha" in _lib.lib.wost_last_error()
    assert _set_k2(plain, []) == 0                      # clearing is always fine
    with pytest.raises(NotImplementedError):
        plain.set_wavenumbers([1.0])
    sc, pts, s = _solver("vc", "reference")
    for bad in ([-0.5], [0.1, float("nan")], [float("inf")]):
        assert _set_k2(s, bad) == _lib.WOST_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        s.set_wavenumbers([0.3, -1.0])
    assert s.num_channels() == 1 and s.wavenumbers is None   # a refused set changes nothing
    s.set_wavenumbers([0.2, 0.8])
    with pytest.raises(ValueError, match="wost_solve_multi"):          # solve() needs one channel
        s.solve(pts, nWalks=64, maxSteps=sc.max_steps, eps=sc.eps)
    with pytest.raises(ValueError):                                    # and so does the recorder
        s.solve(pts, nWalks=64, maxSteps=50, eps=sc.eps, return_history=True)
    s.set_jit(False)                                                   # NK > 1 needs the specialised kernel
    rc, _, _, _ = _multi(s, pts, 64, sc.max_steps, sc.eps)
    assert rc == _lib.WOST_ERR_UNSUPPORTED
    s.set_jit(True)
    s.set_wavenumbers([0.6])                                           # a single non-zero k^2: history works
    u, hist = s.solve(pts[:1], nWalks=8, maxSteps=50, eps=sc.eps, return_history=True)
    assert len(hist[0]) == 8


# ---- 8. the closed form on a half-plane -------------------------------------------------
def test_half_plane_k0(gpu_available):
    """Box [-10, 10] x [-10, 0], Neumann on y = 0, Dirichlet 0 elsewhere, constant alpha = a0,
    a Gaussian electrode (standard deviation s = 0.25, whole-plane integral Q) at the origin,
    compat="fixed". By even reflection about the flat top u_k(r) = Q / (2 pi a0) K0(k r)
    exp(k^2 s^2 / 2) (the Gaussian's mean value under the modified Helmholtz operator; the
    box's image terms are below e^-14). Each estimate must lie within 4 of its own standard
    errors, and each standard error must be <= 2% of the expected value.

    W: the CPU oracle's single solves with sigma = k^2 a0 (sigma_bar 5, 40,000 walks; the
    reference estimator, the only one the oracle has) give per-walk standard deviations of
    0.72, 1.99, 3.9 (k = 1) and 2.1, 16.4, 86.2 (k = 2) times the expected value at
    r = 1, 2, 3: 2% at the worst, k = 2 at r = 3 (K0(6) = 1.2e-3), would take 1.86e7 walks
    (5120 blocks) of that estimator. compat="fixed" has a far smaller variance: measured once
    at 5120 blocks its relative standard errors were 0.044%, 0.076%, 0.12% (k = 1) and
    0.069%, 0.21%, 0.57% (k = 2), and its means lay 0.12%, 0.31%, 0.22% and 0.08%, 0.10%,
    0.58% BELOW the expected values (k = 1 at r = 2: 4.1 standard errors; the others
    0.5-2.7). Every channel is bit for bit its single solve (the tests above), so this
    same-signed relative bias of a few 1e-3 belongs to the existing compat="fixed" screened
    estimator, not to the batching; it is recorded as open in DESIGN.md section 9, and this
    test does not resolve it: W = 640 blocks = 2,621,440 walks is sized for the 2% condition
    alone (1.6% at k = 2, r = 3), where 4 standard errors are 0.5% or more."""
    from scipy.special import k0

    from dcrmontecarlo_amd import WostSolver_2D, PolyLinesSimple
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd import survey

    a0, sd, Q = 2.0, 0.25, 1.0
    D = PolyLinesSimple(np.array([[-10, 0], [-10, -10], [10, -10], [10, 0]], np.float32))
    N = PolyLinesSimple(np.array([[10, 0], [-10, 0]], np.float32))
    s = WostSolver_2D(D, 0.0, N, source=survey.electrode_source((0.0, 0.0), sd, Q), alpha=a0, compat="fixed",
                      sigma_bar=5.0)
    pts = np.array([[1, 0], [2, 0], [3, 0]], np.float32)
    k = np.array([1.0, 2.0])
    n_walks = 640 * 4096
    u, st = s.solve_wavenumbers(pts, k, nWalks=n_walks, maxSteps=2000, eps=1e-3, seed=SEED, return_stats=True)
    r = np.array([1.0, 2.0, 3.0])
    want = Q / (2 * math.pi * a0) * k0(np.outer(k, r)) * np.exp(k * k * sd * sd / 2)[:, None]
    print("expected", want, "\nmean", st.mean, "\nstderr / expected", st.stderr / want, "\nz", (st.mean - want) / st.stderr,
          "\nkernel ms", st.kernel_ms, "mean steps", st.mean_steps)
    assert np.all(st.stderr <= 0.02 * want)
    assert np.all(np.abs(st.mean - want) <= 4.0 * st.stderr)


# ---- solve_sources with wavenumbers set -------------------------------------------------
def test_solve_sources_refuses_a_solver_with_wavenumbers(gpu_available):
    """solve_sources sizes its rows for one value per source; with wavenumbers set the library
    would write 2C+1 doubles per row, so the facade refuses before the solve."""
    sc, pts, s = _solver("vc", "reference", sigma_bar=_max_sigma_prime("vc") + 1.0)
    srcs = _sources(sc, pts, 3)
    kw = dict(nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    want = s.solve_sources(pts, srcs, **kw)
    s.set_wavenumbers([0.4, 0.9])
    for call in (s.solve_sources, s.solve_sources_walks):
        with pytest.raises(ValueError, match="solve_wavenumbers"):
            call(pts, srcs, **kw)
        assert s.num_channels() == 2   # the wavenumbers stay, the single source is back
    u = s.solve_wavenumbers(pts, [0.0], sources=srcs, **kw)
    np.testing.assert_array_equal(u[0], want)
    np.testing.assert_array_equal(s.wavenumbers, [0.4, 0.9])   # restored
    s.set_wavenumbers([0.0])   # one wavenumber: one value per source, allowed
    np.testing.assert_array_equal(s.solve_sources(pts, srcs, **kw), want)
    s.set_wavenumbers(None)
    np.testing.assert_array_equal(s.solve_sources(pts, srcs, **kw), want)


# ---- the 2.5-D survey layer -------------------------------------------------------------
def test_dipole_dipole_survey_25d_on_the_homogeneous_box(gpu_available):
    """run_dipole_dipole_survey_25d over the homogeneous box of the closed-form test: the
    quadripole bookkeeping, dV = V_N - V_M positive, and a standard error that is the one of
    the per-walk weighted sums sum_j w_j v_j, not the root-sum-square of the channels' own
    errors (the channels share walks). rho_a is printed, not asserted: the finite box biases
    the lowest wavenumbers by an amount not derived."""
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey
    from dcrmontecarlo_amd import wavenumber as WN

    a0, dx, n_walks, width, seed = 2.0, 0.5, 4 * 4096, 0.05, 9
    D = np.array([[-10, 0], [-10, -10], [10, -10], [10, 0]], np.float32)
    N = np.array([[10, 0], [-10, 0]], np.float32)
    x = (np.arange(5) - 2.0) * dx
    pts = np.stack([x, np.zeros_like(x)], axis=1).astype(np.float32)
    sc = S.Scenario("box", D, N, g=F.const(0.0), f=F.const(0.0), alpha=F.const(a0), points=pts, max_steps=6000,
                    eps=1e-4)
    k, w = WN.wavenumber_quadrature(dx, 4 * dx, 6)
    s = sc.solver(compat="fixed", sigma_bar=float(k.max()) ** 2)
    r = WN.run_dipole_dipole_survey_25d(sc, n_walks, n_max=2, width=width, seed=seed, solvers=[s])
    np.testing.assert_array_equal(r.quadripoles, [[0, 1, 2, 3], [0, 1, 3, 4], [1, 2, 3, 4]])
    np.testing.assert_array_equal(r.k, k)
    np.testing.assert_array_equal(r.w, w)
    assert r.dv.shape == r.dv_se.shape == r.rho_a.shape == r.rho_a_se.shape == (3,)
    assert r.launches == 1 and len(r.groups) == 1 and r.sigma_bar == [s.sigma_bar]
    print("rho_a / rho", r.rho_a * a0, "+-", r.rho_a_se * a0, "dv / se", r.dv / r.dv_se)
    assert np.all(r.dv > 0) and np.all(r.rho_a > 0)
    geo = np.array([WN.dipole_dipole_geometric_factor(dx, n) for n in (1, 2, 1)])
    np.testing.assert_allclose(r.rho_a, geo * r.dv, rtol=1e-13)
    np.testing.assert_allclose(r.rho_a_se, geo * r.dv_se, rtol=1e-13)
    # the same walks again: transmitters (0, 1) and (1, 2), every channel's per-walk values
    srcs = [survey.dipole_source(pts[0], pts[1], width), survey.dipole_source(pts[1], pts[2], width)]
    vals, _ = s.solve_wavenumbers_walks(pts, k, nWalks=n_walks, maxSteps=sc.max_steps, eps=sc.eps, sources=srcs,
                                        seed=survey.group_seed(seed, 0))
    v = np.tensordot(w, vals.astype(np.float64), axes=(0, 0))           # [S, N, W]
    mean, se = v.mean(axis=2), v.std(axis=2, ddof=1) / math.sqrt(n_walks)
    t, m, n = np.array([0, 0, 1]), r.quadripoles[:, 2], r.quadripoles[:, 3]
    np.testing.assert_allclose(r.dv, mean[t, n] - mean[t, m], rtol=1e-12)
    np.testing.assert_allclose(r.dv_se, np.sqrt(se[t, n] ** 2 + se[t, m] ** 2), rtol=1e-12)
    se_ch = vals.astype(np.float64).std(axis=3, ddof=1) / math.sqrt(n_walks)   # [K, S, N]
    rss = np.sqrt(np.tensordot(w ** 2, se_ch ** 2, axes=(0, 0)))
    rss_dv = np.sqrt(rss[t, n] ** 2 + rss[t, m] ** 2)
    print("stderr", r.dv_se, "root-sum-square of the channels'", rss_dv)
    assert np.all(np.abs(rss_dv - r.dv_se) > 0.05 * r.dv_se)
