"""2.5-D DC resistivity: point electrodes over 2-D geology.

The 2-D solves of :mod:`dcrmontecarlo_amd.survey` give the potential of infinite line
electrodes. Real electrodes are points; for geology that does not vary along strike (y) the
standard treatment Fourier-transforms the 3-D equation along strike,

    u_k(x, z) = int_0^inf u(x, y, z) cos(k y) dy,

which leaves one screened 2-D problem per wavenumber k,

    div(alpha grad u_k) - k^2 alpha u_k = -f          (alpha = conductivity),

and the potential in the electrodes' plane is the inverse transform at y = 0,

    u(x, 0, z) = (2/pi) int_0^inf u_k dk  ~=  sum_j w_j u_{k_j}.

The half-line transform of a point current I delta(x) delta(y) delta(z) is (I/2) delta(x)
delta(z). An ``electrode_source`` of current I -- a Gaussian whose integral over the WHOLE
plane is I, centred on the Neumann surface so that I/2 lies inside the domain -- is
therefore the right 2-D source f: over a homogeneous half-space u_k = I / (2 pi alpha)
K0(k r), and with ``r sum_j w_j K0(k_j r) = 1`` (``wavenumber_quadrature``) the sum is the
point electrode's I / (2 pi alpha r).

Every wavenumber is scored by the same walks (WostSolver_2D.solve_wavenumbers: under delta
tracking a walk's path depends only on sigma_bar), so a 2.5-D survey costs one walk set per
electrode, not one per electrode and wavenumber.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .scenarios import Scenario, torch_linspace
from .survey import (dipole_dipole_quadripoles, dipole_source, group_seed, point_dipole, wenner_quadripoles)


# ---------------------------------------------------------------------------
# Bessel K0 without scipy (Abramowitz & Stegun 9.8.5-9.8.6, |error| < 2e-7): the
# quadrature's least squares needs no more, and the package must not depend on scipy.
def bessel_k0(x) -> np.ndarray:
    x = np.asarray(x, np.float64)
    out = np.empty_like(x)
    small = x <= 2.0
    xs = x[small]
    t = (xs / 3.75) ** 2
    i0 = 1.0 + t * (3.5156229 + t * (3.0899424 + t * (1.2067492 + t * (0.2659732 + t * (0.0360768 + t * 0.0045813)))))
    y = (xs / 2.0) ** 2
    out[small] = -np.log(xs / 2.0) * i0 + (-0.57721566 + y * (0.42278420 + y * (0.23069756 + y * (
        0.03488590 + y * (0.00262698 + y * (0.00010750 + y * 0.00000740))))))
    xl = x[~small]
    z = 2.0 / xl
    out[~small] = np.exp(-xl) / np.sqrt(xl) * (1.25331414 + z * (-0.07832358 + z * (0.02189568 + z * (
        -0.01062446 + z * (0.00587872 + z * (-0.00251540 + z * 0.00053208))))))
    return out


def wavenumber_quadrature(r_min: float, r_max: float, n: int = 8):
    """Wavenumbers and weights (k, w) of the inverse transform for electrode distances in
    [r_min, r_max]: k log-spaced from 0.1 / r_max to 4 / r_min, w from linear least squares
    so that ``r * sum_j w_j K0(k_j r) = 1`` on log-spaced r in [r_min, r_max] -- the
    inverse cosine transform of the half-space solution, the 2/pi folded into w.
    n = 8 at r_max / r_min = 100 is exact to 1.1e-3 (n = 6: 1.3e-2, n = 10: 1.1e-4);
    some weights are slightly negative. More wavenumbers than the range supports make the
    least squares ill-conditioned -- n = 8 at r_max / r_min = 2 fits to 4e-6 with weights of
    alternating sign up to 570 that multiply the Monte-Carlo noise, where n = 4 fits to
    1.6e-4 with positive weights (r_max / r_min = 10: n = 6, 9e-4): the surveys choose n
    from the ratio."""
    if not (r_min > 0 and r_max >= r_min) or n < 1:
        raise ValueError("need 0 < r_min <= r_max and n >= 1")
    k = np.geomspace(0.1 / r_max, 4.0 / r_min, int(n)) if n > 1 else np.array([1.0 / math.sqrt(r_min * r_max)])
    r = np.geomspace(r_min, r_max, max(64, 16 * int(n)))
    A = r[:, None] * bessel_k0(k[None, :] * r[:, None])
    w, *_ = np.linalg.lstsq(A, np.ones_like(r), rcond=None)
    return k, w


def sigma_bar_for(solver, k_max: float) -> float:
    """The sigma_bar a 2.5-D solver needs for collision weights in [0, 1]: the largest
    sigma' of ``solver``'s problem on the reference's 50 x 50 grid over the domain's
    bounding box (buildModifiedSigma's grid, solvers/WoStSolver.py:130-136) plus k_max^2.
    ``solver``: a WostSolver_2D of the problem (any sigma_bar), or a Scenario (a solver is
    built for the evaluation). The library's own estimate is the RANGE of sigma' (max - min,
    quirk Q8), which the k^2 shift does not change -- hence this function."""
    if isinstance(solver, Scenario):
        solver = solver.solver()
    if not solver.use_delta_tracking:
        raise NotImplementedError("wavenumbers need delta tracking: give alpha (a constant is enough)")
    (x0, x1), (y0, y1) = solver.domain_bounds
    gx, gy = np.meshgrid(torch_linspace(x0, x1, 50), torch_linspace(y0, y1, 50), indexing="ij")
    sp = solver.eval_field("sigma_prime", np.stack([gx.ravel(), gy.ravel()], axis=1))[:, 0].astype(np.float64)
    sp = sp[np.isfinite(sp)]
    if not sp.size:
        raise ValueError("sigma' could not be evaluated at any grid point")
    return max(float(sp.max()), 0.0) + float(k_max) ** 2


def wenner_geometric_factor(a: float) -> float:
    """rho_a = K dV / I for Wenner-alpha point electrodes A M N B at spacing a on a flat
    half-space: K = 2 pi a (dV = V_M - V_N)."""
    return 2.0 * math.pi * float(a)


def dipole_dipole_geometric_factor(a: float, n: int) -> float:
    """rho_a = K dV / I for point-electrode dipoles A B | M N of length a, n a apart:
    K = pi n (n + 1) (n + 2) a, for the polarity that is positive over a half-space,
    dV = V_N - V_M with A the current source."""
    return math.pi * n * (n + 1) * (n + 2) * float(a)


def halfspace_potential(rho: float, current: float, r) -> np.ndarray:
    """Potential of a point electrode on a homogeneous half-space: rho I / (2 pi r)."""
    return rho * current / (2.0 * math.pi * np.asarray(r, np.float64))


# ---------------------------------------------------------------------------
@dataclass
class Transformed:
    """Inverse-transformed potentials sum_j w_j u_{k_j} of S sources at N points."""

    mean: np.ndarray      # [S, N]
    stderr: np.ndarray    # [S, N] from the per-walk weighted sums (channels share walks)
    walk_steps: int
    launches: int
    kernel_ms: float


def wavenumber_groups(k, groups: int = 1):
    """Index groups of the wavenumbers, low k first: ``groups`` contiguous runs of the
    sorted k of (almost) equal length. A group gets its own solver and sigma_bar: a high k
    forces a large sigma_bar, which shortens every channel's steps."""
    order = np.argsort(np.asarray(k, np.float64))
    return [g for g in np.array_split(order, max(1, min(int(groups), len(order)))) if len(g)]


def transform_weights(w, n_sources: int = 1) -> np.ndarray:
    """Weight rows of the inverse transform for ``WostSolver_2D.solve_combinations``: float64
    [S, K*S], row s holding the quadrature weight w[j] at channel j*S + s (wavenumber j major,
    source s minor: set_wavenumbers' channel order) and 0 elsewhere."""
    w = np.asarray(w, np.float64).ravel()
    S, K = int(n_sources), w.size
    if S < 1 or K < 1:
        raise ValueError("transform_weights needs at least one weight and one source")
    out = np.zeros((S, K * S), np.float64)
    for s in range(S):
        out[s, s::S] = w
    return out


def _are_point_sources(sources) -> bool:
    from .solvers.WoStSolver import is_point_source

    return all(is_point_source(s) or isinstance(s, (list, tuple)) for s in sources)


def _one_launch(solver, sources, n_k: int) -> bool:
    """Whether ``sources`` x n_k wavenumbers fit one launch of ``solver`` (point sources: also
    the charges, WOST_MAX_POINT_CHARGES)."""
    from . import _lib
    from .solvers.channels import charge_lists, point_source_chunks

    if len(sources) * n_k > _lib.WOST_MAX_SOURCES:
        return False
    return not _are_point_sources(sources) or len(point_source_chunks(
        charge_lists(sources), _lib.WOST_MAX_SOURCES // max(1, n_k), _lib.WOST_MAX_POINT_CHARGES)) == 1


def _transformed_group_device(solver, pts, sources, kk, ww, n_walks, max_steps, eps, seed):
    """One launch's sum_j w_j u_{k_j} of its sources, reduced on the device: a SolveStats with
    [S, N] mean and stderr. The solver's wavenumbers and source are restored."""
    from .solvers.channels import Launch

    fields = None if _are_point_sources(sources) else solver.source_fields(sources)
    with solver.channels_installed(fields, k=kk) as install:   # (point sources come with the launch)
        install(Launch((0, 1), (0, len(kk)), (0, len(sources)), None if fields is not None else tuple(sources)))
        _, st = solver.solve_combinations(pts, transform_weights(ww, len(sources)), n_walks, max_steps, eps, seed=seed,
                                          return_stats=True)
    return st


def transformed_potentials(solvers, groups, points, sources, k, w, n_walks: int, max_steps: int, eps: float,
                           seed: int = 0, device_reduce: bool = False) -> Transformed:
    """sum_j w_j u_{k_j} of every source (fields, or point sources: survey.point_electrode /
    point_dipole, one kind per call) at every point. ``groups``: index arrays into k,
    group g solved by ``solvers[g]`` (wavenumber_groups). Within a group all channels share
    their walks, so the standard error comes from the per-walk weighted sums
    v = sum_j w_j v_j, never from the channels' own errors (they are correlated); groups
    use different seeds and handles, so their errors add in quadrature. Holds one launch's
    per-walk values at a time ([16, N, n_walks] floats) and one chunk's weighted sums.

    device_reduce: form and reduce the per-walk weighted sums on the device
    (WostSolver_2D.solve_combinations) wherever a group's wavenumbers and a
    source chunk fit one launch (WOST_MAX_SOURCES channels): no per-walk value crosses the bus.
    A group of more wavenumbers than that keeps the host path (a combination across launches
    needs per-walk state). Mean and standard error then agree with the host path to float64
    rounding (another summation order), not bit for bit; the default False is the host path.
    The device's variance is the one-pass (sum v^2 - (sum v)^2 / n) / (n - 1) of its block
    sums, where numpy's is two-pass: its cancellation error grows like (Q + S^2/n) / (Q - S^2/n)
    times n 2^-53, so with |mean| >> the per-walk standard deviation the reported error loses
    digits the host path keeps (a single walk gives 0 on both paths)."""
    k = np.asarray(k, np.float64)
    w = np.asarray(w, np.float64)
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    S, N = len(sources), len(pts)
    mean = np.zeros((S, N))
    var = np.zeros((S, N))
    steps = launches = 0
    ms = 0.0
    from . import _lib

    for g, (solver, idx) in enumerate(zip(solvers, groups)):
        idx = np.asarray(idx, np.int64)
        # source chunks whose channels fit a launch with as many of the group's wavenumbers as possible
        s_chunk = max(1, min(S, _lib.WOST_MAX_SOURCES // min(len(idx), _lib.WOST_MAX_SOURCES)))
        for s0 in range(0, S, s_chunk):
            s1 = min(S, s0 + s_chunk)
            k_chunk = max(1, _lib.WOST_MAX_SOURCES // (s1 - s0))
            if device_reduce and _one_launch(solver, sources[s0:s1], len(idx)):
                st = _transformed_group_device(solver, pts, sources[s0:s1], k[idx], w[idx], n_walks, max_steps, eps,
                                               group_seed(seed, g))
                mean[s0:s1] += st.mean
                var[s0:s1] += st.stderr ** 2
                launches += 1
                ms += solver.last_timing["walk_kernel_ms"]
                steps += int(solver.last_point_sums[:, -1].sum())
                continue
            acc = np.zeros((s1 - s0, N, int(n_walks)))
            for j0 in range(0, len(idx), k_chunk):
                jj = idx[j0:j0 + k_chunk]
                # (the same seed: the chunks of one group share their walks)
                vals, st = solver.solve_wavenumbers_walks(pts, k[jj], nWalks=n_walks, maxSteps=max_steps, eps=eps,
                                                          sources=sources[s0:s1], seed=group_seed(seed, g))
                acc += np.tensordot(w[jj], vals.astype(np.float64), axes=(0, 0))
                launches += 1
                ms += solver.last_timing["walk_kernel_ms"]
                steps += int(st.sum(dtype=np.uint64))
            m = acc.mean(axis=2)
            mean[s0:s1] += m
            var[s0:s1] += acc.var(axis=2, ddof=1 if n_walks > 1 else 0) / n_walks
    return Transformed(mean, np.sqrt(var), steps, launches, ms)


@dataclass
class Survey25DResult:
    quadripoles: np.ndarray   # [Q, 4] electrode indices (Wenner: A M N B; dipole-dipole: A B M N)
    dv: np.ndarray            # [Q] potential difference per unit current
    dv_se: np.ndarray         # [Q]
    rho_a: np.ndarray         # [Q] geometric factor x dv
    rho_a_se: np.ndarray      # [Q]
    k: np.ndarray             # the wavenumbers and
    w: np.ndarray             # their quadrature weights
    groups: list              # index groups of k, one solver each
    sigma_bar: list           # the groups' sigma_bar
    walk_steps: int
    launches: int
    kernel_ms: float


def _solvers_25d(sc: Scenario, k, groups, compat, device, solvers, electrodes="gaussian"):
    idx = wavenumber_groups(k, groups) if isinstance(groups, int) else [np.asarray(g, np.int64) for g in groups]
    if solvers is None:
        kw = {} if device is None else {"device": device}
        if electrodes == "point":   # a point-source solver has no source field
            import dataclasses

            sc = dataclasses.replace(sc, f=None)
        probe = sc.solver(compat=compat, **kw)
        solvers = [sc.solver(compat=compat, sigma_bar=sigma_bar_for(probe, float(np.max(k[g]))), **kw) for g in idx]
    if len(solvers) != len(idx):
        raise ValueError(f"{len(idx)} wavenumber groups need as many solvers, got {len(solvers)}")
    return list(solvers), idx


def _run_25d(sc, quad, tx_cols, dv_of, factor, n_walks, width, n_k, groups, seed, device, compat, solvers,
             r_min, r_max, electrodes="gaussian", device_reduce=False):
    if electrodes not in ("gaussian", "point"):
        raise ValueError(f'electrodes must be "gaussian" or "point", got {electrodes!r}')
    E = len(sc.points)
    x = np.asarray(sc.points, np.float64)
    if not len(quad):
        raise ValueError(f"{E} electrodes give no quadripole")
    if n_k is None:   # as many wavenumbers as the range of distances supports (wavenumber_quadrature)
        n_k = 4 if r_max <= 3.0 * r_min else 6 if r_max <= 12.0 * r_min else 8
    k, w = wavenumber_quadrature(r_min, r_max, n_k)
    solvers, idx = _solvers_25d(sc, k, groups, compat, device, solvers, electrodes)
    tx = np.unique(quad[:, tx_cols], axis=0)
    if electrodes == "point":   # (I / 2) delta at each electrode: no width
        srcs = [point_dipole(x[a], x[b]) for a, b in tx]
    else:
        srcs = [dipole_source(x[a], x[b], width) for a, b in tx]
    tr = transformed_potentials(solvers, idx, sc.points, srcs, k, w, n_walks, sc.max_steps, sc.eps, seed,
                                device_reduce=device_reduce)
    row = {(int(a), int(b)): i for i, (a, b) in enumerate(tx)}
    t = np.array([row[(int(q[tx_cols[0]]), int(q[tx_cols[1]]))] for q in quad], np.int64)
    hi, lo = dv_of(quad)
    # the two receivers are different query points: independent walks
    dv = tr.mean[t, hi] - tr.mean[t, lo]
    se = np.sqrt(tr.stderr[t, hi] ** 2 + tr.stderr[t, lo] ** 2)
    K = factor(quad, x)
    return Survey25DResult(quad, dv, se, K * dv, np.abs(K) * se, k, w, [np.asarray(g) for g in idx],
                           [s.sigma_bar for s in solvers], tr.walk_steps, tr.launches, tr.kernel_ms)


def run_wenner_survey_25d(sc: Scenario, n_walks: int, a: int = 1, width: float = 0.5, n_k: int | None = None,
                          groups=1, seed: int = 0, device: int | None = None, compat: str = "fixed",
                          solvers=None, electrodes: str = "gaussian", device_reduce: bool = False) -> Survey25DResult:
    """2.5-D Wenner-alpha survey of ``sc`` (its points are the surface electrodes, equally
    spaced; its alpha the conductivity): apparent resistivity of point electrodes,
    rho_a = 2 pi a dV / I with dV = V_M - V_N for the transmitter A+ / B-. Sources x
    wavenumbers are scored by shared walks, summed with the quadrature weights of
    ``wavenumber_quadrature`` over the survey's electrode distances (a .. 2a), with ``n_k``
    wavenumbers (default: 4 for this range) in ``groups`` groups (an int, or index groups of
    k; one solver per group with sigma_bar = max sigma' + the group's largest k^2). No
    homogeneous background solve is needed: the geometric factor is the point electrode's.
    compat: "fixed" by default -- the reference estimator's quirks bias screened solves by
    factors, and these numbers are meant to be compared with field data; its
    walks need ~d^2 sigma_bar / 4 steps from Dirichlet distance d (set sc.max_steps).
    electrodes: "gaussian" (default) injects through Gaussians of standard deviation ``width``;
    "point" through point electrodes scored exactly (compat="fixed" only; ``width`` is
    ignored, and ``sc`` must have no source field: its solvers are built without one).
    device_reduce: transformed_potentials' -- the weighted sums formed and reduced on the device
    (results equal to float64 rounding, not bit for bit; default False)."""
    quad = wenner_quadripoles(len(sc.points), a)
    x = np.asarray(sc.points, np.float64)
    dx = float(np.linalg.norm(x[1] - x[0])) if len(x) > 1 else 1.0
    return _run_25d(sc, quad, [0, 3], lambda q: (q[:, 1], q[:, 2]),
                    lambda q, xy: np.full(len(q), wenner_geometric_factor(a * dx)), n_walks, width, n_k, groups, seed,
                    device, compat, solvers, a * dx, 2 * a * dx, electrodes, device_reduce)


def run_dipole_dipole_survey_25d(sc: Scenario, n_walks: int, n_max: int = 4, width: float = 0.5,
                                 n_k: int | None = None, groups=1, seed: int = 0, device: int | None = None,
                                 compat: str = "fixed", solvers=None, electrodes: str = "gaussian",
                                 device_reduce: bool = False) -> Survey25DResult:
    """2.5-D dipole-dipole pseudosection: quadripoles (A, B, M, N) = (c, c+1, c+1+n, c+2+n),
    n = 1..n_max, rho_a = pi n (n+1) (n+2) a dV / I with dV = V_N - V_M (positive over a
    half-space). The quadrature covers the electrode distances a .. (n_max + 2) a.
    electrodes, device_reduce: as in run_wenner_survey_25d."""
    quad = dipole_dipole_quadripoles(len(sc.points), n_max)
    x = np.asarray(sc.points, np.float64)
    dx = float(np.linalg.norm(x[1] - x[0])) if len(x) > 1 else 1.0

    def factor(q, xy):
        n = q[:, 2] - q[:, 1]
        return np.array([dipole_dipole_geometric_factor(dx, int(v)) for v in n])

    return _run_25d(sc, quad, [0, 1], lambda q: (q[:, 3], q[:, 2]), factor, n_walks, width, n_k, groups, seed,
                    device, compat, solvers, dx, (n_max + 2) * dx, electrodes, device_reduce)


def greens_section_25d(solver, points, grid, r_min: float, r_max: float, n: int | None = None, *,
                       per_wavenumber: bool = False, **solve_kw):
    """The 2.5-D potential section of a point electrode (DESIGN.md 7f "Channel maps"): the map
    of sum_j (w_j / 2) G_{k_j}(x_p, .) for every query point x_p, the wavenumbers and weights
    (k, w) of ``wavenumber_quadrature(r_min, r_max, n)`` (``n`` None: 4, 6 or 8 from r_max /
    r_min, as the surveys choose it), formed per deposit on the device in one launch
    (``WostSolver_2D.solve_greens_maps`` with the single row w / 2: the I / 2 convention of
    DESIGN.md 7a for a point current). By self-adjointness the row of x_p is the 3-D
    potential, per unit point current at x_p, in the plane of the profile, averaged over each
    cell -- for distances within [r_min, r_max] of the electrode, where the quadrature holds.
    Returns (GreensMap, k, w); with ``per_wavenumber`` (GreensMap, [GreensMap of G_{k_j}] * K,
    k, w), the unit rows (chunked over launches of at most 4 maps, each walking again).

    ``solver``: a compat="fixed" WostSolver_2D with delta tracking whose sigma_bar covers
    max k^2 (``sigma_bar_for``); its wavenumbers are set for the call and restored afterwards.
    ``solve_kw``: nWalks, maxSteps, eps, seed, replicas, quantum, walk_begin, walk_end. The
    float32 rounding of w / 2 is the kernel's (solve_greens_maps). A query point ON the
    Neumann polyline -- a surface electrode -- starts as every field-source solve starts it
    (DESIGN.md 9 item 0a); this function does not address that."""
    if n is None:
        n = 4 if r_max <= 3.0 * r_min else 6 if r_max <= 12.0 * r_min else 8
    k, w = wavenumber_quadrature(r_min, r_max, n)
    rows = [w / 2.0] + ([row for row in np.eye(k.size)] if per_wavenumber else [])
    saved = solver.wavenumbers
    solver.set_wavenumbers(k)
    try:
        maps = solver.solve_greens_maps(points, grid, np.asarray(rows, np.float64), **solve_kw)
    finally:
        solver.set_wavenumbers(saved)
    return (maps[0], maps[1:], k, w) if per_wavenumber else (maps[0], k, w)
