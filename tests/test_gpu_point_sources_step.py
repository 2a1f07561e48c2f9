"""The point-source step score on the device against closed forms ("Checks").

With maxSteps = 1, g = 0 and compat="fixed" a walk takes step 0, scores the charges, moves
and ends by adding g w = 0. The score does not depend on the step's direction:

    r   = max(min(dD(x), dN_silhouette(x)), eps / 2), then boundary_corner_radius when x starts
          on a Neumann segment
    v_s = b sum over the charges p of source s with r_p < r (and t_p < 88 under delta
          tracking) that are visible from x, in charge order, of
            q_p ln(r / max(r_p, eps / 2)) / 2 pi                                  (Laplace)
            q_p G(max(r_p, eps / 2), r) rsqrt(alpha(z_p) alpha(x)) w_j,  w_j = 1  (delta tracking)
    b   = 2 when x starts on the Neumann polyline, else 1

so all 128 walks of a point (two waves) must return the same float32 with steps == 1, every
wavenumber channel the same value, and that value is a closed form of the geometry. Every
case asserts exactly that, the value against the reference below.

The reference. G in double (scipy's exponentially scaled k0e / i0e / k1e / i1e), visibility
by tests/test_point_sources.py's Fraction predicate, everything at the float32 inputs the
kernel receives: the vertices, points, charges, float32(sqrt(sigma_bar)), float32(sigma_bar)
in the cut-off, eps / 2. The radius r is formed twice: in double, where every decision it and
the score rest on (silhouette signs, corner sides, in-ball, cut-off, clamp, visibility) is
asserted to be at least 2^-14 relative away from its threshold or else to be an exact tie of
a designed configuration (a point exactly on a segment's line), whose answer the case states;
and op by op in float32, the kernel's own IEEE sequence (poly_distance, silhouette_distance,
boundary_corner_radius: contraction off, correctly rounded sqrt). G is evaluated at the
float32 radius, because the distance to a boundary 0.004 away is a difference of coordinates
of size 1 and carries their rounding, hundreds of ulps of r, which is no property of the
score; the two radii are asserted to agree within 8 ulps of the largest coordinate.

The bound, per charge (u = 2^-23, an ulp's relative size; ulp(.) is float32's), before the
factor |q| b rsqrt(alpha alpha):
  Laplace, ln(r rcp(r_p)) / 2 pi:
      the logarithm's argument: rcp 1 u, the product u / 2, the radii 4 u each -> 9.5 u absolute
      in the logarithm, over 2 pi; the value: v_log 1, its ln 2 product 1, the 1 / 2 pi product 1,
      q 1, b 1 -> 5 ulp(value).
  delta tracking, [K0(t) - K0(s) I0(t) / I0(s)] / 2 pi, first - second (the host test's bound):
      polynomials (A&S 9.8.1-9.8.6)   eK(t) + eK(s) I0(t) / I0(s) + second (eI(t) + eI(s))
                                      eK(x) = 1e-8 (x <= 2), 1.9e-7 exp(-x) / sqrt(x);
                                      eI(x) = 1.6e-7 / I0(x) (x <= 3.75), 1.9e-7 / (sqrt(x) exp(-x) I0(x))
      rounding                        8 ulp(max(first, second))
    and what the device adds:
      hardware rcp / rsq / log / exp  1 ulp each of the term they are a factor of: at most 4 in
                                      the first term (rcp, rsq, exp, log) and 8 in the second
                                      (rcp and rsq or exp in each of K0e(s), I0e(t), I0e(s), the
                                      quotient's rcp, the exponential) -> 4 ulp(first) + 8 ulp(second)
      __expf(x) = exp2(x log2 e)      |x| u of its factor: s > 2 >= t: (|t - 2 s| + [t <= 3.75] t +
                                      [s <= 3.75] s) u second; t > 2: t u |first - second| +
                                      (2 (s - t) + [t <= 3.75] t + [s <= 3.75] s) u second
      the float32 radii               |dG/dr| 4 ulp(r) + |dG/dr_p| 4 ulp(r_p), with
                                      dG/dr = I0(t) / (r I0(s)^2),
                                      dG/dr_p = -sqrt_sb (K1(t) + K0(s) I1(t) / I0(s))
    all over 2 pi; the value: q 1, b 1, the alpha product 1, its rsq 1, alpha's own float32
    evaluations under the square root 1 -> 5 ulp(value); and float32's smallest normal,
    absolute (a charge just inside t = 88 scores 1e-40).
A source's sum adds half an ulp of the sum of the magnitudes per addition. A point no charge
scores at has the bound 0: it must read exactly 0.

Measured on one MI355X (largest error / bound, printed by every test): Laplace 0.30 and 0.35
(one charge, 64- and 32-gon; r_p / r = 1e-2 and 1e-3, where the value is largest) and 0.39 and
0.32 (32 charges); delta tracking 0.26 and 0.20 (t = 1.6 below s = 1.8; a charge next to the
sphere), 0.04 at sigma_bar = 1e-8 (0.26 against the logarithm's own bound), 0.20 through 2 and 4
wavenumbers; the Neumann geometries 0.07 to 0.19. The device stays inside the derived bound
everywhere. It does leave the host test's bound (polynomials + 8 ulps), as the float32 product
inside __expf must make it: 4.7 times that bound at t = 40, s = 106 (38 ulps of the value), 2.9
times at t = 52, 1.3 times at t = 1.6; the __expf terms above account for it. Beyond t = 87.34
__expf(-t) is below float32's smallest normal and reads 0, so the charges between there and
the cut-off at 88 score 0 instead of 1e-40 per unit strength: inside the absolute tolerance."""
import functools
import math

import numpy as np
import pytest

from test_point_sources import segments_at, visibility_exact

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -23
MARGIN = 2.0 ** -14
EPS = 1e-4
RMIN32 = F32(EPS) / F32(2)
RMIN = float(RMIN32)
TINY = 2.0 ** -126
W = 128
SEED = 5
TWO_PI = 2.0 * math.pi


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ---- geometry: the step's radius, in double (with its decisions' margins) and in float32 -------
def _arc(n_seg, a0, a1, radius=1.0):
    th = np.linspace(a0, a1, n_seg + 1)
    v = radius * np.stack([np.cos(th), np.sin(th)], axis=1)
    v[np.abs(v) < 1e-15] = 0.0
    return v.astype(np.float32)


def _distance(V, p, dt):
    """poly_distance: the least distance to the segments' clamped projections, op by op in dt."""
    V, p = V.astype(dt), p.astype(dt)
    ax, ay, bx, by = V[:-1, 0], V[:-1, 1], V[1:, 0], V[1:, 1]
    ux, uy, vx, vy = bx - ax, by - ay, p[0] - ax, p[1] - ay
    t = (vx * ux + vy * uy) / (ux * ux + uy * uy)
    t = np.minimum(np.maximum(t, dt(0)), dt(1))
    ex, ey = ((dt(1) - t) * ax + t * bx) - p[0], ((dt(1) - t) * ay + t * by) - p[1]
    return np.sqrt((ex * ex + ey * ey).min())


def _silhouette(V, p, dt, limit=None):
    """silhouette_distance: interior vertex j counts when its two segments' cross products have
    opposite signs. limit (the double pass): the margins of the vertices nearer than that."""
    V, p = V.astype(dt), p.astype(dt)
    if len(V) < 3:
        return dt(np.inf)
    ax, ay, bx, by = V[:-1, 0], V[:-1, 1], V[1:, 0], V[1:, 1]
    wx, wy = p[0] - ax, p[1] - ay
    c = (bx - ax) * wy - (by - ay) * wx
    d2 = (wx * wx + wy * wy)[1:]
    if limit is not None:
        mag = max(float(np.abs(V).max()), float(np.abs(p).max()))
        rel = np.abs(c) / (np.hypot(bx - ax, by - ay) * mag)
        near = np.sqrt(d2) < limit * (1.0 + MARGIN)
        for k in np.nonzero(near)[0]:   # (an exact 0: x on that segment's line, a designed tie -- never a silhouette)
            assert all(c[j] == 0.0 or rel[j] >= MARGIN for j in (k, k + 1)), ("silhouette sign", p, k + 1, rel[k], rel[k + 1])
    sil = c[:-1] * c[1:] < 0
    return np.sqrt(d2[sil].min()) if sil.any() else dt(np.inf)


def _corner(V, p, code, r, dt, check=False):
    """boundary_corner_radius."""
    V, p = V.astype(dt), p.astype(dt)
    s = abs(code) - 1
    a, b = V[s], V[s + 1]
    nx, ny = -(b[1] - a[1]), b[0] - a[0]
    if code < 0:
        nx, ny = -nx, -ny
    nv = len(V)
    closed = bool((V[0] == V[-1]).all())
    inext = s + 2 if s + 2 < nv else (1 if closed and nv > 3 else -1)
    iprev = s - 1 if s >= 1 else (nv - 2 if closed and nv > 3 else -1)
    r2 = r * r
    for i, e in ((inext, b), (iprev, a)):
        if i < 0:
            continue
        c = V[i]
        d2 = (p[0] - e[0]) * (p[0] - e[0]) + (p[1] - e[1]) * (p[1] - e[1])
        dot = (c[0] - e[0]) * nx + (c[1] - e[1]) * ny
        if check:   # (an exact 0: the next segment goes straight on, a designed tie -- no cut)
            assert dot == 0.0 or abs(dot) >= MARGIN * math.hypot(nx, ny) * math.hypot(c[0] - e[0], c[1] - e[1]), ("corner side", p, i)
        if dot < 0 and d2 < r2:
            r2 = d2
    return np.sqrt(r2) if r2 < r * r else r


class Case:
    """A domain: Dirichlet polyline D, Neumann polyline N (or None) with `inner` = +1 when its
    left normals point into the domain, -1 when its right normals do; sigma_bar (None: Laplace)
    and alpha (a function of double coordinates) under delta tracking."""

    def __init__(self, D, N=None, inner=1, sigma_bar=None, alpha=None):
        self.D = np.asarray(D, np.float32)
        self.N = None if N is None else np.asarray(N, np.float32)
        self.inner, self.sigma_bar, self.alpha = inner, sigma_bar, alpha
        self.mag = max(float(np.abs(self.D).max()), 0.0 if self.N is None else float(np.abs(self.N).max()))
        self._radii = {}

    def code(self, p):
        segs = [] if self.N is None else segments_at(self.N, p)
        return self.inner * (segs[0] + 1) if segs else 0

    def radius(self, p, code):
        """The step's radius as the kernel's float32 operations give it, checked against double."""
        p = np.asarray(p, np.float32)
        key = (p.tobytes(), code)
        if key not in self._radii:
            self._radii[key] = self._radius(p, code)
        return self._radii[key]

    def _radius(self, p, code):
        out = []
        for dt in (np.float64, np.float32):
            chk = dt is np.float64
            dd = _distance(self.D, p, dt)
            if chk:
                assert dd > EPS * (1.0 + MARGIN), ("the walk must take its step", p, dd)
            r = dd
            if self.N is not None:
                dn = _silhouette(self.N, p, dt, limit=float(dd) if chk else None)
                r = min(dn, dd)
            r = max(r, dt(RMIN32))
            if code:
                r = max(_corner(self.N, p, code, r, dt, check=chk), dt(RMIN32))
            out.append(float(r))
        assert abs(out[0] - out[1]) <= 8.0 * _ulp32(max(self.mag, float(np.abs(p).max()))), ("radius", p, out)
        return out[1]


# ---- the ball's Green's function in double, with the bound of the module's docstring -----------
DEVICE_TERMS = True      # False (a measurement, never a test): the host test's bound alone


def _laplace(rp, r):
    g = np.log(r / rp) / TWO_PI
    return g, np.full_like(g, 9.5 * U / TWO_PI), 5.0


def _screened(rp, r, sq):
    from scipy.special import i0e, i1e, k0e, k1e

    t, s = rp * sq, r * sq
    first = k0e(t) * np.exp(-t)
    i_ratio = i0e(t) / i0e(s) * np.exp(t - s)
    second = k0e(s) * np.exp(-s) * i_ratio
    eK = lambda x: np.where(x <= 2.0, 1e-8, 1.9e-7 * np.exp(-x) / np.sqrt(x))
    eI = lambda x: np.where(x <= 3.75, 1.6e-7 / (i0e(x) * np.exp(np.minimum(x, 700.0))), 1.9e-7 / (np.sqrt(x) * i0e(x)))
    poly = eK(t) + eK(np.float64(s)) * i_ratio + second * (eI(t) + eI(np.float64(s)))
    host = 8.0 * _ulp32(np.maximum(first, second))
    hw = 4.0 * _ulp32(first) + 8.0 * _ulp32(second)
    small = np.where(t <= 3.75, t, 0.0) + (s if s <= 3.75 else 0.0)
    expo = np.where(t <= 2.0, (np.abs(t - 2.0 * s) + small) * U * second,
                    t * U * np.abs(first - second) + (2.0 * (s - t) + small) * U * second)
    if s <= 2.0:
        expo = np.zeros_like(t)             # (that range takes no exponential)
    dg_dr = i0e(t) / i0e(s) ** 2 * np.exp(t - 2.0 * s) / r
    dg_drp = sq * (k1e(t) * np.exp(-t) + k0e(s) * i1e(t) / i0e(s) * np.exp(t - 2.0 * s))
    rad = dg_dr * 4.0 * _ulp32(r) + dg_drp * 4.0 * _ulp32(rp)
    if not DEVICE_TERMS:
        return (first - second) / TWO_PI, (poly + host) / TWO_PI, 0.0
    return (first - second) / TWO_PI, (poly + host + hw + expo + rad) / TWO_PI, 5.0


def reference(case, pts, charges, designed=None):
    """want, bound [NS, n] of the one-step solve of `charges` = [(x, y, q, source), ...] (sources
    ascending) at `pts`, and the counts (in the ball and scored, in the ball and not visible,
    outside the ball or beyond the cut-off). designed: {(x, y, zx, zy): visible} for the exact
    ties, whose answers are stated instead of asserted to be firm."""
    pts = np.asarray(pts, np.float32)
    Z = np.array([c[:2] for c in charges], np.float32).astype(np.float64)
    q = np.array([c[2] for c in charges], np.float32).astype(np.float64)
    src = np.array([c[3] for c in charges], np.int64)
    ns = int(src.max()) + 1
    want, bound = np.zeros((ns, len(pts))), np.zeros((ns, len(pts)))
    counts = np.zeros(3, np.int64)
    delta = case.sigma_bar is not None
    if delta:
        sq = float(F32(math.sqrt(case.sigma_bar)))
        sb = float(F32(case.sigma_bar))
        az = case.alpha(Z[:, 0], Z[:, 1])
    for i, p in enumerate(pts):
        code = case.code(p)
        r = case.radius(p, code)
        x = p.astype(np.float64)
        d = np.hypot(Z[:, 0] - x[0], Z[:, 1] - x[1])
        assert np.all(np.abs(d / r - 1.0) >= MARGIN), ("in-ball", p, r, d / r)
        inb = d < r
        if delta:
            tt = d * math.sqrt(sb)
            assert np.all(np.abs(tt[inb] / 88.0 - 1.0) >= MARGIN), ("cut-off", p, tt[inb])
            inb &= tt < 88.0
        assert np.all(np.abs(d[inb] / RMIN - 1.0) >= MARGIN), ("clamp", p, d[inb])
        counts[2] += int((~inb).sum())
        idx = np.nonzero(inb)[0]
        if case.N is not None:
            keep = []
            for k in idx:
                vis, margin = visibility_exact(case.N, p, Z[k], code)
                key = (float(p[0]), float(p[1]), float(Z[k, 0]), float(Z[k, 1]))
                if designed is not None and key in designed:
                    assert vis == designed[key], ("designed visibility", key, vis)
                else:
                    assert margin >= MARGIN, ("visibility", key, code, vis, margin)
                if vis:
                    keep.append(k)
            counts[1] += len(idx) - len(keep)
            idx = np.array(keep, np.int64)
        counts[0] += len(idx)
        if not len(idx):
            continue
        rp = np.maximum(d[idx], RMIN)
        g, bg, ulps = _screened(rp, r, sq) if delta else _laplace(rp, r)
        f = 2.0 if code else 1.0
        if delta:
            f = f / np.sqrt(az[idx] * float(case.alpha(x[0], x[1])))
        v = q[idx] * f * g
        bv = np.abs(q[idx]) * f * bg + ulps * _ulp32(v) + (TINY if delta else 0.0)
        for s in range(ns):
            m = src[idx] == s
            if m.any():
                want[s, i] = v[m].sum()
                bound[s, i] = bv[m].sum() + 0.5 * (int(m.sum()) - 1) * float(_ulp32(np.abs(v[m]).sum()))
    return want, bound, counts


# ---- solves ------------------------------------------------------------------------------------
def _solver(case, alpha_field=None):
    from dcrmontecarlo_amd import PolyLinesSimple, WostSolver_2D

    kw = {} if case.sigma_bar is None else dict(alpha=alpha_field, sigma_bar=case.sigma_bar)
    s = WostSolver_2D(PolyLinesSimple(case.D), 0.0, None if case.N is None else PolyLinesSimple(case.N),
                      compat="fixed", **kw)
    if case.sigma_bar is not None:
        s.set_fixed_step_check(False)
    return s


def _sources(charges):
    ns = max(c[3] for c in charges) + 1
    return [[((float(F32(c[0])), float(F32(c[1]))), float(F32(c[2]))) for c in charges if c[3] == s] for s in range(ns)]


def _one_value(vals, steps):
    """[..., n, W] per-walk values -> [..., n]: every walk took one step and all walks of a point
    returned the same bits."""
    assert np.all(steps == 1)
    bits = np.ascontiguousarray(vals).view(np.uint32)
    assert np.all(bits == bits[..., :1]), "walks of one point differ"
    return vals[..., 0].astype(np.float64)


def _compare(got, want, bound, worst, what):
    err = np.abs(got - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    k = np.unravel_index(int(ratio.argmax()), ratio.shape)
    if ratio[k] > worst[0]:
        worst[:] = [float(ratio[k]), f"{what} at {k}: got {got[k]!r} want {want[k]!r} bound {bound[k]:.3e}"]
    assert np.all(err <= bound), (what, k, got[k], want[k], bound[k], float(ratio[k]))


def _run(solver, case, pts, charges, worst, what, designed=None):
    want, bound, counts = reference(case, pts, charges, designed)
    vals, steps = solver.solve_point_sources_walks(pts, _sources(charges), nWalks=W, maxSteps=1, eps=EPS, seed=SEED)
    assert solver.last_timing["jit"] == 1
    got = _one_value(vals, steps)
    _compare(got, want, bound, worst, what)
    return got, want, counts


# ---- 1. and 2.: the regular polygons -----------------------------------------------------------
N_POINTS = 48


@functools.lru_cache(maxsize=None)
def _polygon_points(n_gon):
    """48 points on a golden-angle spiral at relative depths 0.004 .. 0.95 below the inscribed
    circle: the radius dD spans 0.004 .. 0.95, two and a half decades."""
    depth = np.geomspace(0.004, 0.95, N_POINTS)
    phi = 2.399963229728653 * np.arange(N_POINTS) + 0.1
    rho = math.cos(math.pi / n_gon) * (1.0 - depth)
    p = np.stack([rho * np.cos(phi), rho * np.sin(phi)], axis=1).astype(np.float32)
    p.setflags(write=False)
    return p


def _about(x, r, ratio, phi):
    """The float32 point at distance ratio r from x in direction phi."""
    return (float(F32(x[0] + ratio * r * math.cos(phi))), float(F32(x[1] + ratio * r * math.sin(phi))))


def _firm(case, pts, z):
    """No decision about a charge at z rests on rounding at any of the points (what reference()
    asserts): the generators below turn a charge about its own point until this holds."""
    for p in pts:
        code = case.code(p)
        r = case.radius(p, code)
        d = math.hypot(z[0] - float(p[0]), z[1] - float(p[1]))
        if abs(d / r - 1.0) < 2.0 * MARGIN:
            return False
        if d < r:
            if abs(d / RMIN - 1.0) < 2.0 * MARGIN:
                return False
            if case.sigma_bar is not None and abs(d * math.sqrt(float(F32(case.sigma_bar))) / 88.0 - 1.0) < 2.0 * MARGIN:
                return False
            if case.N is not None and visibility_exact(case.N, p, z, code)[1] < 2.0 * MARGIN:
                return False
    return True


def _place(case, pts, x, r, ratio, phi):
    """_about(x, r, ratio, phi'), phi' the first of phi, phi + 0.05, ... that is _firm."""
    for n in range(100):
        z = _about(x, r, ratio, phi + 0.05 * n)
        if _firm(case, pts, z):
            return z
    raise AssertionError(("no firm direction", x, r, ratio))


LAPLACE_RATIOS = (1e-4, 1e-3, 1e-2, 0.1, 0.3, 0.6, 0.9, 0.99, 0.999, 1.0 - 2.0 ** -12, 1.0 + 2.0 ** -12, 1.5, 30.0)


@pytest.mark.parametrize("n_gon", [64, 32])
def test_laplace_one_charge(gpu_available, n_gon):
    """Regular n-gon, circumradius 1 (64: the staged polyline, 32: the compiled-in one), PC = 1,
    NS = 1: for 12 of the 48 points a charge at r_p / r = 1e-4 .. 0.999, at (1 -+ 2^-12) r (the
    outer one scores exactly 0), outside the ball and far outside the polygon, and on the point
    itself (the rmin clamp); every solve is compared at all 48 points."""
    case = Case(_arc(n_gon, 0.0, TWO_PI))
    pts = _polygon_points(n_gon)
    s = _solver(case)
    worst, total = [0.0, ""], np.zeros(3, np.int64)
    for j, i in enumerate(range(0, N_POINTS, 4)):
        r = case.radius(pts[i], 0)
        zs = [_place(case, pts, pts[i], r, ratio, 0.7 + 1.1 * j + 0.37 * k) for k, ratio in enumerate(LAPLACE_RATIOS)]
        zs.append((float(pts[i][0]), float(pts[i][1])))
        for k, z in enumerate(zs):
            got, want, counts = _run(s, case, pts, [(z[0], z[1], (-1.5) ** (k % 3), 0)], worst, f"point {i} charge {k}")
            total += counts
            if k < 9 or k == 13:
                assert want[0, i] != 0.0
            if k == 9:
                assert 0.0 < want[0, i] < 2.0 ** -11          # just inside the ball
            if k in (10, 11, 12):
                assert got[0, i] == 0.0                        # just outside, outside, far outside
    print(f"laplace {n_gon}-gon, one charge: scored / hidden / outside {total.tolist()}, largest error / bound {worst}")
    assert s.last_timing["jit_ms"] == 0.0                      # one kernel served every charge set


def _max_charges(case, pts, i, j):
    """32 charges in 16 sources of 1 and 3 charges, unequal strengths of both signs, about point
    i: r_p / r from 1e-4 to 0.999, four beyond the ball, one on the point."""
    r = case.radius(pts[i], 0)
    ratios = list(np.geomspace(1e-4, 0.999, 26)) + [1.0 - 2.0 ** -12, 1.0 + 2.0 ** -12, 1.3, 4.0, 40.0]
    rng = np.random.default_rng(100 + j)
    zs = [_place(case, pts, pts[i], r, ratio, rng.uniform(0.0, TWO_PI)) for ratio in ratios] + [(float(pts[i][0]), float(pts[i][1]))]
    order = rng.permutation(32)
    qs = rng.uniform(0.25, 3.0, 32) * rng.choice([-1.0, 1.0], 32)
    src = np.repeat(np.arange(16), [1, 3] * 8)
    return [(zs[o][0], zs[o][1], float(F32(qs[k])), int(src[k])) for k, o in enumerate(order)]


@pytest.mark.parametrize("n_gon", [64, 32])
def test_laplace_32_charges_in_16_sources(gpu_available, n_gon):
    """PC = 32, NS = 16, the maxima: every channel holds the sum of its own charges, in charge
    order."""
    case = Case(_arc(n_gon, 0.0, TWO_PI))
    pts = _polygon_points(n_gon)
    s = _solver(case)
    worst, total = [0.0, ""], np.zeros(3, np.int64)
    for j, i in enumerate(range(1, N_POINTS, 6)):
        charges = _max_charges(case, pts, i, j)
        got, want, counts = _run(s, case, pts, charges, worst, f"point {i}")
        total += counts
        assert got.shape == (16, N_POINTS) and np.count_nonzero(want[:, i]) >= 12
        assert len({got[c].tobytes() for c in range(16)}) == len({want[c].tobytes() for c in range(16)}) >= 12
    print(f"laplace {n_gon}-gon, 32 charges: scored / hidden / outside {total.tolist()}, largest error / bound {worst}")
    assert total[0] > 300 and s.last_timing["jit_ms"] == 0.0


# ---- 2. delta tracking -------------------------------------------------------------------------
SQRT_SB = 400.0
T_CUT = 87.15      # between 87 and 87.33, beyond which __expf(-t) is below float32's smallest normal and reads 0
T_VALUES = (1e-3, 0.05, 0.5, 1.9, 2.1, 3.7, 3.8, 10.0, 40.0, T_CUT, 88.0 * (1.0 - 2.0 ** -10), 88.0 * (1.0 + 2.0 ** -10))
S_RATIOS = (1e-4, 1e-2, 0.3, 0.9, 0.999, 1.0 - 2.0 ** -12, 1.0 + 2.0 ** -12, 3.0)


def _alpha(x, y):
    return 1.0 + 0.5 * x


def _alpha_field():
    from dcrmontecarlo_amd import fields as F

    return 1.0 + F.X / 2


def _delta_pairs(case, pts, i, j):
    """Two-charge sets (one per source) about point i: t = r_p sqrt(sigma_bar) on both sides of
    2, of 3.75 and of 88, and r_p / r from 1e-4 to (1 +- 2^-12)."""
    r = case.radius(pts[i], 0)
    sq = float(F32(math.sqrt(case.sigma_bar)))
    ratios = [t / (r * sq) for t in T_VALUES if t / (r * sq) < 0.9995] + list(S_RATIOS)
    if len(ratios) % 2:
        ratios.append(0.5)
    zs = [_place(case, pts, pts[i], r, ratio, 0.3 + 0.9 * j + 0.41 * k) for k, ratio in enumerate(ratios)]
    # (the charge at t = T_CUT scores 3e-40 per unit strength: at 1000 it is far above the absolute
    # tolerance, so a cut-off anywhere below it would show)
    qs = [1000.0 if abs(ratio * r * sq - T_CUT) < 1e-6 else (1.25, -0.75)[k % 2] for k, ratio in enumerate(ratios)]
    return [[(zs[k][0], zs[k][1], qs[k], 0), (zs[k + 1][0], zs[k + 1][1], qs[k + 1], 1)] for k in range(0, len(zs), 2)]


@pytest.mark.parametrize("n_gon", [64, 32])
def test_screened_two_sources(gpu_available, n_gon):
    """alpha = 1 + x / 2 (a Field: the per-solve alpha(z_p) launch and rsqrt(alpha(z_p) alpha(x))),
    sigma_bar = 160000: s = r sqrt(sigma_bar) runs from 1.3 to 380 over the 48 points, on both
    sides of 2 and of 3.75, so with the charges' t all three ranges of ball_greens_screened and
    both branches of bessel_i0e are taken, for t and for s. Charges at t = 88 (1 -+ 2^-10): the
    outer one scores exactly 0."""
    case = Case(_arc(n_gon, 0.0, TWO_PI), sigma_bar=SQRT_SB ** 2, alpha=_alpha)
    pts = _polygon_points(n_gon)
    s = _solver(case, _alpha_field())
    worst, total = [0.0, ""], np.zeros(3, np.int64)
    seen = set()
    sq = float(F32(SQRT_SB))
    for j, i in enumerate(list(range(0, 12)) + list(range(12, N_POINTS, 3))):
        r = case.radius(pts[i], 0)
        for k, pair in enumerate(_delta_pairs(case, pts, i, j)):
            got, want, counts = _run(s, case, pts, pair, worst, f"point {i} pair {k}")
            total += counts
            for c in range(2):
                t = math.hypot(pair[c][0] - float(pts[i][0]), pair[c][1] - float(pts[i][1])) * sq
                if want[c, i] != 0.0:
                    seen.add(("s<=2" if r * sq <= 2 else "t<=2<s" if t <= 2 else "2<t", t <= 3.75, r * sq <= 3.75))
                if 88.0 < t < 88.1 and t < r * sq:
                    assert got[c, i] == 0.0
                    seen.add("beyond 88")
                if 87.9 < t < 88.0 and t < r * sq:
                    assert want[c, i] != 0.0 and abs(want[c, i]) < TINY
                    seen.add("below 88")
                if pair[c][2] == 1000.0:
                    assert abs(t - T_CUT) < 0.01 and want[c, i] > 10.0 * TINY and abs(got[c, i] / want[c, i] - 1.0) < 0.1
                    seen.add("just below the cut-off")
    print(f"screened {n_gon}-gon: scored / hidden / outside {total.tolist()}, ranges {sorted(map(str, seen))}, "
          f"largest error / bound {worst}")
    assert {("s<=2", True, True), ("t<=2<s", True, True), ("t<=2<s", True, False), ("2<t", True, True),
            ("2<t", True, False), ("2<t", False, False), "beyond 88", "below 88", "just below the cut-off"} <= seen
    assert s.last_timing["jit_ms"] == 0.0


def test_screened_small_sigma_bar_is_the_logarithm(gpu_available):
    """sigma_bar = 1e-8: s <= 4e-5, the value is ln(r / r_p) / 2 pi rsqrt(alpha alpha) to the
    Laplace bound plus the two K0 polynomials' own roundings (2 ulp(0.5772) / 2 pi), which is
    far below the screened bound's 8 ulp(K0(t))."""
    case = Case(_arc(64, 0.0, TWO_PI), sigma_bar=1e-8, alpha=_alpha)
    pts = _polygon_points(64)
    s = _solver(case, _alpha_field())
    worst, tight = [0.0, ""], [0.0, ""]
    lap = Case(case.D)
    for j, i in enumerate(range(2, N_POINTS, 9)):
        r = case.radius(pts[i], 0)
        zs = [_place(case, pts, pts[i], r, ratio, 0.2 + 0.8 * j + 0.43 * k) for k, ratio in enumerate(LAPLACE_RATIOS[:10])]
        for k in range(0, 10, 2):
            pair = [(zs[k][0], zs[k][1], 1.25, 0), (zs[k + 1][0], zs[k + 1][1], -0.75, 1)]
            got, want, _ = _run(s, case, pts, pair, worst, f"point {i} pair {k}")
            wl, bl, _ = reference(lap, pts, pair)          # (one charge per source: q ln(r / r_p) / 2 pi)
            f = 1.0 / np.sqrt(np.outer([_alpha(float(F32(c[0])), 0.0) for c in pair], _alpha(pts[:, 0].astype(np.float64), 0.0)))
            extra = np.where(wl != 0.0, 2.0 * float(_ulp32(0.5772)) / TWO_PI * np.array([[1.25], [0.75]]), 0.0)
            # (the alpha factor: its product, its rsq, alpha's own evaluations -> 3 ulps)
            _compare(got, wl * f, (bl + extra) * f + 3.0 * _ulp32(wl * f), tight, f"point {i} pair {k} (logarithm)")
    print(f"screened, sigma_bar 1e-8: largest error / bound {worst}; against the logarithm {tight}")


@pytest.mark.parametrize("nk", [2, 4])
def test_screened_wavenumber_channels(gpu_available, nk):
    """The same problem through solve_wavenumbers_walks with NK = 2 and 4 wavenumbers and two
    sources: w_j = 1 at step 0, so all NK x NS channels equal the closed form and the
    wavenumber channels of a source equal each other bit for bit (total[j * NS + s])."""
    case = Case(_arc(64, 0.0, TWO_PI), sigma_bar=SQRT_SB ** 2, alpha=_alpha)
    pts = _polygon_points(64)
    s = _solver(case, _alpha_field())
    worst, both = [0.0, ""], 0
    k = np.array([0.5, 1.0, 2.0, 3.0])[:nk]
    for j, i in enumerate(range(3, N_POINTS, 8)):
        for n, pair in enumerate(_delta_pairs(case, pts, i, j)[::3]):
            want, bound, _ = reference(case, pts, pair)
            vals, steps = s.solve_wavenumbers_walks(pts, k, nWalks=W, maxSteps=1, eps=EPS, sources=_sources(pair), seed=SEED)
            assert vals.shape == (nk, 2, N_POINTS, W) and s.last_timing["jit"] == 1
            got = _one_value(vals, steps)
            for c in range(nk):
                np.testing.assert_array_equal(got[c].view(np.uint64), got[0].view(np.uint64))
                _compare(got[c], want, bound, worst, f"point {i} pair {n} wavenumber {c}")
            both += int(np.any(got[0, 0] != 0.0) and np.any(got[0, 1] != 0.0) and got[0, 0].tobytes() != got[0, 1].tobytes())
    print(f"screened, {nk} wavenumbers x 2 sources: {both} solves with two different non-zero sources, largest error / bound {worst}")
    assert both >= 10


# ---- 3. Neumann: visibility, b, the corner radius ----------------------------------------------
def _half_arc():
    return _arc(32, math.pi, TWO_PI)


def _ring(case, pts, x, r, phase):
    """Eight float32 charges about x: at 0.35 r and 0.8 r in four directions each."""
    return [_place(case, pts, x, r, ratio, phase + 0.5 * math.pi * k + (0.6 if ratio > 0.5 else 0.0))
            for ratio in (0.35, 0.8) for k in range(4)]


def _geometry(name):
    """(case, query points, designed charges, {designed tie: visible}) of the host visibility
    tests' polylines, each closed by a Dirichlet polyline. Charges in the air (outside the
    domain, inside a ball) are what is in a ball and not visible: where the radius stops at the
    nearest silhouette vertex, every point of the domain in the ball is visible."""
    tie = {}
    if name in ("flat", "flat, delta tracking"):
        kw = dict(sigma_bar=100.0, alpha=lambda x, y: 2.0 + 0.0 * x) if name != "flat" else {}
        case = Case(_half_arc(), [[1, 0], [-1, 0]], 1, **kw)
        pts = [(0.3, -0.4), (-0.5, -0.0625), (0.5, 0.0), (-0.25, 0.0)]
        zs = [(0.0, 0.0), (0.375, 0.0), (-0.125, 0.0), (0.3, -0.3), (0.4375, 0.0625), (-0.25, 0.125)]
    elif name == "split":
        case = Case(_half_arc(), np.stack([np.linspace(1, -1, 9), np.zeros(9)], axis=1), 1)
        pts = [(0.3, -0.4), (0.25, 0.0), (0.625, 0.0), (-0.0625, -0.125)]
        zs = [(0.0, 0.0), (0.5, 0.0), (0.3125, 0.0), (0.25, -0.25), (0.25, 0.0625)]
        for x in pts[1:3]:          # both on the straight surface: along the boundary, visible
            for z in zs[:3]:
                tie[x + z] = True
    elif name == "valley":
        case = Case([[-1, 1], [-2, 0], [-1.5, -2], [1.5, -2], [2, 0], [1, 1]], [[1, 1], [0, 0], [-1, 1]], 1)
        # (the ball of a walker on a slope stops at the re-entrant vertex (0, 0), so that vertex and the
        # other slope lie on or beyond its sphere: no charge is put on the vertex itself)
        pts = [(0.25, 0.25), (0.75, 0.5), (0.125, -0.5), (-0.375, 0.375)]
        zs = [(-0.125, 0.125), (0.4375, 0.4375), (0.375, 0.5), (0.0, 0.25), (0.25, 0.0), (-0.625, 0.5), (0.125, 0.125)]
    elif name == "hill":
        case = Case([[-1, -1], [-1.5, -3], [1.5, -3], [1, -1]], [[1, -1], [0, 0], [-1, -1]], 1)
        pts = [(0.25, -0.25), (0.125, -1.0), (-0.375, -0.375), (-0.25, -0.875)]
        zs = [(-0.25, -0.25), (0.0, 0.0), (0.4375, -0.4375), (0.0, -0.5), (0.25, -0.125), (-0.375, -0.25)]
    elif name == "notch":
        case = Case([[-2, 0], [-2, -3], [2, -3], [2, 0]], [[2, 0], [0.625, 0], [0.5, -1], [0.375, 0], [-2, 0]], 1)
        pts = [(1.5, -0.25), (1.0, 0.0), (0.5, -1.5), (0.0, 0.0), (0.75, -0.5)]
        zs = [(-1.0, 0.0), (0.25, 0.0), (1.25, 0.0), (0.515625, -0.5), (0.5625, -0.5), (0.4375, -0.5), (0.5, -1.25)]
        # both on the surface with the notch between them: the ray runs along the surface into the
        # notch's first vertex, a crossing at a vertex -- blocked
        tie[(1.0, 0.0, 0.25, 0.0)] = False
    else:
        assert name == "wedge"
        case = Case(_arc(48, 0.0, 1.5 * math.pi), [[1, 0], [0, 0], [0, -1]], -1)
        e = lambda rho, deg: (rho * math.cos(math.radians(deg)), rho * math.sin(math.radians(deg)))
        # (0.125, 0): on the face phi = 0 next to the re-entrant corner. Its ball stops at the corner,
        # r = 0.125: the charge 0.09 away scores with that radius, the one 0.3 away -- inside the
        # uncut radius 0.875 -- exactly 0
        pts = [(0.125, 0.0), e(0.6, 252), e(0.5, 108), (0.0, -0.5), (0.5, 0.0)]
        zs = [(0.1875, 0.0625), (0.125, 0.3), e(0.6, 18), (0.25, -0.25), (-0.25, -0.375), (0.0625, 0.0), (0.0, -0.25)]
        tie[(0.125, 0.0, 0.0625, 0.0)] = True
        tie[(0.5, 0.0, 0.0625, 0.0)] = True
        tie[(0.0, -0.5, 0.0, -0.25)] = True
    f = lambda p: (float(F32(p[0])), float(F32(p[1])))
    pts = np.array([f(p) for p in pts], np.float32)
    tie = {f(k[:2]) + f(k[2:]): v for k, v in tie.items()}
    return case, pts, [f(z) for z in zs], tie


def _neumann_charge_sets(case, pts, zs):
    """Sets of 8 charges in 2 sources (5 and 3): the designed charges, then a ring about every
    query point."""
    allz = list(zs)
    for i, p in enumerate(pts):
        allz += _ring(case, pts, p, case.radius(p, case.code(p)), 0.2 + 0.35 * i)
    while len(allz) % 8:
        allz.append((40.0 + len(allz), 40.0))
    qs = (1.0, -0.5, 2.0, 0.75, -1.25, 1.5, -2.0, 0.5)
    return [[(z[0], z[1], qs[k], 0 if k < 5 else 1) for k, z in enumerate(allz[n:n + 8])] for n in range(0, len(allz), 8)]


@pytest.mark.parametrize("name", ["flat", "split", "valley", "hill", "notch", "wedge", "flat, delta tracking"])
def test_neumann_geometries(gpu_available, name):
    """The polylines of the host visibility tests, closed by a Dirichlet polyline; query points
    in the interior and on the surface (b = 2; one at a vertex), charges on the surface, in the
    interior and in the air. Visibility is the Fraction predicate's, for the exact ties
    DESIGN.md 7b's. The scan kernel and the tree kernel agree bit for bit, and with the
    reference within the bound. "flat, delta tracking" is the half disk with alpha = 2."""
    case, pts, zs, tie = _geometry(name)
    sets = _neumann_charge_sets(case, pts, zs)
    worst, total = [0.0, ""], np.zeros(3, np.int64)
    res = []
    for tree in (False, True):
        s = _solver(case, 2.0)
        s.set_segment_tree(0 if tree else -1)
        out = []
        for n, charges in enumerate(sets):
            got, want, counts = _run(s, case, pts, charges, worst, f"{name} set {n} tree {tree}", tie)
            assert s.last_timing["tree"] == (1 if tree else 0)
            out.append(got)
            total += counts
        res.append(np.stack(out))
    np.testing.assert_array_equal(res[0].view(np.uint64), res[1].view(np.uint64))
    codes = [case.code(p) for p in pts]
    print(f"{name}: boundary codes {codes}, scored / hidden / outside {(total // 2).tolist()}, largest error / bound {worst}")
    assert any(codes) and not all(codes) and total[0] > 0 and total[1] > 0 and total[2] > 0
    if name == "wedge":
        # the corner radius: the first designed charge scores 2 ln(0.125 / r_p) / 2 pi at (0.125, 0),
        # the second exactly 0 (they are charges 0 and 1 of set 0, both of source 0)
        # the corner radius: at (0.125, 0) the ball stops at the corner, so of the first two designed
        # charges the reference scores the one 0.088 away with r = 0.125 and leaves out the one 0.3
        # away, which the uncut radius would hold
        assert case.radius(pts[0], codes[0]) == 0.125
        assert math.hypot(zs[0][0] - 0.125, zs[0][1]) < 0.125 < math.hypot(zs[1][0] - 0.125, zs[1][1]) < 0.8
        only, _, _ = reference(case, pts[:1], [sets[0][0], sets[0][1]], tie)
        assert abs(only[0, 0] - 2.0 * math.log(0.125 / math.hypot(0.0625, 0.0625)) / TWO_PI) < 1e-12
