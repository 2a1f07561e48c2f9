"""The field zoo: coefficient fields that exercise every factor kind's value, gradient and
Laplacian, their float64 reference, and the tolerances. Shared by tests/test_field_zoo.py
(a host build of wost_device.h) and tests/test_gpu_field_zoo.py (the device).

Reference: float64 torch autograd of ``field(p)`` (fields._eval_torch: torch's derivative
rules, not the header's), with p the float32 points cast to float64 and the parameters
rounded to float32 as the device receives them.

Tolerance per field F and component c (value, d/dx, d/dy, Laplacian), nothing hard-coded:

    scale_c = max |reference_c| over the finite points
    e32_c   = max |float32 torch autograd - float64 torch autograd| (reference arithmetic only)
    tol_c   = max(8 e32_c, 16 * 2^-23 * scale_c)

The factor 8 covers what the device adds over IEEE float32: 1 ulp per v_rcp / v_rsq and
|x| 2^-23 per __expf(x) with |x| <= 8 (the budget of DESIGN 7b). Condition on the inputs,
asserted when the zoo is built: tol_c <= 2e-5 scale_c. A field that breaks it is badly
conditioned and has to be changed, not the cap.

sigma' (reference_sigma_prime) has the majorant
    M = |sigma|/a + 0.5 (|lap|/a + |grad a|^2 / (2 a^2)).
Its tolerance is four times the first-order change of M's terms when every jet component
moves by its own tol_c (the relative tolerance r_c = tol_c / scale_c applied to the
component's scale: the error does not vanish where the component does), plus r M for the
arithmetic of sigma' itself, r the largest r_c:
    4 (tol_sigma/a + |sigma| tol_a/a^2 + 0.5 (tol_lap/a + (|lap| + 1e-8) tol_a/a^2
       + (|gx| tol_gx + |gy| tol_gy)/a^2 + |grad a|^2 tol_a/a^3) + r M).
"""
import functools
import math

import numpy as np

from dcrmontecarlo_amd import _lib
from dcrmontecarlo_amd import fields as F
from dcrmontecarlo_amd.fields import X, Y

# torch brings its own copy of the HIP runtime, and its autograd engine initialises it on the
# first backward; libwost's runtime then finds no device in this process ("no ROCm-capable
# device is detected"). Initialised first, both work: so the library's comes up here, before
# the reference below runs its first backward. (Without a device this returns 0 and is harmless.)
_lib.device_count()

BOX = 1.2                       # the zoo's domain [-BOX, BOX]^2
N_UNIFORM = 256
N_POINTS = 300                  # points of an ordinary field: uniform, special, uniform again
SEED = 20260
COMPONENTS = ("value", "d/dx", "d/dy", "laplacian")
CAP = 2e-5

# every coordinate below that a test needs exactly is a dyadic rational (exact in float32)
RADIAL_CENTRE = (0.25, -0.125)
RADIAL_R = 0.7
IND_BOX = (-0.5, 0.75, -0.25, 1.0)
IND_DISK_C, IND_DISK_R = (0.25, -0.5), 0.5
GRID_X0, GRID_HX, GRID_NX = -0.9375, 0.1875, 11     # nodes -0.9375 .. 0.9375
GRID_Y0, GRID_HY, GRID_NY = -1.0, 0.25, 9           # nodes -1 .. 1
GRID_VALUES = (0.5 * np.random.default_rng(SEED + 1).random((GRID_NY, GRID_NX))).astype(np.float32)

SHARP_C1, SHARP_R1 = (-0.5, 0.5), 0.4               # smooth_circle (k = -100)
SHARP_C2, SHARP_S2 = (0.25, -0.875), 0.03           # the narrow Gaussian
SHARP_C3 = (0.5, -0.4)                              # the oblique Gaussian
SHARP_DISK = ((-0.75, -0.75), 0.25)
# where `sharp`'s derivatives are largest: the narrow Gaussian's centre (Laplacian -6 / s^2)
# and the points one width from it (gradient 3 e^-1/2 / s). With them among the points the
# scales are the field's own maxima whatever the random draw; the float32 rounding of the
# sigmoids' arguments (d to half an ulp times k = 100, 200 y to half an ulp: dz <= 4e-6) then
# stays below the cap in the worst case and not by the luck of a draw:
#   d/dx:  2 k max|s2| dz = 2 * 100 * 0.096 * 4e-6 = 7.7e-5 of 60.7, times 8: 1.0e-5 of scale
#   lap:   2 k^2 max|s3| dz = 2 * 1e4 * 0.125 * 4e-6 = 1.0e-2 of 6667, times 8: 1.2e-5 of scale
# (s2, s3: the sigmoid's second and third derivatives)
SHARP_PEAKS = [SHARP_C2] + [(SHARP_C2[0] + sx * SHARP_S2, SHARP_C2[1] + sy * SHARP_S2)
                            for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1))]


def _tab():
    return F.tabulated(GRID_VALUES, GRID_X0, GRID_Y0, GRID_HX, GRID_HY)


def _zoo():
    pi = math.pi
    z = {}
    z["mono"] = 1e-3 * X**15 * Y**3 + X * Y - 2 * Y**2 + 3 + 0.25 * X**2 * Y**4
    z["exp_general"] = F.exp(-0.5 * X**2 - 0.8 * Y**2 + 0.6 * X * Y + 0.3 * X - 0.4 * Y + 0.2)
    # det = 4AB - C^2 = 0: not centred, so lx, ly and q0 stay nonzero
    z["exp_general_det0"] = F.exp(-0.5 * X**2 - 0.5 * Y**2 + 1.0 * X * Y + 0.3 * X - 0.4 * Y + 0.2)
    z["exp_diag"] = F.exp(-1.5 * (X - 0.25)**2 - 0.75 * (Y + 0.5)**2)
    z["exp_linear"] = F.exp(0.3 * X - 0.2 * Y)
    z["trig_product"] = F.sin(2 * X + Y + 0.5) * F.cos(X - 3 * Y) * X**2
    z["sigmoid_lin"] = F.sigmoid(1.5 * X - 2.0 * Y + 0.3)
    z["sigmoid_radial_neg"] = F.sigmoid_radial(-4.0, RADIAL_CENTRE, RADIAL_R)
    z["sigmoid_radial_pos"] = F.sigmoid_radial(4.0, RADIAL_CENTRE, RADIAL_R)
    z["three_factors"] = F.exp(-(X**2 + Y**2)) * F.sin(pi * X) * F.sigmoid(2 * Y) * Y
    z["indicators"] = ((1 + X * Y) * F.indicator_box(*IND_BOX)
                       + 0.5 * F.indicator_disk(IND_DISK_C, IND_DISK_R) * F.sin(X))
    z["grid"] = 2 + _tab() * F.cos(Y)
    dx, dy = X - SHARP_C3[0], Y - SHARP_C3[1]
    z["sharp"] = (1 + 2 * F.smooth_circle(SHARP_C1, SHARP_R1) + 0.5 * F.sigmoid(200 * Y - 80)
                  + 3 * F.gaussian(SHARP_C2, SHARP_S2) + F.exp(-400 * dx**2 - 300 * dy**2 + 100 * dx * dy)
                  + 0.25 * F.indicator_disk(*SHARP_DISK))
    return z


ZOO = _zoo()
# what is added to a field to make it an alpha (>= 0.3 on the box; asserted below)
_SHIFT = {"mono": 2.0, "exp_general": 0.3, "exp_general_det0": 0.3, "exp_diag": 0.3, "exp_linear": 0.0,
          "trig_product": 2.0, "sigmoid_lin": 0.3, "sigmoid_radial_neg": 0.3, "sigmoid_radial_pos": 0.3,
          "three_factors": 1.5, "indicators": 1.0, "grid": 0.0, "sharp": 0.0}
POSITIVE = {k: (ZOO[k] + _SHIFT[k] if _SHIFT[k] else ZOO[k]) for k in ZOO}
SIGMAS = {"zero": None, "trig": ZOO["trig_product"] + 2}


def kinds_of(field):
    return {f.kind for t in field.terms for f in t.factors} | ({F.FK_MONO} if any(t.mono != (0, 0) for t in field.terms)
                                                             else set())


def _packed_exp(field):
    return [p for k, p in field.pack()[1] if k == F.FK_EXP_QUAD]


# the structure the names promise
assert all(np.float32(v) == 0 for v in _packed_exp(ZOO["exp_diag"])[0][4:8])
assert all(np.float32(v) != 0 for v in _packed_exp(ZOO["exp_general_det0"])[0][4:8])
assert np.float32(_packed_exp(ZOO["exp_general"])[0][4]) != 0 and np.float32(_packed_exp(ZOO["exp_general"])[0][7]) != 0
assert set().union(*[kinds_of(f) for f in ZOO.values()]) == set(range(1, 10))


# ---------------------------------------------------------------------------
# points
# ---------------------------------------------------------------------------
def _grid_u(p):
    p = np.asarray(p, np.float64)
    return (p[:, 0] - GRID_X0) / GRID_HX, (p[:, 1] - GRID_Y0) / GRID_HY


def grid_unambiguous(p, margin=2.0**-6):
    """At least `margin` of a cell from every node line and from the grid's edge, where the
    clamp and the C1-only spline leave the derivative ambiguous."""
    ok = np.ones(len(p), bool)
    for u, n in zip(_grid_u(p), (GRID_NX, GRID_NY)):
        inside = (u > -margin) & (u < n - 1 + margin)
        ok &= ~inside | (np.abs(u - np.rint(u)) >= margin)
    return ok


def grid_outside(p):
    ux, uy = _grid_u(p)
    return (ux < 0) | (ux > GRID_NX - 1) | (uy < 0) | (uy > GRID_NY - 1)


def _uniform(n, seed, keep=None):
    rng = np.random.default_rng(seed)
    out = np.zeros((0, 2), np.float32)
    while len(out) < n:
        p = rng.uniform(-BOX, BOX, size=(4 * n, 2)).astype(np.float32)
        out = np.concatenate([out, p if keep is None else p[keep(p)]])
    return out[:n]


SPECIAL = {
    "radial_centre": [RADIAL_CENTRE],
    "origin": [(0.0, 0.0)],
    # closed sets: the edge belongs
    "box_edge": [(IND_BOX[0], 0.0), (IND_BOX[1], 0.5), (0.0, IND_BOX[2]), (0.125, IND_BOX[3]), (IND_BOX[1], IND_BOX[3])],
    "disk_edge": [(IND_DISK_C[0] + IND_DISK_R, IND_DISK_C[1]), (IND_DISK_C[0], IND_DISK_C[1] + IND_DISK_R)],
    "just_outside": [(np.nextafter(np.float32(IND_BOX[1]), np.float32(2)), 0.5),
                     (np.nextafter(np.float32(IND_DISK_C[0] + IND_DISK_R), np.float32(2)), IND_DISK_C[1])],
    "outside_grid": [(1.1, 0.3), (-1.15, -0.6), (0.4, 1.1), (-0.2, -1.15), (1.1, 1.15), (-1.0, 1.05)],
}


def special_points(*names):
    return np.array([p for n in (names or SPECIAL) for p in SPECIAL[n]], np.float32)


def grid_nodes():
    """Every node of the tabulated grid (exact float32 coordinates) and its value."""
    i, j = np.meshgrid(np.arange(GRID_NX), np.arange(GRID_NY), indexing="xy")
    p = np.stack([GRID_X0 + GRID_HX * i.ravel(), GRID_Y0 + GRID_HY * j.ravel()], axis=1)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32), GRID_VALUES[j.ravel(), i.ravel()]


# ---- the saturating alpha's regions -------------------------------------------------------
def _radial_saturation(k, R):
    """wost_device.h radial_saturation, float32 operation by operation."""
    f = np.float32
    k, R = f(k), f(R)
    ak = np.abs(k)
    out_band = f(90.0 if k < 0 else 20.0) / ak
    in_band = f(20.0 if k < 0 else 90.0) / ak
    ho, hi = R + out_band, R - in_band
    m = f(1e-3) * (np.abs(R) + out_band + in_band) + f(1e-30)
    lo2 = (hi - m) * (hi - m) if hi - m > 0 else f(-1.0)
    return lo2, (ho + m) * (ho + m)


def factor_saturation(field, pts):
    """The header's sat_* predicates in numpy float32, every product and sum rounded on its
    own: per factor with a transcendental, (kind name, state [N]) with state 0 in the
    transition band, +1 / -1 saturated (sigmoids: +1 is the value 1, -1 the value 0;
    Gaussians: -1). tests/test_field_zoo.py checks it against the library's own."""
    f = np.float32
    x, y = np.asarray(pts, np.float32)[:, 0], np.asarray(pts, np.float32)[:, 1]
    out = []
    for kind, p in field.pack()[1]:
        p = [f(v) for v in p]
        if kind == F.FK_SIGMOID_RADIAL:
            dx, dy = x - p[1], y - p[2]
            d2 = dx * dx + dy * dy
            lo2, hi2 = _radial_saturation(p[0], p[3])
            s_out = -1 if p[0] < 0 else 1
            out.append(("sat_sigmoid_radial", np.where(d2 >= hi2, s_out, np.where(d2 <= lo2, -s_out, 0))))
        elif kind == F.FK_SIGMOID_LIN:
            z = p[0] * x + p[1] * y + p[2]
            out.append(("sat_sigmoid_lin", np.where(z >= f(21.0), 1, np.where(z <= f(-91.0), -1, 0))))
        elif kind == F.FK_EXP_QUAD:
            dx, dy = x - p[0], y - p[1]
            diag = all(v == 0 for v in p[4:8])
            q = p[2] * (dx * dx) + p[3] * (dy * dy)
            if not diag:
                q = q + p[4] * (dx * dy) + p[5] * dx + p[6] * dy + p[7]
            out.append(("sat_exp_quad_diag" if diag else "sat_exp_quad", np.where(q < f(-111.0), -1, 0)))
    return out


def field_saturated(field, pts):
    """The whole-field predicate of the generated alpha jet: every factor saturated."""
    return np.all([s != 0 for _, s in factor_saturation(field, pts)], axis=0)


SHARP_PER_REGION = 32


@functools.lru_cache(maxsize=None)
def sharp_regions():
    """{region name: points}: for every factor of `sharp` that has a transition band,
    SHARP_PER_REGION points inside that band, and for each of its saturated states
    SHARP_PER_REGION points where the whole field is saturated with the factor in that
    state. (The smooth circle's inner disk d <= 0.2 lies above the line sigmoid's band.)"""
    field = ZOO["sharp"]
    cand = _uniform(60000, SEED + 2)
    # candidates near each centre, where the narrow transition bands are
    rng = np.random.default_rng(SEED + 3)
    for c, r in ((SHARP_C1, 0.6), (SHARP_C2, 0.5), (SHARP_C3, 0.7)):
        cand = np.concatenate([cand, (np.asarray(c) + rng.uniform(-r, r, size=(20000, 2))).astype(np.float32)])
    cand = cand[np.all(np.abs(cand) <= BOX, axis=1)]
    fs = factor_saturation(field, cand)
    whole = np.all([s != 0 for _, s in fs], axis=0)
    regions = {}
    for name, s in fs:
        regions[f"{name}:band"] = cand[s == 0][:SHARP_PER_REGION]
        for state in sorted(set(np.unique(s)) - {0}):
            regions[f"{name}:{'one' if state > 0 else 'zero'}"] = cand[whole & (s == state)][:SHARP_PER_REGION]
    assert len(regions) == 4 + 2 + 2 + 1 + 1, sorted(regions)
    for name, p in regions.items():
        assert len(p) >= SHARP_PER_REGION >= 32, (name, len(p))
    return regions


@functools.lru_cache(maxsize=None)
def points_for(name):
    """The float32 points [N, 2] at which field `name` is compared with the reference."""
    if name == "grid":
        # the node lines and the edge are covered by exact cases of their own (grid_nodes,
        # SPECIAL["outside_grid"]); here every point has an unambiguous derivative
        p = np.concatenate([_uniform(N_UNIFORM, SEED, grid_unambiguous), special_points("outside_grid")])
        p = np.concatenate([p, _uniform(N_POINTS - len(p), SEED + 4, grid_unambiguous)])
        assert np.all(grid_unambiguous(p)) and grid_outside(p).sum() >= 6
        return p
    p = np.concatenate([_uniform(N_UNIFORM, SEED), special_points()])
    p = np.concatenate([p, _uniform(N_POINTS - len(p), SEED + 4)])
    if name == "sharp":   # its regions, the smooth circle's centre (inside the inner band), its peaks
        p = np.concatenate([p] + list(sharp_regions().values())
                           + [np.array([SHARP_C1], np.float32), np.array(SHARP_PEAKS, np.float32)])
    return p


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
def _autograd_jet(field, pts, dtype):
    import torch

    p = torch.tensor(np.asarray(pts, np.float32), dtype=dtype, requires_grad=True)
    with torch.enable_grad():
        v = field(p)
        out = torch.zeros((p.shape[0], 4), dtype=dtype)
        out[:, 0] = v.detach()
        if v.requires_grad:     # (indicators only, or a constant: no differentiable part, zeros)
            g = torch.autograd.grad(v.sum(), p, create_graph=True)[0]
            out[:, 1:3] = g.detach()
            if g.requires_grad:
                for i in range(2):
                    out[:, 3] += torch.autograd.grad(g[:, i].sum(), p, retain_graph=True)[0][:, i]
    return out.numpy().astype(np.float64)


def reference_jet(field, pts):
    """[N, 4] float64 (value, d/dx, d/dy, Laplacian) by float64 torch autograd of field(p),
    p the float32 points cast to float64: the gradient with create_graph=True, the
    Laplacian the trace of the second backward. NaN is kept."""
    import torch

    return _autograd_jet(field, pts, torch.float64)


def float32_jet(field, pts):
    """The same in float32 torch: reference arithmetic only, for e32."""
    import torch

    return _autograd_jet(field, pts, torch.float32)


@functools.lru_cache(maxsize=None)
def reference(name, positive=False):
    """(points, reference jet [N, 4], scale [4], e32 [4], tol [4]) of a zoo field."""
    field = (POSITIVE if positive else ZOO)[name]
    pts = points_for(name)
    ref = reference_jet(field, pts)
    f32 = float32_jet(field, pts)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(f32)), name
    scale = np.array([np.abs(ref[fin[:, c], c]).max() for c in range(4)])
    e32 = np.array([np.abs(f32[fin[:, c], c] - ref[fin[:, c], c]).max() for c in range(4)])
    tol = np.maximum(8.0 * e32, 16.0 * 2.0**-23 * scale)
    for a in (pts, ref, scale, e32, tol):
        a.setflags(write=False)
    return pts, ref, scale, e32, tol


def reference_sigma_prime(alpha_jet, sigma_value, detached):
    """buildModifiedSigma's sigma' (the reference's solvers/WoStSolver.py:80-127 with
    utils.torchLaplacian / torchGradient), written out in float64 from a reference jet of
    alpha [N, 4] and sigma's values [N]:
        alpha_c = clamp(alpha, min=1e-8)        (its derivatives are 0 where it clamps)
        sigma / alpha_c                          (all there is when autograd raises: detached)
        + 0.5 ((1e-8 + lap alpha_c) / alpha_c - |grad log(alpha_c + 1e-8)|^2 / 2)."""
    a = np.asarray(alpha_jet, np.float64)
    s = np.asarray(sigma_value, np.float64)
    eps = 1e-8
    clamped = a[:, 0] < eps
    ac = np.where(clamped, eps, a[:, 0])
    ratio = s / ac
    if detached:
        return ratio
    gx, gy, lap = (np.where(clamped, 0.0, a[:, c]) for c in (1, 2, 3))
    lg2 = (gx / (ac + eps)) ** 2 + (gy / (ac + eps)) ** 2
    return ratio + 0.5 * ((eps + lap) / ac - lg2 / 2.0)


def sigma_prime_tolerance(alpha_jet, alpha_tol, alpha_scale, sigma_value, sigma_tol, sigma_scale, detached):
    """[N] (the module docstring's derivation)."""
    a = np.abs(np.asarray(alpha_jet, np.float64))
    s = np.abs(np.asarray(sigma_value, np.float64))
    av = a[:, 0]
    ta, tgx, tgy, tl = alpha_tol
    r = max(float(np.max(np.asarray(alpha_tol) / np.asarray(alpha_scale))),
            float(sigma_tol / sigma_scale) if sigma_scale > 0 else 0.0)
    g2 = a[:, 1] ** 2 + a[:, 2] ** 2
    major = s / av
    first = sigma_tol / av + s * ta / av**2
    if not detached:
        major = major + 0.5 * (a[:, 3] / av + g2 / (2 * av**2))
        first = first + 0.5 * (tl / av + (a[:, 3] + 1e-8) * ta / av**2 + (a[:, 1] * tgx + a[:, 2] * tgy) / av**2
                               + g2 * ta / av**3)
    return 4.0 * (first + r * major)


@functools.lru_cache(maxsize=None)
def reference_sigma_prime_case(name, sigma_key, detached):
    """(points, reference sigma' [N], tolerance [N]) for alpha = POSITIVE[name] and sigma =
    SIGMAS[sigma_key] at the alpha's points."""
    pts, aref, ascale, _, atol = reference(name, True)
    sigma = SIGMAS[sigma_key]
    if sigma is None:
        sv, stol, sscale = np.zeros(len(pts)), 0.0, 0.0
    else:
        sv = reference_jet(sigma, pts)[:, 0]
        sscale = float(np.abs(sv).max())
        e32 = float(np.abs(float32_jet(sigma, pts)[:, 0] - sv).max())
        stol = max(8.0 * e32, 16.0 * 2.0**-23 * sscale)
        assert stol <= CAP * sscale
    ref = reference_sigma_prime(aref, sv, detached)
    tol = sigma_prime_tolerance(aref, atol, ascale, sv, stol, sscale, detached)
    ref.setflags(write=False)
    tol.setflags(write=False)
    return pts, ref, tol


def compare_sigma_prime(got, name, sigma_key, detached):
    """The largest |got - reference| / tolerance; NaN exactly where the reference is."""
    _, ref, tol = reference_sigma_prime_case(name, sigma_key, detached)
    got = np.asarray(got, np.float64)
    nan = np.isnan(ref)
    what = f"sigma'({name}, sigma={sigma_key}, detached={detached})"
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern differs"
    assert np.all(np.isfinite(got[~nan])), f"{what}: not finite"
    err, t = np.abs(got[~nan] - ref[~nan]), tol[~nan]
    assert np.all(err[t == 0] == 0), f"{what}: not exact where the tolerance is 0 (sigma = 0, detached)"
    return float(np.max(err[t > 0] / t[t > 0], initial=0.0))


# ---------------------------------------------------------------------------
# walk problems on the zoo (tests/test_gpu_field_zoo.py; the oracle's part runs on the host)
# ---------------------------------------------------------------------------
SQUARE = np.array([[-BOX, -BOX], [BOX, -BOX], [BOX, BOX], [-BOX, BOX], [-BOX, -BOX]], np.float32)
NEUMANN_TOP = np.array([[-BOX, BOX], [BOX, BOX]], np.float32)
WALK_POINTS = np.array([[0.1, 0.2], [-0.6, 0.5], [0.7, -0.7], [-0.3, -0.9]], np.float32)
WALKS, MAX_STEPS, EPS, WALK_SEED = 2048, 200, 1e-3, 20261
ROTATION = ("three_factors", "trig_product", "indicators", "grid", "exp_general_det0", "sigmoid_radial_neg")
# sigma_bar per problem, fixed here so that device and oracle walk the same problem: the
# oracle's own estimate (max - min of sigma' over its 50 x 50 grid: 31.5, 6.6, 9.6, 3.5, 17.2,
# 2.7) rounded up; `sharp`: 30 (the grid misses its narrow bands, where sigma' reaches
# thousands), with which a walk moves ~2 / sqrt(30) = 0.37 per step and crosses saturated
# regions and bands alike
SIGMA_BAR = {"rot0": 32.0, "rot1": 8.0, "rot2": 10.0, "rot3": 4.0, "rot4": 18.0, "rot5": 3.0, "sharp": 30.0}


@functools.lru_cache(maxsize=None)
def problems():
    """{name: Scenario}: rot0..rot5 put every zoo field of ROTATION -- together every factor
    kind -- once in every slot (g, f, sigma, alpha; the last two in their positive variants);
    rot1 has a Neumann line on top; `sharp` is the saturating alpha with sigma = 0."""
    from dcrmontecarlo_amd.scenarios import Scenario

    out = {}
    n = len(ROTATION)
    for k in range(n):
        g, f, s, a = (ROTATION[(k + i) % n] for i in range(4))
        out[f"rot{k}"] = Scenario(f"zoo_rot{k}", SQUARE, NEUMANN_TOP if k == 1 else None, g=ZOO[g], f=ZOO[f],
                                  sigma=POSITIVE[s], alpha=POSITIVE[a], points=WALK_POINTS, n_walks=WALKS,
                                  max_steps=MAX_STEPS, eps=EPS)
    out["sharp"] = Scenario("zoo_sharp", SQUARE, None, g=ZOO["mono"], f=ZOO["exp_diag"], sigma=None,
                            alpha=ZOO["sharp"], points=WALK_POINTS, n_walks=WALKS, max_steps=MAX_STEPS, eps=EPS)
    for slot in ("g", "f", "sigma", "alpha"):   # every kind in every slot
        assert set().union(*[kinds_of(getattr(out[f"rot{k}"], slot)) for k in range(n)]) == set(range(1, 10)), slot
    diag = [all(np.float32(v) == 0 for v in p[4:8]) for name in ROTATION for p in _packed_exp(ZOO[name])]
    assert any(diag) and not all(diag)           # both exponential forms
    return out


# The oracle against itself with the step directions 1 ulp apart (oracle_self_agreement below,
# 4 points x 2048 walks), as measured; tests/test_field_zoo.py re-measures it. The floor for
# the device's share of walks identical to the oracle's is that share minus 0.02, and never
# below 0.95: a problem that cannot reach it is chaotic and has to be replaced.
SELF_AGREEMENT = {"rot0": 0.99988, "rot1": 0.99988, "rot2": 0.99988, "rot3": 0.99988, "rot4": 1.0, "rot5": 1.0,
                  "sharp": 1.0}


def floor(name):
    f = SELF_AGREEMENT[name] - 0.02
    assert f >= 0.95, f"{name} is chaotic: replace the problem"
    return f


def oracle_self_agreement(name, perturbation=1.2e-7):
    """The share of the problem's walks that keep their step count and their value within
    1e-3 |v| + 1e-5 scale when the oracle's step directions move by 1 ulp
    (tests/test_oracle_golden.py test_walk_sensitivity_to_one_ulp)."""
    from oracle import oracle as O

    sc = problems()[name]
    pb = O.Problem.from_scenario(sc, sigma_bar=SIGMA_BAR[name])
    v0, s0 = pb.solve_walks(sc.points, sc.n_walks, sc.max_steps, sc.eps, WALK_SEED)
    try:
        O.set_direction_perturbation(perturbation)
        v1, s1 = pb.solve_walks(sc.points, sc.n_walks, sc.max_steps, sc.eps, WALK_SEED)
    finally:
        O.set_direction_perturbation(0.0)
    scale = max(float(np.abs(v0).max()), 1e-30)
    return float(np.mean((s0 == s1) & (np.abs(v1 - v0) <= 1e-3 * np.abs(v0) + 1e-5 * scale)))


def check_zoo():
    """The conditions on the inputs: every alpha >= 0.3 on its points, every tolerance
    within the cap."""
    for name in ZOO:
        for positive in (False, True):
            pts, ref, scale, e32, tol = reference(name, positive)
            assert np.all(tol <= CAP * scale), (name, positive, (tol / scale).tolist())
            if positive:
                v = ref[:, 0]
                assert np.nanmin(v) >= 0.3, (name, float(np.nanmin(v)))


check_zoo()


def compare(got, name, positive=False, what=""):
    """The largest |got - reference| / tol per component of field `name` (got: [N, 4]);
    NaN exactly where the reference is NaN, finite where it is finite."""
    pts, ref, scale, e32, tol = reference(name, positive)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape
    ratios = np.zeros(4)
    for c in range(4):
        nan = np.isnan(ref[:, c])
        assert np.array_equal(np.isnan(got[:, c]), nan), f"{what}{name}.{COMPONENTS[c]}: NaN pattern differs"
        assert np.all(np.isfinite(got[~nan, c])), f"{what}{name}.{COMPONENTS[c]}: not finite"
        if (~nan).any():
            ratios[c] = float(np.max(np.abs(got[~nan, c] - ref[~nan, c]) / tol[c]))
    return ratios
