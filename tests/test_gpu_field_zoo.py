"""The field zoo on the device (tests/field_zoo.py: the fields, their float64 autograd
reference and the tolerances).

a. eval_field -- the interpreter on the device, with v_exp / v_rcp / v_rsq / v_sin / v_cos in
   place of libm -- against the reference, every zoo field in every slot, and sigma'.
b. The field-specialised (generated) kernel against the interpreting one on zoo problems, bit
   for bit, with the saturating alpha's shortcuts on and off and as one of two models.
c. The device against the CPU oracle on the same problems.
d. param_sources with every factor kind.

Measured on an MI355X, largest |error| / tolerance over the four jet components (a):
MEASURED_JET_RATIO below; sigma': MEASURED_SIGMA_PRIME_RATIO. The oracle's agreement with
itself under a 1-ulp change of the step directions (c), measured on the host, and the floors
derived from it (share - 0.02, never below 0.95): field_zoo.SELF_AGREEMENT / floor(), kept
honest by tests/test_field_zoo.py.
"""
import dataclasses

import numpy as np
import pytest

import field_zoo as Z

pytestmark = pytest.mark.gpu

# (a) largest error / tolerance per field over slots g, f, sigma, alpha and the four
# components, as printed by test_eval_field_matches_the_reference on an MI355X
MEASURED_JET_RATIO = {"mono": 0.059, "exp_general": 0.069, "exp_general_det0": 0.101, "exp_diag": 0.073,
                      "exp_linear": 0.050, "trig_product": 0.257, "sigmoid_lin": 0.123, "sigmoid_radial_neg": 0.116,
                      "sigmoid_radial_pos": 0.130, "three_factors": 0.120, "indicators": 0.086, "grid": 0.117,
                      "sharp": 0.125}
# ... and of sigma' over sigma in {0, trig_product + 2} and detached in {False, True}
MEASURED_SIGMA_PRIME_RATIO = {"mono": 0.008, "exp_general": 0.009, "exp_general_det0": 0.008, "exp_diag": 0.009,
                              "exp_linear": 0.011, "trig_product": 0.022, "sigmoid_lin": 0.023,
                              "sigmoid_radial_neg": 0.014, "sigmoid_radial_pos": 0.014, "three_factors": 0.018,
                              "indicators": 0.008, "grid": 0.020, "sharp": 0.023}
# (c) the device's share of walks identical to the oracle's, as printed by
# test_device_matches_the_oracle on an MI355X (the floors: field_zoo.SELF_AGREEMENT - 0.02)
MEASURED_ORACLE_SHARE = {"rot0": 0.99988, "rot1": 0.99988, "rot2": 1.0, "rot3": 1.0, "rot4": 1.0, "rot5": 1.0,
                         "sharp": 0.99988}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _solver(**fields):
    from dcrmontecarlo_amd.geometry import PolyLinesSimple
    from dcrmontecarlo_amd.solvers import WostSolver_2D

    return WostSolver_2D(PolyLinesSimple(Z.SQUARE), fields.get("g"), None, source=fields.get("f"),
                         sigma=fields.get("sigma"), alpha=fields.get("alpha"), sigma_bar=1.0)


# ---- a. eval_field ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Z.ZOO))
def test_eval_field_matches_the_reference(gpu_available, name):
    from dcrmontecarlo_amd import fields as F

    field = Z.ZOO[name]
    pts = Z.points_for(name)
    s = _solver(g=field, f=field, sigma=field, alpha=field)
    worst = np.zeros(4)
    for slot in ("g", "f", "sigma", "alpha"):
        got = s.eval_field(slot, pts)                     # one launch of the field's ~300 points
        ratios = Z.compare(got, name, what=f"slot {slot}: ")
        worst = np.maximum(worst, ratios)
    print(f"{name}: largest error / tolerance per component {np.round(worst, 3)} -> {worst.max():.3f}")
    sp_worst = 0.0
    alpha = Z.POSITIVE[name]
    for sigma_key, sigma in Z.SIGMAS.items():
        for detached in (False, True):
            sp = _solver(sigma=sigma, alpha=F.detach(alpha) if detached else alpha)
            out = sp.eval_field("sigma_prime", pts)
            ratio = Z.compare_sigma_prime(out[:, 0], name, sigma_key, detached)
            sp_worst = max(sp_worst, ratio)
            # the other columns: alpha's and sigma's values as the slots give them
            np.testing.assert_array_equal(_bits(out[:, 1]), _bits(sp.eval_field("alpha", pts)[:, 0]))
            if sigma is not None:
                np.testing.assert_array_equal(_bits(out[:, 2]), _bits(sp.eval_field("sigma", pts)[:, 0]))
    print(f"{name}: sigma' largest error / tolerance {sp_worst:.3f}")
    assert np.all(worst <= 1.0), worst
    assert sp_worst <= 1.0


def test_eval_field_grid_nodes_and_outside(gpu_available):
    tab = Z._tab()
    s = _solver(g=tab)
    nodes, values = Z.grid_nodes()
    np.testing.assert_array_equal(s.eval_field("g", nodes)[:, 0], values)
    out = Z.special_points("outside_grid")
    j = s.eval_field("g", out)
    outx, outy = np.abs(out[:, 0]) > 0.9375, np.abs(out[:, 1]) > 1.0
    assert np.all(j[outx, 1] == 0) and np.all(j[outy, 2] == 0) and np.all(j[outx & outy, 3] == 0)
    assert outx.any() and outy.any() and (outx & outy).any()


# ---- b. generated code = interpreter ---------------------------------------------------------
def _walks(name, jit=True, **kw):
    sc = Z.problems()[name]
    s = sc.solver(sigma_bar=Z.SIGMA_BAR[name])
    for k, v in kw.items():
        s.set_option(k, v)
    s.set_jit(jit)
    v, st = s.solve_walks(sc.points, nWalks=sc.n_walks, maxSteps=sc.max_steps, eps=sc.eps, seed=Z.WALK_SEED)
    assert s.last_timing["jit"] == (1 if jit else 0)
    return s, v, st


@pytest.mark.parametrize("name", list(Z.SIGMA_BAR))
def test_generated_kernel_equals_the_interpreter(gpu_available, name):
    s, v1, s1 = _walks(name, jit=True)
    _, v0, s0 = _walks(name, jit=False)
    print(f"{name}: mean steps {s1.mean():.1f}, {np.count_nonzero(v1)} non-zero values of {v1.size}, "
          f"tree {s.last_timing['tree']}")
    assert np.count_nonzero(v1) > 0 and np.all(np.isfinite(v1))
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(_bits(v1), _bits(v0))
    if name == "rot1":      # the Neumann line: walks did reflect (a walk that ends on the top would stop there)
        assert s.neumannBoundary is not None
        _, hist = s.solve(Z.WALK_POINTS, nWalks=16, maxSteps=Z.MAX_STEPS, eps=Z.EPS, seed=Z.WALK_SEED,
                          return_history=True)
        near = [float(np.asarray(st["point"], np.float32).ravel()[1]) > Z.BOX - 0.05
                for i in range(len(Z.WALK_POINTS)) for w in hist[i] for st in w["path"][1:]]
        # steps that start next to the Neumann line, where a Dirichlet side would have ended the walk
        # (the oracle's 64 walks have 59 such steps)
        assert sum(near) >= 16


def test_sharp_alpha_shortcuts_on_off_and_as_a_model(gpu_available):
    """The saturating alpha with sigma = 0: the kernel carries the whole-field saturated return
    and the flat-sigma' shortcut. Option flat_sigma_prime = 0 gives the same bits, and so does
    the alpha as model 1 of two (alpha_jet_m1) against a handle created with it."""
    sc = Z.problems()["sharp"]
    src = sc.kernel_source(sigma_bar=Z.SIGMA_BAR["sharp"])
    assert "#define WOST_FLAT_SIGMA_PRIME 1" in src and "WOST_SAT_ALL(sat)" in src
    s, v1, s1 = _walks("sharp")
    _, v0, s0 = _walks("sharp", flat_sigma_prime=0)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(_bits(v1), _bits(v0))
    models = [(None, Z.POSITIVE["three_factors"]), (None, Z.ZOO["sharp"])]
    assert "alpha_jet_m1" in sc.kernel_source(sigma_bar=Z.SIGMA_BAR["sharp"], models=models)
    kw = dict(nWalks=sc.n_walks, maxSteps=sc.max_steps, eps=sc.eps, seed=Z.WALK_SEED)
    vals, steps = s.solve_models_walks(sc.points, models, **kw)
    assert vals.shape == (2, len(sc.points), sc.n_walks) and s.last_timing["jit"] == 1
    for m, model in enumerate(models):
        one = dataclasses.replace(sc, sigma=model[0], alpha=model[1]).solver(sigma_bar=Z.SIGMA_BAR["sharp"])
        wv, ws = one.solve_walks(sc.points, **kw)
        np.testing.assert_array_equal(steps, ws, err_msg=f"model {m}")
        np.testing.assert_array_equal(_bits(vals[m]), _bits(wv), err_msg=f"model {m}")
    np.testing.assert_array_equal(_bits(vals[1]), _bits(v1))


def test_sharp_walks_visit_saturated_regions_and_bands(gpu_available):
    """A problem whose walks never leave one side of the whole-field predicate proves nothing
    about the wave vote: of the recorded step positions of 64 walks at least 5% are
    saturated and at least 5% are not. Measured on an MI355X: 1238 step positions, 20.8%
    saturated."""
    sc = Z.problems()["sharp"]
    s = sc.solver(sigma_bar=Z.SIGMA_BAR["sharp"])
    _, hist = s.solve(sc.points, nWalks=16, maxSteps=sc.max_steps, eps=sc.eps, seed=Z.WALK_SEED, return_history=True)
    walks = [w for i in range(len(sc.points)) for w in hist[i]]
    assert len(walks) == 64
    pos = np.array([np.asarray(st["point"], np.float32) for w in walks for st in w["path"]]).reshape(-1, 2)
    sat = Z.field_saturated(Z.ZOO["sharp"], pos)
    print(f"sharp: {len(pos)} step positions of 64 walks, {sat.mean():.3f} saturated")
    assert len(pos) >= 640 and 0.05 <= sat.mean() <= 0.95


# ---- c. device against the oracle ------------------------------------------------------------
@pytest.mark.parametrize("name", list(Z.SIGMA_BAR))
def test_device_matches_the_oracle(gpu_available, name):
    """As test_gpu_parity.test_device_matches_oracle: the same step count and the value within
    1e-3 |v| + 1e-5 scale for at least Z.floor(name) of the walks. Measured shares of identical
    walks on an MI355X: MEASURED_ORACLE_SHARE."""
    from oracle import oracle as O

    sc = Z.problems()[name]
    s, gv, gs = _walks(name)
    assert s.sigma_bar == Z.SIGMA_BAR[name]
    pb = O.Problem.from_scenario(sc, sigma_bar=s.sigma_bar)
    ov, os_ = pb.solve_walks(sc.points, sc.n_walks, sc.max_steps, sc.eps, Z.WALK_SEED)
    gv, gs = gv.ravel(), gs.ravel()
    scale = max(float(np.abs(ov).max()), 1e-30)
    same = (gs == os_) & (np.abs(gv - ov) <= 1e-3 * np.abs(ov) + 1e-5 * scale)
    print(f"{name}: {same.mean():.5f} of the walks identical to the oracle's (floor {Z.floor(name):.5f}), "
          f"{np.mean(gs == os_):.5f} with its step count")
    assert same.mean() >= Z.floor(name)
    W = sc.n_walks
    om = ov.astype(np.float64).reshape(-1, W).mean(1)
    ose = ov.astype(np.float64).reshape(-1, W).std(1, ddof=1) / np.sqrt(W)
    assert np.all(np.abs(gv.astype(np.float64).reshape(-1, W).mean(1) - om) <= 0.5 * ose + 1e-6 * scale)


# ---- d. param_sources with every kind --------------------------------------------------------
def _zoo_sources():
    return [Z.ZOO["trig_product"], Z.ZOO["three_factors"], Z.ZOO["indicators"] + Z.ZOO["grid"],
            Z.ZOO["exp_general"] + Z.ZOO["sigmoid_radial_pos"]]


def test_param_sources_with_every_kind(gpu_available):
    """Sources that together hold every factor kind, scored by one set of walks with their
    parameters compiled in (param_sources 0) and read from the program buffer (1): the same
    bits, and each source the bits of its single-source solve."""
    srcs = _zoo_sources()
    assert set().union(*[Z.kinds_of(f) for f in srcs]) == set(range(1, 10))
    sc = Z.problems()["rot0"]
    pts = sc.points[:3]
    kw = dict(nWalks=2048, maxSteps=sc.max_steps, eps=sc.eps, seed=Z.WALK_SEED)
    res = {}
    for param in (0, 1):
        s = sc.solver(sigma_bar=Z.SIGMA_BAR["rot0"])
        s.set_option("param_sources", param)
        res[param] = s.solve_sources_walks(pts, srcs, **kw)
        assert res[param][0].shape == (len(srcs), 3, 2048) and s.last_timing["jit"] == 1
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(_bits(res[0][0]), _bits(res[1][0]))
    one = sc.solver(sigma_bar=Z.SIGMA_BAR["rot0"])
    for k, f in enumerate(srcs):
        one.setSourceTerm(f)
        v, st = one.solve_walks(pts, **kw)
        assert np.count_nonzero(v) > 0
        np.testing.assert_array_equal(res[1][1], st, err_msg=f"source {k}")
        np.testing.assert_array_equal(_bits(res[1][0][k]), _bits(v), err_msg=f"source {k}")


def test_param_sources_compile_one_kernel_per_structure(gpu_available, monkeypatch, tmp_path):
    """Two source lists of equal structure and different parameters: with param_sources = 1
    the second solve finds the first one's kernel (last_timing["jit_ms"] == 0: nothing was
    compiled), with param_sources = 0 it compiles its own (jit_ms > 0). jit_ms is 0 on a hit in
    the process's memory cache or in the disk cache, so the test has a disk cache of its own,
    empty at its start, and draws its parameters afresh (the seed is printed), so that the
    memory cache cannot hold a param_sources = 0 kernel of these parameters either. Nothing is
    asserted about the first solve's compile: with param_sources = 1 its text holds no
    parameter, and an earlier test of the process may have compiled it."""
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd.fields import X, Y

    monkeypatch.setenv("WOST_JIT_CACHE", str(tmp_path))
    seed = int(np.random.SeedSequence().entropy % 2**32)
    print(f"parameter seed {seed}")
    rng = np.random.default_rng(seed)

    def sources():
        a, b, c = rng.uniform(0.5, 1.5, 3)
        return [F.sin(a * X + b * Y + c) * F.cos(b * X - a * Y) * X**2,
                F.exp(-a * X**2 - b * Y**2 + 0.5 * c * X * Y + 0.1 * X) * F.sigmoid(a * Y) * Y
                + F.sigmoid_radial(-4.0 * a, (0.1 * b, 0.2 * c), 0.5 + 0.1 * a)]

    sc = Z.problems()["rot0"]
    pts = sc.points[:2]
    kw = dict(nWalks=256, maxSteps=sc.max_steps, eps=sc.eps, seed=Z.WALK_SEED)
    jit_ms = {}
    for param in (1, 0):
        s = sc.solver(sigma_bar=Z.SIGMA_BAR["rot0"])
        s.set_option("param_sources", param)
        first, second = sources(), sources()
        s.solve_sources(pts, first, **kw)
        assert s.last_timing["jit"] == 1
        u = s.solve_sources(pts, second, **kw)
        jit_ms[param] = s.last_timing["jit_ms"]
        assert s.last_timing["jit"] == 1
        # (and the kernel that was found scores the second list: each source its single solve)
        one = sc.solver(sigma_bar=Z.SIGMA_BAR["rot0"])
        for k, f in enumerate(second):
            one.setSourceTerm(f)
            np.testing.assert_array_equal(_bits(u[k]), _bits(np.asarray(one.solve(pts, **kw)).ravel()))
    print(f"second list's compile time: param_sources=1 {jit_ms[1]:.1f} ms, param_sources=0 {jit_ms[0]:.1f} ms")
    assert jit_ms[1] == 0.0 and jit_ms[0] > 0.0
