"""Option flat_sigma_prime (the walk's sigma' shortcut at a flat alpha jet, wost_device.h
flat_alpha_min) changes how the sigma = 0 kernels run, never what they compute: with the
option on and off, per-walk values and step counts are the same bits, seeds fixed.

The cases are the kernels that share walk_body's two delta branches -- reference mode, the
tree kernel, compat="fixed", a multi-source kernel -- on fields where the per-lane guard
decides differently: C4 (alpha 10 .. 1000, every saturated lane trivial), the notebook's
field (alpha 1e-3 .. 1e-2 with 1/sigma_bar of its own), its air term (alpha ~ 1e-8: the
full path), and a C4-like field whose background alpha is the float just below and just
above the bound."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _both(make, solve):
    """solve(solver) with the option on and off -> the two results."""
    out = []
    for flat in (1, 0):
        s = make()
        s.set_option("flat_sigma_prime", flat)
        assert s.get_option("flat_sigma_prime") == flat
        r = solve(s)
        assert s.last_timing["jit"] == 1
        assert s.options_report()["non_default"].get("flat_sigma_prime") == (None if flat else 0)
        out.append(r)
    return out


def _same_bits(a, b):
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


CASES = {
    # name: (scenario, its keyword arguments, points, walks, seed, tree kernel)
    "dcr_dipole": ("dcr_dipole", {}, lambda p: p[20:24], 4096, 7, 0),
    "notebook_dcr": ("notebook_dcr", {}, lambda p: p, 1024, 9, 0),
    "wenner_topography": ("wenner_topography", {}, lambda p: p[::32], 256, 10, 1),
}


@pytest.mark.parametrize("case", list(CASES))
def test_walks_do_not_depend_on_the_option(gpu_available, case):
    from dcrmontecarlo_amd import scenarios as S

    name, kw, pick, W, seed, tree = CASES[case]
    sc = S.ALL[name](**kw)
    pts = pick(sc.points)
    assert len(pts) == {"dcr_dipole": 4, "notebook_dcr": 21, "wenner_topography": 8}[case]

    def solve(s):
        v, st = s.solve_walks(pts, nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=seed)
        assert s.last_timing["tree"] == tree
        return v, st

    on, off = _both(lambda: sc.solver(device=0), solve)
    assert on[1].mean() > 5            # the walks step (and collide)
    _same_bits(on, off)


def test_fixed_delta_walks_do_not_depend_on_the_option(gpu_available):
    from dcrmontecarlo_amd import scenarios as S

    sc = S.dcr_dipole(n_electrodes=48, n_walks=1)
    pts = sc.points[20:24]

    def make():
        s = sc.solver(device=0, compat="fixed")
        s.set_fixed_step_check(False)   # (its walks end at maxSteps: every step a collision test)
        return s

    on, off = _both(make, lambda s: s.solve_walks(pts, nWalks=1024, maxSteps=200, eps=sc.eps, seed=23))
    _same_bits(on, off)


def test_multi_source_walks_do_not_depend_on_the_option(gpu_available):
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey

    sc = S.dcr_dipole(n_electrodes=48, n_walks=1)
    pts = sc.points[:5]
    srcs = [survey.electrode_source((-60.0 + 40.0 * k, 0.0), 7.0, current=1.0 + k) for k in range(3)]
    on, off = _both(lambda: sc.solver(device=0),
                    lambda s: s.solve_sources_walks(pts, srcs, nWalks=3000, maxSteps=sc.max_steps, eps=sc.eps, seed=23))
    assert on[0].shape == (3, 5, 3000)
    _same_bits(on, off)


@pytest.mark.parametrize("side", ["below", "above"])
def test_background_alpha_next_to_the_bound(gpu_available, side):
    """C4's geometry and source with alpha scaled so that the saturated background is the
    float just below (no background lane is trivial) or just above (all are) the bound
    0.1678f * (1 / sigma_bar); sigma' does not depend on alpha's scale, so sigma_bar = 10."""
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd import scenarios as S

    sc = S.dcr_dipole(n_electrodes=48, n_walks=1)
    amin = np.float32(0.1678) * np.float32(1.0 / 10.0)
    bg = float(np.nextafter(amin, np.float32(0.0 if side == "below" else 1.0), dtype=np.float32))
    assert (np.float32(bg) < amin) if side == "below" else (np.float32(bg) > amin)
    sc.alpha = (bg + (0.1 * bg - bg) * F.smooth_circle((-20.0, -30.0), 10.0)
                + (10.0 * bg - bg) * F.smooth_circle((25.0, -40.0), 10.0))
    pts = sc.points[[16, 30]]

    def make():
        s = sc.solver(device=0, sigma_bar=10.0)
        assert s.sigma_bar == 10.0
        return s

    on, off = _both(make, lambda s: s.solve_walks(pts, nWalks=2048, maxSteps=sc.max_steps, eps=sc.eps, seed=31))
    assert on[1].mean() > 5
    _same_bits(on, off)
