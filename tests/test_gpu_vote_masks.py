"""The walk loop's wave votes on scalar lane masks (wost_walk.h `live`, wost_device.h WaveMask)
where they can go wrong: waves with idle lanes, waves that are never full, a last partial
refill, and walks that finish without a step. Every case draws the CPU oracle's walks on the
same Philox streams and is compared the way tests/test_gpu_parity.py compares them: a walk
agrees when its step count is the oracle's and its value is within 1e-3 relative (1e-5 of the
scale absolute), and the share of agreeing walks must reach the scenario's floor
(test_oracle_golden.AGREEMENT_FLOOR; 0.99 for the tree kernel, as tests/test_gpu_c5.py). With
one walk, or with walks that take no step, that is every walk.

An error in the loop's exit vote would be a hang, not a wrong number: run this file before the
rest of the GPU suite, under a time limit of its own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 31337


def _solver(name):
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd.geometry import PolyLinesSimple
    from dcrmontecarlo_amd.solvers import WostSolver_2D

    sc = S.ALL[name]()
    return sc, WostSolver_2D(PolyLinesSimple(sc.dirichlet), sc.g, PolyLinesSimple(sc.neumann) if sc.neumann is not None
                             else None, source=sc.f, sigma=sc.sigma, alpha=sc.alpha)


def _oracle(sc, s, pts, W, max_steps, eps):
    from oracle import oracle as O

    pb = O.Problem.from_scenario(sc, sigma_bar=s.sigma_bar or 0.0)
    return pb.solve_walks(pts, W, max_steps, eps, SEED)


def _agreement(gv, gs, ov, os_):
    gv, gs = gv.ravel(), gs.ravel()
    scale = max(float(np.abs(ov).max()), 1e-30)
    same = (gs == os_) & (np.abs(gv - ov) <= 1e-3 * np.abs(ov) + 1e-5 * scale)
    print(f"{same.sum()} of {same.size} walks agree; steps equal on {(gs == os_).sum()}; total steps {int(gs.sum())}")
    return same


def _dcr():
    # (a solver per test: tests/conftest.py makes each one compile its kernel before its first
    # solve; the kernel cache makes the later ones cheap)
    return _solver("dcr_dipole")


@pytest.mark.parametrize("npts,W", [(1, 1), (3, 37), (5, 129)])
def test_sparse_waves_match_oracle(gpu_available, npts, W):
    """One lane of one wave; a wave that is never full; a last partial refill."""
    from test_oracle_golden import AGREEMENT_FLOOR

    sc, s = _dcr()
    pts = sc.points[16:16 + npts]
    gv, gs = s.solve_walks(pts, nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    assert s.last_timing["jit"] == 1
    ov, os_ = _oracle(sc, s, pts, W, sc.max_steps, sc.eps)
    assert gv.shape == (npts, W) and np.all(np.isfinite(gv))
    assert _agreement(gv, gs, ov, os_).mean() >= AGREEMENT_FLOOR["dcr_dipole"]


@pytest.mark.parametrize("kw", [dict(max_steps=0), dict(eps=1.0), dict(eps=2.5)], ids=["maxSteps0", "eps1", "eps2.5"])
def test_walks_without_a_step_finish_at_the_next_iteration(gpu_available, kw):
    """A freshly refilled walk that already fails the while-condition takes no step: every lane of
    every wave is refilled and finished in turn, 2 x 4096 times."""
    sc, s = _dcr()
    pts = sc.points[16:18]
    W = 4096
    max_steps, eps = kw.get("max_steps", sc.max_steps), kw.get("eps", sc.eps)
    gv, gs = s.solve_walks(pts, nWalks=W, maxSteps=max_steps, eps=eps, seed=SEED)
    ov, os_ = _oracle(sc, s, pts, W, max_steps, eps)
    assert np.all(os_ == 0)
    same = _agreement(gv, gs, ov, os_)
    assert np.all(gs == 0) and same.all()


def test_precompiled_kernel_matches_oracle(gpu_available):
    """The interpreted path (wost_kernels.hip) shares the loop."""
    from test_oracle_golden import AGREEMENT_FLOOR

    sc, s = _dcr()
    s.set_jit(False)
    pts = sc.points[16:21]
    W = 129
    gv, gs = s.solve_walks(pts, nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    assert s.last_timing["jit"] == 0
    ov, os_ = _oracle(sc, s, pts, W, sc.max_steps, sc.eps)
    assert _agreement(gv, gs, ov, os_).mean() >= AGREEMENT_FLOOR["dcr_dipole"]


def test_variable_coefficients_matches_oracle(gpu_available):
    """C3: the collision branch's votes always enter their slow side (sigma != 0, detached alpha)."""
    from test_oracle_golden import AGREEMENT_FLOOR

    sc, s = _solver("variable_coefficients")
    pts = sc.points[:3]
    W = 300
    gv, gs = s.solve_walks(pts, nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    assert s.last_timing["jit"] == 1
    ov, os_ = _oracle(sc, s, pts, W, sc.max_steps, sc.eps)
    assert _agreement(gv, gs, ov, os_).mean() >= AGREEMENT_FLOOR["variable_coefficients"]


def test_tree_kernel_with_pools_matches_oracle(gpu_available):
    """C5's tree kernel: the walk pools' exchanges and the cooperative tree queries, in waves that
    are never full (3 electrodes x 150 walks)."""
    from oracle import oracle as O
    from dcrmontecarlo_amd import scenarios as S

    sc = S.wenner_topography()
    s = sc.solver(device=0)
    pts = sc.points[4::32][:3]
    W = 150
    gv, gs = s.solve_walks(pts, nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    assert s.last_timing["tree"] == 1 and s.last_timing["jit"] == 1
    sb = O.Problem.from_scenario(sc).sigma_bar()
    assert s.sigma_bar == pytest.approx(sb, rel=1e-5)
    ov, os_ = O.Problem.from_scenario(sc, sigma_bar=sb).solve_walks(pts, W, sc.max_steps, sc.eps, SEED)
    assert _agreement(gv, gs, ov, os_).mean() >= 0.99
