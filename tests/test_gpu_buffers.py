"""A handle's device buffers (wost_handle.h DeviceBuffer) across growth and reuse: one handle
solves a small size, a larger one (every per-solve buffer grows: the staging, the per-walk
workspace, the block sums, the query points' alpha under delta tracking, the walk pools of
the tree kernel), then the small size again (the grown buffers are reused). Each result
must equal, bit for bit, a fresh handle's solve of that size with the same seed."""
import numpy as np
import pytest

from dcrmontecarlo_amd import scenarios as S

pytestmark = pytest.mark.gpu

SIZES = [(4, 64), (64, 256), (4, 64)]   # (points, walks per point), in turn on one handle
SEED = 20


def _solver(sc):
    s = sc.solver(device=0)
    s.set_option("jit_race", 0)   # (as tests/conftest.py: the kernel compiled before the first solve)
    return s


def _walks(s, sc, n, W):
    pts = np.resize(sc.points, (n, 2)).astype(np.float32)
    v, st = s.solve_walks(pts, nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    return np.asarray(v).view(np.uint32).copy(), np.asarray(st).copy()


# variable_coefficients: delta tracking (the point-alpha buffer); wenner_topography: the
# segment tree (the walk pools)
@pytest.mark.parametrize("name", ["variable_coefficients", "wenner_topography"])
def test_buffers_grow_and_are_reused(name):
    sc = S.ALL[name]()
    fresh = {size: _walks(_solver(sc), sc, *size) for size in set(SIZES)}
    s = _solver(sc)
    for k, size in enumerate(SIZES):
        v, st = _walks(s, sc, *size)
        assert v.size == size[0] * size[1]
        assert np.array_equal(v, fresh[size][0]), f"{name}: solve {k} {size}: values differ from a fresh handle's"
        assert np.array_equal(st, fresh[size][1]), f"{name}: solve {k} {size}: steps differ from a fresh handle's"
    t = s.last_timing
    assert t["jit"] == 1
    assert t["tree"] == (1 if name == "wenner_topography" else 0)
