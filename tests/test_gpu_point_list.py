"""Walk ranges over a subset of the points on the device (wost_solve_range_points,
WostSolver_2D.solve_range(point_ids=...)). The listed points keep the ids they
have in the solve of all points: the point-list kernel reads pid = point_list[range_point0 +
q] where the range path computes range_point0 + q, and everything indexed by the point --
the walk id and its Philox stream, points, point_alpha (every model's row), point_code --
follows the true id, while outputs follow the launch's local index.

* zero-step walks return g(x0) = x0.x, so every walk names its point: a list of every third
  point plus the last, in one launch and across launches (range_point0 > 0);
* list rows are bitwise the full range's rows of the listed points -- block rows, per-walk
  values and steps -- for a list with gaps, a single point and all points, with one channel,
  3 sources, 2 models, point charges (surface points, compat="fixed"), the tree kernel with
  its walk pools, and ids beyond 2^40;
* a plain solve_range afterwards keeps its bits; bad lists and a disabled kernel refuse.

Shapes: ranges of 2 blocks (8192 walks), 3 to 8 points, maxSteps 200 on the DCR box.
tests/test_point_list_plan.py checks the same id arithmetic on the host."""
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 4096   # WOST_BLOCK_WALKS
SEED = 29
STEPS = 200


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _range(s, pts, W, w0, w1, ids=None, **kw):
    """(block rows [rows, blocks, 2C+1], values [rows, w1 - w0, C], steps [rows, w1 - w0])."""
    rows = len(pts) if ids is None else len(ids)
    C = s.num_channels()
    v = np.full((rows, w1 - w0, C), np.nan, np.float32)
    k = np.full((rows, w1 - w0), 0xFFFFFFFF, np.uint32)
    r = s.solve_range(pts, W, w0, w1, point_ids=ids, walk_values=v, walk_steps=k, **kw)
    return r, v, k


def _check_lists(s, pts, W, w0, w1, lists, what, **kw):
    """Every list's outputs are bitwise the listed rows of the range without a list; then the
    range without a list again (after the list solves) keeps its bits."""
    full = _range(s, pts, W, w0, w1, **kw)
    assert s.last_timing["jit"] == 1
    assert np.isfinite(full[1]).all() and full[2].max() != 0xFFFFFFFF
    assert full[0].shape[1] == -(-(w1 - w0) // B)
    assert np.any(full[1] != 0), f"{what}: every walk scored 0, nothing to compare"
    for ids in lists:
        got = _range(s, pts, W, w0, w1, ids=np.asarray(ids), **kw)
        assert s.last_timing["jit"] == 1 and s.last_timing["total_walks"] == len(ids) * (w1 - w0)
        np.testing.assert_array_equal(got[0], full[0][ids], err_msg=f"{what}, list {ids}: block rows")
        np.testing.assert_array_equal(_bits(got[1]), _bits(full[1][ids]), err_msg=f"{what}, list {ids}: values")
        np.testing.assert_array_equal(got[2], full[2][ids], err_msg=f"{what}, list {ids}: steps")
    again = _range(s, pts, W, w0, w1, **kw)
    for a, b, name in zip(again, full, ("block rows", "values", "steps")):
        np.testing.assert_array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b,
                                      err_msg=f"{what}: plain range after the list solves, {name}")
    return full


# ---------------------------------------------------------------- zero-step walks name their point
N_MAP = 70_000


def _map_points(n):
    x = ((np.arange(n) + 1) * 2.0 ** -17).astype(np.float32)   # exact in float32, all distinct
    return np.stack([x, np.full(n, 0.5, np.float32)], axis=1)


@functools.lru_cache(maxsize=None)
def _map_solver():
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd.geometry import PolyLinesSimple
    from dcrmontecarlo_amd.solvers import WostSolver_2D

    sq = PolyLinesSimple(np.array([[0, 0], [1, 0], [1, 1], [0, 1], [0, 0]], np.float32))
    return WostSolver_2D(sq, F.X, device=0)


def _map_list():
    return np.concatenate([np.arange(1, N_MAP, 3), [N_MAP - 1]]).astype(np.int32)


def test_zero_step_walks_name_their_point(gpu_available):
    """maxSteps = 0: a walk returns g(x0) = x0.x. Walks [4096, 4096 + 49) of every third point
    and the last: local index l is walk l % 49 of the point at list position l / 49, and
    49 equal float32 values add exactly in double."""
    s, pts, ids = _map_solver(), _map_points(N_MAP), _map_list()
    assert ids[0] == 1 and ids[-1] == N_MAP - 1 and ids[-2] == N_MAP - 3 and len(ids) == 23_334
    rows = s.solve_range(pts, B + 49, B, B + 49, maxSteps=0, seed=5, point_ids=ids)
    assert rows.shape == (len(ids), 1, 3) and s.last_timing["jit"] == 1
    np.testing.assert_array_equal(rows[:, 0, 0], 49.0 * pts[ids, 0].astype(np.float64))
    assert not rows[:, 0, 2].any()


def test_zero_step_walks_name_their_point_across_launches(gpu_available):
    """The same list with a range of 4096 walks: 9.6e7 zero-step walks, more than one launch
    holds (2^26), so the later launches start at a list position range_point0 > 0."""
    s, pts, ids = _map_solver(), _map_points(N_MAP), _map_list()
    rows = s.solve_range(pts, 2 * B, B, 2 * B, maxSteps=0, seed=5, point_ids=ids)
    assert rows.shape == (len(ids), 1, 3)
    assert s.last_timing["n_launches"] >= 2 and s.last_timing["total_walks"] == len(ids) * B
    np.testing.assert_array_equal(rows[:, 0, 0], float(B) * pts[ids, 0].astype(np.float64))
    assert not rows[:, 0, 2].any()


# ---------------------------------------------------------------- list rows = the full range's rows
LISTS6 = ([0, 2, 5], [3], [0, 1, 2, 3, 4, 5])


@functools.lru_cache(maxsize=None)
def _dd():
    """dcr_dipole's first 6 electrodes with a transmitter dipole at two of them (the scenario's
    own source is 45 units away and scores exact zeros) and sigma_bar = 0.02, so that walks
    cross the inclusions (tests/test_gpu_models.py says why)."""
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey

    sc = S.dcr_dipole(6, n_walks=3 * B)
    return dataclasses.replace(sc, f=survey.dipole_source(sc.points[2], sc.points[3], 0.5), max_steps=STEPS)


def _dd_solver(compat, sc=None):
    s = (sc or _dd()).solver(compat=compat, sigma_bar=0.02, device=0)
    if compat == "fixed":
        s.set_fixed_step_check(False)   # (the +-100 box truncates walks at maxSteps; fine here)
    return s


@pytest.mark.parametrize("compat", ["reference", "fixed"])
def test_list_rows_equal_the_full_ranges_rows(gpu_available, compat):
    """One channel: point_alpha[pid] is the listed point's."""
    sc = _dd()
    s = _dd_solver(compat)
    full = _check_lists(s, sc.points, 3 * B, B, 3 * B, LISTS6, f"dcr_dipole {compat}", maxSteps=STEPS, eps=sc.eps,
                        seed=SEED)
    assert len({full[1][p].tobytes() for p in range(6)}) == 6   # (the points differ: a wrong row would show)


def test_list_rows_with_three_sources(gpu_available):
    from dcrmontecarlo_amd import survey

    sc = _dd()
    s = _dd_solver("reference")
    e = sc.points
    srcs = [sc.f, survey.dipole_source(e[0], e[5], 0.5), survey.dipole_source(e[1], e[4], 0.5)]
    with s.sources_installed(s.source_fields(srcs)):
        assert s.num_channels() == 3
        full = _check_lists(s, e, 3 * B, B, 3 * B, LISTS6, "3 sources", maxSteps=STEPS, eps=sc.eps, seed=SEED)
    assert full[0].shape == (6, 2, 7) and len({full[1][..., c].tobytes() for c in range(3)}) == 3


def test_list_rows_with_two_models(gpu_available):
    """The [M][N] alpha rows of models 1.. are read at the listed point's id."""
    from dcrmontecarlo_amd import fields as F

    sc = _dd()
    s = _dd_solver("reference")
    with s.models_installed([(None, sc.alpha), (None, F.const(100.0))]):
        assert s.num_channels() == 2
        full = _check_lists(s, sc.points, 3 * B, B, 3 * B, LISTS6, "2 models", maxSteps=STEPS, eps=sc.eps, seed=SEED)
    assert full[0].shape == (6, 2, 5) and full[1][..., 0].tobytes() != full[1][..., 1].tobytes()


def test_list_rows_with_point_charges_on_surface_points(gpu_available):
    """compat="fixed" point charges; the query points lie on the Neumann top, so a walk starts
    as a boundary walk through point_code[pid]."""
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey
    from dcrmontecarlo_amd.wavenumber import sigma_bar_for

    sc = dataclasses.replace(S.dcr_dipole(n_electrodes=8), f=None)
    s = sc.solver(compat="fixed", sigma_bar=sigma_bar_for(sc.solver(), 0.0) + 2.5, device=0)
    s.set_fixed_step_check(False)
    e = np.asarray(sc.points, np.float64)
    s.set_point_sources([survey.point_dipole(e[2], e[3])])
    _check_lists(s, sc.points, 3 * B, B, 3 * B, ([1, 3, 7], [2], list(range(8))), "point charges", maxSteps=sc.max_steps,
                 eps=sc.eps, seed=SEED)


def test_list_rows_on_the_tree_kernel_with_pools(gpu_available):
    """wenner_topography's 10,000-segment surface: the segment-tree kernel, walk pools at
    their defaults (a parked walk holds its id and state, never its point)."""
    from dcrmontecarlo_amd import scenarios as S

    sc = S.wenner_topography()
    pts = np.ascontiguousarray(sc.points[[40, 128, 200]])
    s = sc.solver(device=0)
    _check_lists(s, pts, 3 * B, B, 3 * B, ([0, 2], [1], [0, 1, 2]), "wenner_topography", maxSteps=sc.max_steps,
                 eps=sc.eps, seed=SEED)
    assert s.last_timing["tree"] == 1


def test_list_rows_at_ids_beyond_2_to_the_40(gpu_available):
    """poisson_square at W = 2^40 + 1000, the last two blocks of each point (one partial)."""
    from dcrmontecarlo_amd import scenarios as S

    sc = S.poisson_square()
    pts = np.ascontiguousarray(sc.points[[3, 17, 41]])
    W = (1 << 40) + 1000
    nbpp = -(-W // B)
    s = sc.solver(device=0)
    full = _check_lists(s, pts, W, (nbpp - 2) * B, W, ([0, 2], [2], [0, 1, 2]), "poisson_square 2^40",
                        maxSteps=sc.max_steps, eps=sc.eps, seed=SEED)
    assert full[0].shape == (3, 2, 3) and full[1].shape == (3, B + 1000, 1)


# ---------------------------------------------------------------- refusals
def test_bad_lists_and_a_disabled_kernel_refuse(gpu_available):
    sc = _dd()
    s = _dd_solver("reference")
    kw = dict(maxSteps=STEPS, eps=sc.eps, seed=SEED)
    for bad in ([2, 1], [1, 1], [0, 6], [-1, 2], []):
        with pytest.raises(ValueError):
            s.solve_range(sc.points, 2 * B, 0, B, point_ids=np.asarray(bad, np.int64), **kw)
    ok = s.solve_range(sc.points, 2 * B, 0, B, point_ids=[1, 4], **kw)
    s.set_jit(False)
    with pytest.raises(NotImplementedError, match="field-specialised"):
        s.solve_range(sc.points, 2 * B, 0, B, point_ids=[1, 4], **kw)
    # ... while the range without a list runs on the precompiled kernel, with the same bits
    plain = s.solve_range(sc.points, 2 * B, 0, B, **kw)
    assert s.last_timing["jit"] == 0
    np.testing.assert_array_equal(plain[[1, 4]], ok)


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_solvers():
    yield
    for f in (_map_solver, _dd):
        f.cache_clear()
