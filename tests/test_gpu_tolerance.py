"""WostSolver_2D.solve_to_tolerance on the device: walks run in doubling rounds
over the points still unconverged, through the point-list kernel, and a point that stops
after n_p walks holds bit for bit the sums of walks [0, n_p) of the fixed solve with nWalks =
max_walks.

Shapes: 6 points (wenner_topography: 3), min_walks = 4096, max_walks = 8 * 4096 + 100, so the
checkpoints are 4096, 8192, 16384, 32768, 32868.

The points and tolerances were chosen on the CPU with the oracle (Problem.solve_walks, seed
29; the device draws the oracle's walks) so that the n_p take at least two values, a point
stops in round 0 and a point runs to max_walks; each test asserts those three conditions on
what the device did. The oracle's relative standard errors se / |mean| at the checkpoints:

laplace_square(6), rel_tol = 0.04
    p0  0.0111                                    -> 4096
    p1  0.0114                                    -> 4096
    p2  0.0574  0.0427  0.0300                    -> 16384
    p3  0.1977  0.1264  0.0987  0.0708  0.0707    -> 32868, not converged
    p4  0.0102                                    -> 4096
    p5  0.0636  0.0459  0.0340                    -> 16384
dcr_dipole(6), transmitter dipole at electrodes 2 and 3, sigma_bar = 0.02, maxSteps = 200
(tests/test_gpu_models.py says why), rel_tol = 0.15; the values are heavy-tailed, so an
error can grow from one checkpoint to the next
    p0  0.424   0.990   0.980   0.970   0.969     -> 32868, not converged
    p1  1.110   0.489   0.190   0.133             -> 32768
    p2  0.0825                                    -> 4096
    p3  0.0901                                    -> 4096
    p4  0.515   0.368   0.384   0.170   0.170     -> 32868, not converged
    p5  1.46    2.12    16.0    1.06    1.02      -> 32868, not converged
the same with 3 sources (dipoles 2-3, 0-5, 1-4), rel_tol = 0.25: channel 0 as above, and
    p1  ch1 0.148                ch2 0.0656                       -> 16384 (channel 0: 0.190)
    p2  ch1 0.160                ch2 0.224                        -> 4096
    p3  ch1 4.55 0.616 0.308 0.175 0.176   ch2 0.416 0.536 0.408 0.360 0.362
                                           -> 32868, though channel 0 (0.0901) had converged in round 0
    p0, p4, p5                             -> 32868 (channel 0 or 1 never converges)
wenner_topography, points [40, 128, 200] (the tree kernel), rel_tol = 0.5
    p0  0.815   0.623   0.422                     -> 16384
    p1  1.00    1.05    1.36    19.9    19.9      -> 32868, not converged (867 of its walks score)
    p2  0.210                                     -> 4096
"""
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 4096   # WOST_BLOCK_WALKS
MIN_WALKS = B
MAX_WALKS = 8 * B + 100
ENDS = [B, 2 * B, 4 * B, 8 * B, MAX_WALKS]
SEED = 29

# name -> (rel_tol, abs_tol)
TOLERANCES = {"laplace_square": (0.04, 0.0), "dcr_dipole": (0.15, 0.0), "dcr_dipole_3_sources": (0.25, 0.0),
              "wenner_topography": (0.5, 0.0)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(solver, points, solve arguments, source fields to install or None)."""
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey

    if name == "laplace_square":
        sc = S.laplace_square(6)
        return sc.solver(device=0), sc.points, dict(maxSteps=sc.max_steps, eps=sc.eps, seed=SEED), None
    if name.startswith("dcr_dipole"):
        sc = S.dcr_dipole(6, n_walks=MAX_WALKS)
        e = sc.points
        srcs = [survey.dipole_source(e[a], e[b], 0.5) for a, b in ((2, 3), (0, 5), (1, 4))]
        s = dataclasses.replace(sc, f=srcs[0]).solver(sigma_bar=0.02, device=0)
        return s, e, dict(maxSteps=200, eps=sc.eps, seed=SEED), (srcs if name.endswith("3_sources") else None)
    sc = S.wenner_topography()
    pts = np.ascontiguousarray(sc.points[[40, 128, 200]])
    return sc.solver(device=0), pts, dict(maxSteps=sc.max_steps, eps=sc.eps, seed=SEED), None


class _installed:
    """The case's sources on its solver (nothing for a single-channel case)."""

    def __init__(self, name):
        self.s, _, _, self.srcs = _case(name)

    def __enter__(self):
        self.cm = self.s.sources_installed(self.s.source_fields(self.srcs)) if self.srcs else None
        if self.cm:
            self.cm.__enter__()

    def __exit__(self, *a):
        if self.cm:
            self.cm.__exit__(*a)


@functools.lru_cache(maxsize=None)
def _adaptive(name):
    s, pts, kw, _ = _case(name)
    rel, ab = TOLERANCES[name]
    with _installed(name):
        u, st = s.solve_to_tolerance(pts, rel_tol=rel, abs_tol=ab, min_walks=MIN_WALKS, max_walks=MAX_WALKS, **kw)
    assert s.last_timing["jit"] == 1
    print(f"{name}: n_p {st.walks.tolist()} converged {st.converged.tolist()} rounds {st.rounds}")
    print(f"{name}: stderr / |mean| {np.array2string(st.stderr / np.abs(st.mean), precision=4)}")
    return u, st


@functools.lru_cache(maxsize=None)
def _prefix_rows(name):
    """{n: point rows of solve_range(points, MAX_WALKS, 0, n), summed in block order} at every checkpoint."""
    s, pts, kw, _ = _case(name)
    out = {}
    with _installed(name):
        for n in ENDS:
            blocks = s.solve_range(pts, MAX_WALKS, 0, n, **kw)
            rows = np.zeros((blocks.shape[0], blocks.shape[2]))
            for k in range(blocks.shape[1]):
                rows = rows + blocks[:, k, :]
            out[n] = rows
    return out


def _check_case(name):
    from dcrmontecarlo_amd.solvers.WoStSolver import tolerance_rule

    s, pts, kw, srcs = _case(name)
    rel, ab = TOLERANCES[name]
    u, st = _adaptive(name)
    N, C = len(pts), len(srcs) if srcs else 1
    n_p = st.walks
    # the three conditions the points and tolerances were chosen for: a genuine subset ran
    assert len(set(n_p.tolist())) >= 2, n_p
    assert (n_p == ENDS[0]).any(), n_p
    assert (n_p == MAX_WALKS).any(), n_p
    assert set(n_p.tolist()) <= set(ENDS) and st.rounds == ENDS.index(int(n_p.max())) + 1
    assert st.total_walks == int(n_p.sum())
    assert np.all(n_p[~st.converged] == MAX_WALKS)
    # every point's sums are the prefix [0, n_p) of the fixed solve, bit for bit
    prefix = _prefix_rows(name)
    assert st.sums.shape == (N, 2 * C + 1)
    for p in range(N):
        np.testing.assert_array_equal(st.sums[p], prefix[int(n_p[p])][p], err_msg=f"{name}: point {p}, n_p {n_p[p]}")
    assert st.total_steps == int(st.sums[:, -1].sum())
    # the rule: met at n_p by every stopped point, met at no earlier checkpoint by any point
    for p in range(N):
        for n in ENDS[:ENDS.index(int(n_p[p]))]:
            assert not tolerance_rule(prefix[n][p:p + 1], n, rel, ab)[2][0], f"{name}: point {p} had converged at {n}"
        mean, se, ok = tolerance_rule(prefix[int(n_p[p])][p:p + 1], int(n_p[p]), rel, ab)
        assert bool(ok[0]) == bool(st.converged[p])
        np.testing.assert_array_equal(np.reshape(st.mean, (C, N))[:, p], mean[:, 0])
        np.testing.assert_array_equal(np.reshape(st.stderr, (C, N))[:, p], se[:, 0])
        if st.converged[p]:
            assert np.all(se[:, 0] <= np.maximum(ab, rel * np.abs(mean[:, 0])))
    want_u = np.reshape(st.mean, (C, N)).astype(np.float32)
    np.testing.assert_array_equal(np.asarray(u).view(np.uint32), np.ascontiguousarray(want_u.T if C == 1 else want_u).view(np.uint32))
    return st, prefix


@pytest.mark.parametrize("name", ["laplace_square", "dcr_dipole", "wenner_topography"])
def test_points_stop_at_their_tolerance_with_the_fixed_solves_bits(gpu_available, name):
    _check_case(name)


def test_a_second_call_gives_the_same_bits(gpu_available):
    s, pts, kw, _ = _case("dcr_dipole")
    u0, st0 = _adaptive("dcr_dipole")
    rel, ab = TOLERANCES["dcr_dipole"]
    u1, st1 = s.solve_to_tolerance(pts, rel_tol=rel, abs_tol=ab, min_walks=MIN_WALKS, max_walks=MAX_WALKS, **kw)
    np.testing.assert_array_equal(np.asarray(u1).view(np.uint32), np.asarray(u0).view(np.uint32))
    np.testing.assert_array_equal(st1.sums, st0.sums)
    np.testing.assert_array_equal(st1.walks, st0.walks)
    assert (st1.rounds, st1.total_walks, st1.total_steps) == (st0.rounds, st0.total_walks, st0.total_steps)


def test_a_point_stops_only_when_all_three_channels_have_converged(gpu_available):
    from dcrmontecarlo_amd.solvers.WoStSolver import tolerance_rule

    name = "dcr_dipole_3_sources"
    st, prefix = _check_case(name)
    rel, ab = TOLERANCES[name]
    assert st.mean.shape == st.stderr.shape == (3, 6)
    # some point went on although one of its channels, taken alone, had converged
    went_on = 0
    for p in range(6):
        for n in ENDS[:ENDS.index(int(st.walks[p]))]:
            row = prefix[n][p]
            alone = [tolerance_rule(row[[2 * c, 2 * c + 1, 6]][None, :], n, rel, ab)[2][0] for c in range(3)]
            assert not all(alone)
            went_on += any(alone)
    assert went_on > 0
    # channel 0 is the single-source solve's: the same walks, the same prefix rows
    single = _prefix_rows("dcr_dipole")
    for n in ENDS:
        np.testing.assert_array_equal(prefix[n][:, [0, 1, 6]], single[n])


@pytest.mark.parametrize("name", ["laplace_square", "dcr_dipole_3_sources"])
def test_zero_tolerances_are_the_fixed_solve(gpu_available, name):
    s, pts, kw, srcs = _case(name)
    with _installed(name):
        u, st = s.solve_to_tolerance(pts, min_walks=MIN_WALKS, max_walks=MAX_WALKS, **kw)
    assert np.all(st.walks == MAX_WALKS) and not st.converged.any() and st.rounds == len(ENDS)
    assert st.total_walks == len(pts) * MAX_WALKS
    if srcs:
        want = s.solve_sources(pts, srcs, nWalks=MAX_WALKS, **kw)
        assert u.shape == want.shape == (3, len(pts))
    else:
        want = s.solve(pts, nWalks=MAX_WALKS, **kw)
        assert u.shape == want.shape == (len(pts), 1)
        np.testing.assert_array_equal(st.sums, s.last_point_sums)
    np.testing.assert_array_equal(np.asarray(u).view(np.uint32), np.asarray(want).view(np.uint32))


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_solvers():
    yield
    for f in (_adaptive, _prefix_rows, _case):
        f.cache_clear()
