"""Weighted channel combinations reduced on the device: wost_block_combine forms
L combinations v_l = sum_c w[l][c] val[walk][c] of a launch's C channels per walk and reduces
those per block, in wost_block_reduce's order. A unit row must give that channel's own sums
bit for bit, any weights the host restatement's (wost_combine_blocks_host) bit for bit.

Shapes follow tests/test_gpu_tolerance.py's dcr_dipole case: dcr_dipole(6), sigma_bar = 0.02,
maxSteps = 200 (tests/test_gpu_models.py says why), dipole sources at electrodes (2,3), (0,5),
(1,4), wavenumbers installed, W = 2 * 4096 + 100 walks (the last block is partial), seed 29.

Bounds against the numpy paths (transformed potentials, model differences) are derived, not measured: a double sum of n
terms has a relative error of n 2^-53 on sum|v|, likewise on sum v^2, which bounds the
difference of the two paths' sums S; for the variance (Q - S^2/n) / (n - 1) this gives the
relative bound 4 n 2^-53 (Q + S^2/n) / (Q - S^2/n), with Q and S the combination's sums
(asserted in its absolute form, so that a point whose values are all 0 must agree exactly).
The per-walk values themselves differ by roundings of 2^-53 per term, n times below that.
Each test prints its largest ratio of error to bound.

solve_to_tolerance(combinations=...): points and tolerance were chosen on the CPU
with the oracle's walks (Problem.solve_walks with sigma = k^2 alpha, sigma_bar 0.02, seed 29: the
device draws the oracle's walks), wavenumbers k = (0.02, 0.05, 0.14), quadrature weights
(1.0, 0.8, 0.6), transmitter dipole (2,3), checkpoints 4096, 8192, 8292, rel_tol = 0.086. The
oracle's relative standard errors se / |mean| there, for the transformed potential u = sum_j
w_j u_kj and for the channel of k = 0.14 alone (k^2 = 0.0196 of sigma_bar = 0.02: it scores
little but collision-free walks, and is the noisiest):
          u at 4096, 8192, 8292          -> n_p                   k = 0.14 alone
    p0    0.383   0.973   0.973          -> 8292, not converged   0.399   0.402   0.409
    p1    0.322   0.236   0.238          -> 8292, not converged   0.330   0.268   0.268
    p2    0.0814                         -> 4096                  0.0911 (not converged at 4096)
    p3    0.0951  0.0669                 -> 8192                  0.0990  0.0687
    p4    0.379   0.252   0.247          -> 8292, not converged   0.356   0.229   0.224
    p5    0.529   0.369   0.368          -> 8292, not converged   0.463   0.312   0.312
"""
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 4096
W = 2 * B + 100
BEGIN = np.array([0, B, 2 * B, W], np.int64)
SEED = 29
U = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _point_rows(blocks):
    rows = np.zeros((blocks.shape[0], blocks.shape[2]))
    for k in range(blocks.shape[1]):
        rows = rows + blocks[:, k, :]
    return rows


@functools.lru_cache(maxsize=None)
def _dipole():
    """(solver, electrodes, solve arguments, the three dipole sources)."""
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey

    sc = S.dcr_dipole(6, n_walks=W)
    e = sc.points
    srcs = [survey.dipole_source(e[a], e[b], 0.5) for a, b in ((2, 3), (0, 5), (1, 4))]
    s = dataclasses.replace(sc, f=srcs[0]).solver(sigma_bar=0.02, device=0)
    return s, e, dict(maxSteps=200, eps=sc.eps, seed=SEED), srcs


class _channels:
    """K wavenumbers x the three sources on the dipole case's solver."""

    def __init__(self, k, n_sources=3):
        self.s, _, _, srcs = _dipole()
        self.k, self.srcs = k, srcs[:n_sources]

    def __enter__(self):
        self.cm = self.s.sources_installed(self.s.source_fields(self.srcs))
        self.cm.__enter__()
        self.s.set_wavenumbers(self.k)
        return self.s

    def __exit__(self, *a):
        self.s.set_wavenumbers(None)
        self.cm.__exit__(*a)


def combine_host(values, begin, weights):
    import ctypes

    from dcrmontecarlo_amd import _lib

    values = np.ascontiguousarray(values, np.float32)
    begin = np.ascontiguousarray(begin, np.int64)
    w = np.ascontiguousarray(weights, np.float64)
    out = np.zeros((len(begin) - 1, 2 * w.shape[0]), np.float64)
    _lib.check(_lib.lib.wost_combine_blocks_host(_lib.fptr(values), begin.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                 len(begin) - 1, values.shape[1], _lib.dptr(w), w.shape[0],
                                                 _lib.dptr(out)), "wost_combine_blocks_host")
    return out


# ---- unit rows --------------------------------------------------------------------------------
def _check_unit_rows(s, pts, kw, w_begin, w_end, ids=None):
    C = s.num_channels()
    rows = len(pts) if ids is None else len(ids)
    chan = s.solve_range(pts, W, w_begin, w_end, point_ids=ids, **kw)
    psum, cps = np.full((rows, 2 * C + 1), np.nan), np.full((rows, 2 * C + 1), np.nan)
    comb = s.solve_range_combinations(pts, np.eye(C), W, w_begin, w_end, point_ids=ids, point_sums=psum,
                                      channel_point_sums=cps, **kw)
    assert s.last_timing["jit"] == 1 and s.last_combine_ms > 0.0
    assert comb.shape == chan.shape == (rows, -(-(w_end - w_begin) // B), 2 * C + 1)
    np.testing.assert_array_equal(_bits(comb), _bits(chan))            # channel entries and step sums
    np.testing.assert_array_equal(_bits(psum), _bits(_point_rows(chan)))
    np.testing.assert_array_equal(_bits(cps), _bits(_point_rows(chan)))
    assert np.count_nonzero(chan[:, :, :-1]) > 0 and np.all(chan[:, :, -1] > 0)


# wavenumbers of the K = 4, 5 and 8 cases (k^2 <= 0.0196 under sigma_bar = 0.02)
K4 = [0.02, 0.05, 0.08, 0.12]
K5 = [0.01, 0.02, 0.04, 0.08, 0.12]
K8 = [0.01, 0.015, 0.02, 0.03, 0.05, 0.08, 0.11, 0.14]


@pytest.mark.parametrize("variant", ["whole", "range", "list"])
def test_unit_rows_are_the_channels_own_sums(gpu_available, variant):
    _, pts, kw, _ = _dipole()
    with _channels([0.02, 0.1]) as s:   # K = 2, S = 3: L = C = 6
        assert s.num_channels() == 6
        if variant == "whole":
            _check_unit_rows(s, pts, kw, 0, W)
        elif variant == "range":
            _check_unit_rows(s, pts, kw, B, W)
        else:
            _check_unit_rows(s, pts, kw, 0, W, ids=[1, 4])


@pytest.mark.parametrize("k, n_sources, variant", [(K8, 2, "whole"), (K8, 2, "list"), (K4, 2, "range"), (K4, 3, "whole"),
                                                   ([0.02, 0.1], 2, "whole")],
                         ids=["C16-whole", "C16-list", "C8-range", "C12-whole", "C4-whole"])
def test_unit_rows_with_16_byte_loads(gpu_available, k, n_sources, variant):
    """C a multiple of 4 takes the kernel's other instantiation (a walk's values read as float4):
    C = 16 (8 wavenumbers x 2 sources, README's case), and the partial widths 12, 8 and 4, whose
    float4 indices past C are clamped; every variant ends in the partial last block."""
    _, pts, kw, _ = _dipole()
    with _channels(k, n_sources=n_sources) as s:
        assert s.num_channels() == len(k) * n_sources and s.num_channels() % 4 == 0
        if variant == "whole":
            _check_unit_rows(s, pts, kw, 0, W)
        elif variant == "range":
            _check_unit_rows(s, pts, kw, B, W)
        else:
            _check_unit_rows(s, pts, kw, 0, W, ids=[0, 3, 5])


def test_unit_rows_on_the_tree_kernel(gpu_available):
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey

    sc = S.wenner_topography()
    pts = np.ascontiguousarray(sc.points[[40, 128, 200]])
    s = sc.solver(device=0)
    srcs = [sc.f, survey.dipole_source(pts[0], pts[2], 2.0)]
    with s.sources_installed(s.source_fields(srcs)):
        _check_unit_rows(s, pts, dict(maxSteps=sc.max_steps, eps=sc.eps, seed=SEED), 0, W)
    assert s.last_timing["tree"] == 1


# ---- any weights: the host restatement's bits -------------------------------------------------
# (wavenumbers, sources): C = 15 (scalar loads), and 16, 12, 8 (16-byte loads, full and partial width)
CASES = {15: (K5, 3), 16: (K8, 2), 12: (K4, 3), 8: (K4, 2)}


@functools.lru_cache(maxsize=None)
def _walks(C):
    """Per-walk values [N, W, C] and channel block rows of the C-channel case."""
    _, pts, kw, _ = _dipole()
    k, n_sources = CASES[C]
    with _channels(k, n_sources=n_sources) as s:
        assert s.num_channels() == C
        wv = np.empty((len(pts), W, C), np.float32)
        chan = s.solve_range(pts, W, 0, W, walk_values=wv, **kw)
    wv.setflags(write=False)
    return wv, chan


def _weights16(C=15):
    """16 rows: 0..7 dense, 8..13 sparse, 14 a unit row at channel C // 2, 15 empty."""
    rng = np.random.default_rng(C + 1)
    w = rng.standard_normal((16, C))
    w[8:][rng.random((8, C)) < 0.7] = 0.0
    w[15] = 0.0
    w[14] = 0.0
    w[14, C // 2] = 1.0
    return w


@pytest.mark.parametrize("C", [15, 16, 12, 8])
def test_device_rows_are_the_host_restatement_bit_for_bit(gpu_available, C):
    _, pts, kw, _ = _dipole()
    wv, chan = _walks(C)
    w = _weights16(C)
    k, n_sources = CASES[C]
    with _channels(k, n_sources=n_sources) as s:
        comb = s.solve_range_combinations(pts, w, W, 0, W, **kw)
    assert comb.shape == (len(pts), 3, 33)
    for p in range(len(pts)):
        np.testing.assert_array_equal(_bits(comb[p, :, :32]), _bits(combine_host(wv[p], BEGIN, w)), err_msg=f"point {p}")
    np.testing.assert_array_equal(comb[:, :, 32], chan[:, :, 2 * C])
    u = C // 2
    np.testing.assert_array_equal(_bits(comb[:, :, 28:30]), _bits(chan[:, :, 2 * u:2 * u + 2]))   # the unit row
    assert np.all(comb[:, :, 30:32] == 0.0) and np.count_nonzero(comb[:, :, :28]) > 0
    # every channel is weighed by some row, and differs from its neighbours: a swapped or
    # repeated channel would change a dense row
    assert np.all(np.count_nonzero(w, axis=0) >= 8)
    assert len({wv[2, :, c].tobytes() for c in range(C)}) == C


# ---- shards -----------------------------------------------------------------------------------
def test_shards_give_the_full_calls_rows(gpu_available):
    _, pts, kw, _ = _dipole()
    w = _weights16()
    with _channels(K5) as s:
        full_p = np.empty((len(pts), 33))
        full = s.solve_range_combinations(pts, w, W, 0, W, point_sums=full_p, **kw)
        acc = np.zeros((len(pts), 33))
        for k, (a, b) in enumerate(((0, B), (B, 2 * B), (2 * B, W))):
            part_p = np.empty((len(pts), 33))
            part = s.solve_range_combinations(pts, w, W, a, b, point_sums=part_p, **kw)
            assert part.shape == (len(pts), 1, 33)
            np.testing.assert_array_equal(_bits(part[:, 0]), _bits(full[:, k]))
            np.testing.assert_array_equal(_bits(part_p), _bits(full[:, k]))
            acc = acc + part[:, 0]
    np.testing.assert_array_equal(_bits(full_p), _bits(acc))   # point rows: added in block order


def test_a_range_longer_than_one_launch_is_stitched(gpu_available):
    """More than 2^26 walks of a point: block-aligned sub-ranges, one solve each, their combined
    rows scattered like the channels' (laplace_square, one channel; the row -2 x is exact:
    -2 sum and 4 sum^2)."""
    from dcrmontecarlo_amd import scenarios as S

    sc = S.laplace_square(6)
    s = sc.solver(device=0)
    pts = sc.points[:1]
    Wl = (1 << 26) + 3 * B + 5
    kw = dict(maxSteps=sc.max_steps, eps=sc.eps, seed=4)
    chan = s.solve_range(pts, Wl, B, Wl, **kw)
    psum = np.empty((1, 5))
    comb = s.solve_range_combinations(pts, np.array([[1.0], [-2.0]]), Wl, B, Wl, point_sums=psum, **kw)
    assert s.last_timing["n_launches"] >= 2 and s.last_combine_ms > 0.0
    assert comb.shape == (1, -(-Wl // B) - 1, 5)
    want = np.stack([chan[0, :, 0], chan[0, :, 1], -2.0 * chan[0, :, 0], 4.0 * chan[0, :, 1], chan[0, :, 2]], axis=1)
    np.testing.assert_array_equal(_bits(comb[0]), _bits(want))
    np.testing.assert_array_equal(_bits(psum), _bits(_point_rows(comb)))


def test_refusals(gpu_available):
    _, pts, kw, _ = _dipole()
    with _channels([0.02, 0.1]) as s:
        for bad in (np.zeros((0, 6)), np.ones((17, 6)), np.full((1, 6), np.nan), np.array([[1, 0, 0, np.inf, 0, 0.0]])):
            with pytest.raises(ValueError):
                s.solve_range_combinations(pts, bad, W, 0, W, **kw)
        with pytest.raises(ValueError):   # another width than the installed channels
            s.solve_range_combinations(pts, np.ones((1, 5)), W, 0, W, **kw)


# ---- the derived bounds ----------------------------------------------------------------------
def _bounds(v):
    """Per-walk combined values v [..., n] -> (bound on |mean - mean'|, bound on |var - var'| of the
    variance of the mean), from sums of n terms in two orders."""
    n = v.shape[-1]
    S, Q, A = v.sum(-1), (v * v).sum(-1), np.abs(v).sum(-1)
    mean_b = n * U * A / n
    var_b = 4 * n * U * (Q + S * S / n) / (n - 1) / n   # relative bound x (Q - S^2/n) / (n - 1) / n
    return mean_b, var_b


# ---- transformed potentials ---------------------------------------------------------------------
@pytest.mark.parametrize("electrodes", ["gaussian", "point"])
def test_transformed_potentials_on_the_device_agree_with_the_host_path(gpu_available, capsys, electrodes):
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey
    from dcrmontecarlo_amd import wavenumber as wn

    _, pts, kw, srcs = _dipole()
    if electrodes == "gaussian":
        sc = dataclasses.replace(S.dcr_dipole(6, n_walks=W), f=srcs[0])
        solvers = [sc.solver(sigma_bar=0.02, device=0) for _ in range(2)]
    else:   # point dipoles at the same electrodes: compat="fixed", a solver without a source field
        e = np.asarray(pts, np.float64)
        srcs = [survey.point_dipole(e[a], e[b]) for a, b in ((2, 3), (0, 5), (1, 4))]
        sc = dataclasses.replace(S.dcr_dipole(6, n_walks=W), f=None)
        solvers = [sc.solver(compat="fixed", sigma_bar=0.02, device=0) for _ in range(2)]
        for s in solvers:
            s.set_fixed_step_check(False)   # (a +-100 box truncates the walks at maxSteps; fine here)
    k = np.array([0.02, 0.05, 0.08, 0.12])
    w = np.array([1.0, 0.8, -0.3, 0.6])
    groups = [np.array([0, 1]), np.array([2, 3])]
    args = (solvers, groups, pts, srcs, k, w, W, kw["maxSteps"], kw["eps"])
    host = wn.transformed_potentials(*args, seed=SEED)
    dev = wn.transformed_potentials(*args, seed=SEED, device_reduce=True)
    assert dev.launches == host.launches == 2 and dev.walk_steps == host.walk_steps
    # the device's numbers are its own host restatement's, bit for bit
    mean, var = np.zeros((3, 6)), np.zeros((3, 6))
    mean_b, var_b = np.zeros((3, 6)), np.zeros((3, 6))
    for g, idx in enumerate(groups):
        vals, _ = solvers[g].solve_wavenumbers_walks(pts, k[idx], nWalks=W, maxSteps=kw["maxSteps"], eps=kw["eps"],
                                                     sources=srcs, seed=survey.group_seed(SEED, g))   # [K, S, N, W]
        wv = np.ascontiguousarray(vals.transpose(2, 3, 0, 1).reshape(6, W, 6))
        tw = wn.transform_weights(w[idx], 3)
        rows = np.stack([_point_rows(combine_host(wv[p], BEGIN, tw)[None]) [0] for p in range(6)])   # [N, 2S]
        from dcrmontecarlo_amd.solvers.WoStSolver import tolerance_rule

        m, se, _ = tolerance_rule(np.concatenate([rows, np.ones((6, 1))], axis=1), W, 0.0, 0.0)
        mean += m
        var += se ** 2
        v = np.tensordot(w[idx], vals.astype(np.float64), axes=(0, 0))   # [S, N, W]
        mb, vb = _bounds(v)
        mean_b += mb
        var_b += vb
    np.testing.assert_array_equal(_bits(dev.mean), _bits(mean))
    np.testing.assert_array_equal(_bits(dev.stderr), _bits(np.sqrt(var)))
    # ... and the numpy path's to the derived bound
    em, ev = np.abs(dev.mean - host.mean), np.abs(dev.stderr ** 2 - host.stderr ** 2)
    with capsys.disabled():
        print(f"\ntransformed potentials, {electrodes} dipoles: largest error / bound: mean {np.max(em / mean_b):.3g}, variance {np.max(ev / var_b):.3g}")
    assert np.all(em <= mean_b) and np.all(ev <= var_b)
    assert np.count_nonzero(host.mean) == host.mean.size


# ---- paired differences -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _models():
    from dcrmontecarlo_amd import scenarios as S

    sc = S.dcr_dipole(6, n_walks=W)
    return [(None, sc.alpha), (None, S.dcr_alpha_geophysical(1.01)), (None, S.dcr_alpha_geophysical(1.05))]


def test_model_differences_agree_with_the_paired_differences_of_the_walks(gpu_available, capsys):
    from dcrmontecarlo_amd import survey

    s, pts, kw, _ = _dipole()
    models = _models()
    mean, se = s.solve_models_differences(pts, models, nWalks=W, **kw)
    assert mean.shape == se.shape == (2, 6)
    assert s.num_models == 0 and s.wavenumbers is None
    vals, _ = s.solve_models_walks(pts, models, nWalks=W, **kw)   # [M, N, W]
    want_m, want_se = survey.paired_difference(vals)
    d = vals.astype(np.float64)[1:] - vals.astype(np.float64)[:1]
    mean_b, var_b = _bounds(d)
    em, ev = np.abs(mean - want_m[1:]), np.abs(se ** 2 - want_se[1:] ** 2)
    ok = mean_b > 0
    with capsys.disabled():
        print(f"\nmodel differences: largest error / bound: mean {np.max(em[ok] / mean_b[ok], initial=0):.3g}, "
              f"variance {np.max(ev[ok] / var_b[ok], initial=0):.3g}; points with a nonzero difference: {int(ok.sum())}")
    assert np.all(em <= mean_b) and np.all(ev <= var_b)
    assert ok.any()
    with pytest.raises(ValueError, match="paired_difference"):
        s.solve_models_differences(pts, models * 6, nWalks=W, **kw)   # 18 channels


def test_identical_models_differ_by_an_exact_zero(gpu_available):
    s, pts, kw, _ = _dipole()
    m = _models()[1]
    mean, se = s.solve_models_differences(pts, [m, m], nWalks=W, **kw)
    assert mean.shape == (1, 6) and np.all(mean == 0.0) and np.all(se == 0.0)


# ---- solve_to_tolerance on the combination ------------------------------------------------------
KT = [0.02, 0.05, 0.14]
WT = [1.0, 0.8, 0.6]
REL_TOL = 0.086


def test_zero_tolerances_are_the_fixed_combined_solve(gpu_available):
    from dcrmontecarlo_amd import wavenumber as wn

    _, pts, kw, _ = _dipole()
    tw = wn.transform_weights(WT, 3)
    with _channels(KT) as s:
        u, st = s.solve_to_tolerance(pts, min_walks=B, max_walks=W, combinations=tw, **kw)
        want = np.empty((6, 7))
        s.solve_range_combinations(pts, tw, W, 0, W, point_sums=want, **kw)
    assert st.sums.shape == (6, 7) and u.shape == st.mean.shape == st.stderr.shape == (3, 6)
    assert np.all(st.walks == W) and not st.converged.any() and st.rounds == 3
    np.testing.assert_array_equal(_bits(st.sums), _bits(want))
    np.testing.assert_array_equal(u, (want[:, 0:6:2].T / W).astype(np.float32))


def test_points_stop_on_the_combination_not_on_a_high_wavenumber(gpu_available):
    from dcrmontecarlo_amd import wavenumber as wn
    from dcrmontecarlo_amd.solvers.WoStSolver import tolerance_rule

    _, pts, kw, _ = _dipole()
    tw = wn.transform_weights(WT, 1)
    ends = [B, 2 * B, W]
    with _channels(KT, n_sources=1) as s:
        u, st = s.solve_to_tolerance(pts, rel_tol=REL_TOL, min_walks=B, max_walks=W, combinations=tw, **kw)
        prefix, chan = {}, {}
        for n in ends:
            rows = np.empty((6, 3))
            s.solve_range_combinations(pts, tw, W, 0, n, point_sums=rows, **kw)
            prefix[n] = rows
            chan[n] = _point_rows(s.solve_range(pts, W, 0, n, **kw))
    print("n_p", st.walks.tolist(), "converged", st.converged.tolist())
    assert len(set(st.walks.tolist())) >= 2, st.walks
    assert set(st.walks.tolist()) <= set(ends) and np.all(st.walks[~st.converged] == W)
    for p in range(6):   # a prefix of the fixed combined solve, bit for bit; the rule met no earlier
        n_p = int(st.walks[p])
        np.testing.assert_array_equal(_bits(st.sums[p]), _bits(prefix[n_p][p]), err_msg=f"point {p}")
        for n in ends[:ends.index(n_p)]:
            assert not tolerance_rule(prefix[n][p:p + 1], n, REL_TOL, 0.0)[2][0]
        assert bool(tolerance_rule(prefix[n_p][p:p + 1], n_p, REL_TOL, 0.0)[2][0]) == bool(st.converged[p])
    # some point converged on the combination where its highest wavenumber alone had not
    high = 0
    for p in np.flatnonzero(st.converged):
        n_p = int(st.walks[p])
        row = chan[n_p][p, [4, 5, 6]][None, :]
        high += not tolerance_rule(row, n_p, REL_TOL, 0.0)[2][0]
    assert high > 0


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_solvers():
    yield
    for f in (_dipole, _walks, _models):
        f.cache_clear()
