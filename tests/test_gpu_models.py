"""Shared-path model batching on the device (wost_set_models, WostSolver_2D.solve_models;
DESIGN.md 7c).

Under delta tracking a walk's path depends only on sigma_bar and the geometry; the
conductivity (sigma, alpha) enters through the walk's weights alone. One walk therefore
scores M models (x K wavenumbers x S sources): channel c = (m * K + j) * S + s. These tests
pin that every channel is bit for bit the single solve of a fresh solver created with model
m's fields on the batched solver's sigma_bar, that handles without models (or with one) keep
their bits, that walk-range shards, the tree kernels and the facade's chunking agree, the
error returns, the shared-walk surveys, and that pairing lowers the error of a difference.

Shapes: 6 points x 8192 walks (two reduction blocks per point), maxSteps 200.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 8192
STEPS = 200
SEED = 47
COMPATS = ["reference", "fixed"]
# Pairing (test_pairing_lowers_the_error_of_a_difference): the largest ratio paired /
# unpaired standard error measured on an MI355X with these shapes is recorded in DESIGN.md
# 7c; the bound is four times it, capped at 1 (the margin covers the noise of a
# standard-error estimate from 8192 walks).
# Measured: ratios [0, 6.2e-14, 0, 5.8e-32, 0, 5.2e-12] over the six electrodes. They are this
# small because the models differ along a path only where it collides inside the scaled
# inclusion's thin shell (elsewhere sigma' is 0 and the sqrt(a_new / alpha(x)) factors
# telescope), so nearly every per-walk difference is an exact 0.
PAIRED_RATIO_MEASURED = 5.21e-12
PAIRED_RATIO_BOUND = min(1.0, 4.0 * PAIRED_RATIO_MEASURED)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- scenarios and their models ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """(scenario, points, models): models[0] is the scenario's own (sigma, alpha)."""
    from dcrmontecarlo_amd import PolyLinesSimple  # noqa: F401  (the package is importable)
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd.fields import X, Y

    if name == "dd":   # Neumann top, compiled-in polylines, sharp-sigmoid alpha
        # The six electrodes are 45 units and more from the scenario's own source (Gaussians of
        # width 0.5 at x = +-10): measured on the device, 36 of 147,456 walks score anything
        # but an exact 0 under compat="reference" and none under compat="fixed", which would
        # leave nothing to compare. The source is a transmitter dipole at two of the electrodes
        # instead, as in the surveys.
        from dcrmontecarlo_amd import survey

        sc = S.dcr_dipole(6, n_walks=W)
        sc = dataclasses.replace(sc, f=survey.dipole_source(sc.points[2], sc.points[3], 0.5), max_steps=STEPS)
        models = [(None, sc.alpha), (None, F.const(100.0)), (None, S.dcr_alpha_geophysical(1.01))]
        return sc, sc.points, models
    if name in ("vc", "vc_mixed"):   # a 32-segment Neumann circle, non-constant sigma and alpha
        sc = dataclasses.replace(S.variable_coefficients(6, n_walks=W), max_steps=STEPS)
        smooth = 0.5 + 1.5 * F.exp(-2.0 * (X**2 + Y**2))          # the scenario's alpha with its jet
        other = (0.5 + 0.25 * (1 + F.sin(X) * F.cos(Y)), 0.8 + 0.4 * F.exp(-1.0 * (X**2 + Y**2)))
        if name == "vc":
            sc = dataclasses.replace(sc, alpha=smooth)
            return sc, sc.points, [(sc.sigma, smooth), other]
        return sc, sc.points, [(sc.sigma, sc.alpha), other]      # a detached (Q9) alpha and a differentiable one
    if name == "sq":   # Dirichlet only: a square, alpha linear in x
        sq = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1], [-1, -1]], np.float32)
        rng = np.random.default_rng(5)
        pts = rng.uniform(-0.8, 0.8, size=(6, 2)).astype(np.float32)
        sc = S.Scenario("square_linear_alpha", sq, None, g=X**2 - Y**2, f=F.gaussian((0.2, -0.1), 0.3),
                        sigma=F.const(0.5), alpha=2.0 + 0.5 * X, points=pts, n_walks=W, max_steps=STEPS, eps=1e-3)
        return sc, pts, [(sc.sigma, sc.alpha), (0.5 + 0.2 * Y, 1.5 - 0.3 * X), (F.const(1.0), 1.0 + 0.25 * X)]
    raise KeyError(name)


def _with_model(sc, model):
    return dataclasses.replace(sc, sigma=model[0], alpha=model[1])


@functools.lru_cache(maxsize=None)
def _sigma_bar(name):
    """One sigma_bar for the batched solver and its single-model comparisons: the largest
    sigma' of any of the case's models (survey.sigma_bar_for_models)."""
    from dcrmontecarlo_amd import survey

    sc, _, models = _case(name)
    if name == "dd":
        # With the scenario's own estimate (10) or the models' largest sigma', a walk diffuses
        # ~2 sqrt(200 / sigma_bar) = 9 units in 200 steps and never leaves the region where
        # every model's alpha is exactly 100 (the sigmoids saturate in float32): measured on
        # the device, the three channels were then the same numbers and the paired difference
        # an exact 0. A sigma_bar of 0.02 moves a walk ~14 units per step, so the paths cross
        # both inclusions and the models differ along them. (sigma' is 0 outside the
        # inclusions' thin shells; inside them the collision weight is clamped or signed, as
        # it is with the scenario's estimate.)
        return 0.02
    return survey.sigma_bar_for_models(sc.solver(), models)


def _solver(name, compat, model=None, tree=False, **kw):
    """The case's solver on the shared sigma_bar; model: a fresh single-model solver created
    with that model's fields."""
    sc, _, _ = _case(name)
    if model is not None:
        sc = _with_model(sc, model)
    s = sc.solver(compat=compat, sigma_bar=_sigma_bar(name), **kw)
    if compat == "fixed":
        s.set_fixed_step_check(False)   # (dd: a +-100 box truncates the walks at maxSteps; fine here)
    if tree:
        s.set_segment_tree(0)
    return s


def _multi(s, pts, eps, seed=SEED):
    """wost_solve_multi with the handle's channels: block rows [blocks, 2C+1], point rows
    [N, 2C+1], values [N, W, C], steps [N, W]."""
    from dcrmontecarlo_amd import _lib

    p = np.ascontiguousarray(pts, np.float32)
    n, C = len(p), s.num_channels()
    nb = s.num_blocks(n, W)
    blocks = np.zeros((nb, 2 * C + 1))
    rows = np.zeros((n, 2 * C + 1))
    wv = np.empty((n, W, C), np.float32)
    ws = np.empty((n, W), np.uint32)
    rc = _lib.lib.wost_solve_multi(s._h, _lib.fptr(p), n, W, 0, nb, STEPS, float(eps), seed, _lib.dptr(blocks),
                                   _lib.dptr(rows), _lib.fptr(wv), _lib.u32ptr(ws))
    return rc, blocks, rows, wv, ws


def _single(s, pts, eps, seed=SEED):
    """A single-channel solver's block rows [blocks, 3], point rows [N, 3], values, steps,
    mean and stderr."""
    p = np.ascontiguousarray(pts, np.float32)
    n = len(p)
    wv = np.empty(n * W, np.float32)
    ws = np.empty(n * W, np.uint32)
    blocks = s.solve_blocks(p, W, 0, s.num_blocks(n, W), STEPS, eps, seed, wv, ws)
    _, st = s.solve(p, nWalks=W, maxSteps=STEPS, eps=eps, seed=seed, return_stats=True)
    return blocks, s.last_point_sums.copy(), wv.reshape(n, W), ws.reshape(n, W), st


def _check_channel(c, C, batched, single, what):
    """Channel c of a batched solve against its single solve, bit for bit."""
    _, blocks, rows, wv, ws = batched
    sb, sr, sv, ss, _ = single
    assert C == (blocks.shape[1] - 1) // 2
    np.testing.assert_array_equal(ws, ss, err_msg=f"{what}: step counts")
    np.testing.assert_array_equal(_bits(wv[:, :, c]), _bits(sv), err_msg=f"{what}: per-walk values")
    for got, want, kind in ((blocks, sb, "block sums"), (rows, sr, "point sums")):
        np.testing.assert_array_equal(got[:, [2 * c, 2 * c + 1, 2 * C]], want, err_msg=f"{what}: {kind}")


# ---- 1. each channel is its single solve, bit for bit --------------------------------------
def _each_channel(name, compat, tree=False):
    sc, pts, models = _case(name)
    s = _solver(name, compat, tree=tree)
    s.set_models(models)
    M = len(models)
    assert s.num_models == M and s.num_channels() == M
    batched = _multi(s, pts, sc.eps)
    assert batched[0] == 0
    t = s.timing()
    assert t["jit"] == 1 and t["tree"] == (1 if tree else 0)
    u, st = s.solve_models(pts, models, nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED, return_stats=True)
    assert u.shape == (M, len(pts)) and s.num_models == M   # (the solver's own models are restored)
    nonzero = 0
    for m, model in enumerate(models):
        one = _solver(name, compat, model=model, tree=tree)
        assert one.sigma_bar == s.sigma_bar
        single = _single(one, pts, sc.eps)
        _check_channel(m, M, batched, single, f"{name}/{compat} model {m}")
        np.testing.assert_array_equal(st.mean[m], single[4].mean)
        np.testing.assert_array_equal(st.stderr[m], single[4].stderr)
        np.testing.assert_array_equal(_bits(u[m]), _bits(single[4].mean.astype(np.float32)))
        nonzero += int(np.count_nonzero(single[2]))
    print(f"{name}/{compat}{'/tree' if tree else ''}: {nonzero} non-zero walk values of {M * len(pts) * W}; "
          f"mean steps {batched[4].mean():.1f}; u[:, 0] = {u[:, 0]}")
    assert nonzero > 0, "every walk scored exactly 0: the comparison would be empty"
    return batched


@pytest.mark.parametrize("compat", COMPATS)
def test_dcr_dipole_models_are_their_single_solves(gpu_available, compat):
    _each_channel("dd", compat)


def test_variable_coefficients_models_scan_and_tree(gpu_available):
    scan = _each_channel("vc", "reference")
    tree = _each_channel("vc", "reference", tree=True)
    for a, b in zip(scan[1:4], tree[1:4]):
        np.testing.assert_array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32),
                                      b.view(np.uint64 if b.dtype == np.float64 else np.uint32))
    np.testing.assert_array_equal(scan[4], tree[4])


@pytest.mark.parametrize("compat", COMPATS)
def test_dirichlet_only_models_are_their_single_solves(gpu_available, compat):
    _each_channel("sq", compat)


def test_detached_and_differentiable_alpha_in_one_launch(gpu_available):
    _each_channel("vc_mixed", "reference")


# ---- 2. channel layout ---------------------------------------------------------------------
def test_channel_layout_models_wavenumbers_sources(gpu_available):
    """3 models x 2 wavenumbers x 2 sources = 12 channels, c = (m * 2 + j) * 2 + s."""
    from dcrmontecarlo_amd import fields as F

    sc, pts, models = _case("sq")
    srcs = [sc.f, F.gaussian((-0.3, 0.4), 0.25, 2.0)]
    ks = [0.7, 1.9]
    s = sc.solver(sigma_bar=_sigma_bar("sq") + max(ks) ** 2)
    vals, steps = s.solve_models_walks(pts, models, nWalks=W, maxSteps=STEPS, eps=sc.eps, sources=srcs, k=ks,
                                       seed=SEED)
    assert vals.shape == (3, 2, 2, len(pts), W) and s.last_timing["n_launches"] == 1
    u = s.solve_models(pts, models, nWalks=W, maxSteps=STEPS, eps=sc.eps, sources=srcs, k=ks, seed=SEED)
    assert u.shape == (3, 2, 2, len(pts))
    # the raw layout, through the library
    with s.sources_installed(s.source_fields(srcs)):
        s.set_models(models)
        s.set_wavenumbers(ks)
        assert s.num_channels() == 12
        rc, _, rows, wv, ws = _multi(s, pts, sc.eps)
        s.set_wavenumbers(None)
        s.set_models(None)
    assert rc == 0
    for m, model in enumerate(models):
        one = _with_model(sc, model).solver(sigma_bar=s.sigma_bar)
        for si, f in enumerate(srcs):
            one.setSourceTerm(f)
            for j, k in enumerate(ks):
                one.set_wavenumbers([k])
                sv, ss = one.solve_walks(pts, nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED)
                one.solve(pts, nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED)
                c = (m * 2 + j) * 2 + si
                what = f"channel (m={m}, j={j}, s={si})"
                np.testing.assert_array_equal(steps, ss, err_msg=what)
                np.testing.assert_array_equal(_bits(vals[m, j, si]), _bits(sv), err_msg=what)
                np.testing.assert_array_equal(_bits(wv[:, :, c]), _bits(sv), err_msg=what + " raw layout")
                np.testing.assert_array_equal(rows[:, [2 * c, 2 * c + 1, 24]], one.last_point_sums, err_msg=what)
                np.testing.assert_array_equal(_bits(u[m, j, si]),
                                              _bits((one.last_point_sums[:, 0] / W).astype(np.float32)), err_msg=what)
                assert np.count_nonzero(sv) > 0


def test_nine_models_two_sources_are_chunked_by_the_facade(gpu_available):
    from dcrmontecarlo_amd import _lib
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd.fields import X

    sc, pts, _ = _case("sq")
    models = [(sc.sigma, 2.0 + (0.5 - 0.05 * m) * X) for m in range(9)]
    srcs = [sc.f, F.gaussian((-0.3, 0.4), 0.25, 2.0)]
    s = _solver("sq", "reference")
    u = s.solve_models(pts, models, nWalks=W, maxSteps=STEPS, eps=sc.eps, sources=srcs, seed=SEED)
    assert u.shape == (9, 2, len(pts)) and s.last_timing["n_launches"] == 2   # 9 models x 1 source, twice
    for m in (0, 8):
        one = _with_model(sc, models[m]).solver(sigma_bar=s.sigma_bar)
        want = one.solve_sources(pts, srcs, nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED)
        np.testing.assert_array_equal(_bits(u[m]), _bits(want))
    # ... and refused by the library: 9 x 2 = 18 channels
    with s.sources_installed(s.source_fields(srcs)):
        with pytest.raises(ValueError, match="exceed 16 channels"):
            s.set_models(models)
        assert s.num_models == 0 and s.num_channels() == 2
        s.set_models(models[:8])
        assert s.num_channels() == 16
        s.set_models(None)
    assert _lib.WOST_MAX_SOURCES == 16


# ---- 3. nothing moves for existing users ---------------------------------------------------
@pytest.mark.parametrize("jit", [True, False])
def test_own_fields_as_the_one_model_keep_every_bit(gpu_available, jit):
    sc, pts, models = _case("dd")
    s = _solver("dd", "reference")
    s.set_jit(jit)
    kw = dict(nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED)
    v0, s0 = s.solve_walks(pts, **kw)
    s.solve(pts, **kw)
    sums0 = s.last_point_sums.copy()
    assert s.last_timing["jit"] == (1 if jit else 0)
    s.set_models([models[0]])
    assert s.num_models == 1 and s.num_channels() == 1
    v1, s1 = s.solve_walks(pts, **kw)
    s.solve(pts, **kw)   # (one model: wost_solve is fine)
    assert s.last_timing["jit"] == (1 if jit else 0)
    np.testing.assert_array_equal(s0, s1)
    np.testing.assert_array_equal(_bits(v0), _bits(v1))
    np.testing.assert_array_equal(sums0, s.last_point_sums)
    # one OTHER model: the bits of a handle created with it, and eval_field evaluates it
    s.set_models([models[1]])
    one = _solver("dd", "reference", model=models[1])
    one.set_jit(jit)
    v2, s2 = s.solve_walks(pts, **kw)
    w2, t2 = one.solve_walks(pts, **kw)
    np.testing.assert_array_equal(s2, t2)
    np.testing.assert_array_equal(_bits(v2), _bits(w2))
    np.testing.assert_array_equal(s.eval_field("alpha", pts)[:, 0], np.full(len(pts), 100.0, np.float32))
    s.set_models(None)
    assert s.num_models == 0
    np.testing.assert_array_equal(_bits(s.eval_field("alpha", pts)), _bits(_solver("dd", "reference").eval_field("alpha", pts)))


def test_clearing_the_models_gives_the_plain_bits_again(gpu_available):
    sc, pts, models = _case("dd")
    s = _solver("dd", "reference")
    kw = dict(nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED)
    v0, s0 = s.solve_walks(pts, **kw)
    s.set_models(models)
    assert _multi(s, pts, sc.eps)[0] == 0
    with pytest.raises(ValueError, match="wost_solve_multi"):   # wost_solve needs one channel
        s.solve(pts, **kw)
    s.set_models(None)
    v1, s1 = s.solve_walks(pts, **kw)
    np.testing.assert_array_equal(s0, s1)
    np.testing.assert_array_equal(_bits(v0), _bits(v1))


def test_identical_models_give_identical_channels(gpu_available):
    from dcrmontecarlo_amd import survey

    sc, pts, models = _case("dd")
    s = _solver("dd", "reference")
    vals, _ = s.solve_models_walks(pts, [models[2], models[2]], nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED)
    np.testing.assert_array_equal(_bits(vals[0]), _bits(vals[1]))
    mean, se = survey.paired_difference(vals)
    assert np.all(mean == 0.0) and np.all(se == 0.0)


def test_models_info_counts_and_checksums(gpu_available):
    from dcrmontecarlo_amd import _lib

    def info(s):
        n, chk = ctypes.c_int32(-1), ctypes.c_uint64(1)
        assert _lib.lib.wost_models_info(s._h, ctypes.byref(n), ctypes.byref(chk)) == 0
        return n.value, chk.value

    sc, pts, models = _case("dd")
    a, b = _solver("dd", "reference"), _solver("dd", "reference")
    assert info(a) == (0, 0)
    a.set_models(models)
    b.set_models(models)
    assert info(a)[0] == 3 and info(a)[1] != 0 and info(a) == info(b)
    b.set_models(models[::-1])
    assert info(b)[0] == 3 and info(b)[1] != info(a)[1]
    b.set_models(models[:2])
    assert info(b)[0] == 2 and info(b)[1] != info(a)[1]
    a.set_models(None)
    assert info(a) == (0, 0)


def test_model_free_solves_refuse_a_solver_with_models(gpu_available):
    """solve_wavenumbers, solve_sources and their per-walk forms size their buffers for
    wavenumbers x sources: with models installed the library would write models x that, so
    they raise, change nothing, and work again once the models are cleared."""
    from dcrmontecarlo_amd import fields as F

    sc, pts, models = _case("sq")
    srcs = [sc.f, F.gaussian((-0.3, 0.4), 0.25, 2.0)]
    s = sc.solver(sigma_bar=_sigma_bar("sq") + 1.0)
    kw = dict(nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED)
    u_k = s.solve_wavenumbers(pts, [0.5, 1.0], **kw)
    u_s = s.solve_sources(pts, srcs, **kw)
    s.set_models(models[:2])
    for call in (lambda: s.solve_wavenumbers(pts, [0.5], **kw), lambda: s.solve_wavenumbers(pts, [0.5, 1.0], **kw),
                 lambda: s.solve_wavenumbers_walks(pts, [0.5], **kw),
                 lambda: s.solve_wavenumbers(pts, [0.5], sources=srcs, **kw),
                 lambda: s.solve_sources(pts, srcs, **kw), lambda: s.solve_sources_walks(pts, srcs, **kw)):
        with pytest.raises(ValueError, match="set_models"):
            call()
        assert s.num_models == 2 and s.num_channels() == 2 and s.wavenumbers is None
    s.set_models(None)
    np.testing.assert_array_equal(_bits(s.solve_wavenumbers(pts, [0.5, 1.0], **kw)), _bits(u_k))
    np.testing.assert_array_equal(_bits(s.solve_sources(pts, srcs, **kw)), _bits(u_s))


# ---- 4. shards -----------------------------------------------------------------------------
def test_walk_range_halves_merge_to_the_full_solve(gpu_available):
    from dcrmontecarlo_amd import _lib

    sc, pts, models = _case("dd")
    s = _solver("dd", "reference")
    s.set_models(models)
    _, blocks, rows, _, _ = _multi(s, pts, sc.eps)
    half = _lib.WOST_BLOCK_WALKS
    assert W == 2 * half
    lo = s.solve_range(pts, W, 0, half, STEPS, sc.eps, SEED)
    hi = s.solve_range(pts, W, half, W, STEPS, sc.eps, SEED)
    assert lo.shape == hi.shape == (len(pts), 1, 7)
    np.testing.assert_array_equal(lo[:, 0] + hi[:, 0], rows)
    np.testing.assert_array_equal(np.concatenate([lo, hi], axis=1).reshape(-1, 7), blocks)


def test_solve_distributed_one_rank_takes_the_models_channels(gpu_available):
    """wost_solve_distributed over a one-rank communicator scores the handle's C = 3 model
    channels (rows of 2C+1; its agreement key carries the models' checksum): bitwise the
    point sums of wost_solve_multi."""
    from dcrmontecarlo_amd import comm

    sc, pts, models = _case("dd")
    s = _solver("dd", "reference")
    s.set_models(models)
    rows = _multi(s, pts, sc.eps)[2]
    c = comm.Communicator(comm.unique_id(), 1, 0, 0)
    try:
        sums, timing = comm._distributed_sums(s, c, np.ascontiguousarray(pts, np.float32), W, STEPS, sc.eps, SEED)
    finally:
        c.close()
    assert sums.shape == (len(pts), 7) and (timing["walk_begin"], timing["walk_end"]) == (0, W)
    np.testing.assert_array_equal(sums, rows)


# ---- 5. refusals ---------------------------------------------------------------------------
def test_refusals(gpu_available):
    from dcrmontecarlo_amd import _lib
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey

    sc, pts, models = _case("dd")
    s = _solver("dd", "reference")
    # WOST_ERR_INVALID_ARG: a model with both fields NULL (through the library: the facade
    # refuses it before)
    arr = (_lib.WostModel * 2)()
    wf, keep = _lib.make_field(sc.alpha)
    arr[0].alpha = ctypes.pointer(wf)
    assert _lib.lib.wost_set_models(s._h, arr, 2) == _lib.WOST_ERR_INVALID_ARG
    assert b"neither" in _lib.lib.wost_last_error()
    with pytest.raises(ValueError, match="neither"):
        s.set_models([models[0], (None, None)])
    assert s.num_models == 0
    # ... a channel product above WOST_MAX_SOURCES, from each of the three setters
    with pytest.raises(ValueError, match="exceed 16 channels"):
        s.set_models([models[0]] * 17)
    s.set_models(models)                                   # 3 models
    with pytest.raises(ValueError, match="exceed 16 channels"):
        s.set_wavenumbers(np.linspace(0.1, 0.6, 6))        # x 6 wavenumbers
    keep6 = [_lib.make_field(sc.f) for _ in range(6)]
    six = (ctypes.POINTER(_lib.WostField) * 6)(*[ctypes.pointer(wf_) for wf_, _ in keep6])
    assert _lib.lib.wost_set_sources(s._h, six, 6) == _lib.WOST_ERR_INVALID_ARG   # x 6 sources
    assert b"exceed 16 channels" in _lib.lib.wost_last_error()
    s.set_wavenumbers([0.1, 0.2])                          # 3 x 2 = 6 channels: fine
    assert s.num_channels() == 6
    with pytest.raises(ValueError, match="exceed 16 channels"):
        s.set_models([models[0]] * 9)                      # 9 x 2
    assert s.num_models == 3                               # (a refused set changes nothing)
    s.set_wavenumbers(None)
    # wost_solve and wost_solve_history need one channel
    kw = dict(nWalks=64, maxSteps=STEPS, eps=sc.eps, seed=SEED)
    with pytest.raises(ValueError, match="wost_solve_multi"):
        s.solve(pts, **kw)
    with pytest.raises(ValueError, match="wost_solve_multi"):
        s.solve(pts, return_history=True, **kw)
    # WOST_ERR_UNSUPPORTED: several models with the field-specialised kernel disabled, at the solve
    s.set_jit(False)
    rc = _multi(s, pts, sc.eps)[0]
    assert rc == _lib.WOST_ERR_UNSUPPORTED and b"field-specialised" in _lib.lib.wost_last_error()
    s.set_jit(True)
    assert _multi(s, pts, sc.eps)[0] == 0
    # ... a handle without delta tracking
    plain = S.poisson_square(6).solver()
    with pytest.raises(NotImplementedError, match="delta tracking"):
        plain.set_models([(None, F.const(2.0))])
    plain.set_models(None)                                 # (clearing none is fine)
    # ... several models together with point charges, from whichever setter comes second
    ps = dataclasses.replace(sc, f=None).solver(compat="fixed", sigma_bar=_sigma_bar("dd"))
    charges = [survey.point_dipole(sc.points[1], sc.points[2])]
    ps.set_point_sources(charges)
    with pytest.raises(NotImplementedError, match="point sources"):
        ps.set_models(models[:2])
    ps.set_models(models[1:2])                             # (one model is fine)
    ps.set_models(None)
    ps.set_point_sources(None)
    ps.set_models(models[:2])
    with pytest.raises(NotImplementedError, match="several models"):
        ps.set_point_sources(charges)
    assert ps.point_sources is None and ps.num_models == 2


# ---- 6. surveys ----------------------------------------------------------------------------
def _same_survey(a, b):
    for name in ("u_model", "u_background"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    for name in ("model", "background"):
        np.testing.assert_array_equal(getattr(a, name).dv, getattr(b, name).dv, err_msg=name)
        np.testing.assert_array_equal(getattr(a, name).se, getattr(b, name).se, err_msg=name)
    np.testing.assert_array_equal(a.rho.rho_a, b.rho.rho_a)
    np.testing.assert_array_equal(a.rho.se, b.rho.se)
    np.testing.assert_array_equal(a.rho.resolved, b.rho.resolved)
    assert a.walk_steps > 0 and 2 * b.walk_steps == a.walk_steps


def test_shared_walk_surveys_equal_the_default_path(gpu_available):
    from dcrmontecarlo_amd import survey

    sc, _, _ = _case("dd")
    a = survey.run_dipole_dipole(sc, 100.0, W, seed=SEED)
    b = survey.run_dipole_dipole(sc, 100.0, W, seed=SEED, shared_walks=True)
    _same_survey(a, b)
    assert np.count_nonzero(a.u_model) > 0
    a = survey.run_dipole_dipole_survey(sc, 100.0, W, n_max=2, seed=SEED)
    b = survey.run_dipole_dipole_survey(sc, 100.0, W, n_max=2, seed=SEED, shared_walks=True)
    np.testing.assert_array_equal(a.quadripoles, b.quadripoles)
    np.testing.assert_array_equal(a.transmitters, b.transmitters)
    _same_survey(a, b)
    assert np.count_nonzero(a.u_model) > 0


def test_shared_walk_survey_beyond_one_launch(gpu_available):
    """More than 8 transmitters no longer fit one launch with both models (16 channels): the
    launches keep model and background together, are never more than the default path's two
    solvers need, the arrays stay bitwise the default's, and walk_steps counts every launch's
    walk set."""
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import survey
    from dcrmontecarlo_amd.solvers.WoStSolver import _model_chunks

    sc = dataclasses.replace(S.dcr_dipole(12, n_walks=W), max_steps=STEPS)
    n_walks = 4096
    sm = sc.solver()
    sh = survey.homogeneous_solver(sc, 100.0, sm)
    a = survey.run_dipole_dipole_survey(sc, 100.0, n_walks, n_max=2, seed=SEED, solvers=(sm, sh))
    T = len(a.transmitters)
    assert 8 < T <= 16
    default_launches = 2 * -(-T // 16)
    shared = sc.solver()
    b = survey.run_dipole_dipole_survey(sc, 100.0, n_walks, n_max=2, seed=SEED, solvers=shared, shared_walks=True)
    assert _model_chunks(2, T, 1, 16) == (2, 8, 1)
    assert shared.last_timing["n_launches"] == -(-T // 8) <= default_launches
    np.testing.assert_array_equal(a.transmitters, b.transmitters)
    for name in ("u_model", "u_background"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    np.testing.assert_array_equal(a.rho.rho_a, b.rho.rho_a)
    np.testing.assert_array_equal(a.rho.se, b.rho.se)
    # every launch walks the same paths (the seed and the points are the same): its steps, times the launches
    one_set = sm.last_timing["total_steps"]
    assert b.walk_steps == shared.last_timing["n_launches"] * one_set == shared.last_timing["total_steps"]
    assert np.count_nonzero(a.u_model) > 0


# ---- 7. pairing pays -----------------------------------------------------------------------
def test_pairing_lowers_the_error_of_a_difference(gpu_available):
    """u_1 - u_0 for the conductive inclusion scaled by 1.01: the paired standard error
    (per-walk differences on shared paths) against sqrt(se_0^2 + se_1^2) of two solves with
    different seeds. Measured on an MI355X (6 electrodes x 8192 walks, maxSteps 200): the
    ratio paired / unpaired per electrode is recorded in DESIGN.md 7c, its largest value in
    PAIRED_RATIO_MEASURED above; the bound is 4x that, capped at 1."""
    from dcrmontecarlo_amd import survey

    sc, pts, models = _case("dd")
    s = _solver("dd", "reference")
    pair = [models[0], models[2]]
    vals, _ = s.solve_models_walks(pts, pair, nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED)
    mean, se = survey.paired_difference(vals)
    paired = se[1]
    _, st0 = _solver("dd", "reference", model=pair[0]).solve(pts, nWalks=W, maxSteps=STEPS, eps=sc.eps, seed=SEED,
                                                             return_stats=True)
    _, st1 = _solver("dd", "reference", model=pair[1]).solve(pts, nWalks=W, maxSteps=STEPS, eps=sc.eps,
                                                             seed=SEED + 1, return_stats=True)
    unpaired = np.sqrt(st0.stderr ** 2 + st1.stderr ** 2)
    ratio = paired / unpaired
    print("paired difference", mean[1], "\npaired se", paired, "\nunpaired se", unpaired, "\nratio", ratio)
    v64 = vals.astype(np.float64)
    np.testing.assert_allclose(mean[1], v64[1].mean(1) - v64[0].mean(1), rtol=0, atol=1e-12 * np.abs(v64).max())
    assert np.all(paired < unpaired)            # the hard condition: strictly smaller at every point
    assert np.all(ratio <= PAIRED_RATIO_BOUND)
