"""The Dirichlet segment tree on the device (wost_set_dirichlet_tree): the query
(wost_geometry_query DISTANCE | TREE) and whole walks of the field-specialised kernels give the
bits of the full scans, with every trait and channel count the kernels compose with, and the
handle reports which path ran. Host fuzz and generated source: tests/test_dirichlet_tree.py."""
import ctypes
import dataclasses

import numpy as np
import pytest

import dtree_shapes as SH

pytestmark = pytest.mark.gpu

U = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    """Bitwise equal, NaN payload-insensitive."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape
    ok = (U(a) == U(b)) | (np.isnan(a) & np.isnan(b))
    assert ok.all(), f"{(~ok).sum()} of {ok.size} values differ"


def _laplace(verts, tree, jit=True, **kw):
    """X^2 - Y^2 in the polygon `verts`; tree: set_dirichlet_tree's min_segments."""
    from dcrmontecarlo_amd.fields import X, Y
    from dcrmontecarlo_amd.geometry import PolyLinesSimple
    from dcrmontecarlo_amd.solvers import WostSolver_2D

    s = WostSolver_2D(PolyLinesSimple(verts), X**2 - Y**2, **kw)
    s.set_dirichlet_tree(tree)
    s.set_jit(jit)
    return s


def _ran(s, jit, tree):
    t = s.last_timing
    assert (t["jit"], t["dirichlet_tree"]) == (jit, tree), (t["jit"], t["dirichlet_tree"])
    assert s.dirichlet_tree()["last_solve"] == bool(tree)


# ---- 1. the device query ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["ngon641", "zigzag", "ngon6001"])
def test_device_query_equals_scan(gpu_available, name):
    from dcrmontecarlo_amd.geometry import PolyLinesSimple

    verts = {"ngon641": lambda: SH.ngon(641), "zigzag": SH.zigzag, "ngon6001": lambda: SH.ngon(6001)}[name]()
    rng = np.random.default_rng(len(verts))
    lo, hi = verts.min(0), verts.max(0)
    uni = (0.5 * (lo + hi) + (rng.random((4096, 2)) * 2 - 1) * (hi - lo)).astype(np.float32)
    special = np.concatenate([verts[:: max(1, len(verts) // 500)], verts[:-1].mean(0, keepdims=True),
                              np.array([[np.nan, 0.1], [np.inf, 0.0], [1e30, -1e30]], np.float32)])
    pts = np.concatenate([special, uni])[:4096].astype(np.float32)
    assert np.isnan(pts).any()
    poly = PolyLinesSimple(verts)
    scan = poly.distance(pts)
    tree = poly.distance(pts, tree=True)
    _same_bits(scan, tree)
    assert np.isfinite(scan).sum() > 4000


def test_device_query_refuses_a_degenerate_polyline(gpu_available):
    from dcrmontecarlo_amd.geometry import PolyLinesSimple

    verts = SH.ngon(641)
    rep = PolyLinesSimple(np.insert(verts, 100, verts[100], axis=0))
    with pytest.raises(ValueError, match="nonzero length"):
        rep.distance(np.zeros((4, 2), np.float32), tree=True)
    assert np.isnan(rep.distance(np.zeros((4, 2), np.float32))).all()   # the scan: NaN, as the reference


# ---- 2. Laplace at a staged size ----------------------------------------------------------
PTS3 = np.array([[0.1, 0.2], [-0.5, 0.3], [0.0, -0.7]], np.float32)   # test_gpu_long_polylines.py


def test_laplace_staged_size(gpu_available):
    verts = SH.ngon(641)
    kw = dict(nWalks=2048, maxSteps=1000, eps=1e-3, seed=5)
    on = _laplace(verts, 0)
    assert on.dirichlet_tree() == {"min_segments": 0, "leaf_segments": 10, "usable": True, "last_solve": False}
    v0, s0 = on.solve_walks(PTS3, **kw)
    _ran(on, 1, 1)
    off = _laplace(verts, -1)
    v1, s1 = off.solve_walks(PTS3, **kw)
    _ran(off, 1, 0)
    pre = _laplace(verts, 0, jit=False)
    v2, s2 = pre.solve_walks(PTS3, **kw)
    _ran(pre, 0, 0)
    for v, s in ((v1, s1), (v2, s2)):
        np.testing.assert_array_equal(s0, s)
        np.testing.assert_array_equal(U(v0), U(v))
    leaf = _laplace(verts, 0)
    leaf.set_dirichlet_tree(0, 3)                                  # another leaf size: the same bits
    v3, s3 = leaf.solve_walks(PTS3, **kw)
    _ran(leaf, 1, 1)
    np.testing.assert_array_equal(s0, s3)
    np.testing.assert_array_equal(U(v0), U(v3))


# ---- 3. Laplace beyond the LDS budget -----------------------------------------------------
def test_laplace_beyond_the_lds_budget(gpu_available):
    verts = SH.ngon(6001)                                          # 48 KB of vertices
    kw = dict(nWalks=1024, maxSteps=1000, eps=1e-3, seed=5)
    on = _laplace(verts, 0)
    v0, s0 = on.solve_walks(PTS3, **kw)
    _ran(on, 1, 1)
    gl = _laplace(verts, -1)                                       # the scan from global memory (GL)
    v1, s1 = gl.solve_walks(PTS3, **kw)
    _ran(gl, 1, 0)
    pre = _laplace(verts, 0, jit=False)
    v2, s2 = pre.solve_walks(PTS3, **kw)
    _ran(pre, 0, 0)
    for v, s in ((v1, s1), (v2, s2)):
        np.testing.assert_array_equal(s0, s)
        np.testing.assert_array_equal(U(v0), U(v))
    _, st = on.solve(PTS3, nWalks=100_000, maxSteps=1000, eps=1e-3, seed=6, return_stats=True)
    _ran(on, 1, 1)
    exact = PTS3[:, 0].astype(np.float64) ** 2 - PTS3[:, 1].astype(np.float64) ** 2
    # eps |grad u| <= 2e-3, and the polygon is the domain: nothing else biases it
    assert np.all(np.abs(st.mean - exact) <= 5 * st.stderr + 3e-3), (st.mean, exact)


# ---- 4. both trees, both estimators -------------------------------------------------------
@pytest.mark.parametrize("compat", ["reference", "fixed"])
def test_both_trees_both_estimators(gpu_available, compat):
    from dcrmontecarlo_amd.fields import X
    from dcrmontecarlo_amd.geometry import PolyLinesSimple
    from dcrmontecarlo_amd.solvers import WostSolver_2D

    D = SH.resample([[0, -0.5], [1, -0.5], [1, 1], [0, 1], [0, -0.5]], 600)
    xs = np.linspace(1.0, 0.0, 601, dtype=np.float32)
    N = np.stack([xs, np.zeros(601, np.float32)], axis=1)          # y = 0, right to left
    pts = np.array([[0.3, 0.5], [0.6, 0.1], [0.8, 0.7]], np.float32)
    ref = None
    for ntree in (0, -1):
        for dtree in (0, -1):
            s = WostSolver_2D(PolyLinesSimple(D), X, PolyLinesSimple(N), compat=compat)
            s.set_segment_tree(ntree)
            s.set_dirichlet_tree(dtree)
            v, st = s.solve_walks(pts, nWalks=1024, maxSteps=2000, eps=1e-3, seed=7)
            _ran(s, 1, int(dtree == 0))
            assert s.last_timing["tree"] == int(ntree == 0)
            if ref is None:
                ref = (v, st)
            np.testing.assert_array_equal(ref[1], st)
            np.testing.assert_array_equal(U(ref[0]), U(v))
    assert ref[1].max() > 1                                        # (walks that stepped)


# ---- 5. delta tracking, Neumann scan, several channels ------------------------------------
def _vc(tree, **kw):
    from dcrmontecarlo_amd import scenarios as S

    sc = S.variable_coefficients(6, n_walks=4096)
    sc = dataclasses.replace(sc, dirichlet=SH.resample(sc.dirichlet.astype(np.float64), 256), max_steps=200)
    s = sc.solver(**kw)
    s.set_dirichlet_tree(tree)
    return sc, s


def test_delta_tracking_channels(gpu_available):
    from dcrmontecarlo_amd import fields as F
    from dcrmontecarlo_amd import survey
    from dcrmontecarlo_amd.fields import X, Y

    sc, probe = _vc(-1)
    ks = [0.3, 0.9]
    smooth = 0.5 + 1.5 * F.exp(-2.0 * (X**2 + Y**2))
    models = [(sc.sigma, smooth), (0.5 + 0.25 * (1 + F.sin(X) * F.cos(Y)), 0.8 + 0.4 * F.exp(-1.0 * (X**2 + Y**2)))]
    sources = [sc.f, 2.0 * sc.f + 0.1]
    sb_k = probe.sigma_bar + max(ks) ** 2
    sb_m = survey.sigma_bar_for_models(probe, models)
    kw = dict(nWalks=4096, maxSteps=200, eps=sc.eps, seed=9)
    runs = {
        "plain": (None, lambda s: s.solve_walks(sc.points, **kw)),
        "sources": (None, lambda s: s.solve_sources_walks(sc.points, sources, **kw)),
        "wavenumbers": (sb_k, lambda s: s.solve_wavenumbers_walks(sc.points, ks, **kw)),
        "models": (sb_m, lambda s: s.solve_models_walks(sc.points, models, **kw)),
    }
    for name, (sb, run) in runs.items():
        out = []
        for tree in (0, -1):
            _, s = _vc(tree, **({"sigma_bar": sb} if sb else {}))
            out.append(run(s))
            _ran(s, 1, int(tree == 0))
            assert s.last_timing["tree"] == 0                     # the 32-segment Neumann circle is scanned
        np.testing.assert_array_equal(out[0][1], out[1][1], err_msg=name)
        np.testing.assert_array_equal(U(out[0][0]), U(out[1][0]), err_msg=name)
        assert out[0][0].shape[0] == (6 if name == "plain" else 2)
        assert np.isfinite(out[0][0]).all() and np.abs(out[0][0]).max() > 0


# ---- 6. point sources ---------------------------------------------------------------------
def test_point_sources(gpu_available):
    from dcrmontecarlo_amd.geometry import PolyLinesSimple
    from dcrmontecarlo_amd.solvers import WostSolver_2D

    verts = SH.ngon(257)                                           # 256 segments
    pts = np.array([[0.1, 0.2], [-0.5, 0.3], [0.0, -0.7], [0.4, 0.4]], np.float32)
    out = []
    for tree in (0, -1):
        s = WostSolver_2D(PolyLinesSimple(verts), 0.0, compat="fixed")
        s.set_point_sources([[((0.2, 0.1), 1.0), ((-0.3, -0.2), -1.0)]])
        s.set_dirichlet_tree(tree)
        out.append(s.solve_walks(pts, nWalks=2048, maxSteps=1000, eps=1e-3, seed=4))
        _ran(s, 1, int(tree == 0))
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(U(out[0][0]), U(out[1][0]))
    assert np.abs(out[0][0]).max() > 0


# ---- 7. the recorder ----------------------------------------------------------------------
def test_recorder_stores_the_scans_distances(gpu_available):
    from dcrmontecarlo_amd import _lib

    verts = SH.ngon(641)
    pts = np.ascontiguousarray(PTS3[:2])
    n, W, steps = 2, 64, 1000
    recs = []
    for tree in (0, -1):
        s = _laplace(verts, tree)
        sums = np.zeros((n, 3))
        wv, ws = np.empty(n * W, np.float32), np.empty(n * W, np.uint32)
        rec = np.zeros((n * W, steps + 1, _lib.REC_FLOATS), np.float32)
        _lib.check(_lib.lib.wost_solve_history(s._h, _lib.fptr(pts), n, W, steps, 1e-3, 12, _lib.dptr(sums),
                                               _lib.fptr(wv), _lib.u32ptr(ws), _lib.fptr(rec)), "wost_solve_history")
        assert s.dirichlet_tree()["last_solve"] == (tree == 0)
        recs.append((sums, wv, ws, rec))
    a, b = recs
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(U(a[1]), U(b[1]))
    np.testing.assert_array_equal(a[0], b[0])
    used = np.arange(steps + 1)[None, :] <= a[2][:, None]         # records 0 .. steps of each walk
    assert used.sum() > n * W * 2
    _same_bits(a[3][used], b[3][used])                            # x, y, dD, dN (NaN), sample, c, src
    assert np.isfinite(a[3][used][:, 2]).all()                    # the stored Dirichlet distances


# ---- 8. state -----------------------------------------------------------------------------
def test_toggling_on_a_warm_handle(gpu_available):
    verts = SH.ngon(641)
    kw = dict(nWalks=1024, maxSteps=1000, eps=1e-3, seed=2)
    s = _laplace(verts, 0)
    ref = None
    for tree in (0, -1, 0, 100_000, None):
        s.set_dirichlet_tree(tree)
        v, st = s.solve_walks(PTS3, **kw)
        from dcrmontecarlo_amd import _lib
        dflt = _lib.WOST_DTREE_MIN_SEGMENTS_DEFAULT
        want = tree == 0 or (tree is None and 0 <= dflt <= 640)
        _ran(s, 1, int(want))
        if ref is None:
            ref = (v, st)
        np.testing.assert_array_equal(ref[1], st)
        np.testing.assert_array_equal(U(ref[0]), U(v))


def test_repeated_vertex_keeps_scanning(gpu_available):
    """A polyline with a zero-length segment: the scan's distance is NaN everywhere (0/0), as
    the reference's distance_to_polyline_jit. The handle does not admit the tree, scans even
    when the tree is forced, and returns what the scanning kernels return: the recorded
    Dirichlet distance of every step is NaN (the walk's value need not be: Python's
    max(rmin, NaN) of :215 is rmin, and dD > eps then ends the walk)."""
    from dcrmontecarlo_amd import _lib

    verts = SH.ngon(641)
    rep = np.insert(verts, 100, verts[100], axis=0)
    kw = dict(nWalks=256, maxSteps=20, eps=1e-3, seed=2)
    on = _laplace(rep, 0)
    assert on.dirichlet_tree()["usable"] is False
    v0, s0 = on.solve_walks(PTS3, **kw)
    _ran(on, 1, 0)
    pre = _laplace(rep, 0, jit=False)
    v1, s1 = pre.solve_walks(PTS3, **kw)
    np.testing.assert_array_equal(s0, s1)
    _same_bits(v0, v1)
    off = _laplace(rep, -1)
    v2, s2 = off.solve_walks(PTS3, **kw)
    _ran(off, 1, 0)
    np.testing.assert_array_equal(s0, s2)
    _same_bits(v0, v2)
    n, W, steps = 3, 16, 20
    sums = np.zeros((n, 3))
    wv, ws = np.empty(n * W, np.float32), np.empty(n * W, np.uint32)
    rec = np.zeros((n * W, steps + 1, _lib.REC_FLOATS), np.float32)
    pts = np.ascontiguousarray(PTS3)
    _lib.check(_lib.lib.wost_solve_history(on._h, _lib.fptr(pts), n, W, steps, 1e-3, 2, _lib.dptr(sums),
                                           _lib.fptr(wv), _lib.u32ptr(ws), _lib.fptr(rec)), "wost_solve_history")
    assert on.dirichlet_tree()["last_solve"] is False
    assert (ws >= 1).all()
    step = np.arange(steps + 1)[None, :] < ws[:, None]            # the step records of each walk
    assert np.isnan(rec[..., 2][step]).all()                      # dD: NaN where the reference's is
