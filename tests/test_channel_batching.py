"""Channel batching on the CPU (dcrmontecarlo_amd/solvers/channels.py and WostSolver_2D's
launch plan runner): the launch plan as a pure function, and every multi-launch solve path
against a recording stand-in for libwost.

The stand-in (FakeLib) implements the entry points these paths use, logs every call with its
scalar arguments, answers wost_num_channels from what is installed and fills the output
arrays of wost_solve_multi with values unique per (launch, channel, point, walk). It does
not walk, so the cases use 3 query points and 5 walks.

tests/golden/channel_batching_parent.json holds what the cases gave on the commit before
the plan and runner replaced the four hand-written solve loops: per case the call log, a
SHA-256 of every returned array (with shape and dtype) and every SolveStats field, the final
``last_timing`` and the solver's attributes. The cases must give the same here. To record the
file again (on a commit whose behaviour is the contract), run this module's cases in one
process with WOST_RECORD_CHANNEL_GOLDEN=1 in the environment."""
import ctypes
import dataclasses
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "channel_batching_parent.json")
RECORD = os.environ.get("WOST_RECORD_CHANNEL_GOLDEN") == "1"
PTS = np.array([[0.25, 0.25], [0.5, 0.5], [0.75, 0.3]], np.float32)
N, W = 3, 5


# ---- the stand-in ----------------------------------------------------------------------------
def _coefs(field_ptr):
    """A wost_field pointer's term coefficients (the cases' fields are constants: one term each)."""
    if not field_ptr:
        return None
    f = field_ptr.contents
    return [float(f.terms[i].coef) for i in range(f.n_terms)]


class FakeLib:
    """libwost's entry points of the channel paths, recording. ``fail_launch``: the launch
    (1-based) whose wost_solve_multi returns WOST_ERR_INVALID_ARG."""

    def __init__(self, fail_launch=None):
        self.log, self.launch, self.fail_launch = [], 0, fail_launch
        self.sources, self.models, self.wavenumbers = 1, 0, 0

    # -- handle ---------------------------------------------------------------------------------
    def wost_create(self, prob, h):
        h._obj.value = 0x1000
        self.log.append(["wost_create"])
        return 0

    def wost_destroy(self, h):
        self.log.append(["wost_destroy"])

    def wost_last_error(self):
        return b"the stand-in refused"

    def wost_get_info(self, h, sigma_bar, delta):
        sigma_bar._obj.value, delta._obj.value = 3.5, 1
        self.log.append(["wost_get_info"])
        return 0

    def wost_num_blocks(self, n, walks):
        self.log.append(["wost_num_blocks", int(n), int(walks)])
        return int(n) * -(-int(walks) // 4096)

    def wost_dirichlet_tree_info(self, h, a, b, c, d):
        for x, v in zip((a, b, c, d), (128, 10, 1, 0)):
            x._obj.value = v
        self.log.append(["wost_dirichlet_tree_info"])
        return 0

    # -- channels -------------------------------------------------------------------------------
    def wost_set_field(self, h, slot, field):
        self.log.append(["wost_set_field", int(slot), _coefs(field)])
        if slot == 1:
            self.sources = 1
        return 0

    def wost_set_sources(self, h, arr, n):
        self.log.append(["wost_set_sources", int(n), [_coefs(arr[i]) for i in range(n)]])
        self.sources = int(n)
        return 0

    def wost_set_point_sources(self, h, arr, n, n_sources):
        self.log.append(["wost_set_point_sources", int(n), int(n_sources),
                         [[arr[i].x, arr[i].y, arr[i].strength, arr[i].source] for i in range(n)]])
        self.sources = max(1, int(n_sources))
        return 0

    def wost_set_models(self, h, arr, n):
        self.log.append(["wost_set_models", int(n), [[_coefs(arr[i].sigma), _coefs(arr[i].alpha)] for i in range(n)]])
        self.models = int(n)
        return 0

    def wost_models_info(self, h, n, checksum):
        n._obj.value = self.models
        self.log.append(["wost_models_info"])
        return 0

    def wost_set_wavenumbers(self, h, k2, n):
        self.log.append(["wost_set_wavenumbers", int(n), [float(k2[i]) for i in range(n)]])
        self.wavenumbers = int(n)
        return 0

    def channels(self):
        return max(1, self.models) * max(1, self.wavenumbers) * self.sources

    def wost_num_channels(self, h, n):
        n._obj.value = self.channels()
        self.log.append(["wost_num_channels", self.channels()])
        return 0

    # -- solves ---------------------------------------------------------------------------------
    def wost_last_timing(self, h, t):
        for i, (name, typ) in enumerate(type(t._obj)._fields_):
            v = (i + 1) * self.launch
            setattr(t._obj, name, v + 0.5 if typ is ctypes.c_double else v)
        self.log.append(["wost_last_timing"])
        return 0

    def wost_solve_multi(self, h, pts, n, walks, b0, b1, max_steps, eps, seed, block_sums, point_sums, wv, ws):
        self.launch += 1
        L, C = self.launch, self.channels()
        self.log.append(["wost_solve_multi", int(n), int(walks), int(b0), int(b1), int(max_steps), float(eps),
                         int(seed), bool(block_sums), bool(point_sums), bool(wv), bool(ws), C])
        if L == self.fail_launch:
            return -1
        p = np.arange(n, dtype=np.float64)[:, None]
        c = np.arange(C, dtype=np.float64)[None, :]
        rows = np.ctypeslib.as_array(point_sums, shape=(n, 2 * C + 1))
        s = (L * 100.0 + c * 7.0 + p) * 0.37 + 1.0
        rows[:, 0:2 * C:2] = s
        rows[:, 1:2 * C:2] = s * s / walks + (L + 2.0 * c + 3.0 * p + 1.0) * 1.3
        rows[:, -1] = 50.0 * walks + L * 10.0 + p[:, 0]
        if wv:
            w = np.arange(walks, dtype=np.float64)
            v = np.ctypeslib.as_array(wv, shape=(n, walks, C))
            v[...] = L * 1000.0 + c[None] * 50.0 + p[:, :, None] * 7.0 + w[None, :, None] * 0.125
            st = np.ctypeslib.as_array(ws, shape=(n, walks))
            st[...] = (L * 100 + p * 10 + w[None, :]).astype(np.uint32)
        return 0

    def wost_solve_range_combined(self, h, pts, n, ids, n_ids, walks, w0, w1, max_steps, eps, seed, weights, n_rows,
                                  block_sums, point_sums, channel_sums):
        self.launch += 1
        C = self.channels()
        wts = np.ctypeslib.as_array(weights, shape=(n_rows, C))
        self.log.append(["wost_solve_range_combined", int(n), bool(ids), int(n_ids), int(walks), int(w0), int(w1),
                         int(max_steps), float(eps), int(seed), int(n_rows), hashlib.sha256(wts.tobytes()).hexdigest(),
                         bool(point_sums), bool(channel_sums), C])
        blocks = -(-(int(w1) - int(w0)) // 4096)
        bs = np.ctypeslib.as_array(block_sums, shape=(n, blocks, 2 * n_rows + 1))
        p = np.arange(n, dtype=np.float64)[:, None, None]
        r = np.arange(n_rows, dtype=np.float64)[None, None, :]
        s = (self.launch * 100.0 + r * 7.0 + p) * 0.37 + 1.0
        bs[:, :, 0:2 * n_rows:2] = s
        bs[:, :, 1:2 * n_rows:2] = s * s / walks + (2.0 * r + 3.0 * p + 1.0) * 1.3
        bs[:, :, -1] = 50.0 * walks + p[:, :, 0]
        return 0

    def wost_last_combine_ms(self, h, ms):
        ms._obj.value = 0.75
        self.log.append(["wost_last_combine_ms"])
        return 0


# ---- what a case leaves behind ---------------------------------------------------------------
def _digest(x):
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        return {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}
    if dataclasses.is_dataclass(x):
        return {f.name: _digest(getattr(x, f.name)) for f in dataclasses.fields(x)}
    if isinstance(x, (tuple, list)):
        return [_digest(v) for v in x]
    return x


def _state(s):
    return {"wavenumbers": None if s.wavenumbers is None else [float(k) for k in s.wavenumbers],
            "models": repr(s.models), "point_sources": repr(s.point_sources)}


def _square():
    from dcrmontecarlo_amd import PolyLinesSimple

    return PolyLinesSimple(np.array([[0, 0], [1, 0], [1, 1], [0, 1], [0, 0]], np.float32))


def _field_solver():
    from dcrmontecarlo_amd import WostSolver_2D

    return WostSolver_2D(_square(), 0.0, None, source=2.0, sigma=0.5, alpha=1.0, compat="fixed", device=0)


def _point_solver():
    from dcrmontecarlo_amd import WostSolver_2D

    return WostSolver_2D(_square(), 0.0, None, sigma=0.5, alpha=1.0, compat="fixed", device=0)


def _sources(n):
    return [float(i + 1) for i in range(n)]


def _models(n):
    return [(0.125 * (m + 1), 1.0 + m) for m in range(n)]


def _dipoles(n):
    from dcrmontecarlo_amd import survey

    return [survey.point_dipole((0.05 * (i + 1), 0.5), (0.05 * (i + 2), 0.5), 1.0 + i) for i in range(n)]


def _charges(n_sources, per_source):
    return [[((0.01 * (per_source * s + j + 1), 0.25), 1.0 + j) for j in range(per_source)] for s in range(n_sources)]


KW = dict(nWalks=W, maxSteps=77, eps=2e-3)
K5, K20, K2 = np.linspace(0.25, 1.25, 5), np.linspace(0.1, 2.0, 20), np.array([0.5, 1.5])


def _preset(s):
    s.set_wavenumbers([0.3])
    s.set_models(_models(2))


def _transformed(s, sources):
    """wavenumber.transformed_potentials' one-launch device path, on a solver with a wavenumber set."""
    from dcrmontecarlo_amd import wavenumber

    s.set_wavenumbers([0.3])
    return wavenumber.transformed_potentials([s], [np.arange(2)], PTS, sources, K2, [0.4, 0.6], W, 77, 2e-3, seed=9,
                                             device_reduce=True)


def _restoring(s):
    """solve_wavenumbers refuses a solver with models set, so the models come back by hand
    around it; solve_models then runs with both set."""
    s.set_wavenumbers([0.3])
    s.set_models(None)
    a = s.solve_wavenumbers(PTS, K5, sources=_sources(7), seed=5, return_stats=True, **KW)
    s.set_models(_models(2))
    return a, s.solve_models(PTS, _models(9), sources=_sources(2), seed=6, return_stats=True, **KW)


F, P = _field_solver, _point_solver
ST = dict(return_stats=True, **KW)
# name: (solver factory, what runs)
CASES = {
    "sources_19": (F, lambda s: s.solve_sources(PTS, _sources(19), seed=-3, **ST)),
    "sources_19_walks": (F, lambda s: s.solve_sources_walks(PTS, _sources(19), seed=-3, **KW)),
    "point_dipoles_17": (P, lambda s: s.solve_point_sources(PTS, _dipoles(17), seed=4, **ST)),
    "point_dipoles_17_walks": (P, lambda s: s.solve_point_sources_walks(PTS, _dipoles(17), seed=4, **KW)),
    "point_charges_3x12": (P, lambda s: s.solve_point_sources(PTS, _charges(3, 12), seed=4, **ST)),
    "point_charges_3x12_walks": (P, lambda s: s.solve_point_sources_walks(PTS, _charges(3, 12), seed=4, **KW)),
    "wavenumbers_5x7": (F, lambda s: s.solve_wavenumbers(PTS, K5, sources=_sources(7), seed=5, **ST)),
    "wavenumbers_5x7_walks": (F, lambda s: s.solve_wavenumbers_walks(PTS, K5, sources=_sources(7), seed=5, **KW)),
    "wavenumbers_20": (F, lambda s: s.solve_wavenumbers(PTS, K20, seed=5, **ST)),
    "wavenumbers_20_walks": (F, lambda s: s.solve_wavenumbers_walks(PTS, K20, seed=5, **KW)),
    "wavenumbers_2x17_dipoles": (P, lambda s: s.solve_wavenumbers(PTS, K2, sources=_dipoles(17), seed=5, **ST)),
    "wavenumbers_2x17_dipoles_walks": (P, lambda s: s.solve_wavenumbers_walks(PTS, K2, sources=_dipoles(17), seed=5, **KW)),
    "models_9x2": (F, lambda s: s.solve_models(PTS, _models(9), sources=_sources(2), seed=6, **ST)),
    "models_2x9": (F, lambda s: s.solve_models(PTS, _models(2), sources=_sources(9), seed=6, **ST)),
    "models_20": (F, lambda s: s.solve_models(PTS, _models(20), seed=6, **ST)),
    "models_3x2x2": (F, lambda s: s.solve_models(PTS, _models(3), sources=_sources(2), k=K2, seed=6, **ST)),
    "models_3x2x2_walks": (F, lambda s: s.solve_models_walks(PTS, _models(3), sources=_sources(2), k=K2, seed=6, **KW)),
    "models_differences_3x2x2": (F, lambda s: s.solve_models_differences(PTS, _models(3), sources=_sources(2), k=K2,
                                                                         seed=6, **KW)),
    "transformed_on_the_device_2x3": (F, lambda s: _transformed(s, _sources(3))),
    "transformed_on_the_device_2x3_dipoles": (P, lambda s: _transformed(s, _dipoles(3))),
    "restoring_wavenumbers_and_models": (F, _restoring),
    "refuses_sources_with_wavenumbers": (F, lambda s: (s.set_wavenumbers([0.5, 1.5]),
                                                       s.solve_sources(PTS, _sources(3), **KW))),
    "refuses_point_sources_with_wavenumbers": (P, lambda s: (s.set_wavenumbers([0.5, 1.5]),
                                                             s.solve_point_sources(PTS, _dipoles(3), **KW))),
    "refuses_wavenumbers_with_models": (F, lambda s: (s.set_models(_models(2)), s.solve_wavenumbers(PTS, K2, **KW))),
    "refuses_mixed_sources": (F, lambda s: s.solve_wavenumbers(PTS, K2, sources=[1.0, _dipoles(1)[0]], **KW)),
    "refuses_zero_walks": (F, lambda s: s.solve_models(PTS, _models(2), nWalks=0)),
    "failing_wavenumbers_5x7": (F, lambda s: (s.set_wavenumbers([0.3]),
                                              s.solve_wavenumbers(PTS, K5, sources=_sources(7), seed=5, **KW))),
    "failing_models_9x2": (F, lambda s: (_preset(s), s.solve_models(PTS, _models(9), sources=_sources(2), seed=6, **KW))),
    "failing_sources_19": (F, lambda s: s.solve_sources(PTS, _sources(19), seed=-3, **KW)),
}
FAILING_LAUNCH = 2   # of the "failing" cases: the stand-in refuses their second launch


def _run(name, monkeypatch):
    from dcrmontecarlo_amd import _lib

    make, body = CASES[name]
    fake = FakeLib(FAILING_LAUNCH if name.startswith("failing") else None)
    monkeypatch.setattr(_lib, "lib", fake)
    s = make()
    try:
        out = {}
        # (a case's own setters come first in its body; what must come back is their state)
        try:
            out["result"] = _digest(body(s))
        except Exception as e:   # noqa: BLE001 -- the refusals and failing launches are cases
            out["raised"] = [type(e).__name__, str(e)]
        out["state"] = _state(s)
        out["last_timing"] = s.last_timing
        out["log"] = fake.log
    finally:
        s.__del__()   # (while the stand-in is installed: the real wost_destroy must never see this handle)
    return json.loads(json.dumps(out))


# ---- the cases against the parent's record ---------------------------------------------------
@pytest.fixture(scope="module")
def parent():
    if RECORD:
        return {}
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_the_parent(name, parent, monkeypatch):
    got = _run(name, monkeypatch)
    if RECORD:
        parent[name] = got
        if len(parent) == len(CASES):
            with open(GOLDEN, "w") as f:
                json.dump(parent, f, indent=0, sort_keys=True)
        return
    want = parent[name]
    assert got["log"] == want["log"]
    assert got == want


def test_cases_cross_the_boundaries_they_are_meant_to(parent):
    """The record itself: launches per case, and what the failing and refused cases left."""
    if RECORD:
        pytest.skip("recording")
    launches = lambda name: sum(e[0] == "wost_solve_multi" for e in parent[name]["log"])
    assert launches("sources_19") == 2 and launches("point_dipoles_17") == 2 and launches("point_charges_3x12") == 2
    assert launches("wavenumbers_5x7") == 3 and launches("wavenumbers_20") == 2
    assert launches("wavenumbers_2x17_dipoles") == 3
    assert launches("models_9x2") == 2 and launches("models_2x9") == 2 and launches("models_20") == 2
    assert launches("models_3x2x2_walks") == 1
    # k_chunk changes between the point-source runs: 16 dipoles x 1 wavenumber twice, then 1 x 2
    assert [e[-1] for e in parent["wavenumbers_2x17_dipoles"]["log"] if e[0] == "wost_solve_multi"] == [16, 16, 2]
    for name in CASES:
        if name.startswith(("refuses", "failing")):
            assert "raised" in parent[name], name
    for name in ("failing_wavenumbers_5x7", "failing_models_9x2", "failing_sources_19"):
        assert parent[name]["raised"][0] == "ValueError" and launches(name) == 2
    assert parent["failing_wavenumbers_5x7"]["state"]["wavenumbers"] == [0.3]
    assert parent["failing_models_9x2"]["state"]["wavenumbers"] == [0.3]
    assert parent["failing_models_9x2"]["state"]["models"].count("Field(") == 4
    tail = parent["failing_models_9x2"]["log"][-3:]   # the restore, then the case's wost_destroy
    assert tail[0][:2] == ["wost_set_models", 2] and tail[1] == ["wost_set_wavenumbers", 1, [0.3 * 0.3]]


# ---- the plan, as a pure function ------------------------------------------------------------
def test_plan_tiles_the_box_once_within_the_cap_in_the_fewest_launches():
    from dcrmontecarlo_amd.solvers.channels import _model_chunks, plan_launches

    cap = 16
    for M in range(1, 21):
        for K in range(1, 21):
            for S in range(1, 21):
                plan = plan_launches(M, K, S, cap)
                seen = np.zeros((M, K, S), np.int32)
                for ln in plan:
                    assert ln.channels <= cap and ln.charges is None
                    seen[ln.m[0]:ln.m[1], ln.k[0]:ln.k[1], ln.s[0]:ln.s[1]] += 1
                assert np.all(seen == 1), (M, K, S)
                m, s, k = _model_chunks(M, S, K, cap)
                assert len(plan) == -(-M // m) * -(-S // s) * -(-K // k), (M, K, S)


def test_plan_orders_of_the_three_paths():
    from dcrmontecarlo_amd.solvers.channels import plan_launches, point_source_chunks, source_chunks

    box = lambda plan: [(ln.m, ln.k, ln.s) for ln in plan]
    # sources: one run of <= 16 fields per launch
    assert box(plan_launches(1, 1, 19, 16, chunks=source_chunks(19, 16))) == [((0, 1), (0, 1), (0, 16)),
                                                                             ((0, 1), (0, 1), (16, 19))]
    # wavenumbers: source runs outermost, then wavenumber chunks of cap // run length
    assert box(plan_launches(1, 5, 7, 16, chunks=source_chunks(7, 16))) == [((0, 1), (0, 2), (0, 7)), ((0, 1), (2, 4), (0, 7)),
                                                                           ((0, 1), (4, 5), (0, 7))]
    # (not the models' rule, which would score 3 sources x 16 wavenumbers in 3 launches instead of 4)
    assert len(plan_launches(1, 16, 3, 16, chunks=source_chunks(3, 16))) == 4 and len(plan_launches(1, 16, 3, 16)) == 3
    # models: source chunks outermost, then model chunks, then wavenumber chunks
    assert box(plan_launches(9, 1, 2, 16)) == [((0, 9), (0, 1), (0, 1)), ((0, 9), (0, 1), (1, 2))]
    assert box(plan_launches(20, 2, 1, 16)) == [((0, 8), (0, 2), (0, 1)), ((8, 16), (0, 2), (0, 1)),
                                                ((16, 20), (0, 2), (0, 1))]
    # point sources: the runs carry their charges, and the wavenumber chunk is each run's own
    lists = [[((0.0, 0.0), 1.0), ((1.0, 0.0), -1.0)]] * 17
    runs = point_source_chunks(lists, 16, 32)
    assert [len(r) for r in runs] == [16, 1]
    plan = plan_launches(1, 2, 17, 16, point_runs=runs)
    assert box(plan) == [((0, 1), (0, 1), (0, 16)), ((0, 1), (1, 2), (0, 16)), ((0, 1), (0, 2), (16, 17))]
    assert [len(ln.charges) for ln in plan] == [16, 16, 1]
    # the charge cap alone splits 3 sources of 12 charges into 2 + 1; one source over the cap is refused
    assert [len(r) for r in point_source_chunks([[((0.0, 0.0), 1.0)] * 12] * 3, 16, 32)] == [2, 1]
    with pytest.raises(ValueError, match="33 charges exceeds 32"):
        point_source_chunks([[((0.0, 0.0), 1.0)] * 33], 16, 32)


def test_stats_of_channels_stacks_the_channels_of_every_launch():
    from dcrmontecarlo_amd.solvers.WoStSolver import SolveStats, _stats_of_multi, stats_from_sums
    from dcrmontecarlo_amd.solvers.channels import stats_of_channels

    rng = np.random.default_rng(3)
    rows = [rng.random((4, 2 * c + 1)) + 1.0 for c in (3, 2)]
    st = stats_of_channels(rows, 7, kernel_ms=1.5, total_ms=2.5)
    each = [x for r in rows for x in _stats_of_multi(r, 7)]
    assert isinstance(st, SolveStats) and st.mean.shape == (5, 4) and st.stderr.shape == (5, 4)
    for c, x in enumerate(each):
        np.testing.assert_array_equal(st.mean[c], x.mean)
        np.testing.assert_array_equal(st.stderr[c], x.stderr)
    np.testing.assert_array_equal(st.mean_steps, rows[0][:, -1] / 7)
    assert st.total_steps == int(rows[0][:, -1].sum()) and st.walks == 7 and (st.kernel_ms, st.total_ms) == (1.5, 2.5)
    assert stats_of_channels(rows, 7, total_steps=99).total_steps == 99
    assert stats_from_sums is not None
