"""WostSolver_2D on MI355X (reference: solvers/WoStSolver.py:15-353).

Drop-in for the reference class: same constructor arguments, same
``setBoundaryConditions`` / ``setSourceTerm`` / ``solve`` signatures and
defaults, same attributes (``use_delta_tracking``, ``sigma_bar``,
``domain_bounds``, ``sigma_prime``). The walk loop runs in libwost's gfx950
kernel; this class only describes the problem and moves arrays.

Differences a caller sees:

* Coefficient functions become device-evaluable fields
  (:mod:`dcrmontecarlo_amd.fields`): pass fields or numbers directly, or the
  reference's Python callables, which are traced into closed form (exact) or
  tabulated over the domain (approximate, with a warning) by
  :mod:`dcrmontecarlo_amd.trace`.
* Randomness is counter-based: ``solve(..., seed=0)`` is bitwise reproducible
  and independent of the GPU count. Walk ``i`` of point ``p`` uses Philox
  subsequence ``p*nWalks + i``.
* ``solve`` returns a float32 ``[N, 1]`` array (a torch tensor if the points
  were a torch tensor); ``return_stats=True`` adds per-point standard errors
  and mean step counts.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from .. import _lib
from ..fields import Field, as_field, const, detach
from .channels import (Launch, SolveStats, _model_chunks, _stats_of_multi, charge_lists, plan_launches,  # noqa: F401
                       point_source_chunks, source_chunks, stats_from_sums, stats_of_channels)


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


_TIMING_FIELDS = tuple(k for k, _ in _lib.WostTiming._fields_)
# ... of these, the ones a solve of several launches adds up (solve_wavenumbers' chunks)
_SUMMED_TIMINGS = ("walk_kernel_ms", "reduce_kernel_ms", "total_ms", "n_launches", "total_steps", "total_walks",
                   "jit_ms", "span_ms", "precompiled_walks")


def _points_np(a) -> np.ndarray:
    if _is_torch(a):
        a = a.detach().cpu().numpy()
    p = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if p.ndim == 1 and p.shape[0] == 2:
        p = p.reshape(1, 2)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"solvePoints must have shape [N, 2], got {p.shape}")
    return p


def _walk_count(nWalks) -> int:
    nWalks = int(nWalks)
    if nWalks < 1:
        raise ValueError("nWalks must be >= 1")
    return nWalks


def _wavenumbers_of(k) -> np.ndarray:
    kk = np.atleast_1d(np.asarray(k, np.float64)).ravel()
    if kk.size < 1:
        raise ValueError("k must hold at least one wavenumber")
    return kk


class _Run(NamedTuple):
    """What WostSolver_2D._run_plan returns."""

    sums: np.ndarray          # [M, K, S, N, 3] float64
    vals: np.ndarray | None   # [M, K, S, N, W] float32
    steps: np.ndarray | None  # [N, W] uint32
    timings: list             # timing() of every launch
    rows: list                # point rows [N, 2C+1] of every launch


def _field_or_none(f, what: str):
    if f is None:
        return None
    try:
        return as_field(f)
    except TypeError as e:
        raise TypeError(f"{what}: {e}") from None


def _bounds_of(dxy: np.ndarray, nxy) -> list:
    allp = dxy if nxy is None else np.concatenate([dxy, nxy])
    return [[float(allp[:, 0].min()), float(allp[:, 0].max())],
            [float(allp[:, 1].min()), float(allp[:, 1].max())]]


@dataclass
class ToleranceStats:
    """What solve_to_tolerance ran and found, per point (C channels: ``mean`` and ``stderr``
    are [N] when C == 1, else [C, N])."""

    walks: np.ndarray       # [N] int64: n_p, the walks point p ran (a checkpoint of the schedule)
    mean: np.ndarray        # float64: sum / n_p
    stderr: np.ndarray      # float64: sample std / sqrt(n_p)
    converged: np.ndarray   # [N] bool: every channel met the tolerance at n_p (else n_p == max_walks)
    sums: np.ndarray        # [N, 2C+1] float64: wost_solve_range(0, n_p)'s point row (sum, sum^2 per channel, steps)
    rounds: int             # launches of the point-list kernel's solve
    total_walks: int        # sum of n_p
    total_steps: int
    kernel_ms: float        # walk-kernel time summed over the rounds (HIP events)
    total_ms: float         # device time summed over the rounds


def tolerance_schedule(min_walks: int, max_walks: int) -> list:
    """The checkpoints n_0 < n_1 < ... = max_walks of solve_to_tolerance: n_0 is min_walks
    rounded up to whole blocks (WOST_BLOCK_WALKS) and capped at max_walks, then each is twice
    the one before, capped at max_walks. Every end but the last is block-aligned."""
    min_walks, max_walks = int(min_walks), int(max_walks)
    if min_walks < 1 or max_walks < 1:
        raise ValueError("min_walks and max_walks must be >= 1")
    B = _lib.WOST_BLOCK_WALKS
    ends = [min(-(-min_walks // B) * B, max_walks)]
    while ends[-1] < max_walks:
        ends.append(min(2 * ends[-1], max_walks))
    return ends


def tolerance_rule(sums: np.ndarray, n_walks, rel_tol: float, abs_tol: float):
    """The stopping rule on running point rows ``sums`` [P, 2C+1] after ``n_walks`` walks
    (a number or [P]): (mean [C, P], stderr [C, P], converged [P]). Mean and standard error are
    stats_from_sums's. A channel has converged when stderr <= max(abs_tol, rel_tol * |mean|)
    and, unless abs_tol > 0, its sum of squares is > 0: walks that all scored an exact 0 say
    nothing about a relative error. A NaN never converges. A point has converged when every
    channel has."""
    sums = np.asarray(sums, np.float64)
    C = (sums.shape[1] - 1) // 2
    n = np.broadcast_to(np.asarray(n_walks, np.float64), (sums.shape[0],))
    s, q = sums[:, 0:2 * C:2].T, sums[:, 1:2 * C:2].T
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = s / n
        var = np.maximum(q / n - mean * mean, 0.0) * (n / np.maximum(n - 1, 1))
        se = np.sqrt(var / n)
        ok = (se <= np.maximum(abs_tol, rel_tol * np.abs(mean))) & ((q > 0.0) | (abs_tol > 0.0))
    ok &= np.isfinite(se) & np.isfinite(mean)
    return mean, se, ok.all(axis=0)


def run_to_tolerance(run_round, n_points: int, n_channels: int, *, rel_tol: float = 0.0, abs_tol: float = 0.0,
                     min_walks: int = 16384, max_walks: int):
    """The rounds of solve_to_tolerance as a pure function of numpy arrays.
    ``run_round(ids, walk_begin, walk_end)`` returns the block rows [len(ids), blocks, 2C+1]
    of walks [walk_begin, walk_end) of the points ``ids`` (ascending int32), in block order.
    Round 0 runs [0, n_0) of every point, round k [n_{k-1}, n_k) of the points still active
    (tolerance_schedule); after a round a point's running row is its previous row plus the
    round's block rows, added one block at a time in block order (the order in which
    wost_solve_range sums a point's row), and tolerance_rule decides which points stop. A
    stopped point is never run again. Returns (sums [N, 2C+1], walks [N] int64, converged [N]
    bool, rounds)."""
    rel_tol, abs_tol = float(rel_tol), float(abs_tol)
    if not (rel_tol >= 0.0 and abs_tol >= 0.0):
        raise ValueError("rel_tol and abs_tol must be >= 0")
    N, row = int(n_points), 2 * int(n_channels) + 1
    sums = np.zeros((N, row), np.float64)
    walks = np.zeros(N, np.int64)
    converged = np.zeros(N, bool)
    active = np.arange(N, dtype=np.int32)
    begin, rounds = 0, 0
    for end in tolerance_schedule(min_walks, max_walks):
        if active.size == 0:
            break
        blocks = np.asarray(run_round(active.copy(), begin, end), np.float64)
        nbr = -(-(end - begin) // _lib.WOST_BLOCK_WALKS)
        if blocks.shape != (active.size, nbr, row):
            raise ValueError(f"run_round returned {blocks.shape}, expected {(active.size, nbr, row)}")
        acc = sums[active]
        for k in range(nbr):
            acc = acc + blocks[:, k, :]
        sums[active] = acc
        walks[active] = end
        rounds += 1
        done = tolerance_rule(acc, end, rel_tol, abs_tol)[2]
        converged[active] = done
        active = active[~done]
        begin = end
    return sums, walks, converged, rounds


def _range_layout(n_points: int, point_ids, walk_begin, walk_end):
    """The output layout of a walk-range solve (solve_range, solve_range_combinations):
    (point_ids as int32 or None, point rows, blocks per point). ValueError on an empty list
    or ids that are not 32-bit integers; the library checks their order and range."""
    ids = None
    if point_ids is not None:
        ids = np.ascontiguousarray(np.asarray(_np(point_ids)).ravel())
        if ids.size == 0:
            raise ValueError("point_ids must hold at least one point")
        if (not np.issubdtype(ids.dtype, np.integer) or ids.min() < -2**31 or ids.max() >= 2**31):
            raise ValueError("point_ids must be integers that fit 32 bits")
        ids = ids.astype(np.int32)
    rows = n_points if ids is None else ids.shape[0]
    nbr = -(-(int(walk_end) - int(walk_begin)) // _lib.WOST_BLOCK_WALKS)
    return ids, rows, nbr


def _problem(dxy, nxy, g, f, sigma, alpha, compat, device, sigma_bar):
    """wost_problem for the given geometry and fields (None = absent; the library
    applies the sigma = 0 / alpha = 1 defaults itself) and the objects to keep alive."""
    keep = []
    dpoly, k1 = _lib.make_polyline(dxy)
    npoly, k2 = _lib.make_polyline(nxy)
    fields = {}
    for name, fld in (("boundary", g), ("source", f), ("sigma", sigma), ("alpha", alpha)):
        wf, k = _lib.make_field(fld)
        fields[name] = ctypes.pointer(wf) if wf is not None else None
        keep.append(k)
    prob = _lib.WostProblem(dpoly, npoly, fields["boundary"], fields["source"], fields["sigma"], fields["alpha"],
                            _lib.COMPAT[compat], int(device), float(sigma_bar) if sigma_bar else 0.0)
    return prob, keep + [k1, k2]


def kernel_source(dirichletBoundary, dirichletBoundaryFunction=None, neumannBoundary=None, source=None,
                  sigma=None, alpha=None, *, sigma_bar: float | None = None, compat: str = "reference",
                  sources=None, n_wavenumbers: int = 0, models=None, options: dict | None = None,
                  dirichlet_tree: int | None = None, dirichlet_tree_leaf: int = 0, point_list: bool = False,
                  tally: bool = False, tally_maps: int = 0) -> str:
    """HIP source of the field-specialised walk kernel a WostSolver_2D with these
    arguments would compile (no device needed; wost_kernel_source). sources: the fields
    of a multi-source solve (solve_sources; wost_kernel_source_sources); n_wavenumbers: the
    wavenumbers of set_wavenumbers (wost_kernel_source_channels; 0: none); models: the
    (sigma, alpha) pairs of set_models (wost_kernel_source_models; None: that entry point is
    not used, an empty list: it is, with no model); options: {name: value} of set_option
    (wost_kernel_source_options; the plain single-source kernel only); dirichlet_tree: the
    min_segments of set_dirichlet_tree called first (0 forces the Dirichlet tree, -1 forbids
    it, None: the default threshold; wost_kernel_source_dirichlet_tree, the plain
    single-source kernel only), dirichlet_tree_leaf its leaf_segments; point_list: the kernel
    a solve with a point list launches (solve_range(point_ids=...), solve_to_tolerance;
    wost_kernel_source_point_list; with sources, wavenumbers and models, not with options or
    dirichlet_tree); tally: the kernel solve_greens_map launches (wost_kernel_source_tally;
    compat="fixed" and a source, and none of the other keywords: a tally takes one channel);
    tally_maps: the kernel solve_greens_maps launches for that many maps (1..4;
    wost_kernel_source_tally_channels; compat="fixed" and a source; with n_wavenumbers and
    models, not with tally or the other keywords)."""
    if tally_maps and (tally or point_list or options or dirichlet_tree is not None or sources):
        raise ValueError("tally_maps: with n_wavenumbers and models only -- not together with tally, sources, "
                         "point_list, options or dirichlet_tree")
    if tally and (point_list or options or dirichlet_tree is not None or sources or n_wavenumbers or models is not None):
        raise ValueError("tally: one channel only -- not together with sources, n_wavenumbers, models, point_list, "
                         "options or dirichlet_tree")
    if point_list and (options or dirichlet_tree is not None):
        raise ValueError("point_list: not together with options or dirichlet_tree")
    if options and (sources or n_wavenumbers or models is not None):
        raise ValueError("options: only with the problem's own source, no wavenumbers and no models")
    if dirichlet_tree is not None and (options or sources or n_wavenumbers or models is not None):
        raise ValueError("dirichlet_tree: only with the problem's own source, no wavenumbers, models or options")
    dxy = np.asarray(_np(dirichletBoundary.points), dtype=np.float32).reshape(-1, 2)
    nxy = None if neumannBoundary is None else np.asarray(_np(neumannBoundary.points), dtype=np.float32).reshape(-1, 2)
    conv = _Converter(_bounds_of(dxy, nxy))
    g = conv(dirichletBoundaryFunction, "dirichletBoundaryFunction")
    f = conv(source, "source")
    s = conv(sigma, "sigma")
    a = conv(alpha, "alpha", is_alpha=True)
    if a is not None and a.is_constant():
        a = detach(a)
    if compat not in _lib.COMPAT:
        raise ValueError(f"compat must be one of {sorted(_lib.COMPAT)}")
    prob, keep = _problem(dxy, nxy, g, f, s, a, compat, 0, sigma_bar)
    arr, keep_s = _lib.pack_fields([conv(x, "source") for x in (sources or [])])
    n_src = len(sources or [])
    n = ctypes.c_int64(0)
    call = lambda buf, cap: _lib.lib.wost_kernel_source_channels(ctypes.byref(prob), arr, n_src, int(n_wavenumbers),
                                                                  buf, cap, ctypes.byref(n))
    if models is not None:
        marr, keep_m = _lib.pack_models(_model_fields(conv, models))
        call = lambda buf, cap: _lib.lib.wost_kernel_source_models(ctypes.byref(prob), marr, len(models), arr, n_src,
                                                                    int(n_wavenumbers), buf, cap, ctypes.byref(n))
    if point_list:
        marr, nm = (None, 0) if models is None else (marr, len(models))
        call = lambda buf, cap: _lib.lib.wost_kernel_source_point_list(ctypes.byref(prob), marr, nm, arr, n_src,
                                                                        int(n_wavenumbers), buf, cap, ctypes.byref(n))
    if options:
        names = (ctypes.c_char_p * len(options))(*[k.encode() for k in options])
        values = (ctypes.c_double * len(options))(*[float(v) for v in options.values()])
        call = lambda buf, cap: _lib.lib.wost_kernel_source_options(ctypes.byref(prob), names, values, len(options),
                                                                     buf, cap, ctypes.byref(n))
    if dirichlet_tree is not None:
        call = lambda buf, cap: _lib.lib.wost_kernel_source_dirichlet_tree(
            ctypes.byref(prob), int(dirichlet_tree), int(dirichlet_tree_leaf), 0, 0, buf, cap, ctypes.byref(n))
    if tally:
        call = lambda buf, cap: _lib.lib.wost_kernel_source_tally(ctypes.byref(prob), buf, cap, ctypes.byref(n))
    if tally_maps:
        marr, nm = (None, 0) if models is None else (marr, len(models))
        call = lambda buf, cap: _lib.lib.wost_kernel_source_tally_channels(
            ctypes.byref(prob), marr, nm, int(n_wavenumbers), int(tally_maps), buf, cap, ctypes.byref(n))
    _lib.check(call(None, 0), "wost_kernel_source")
    buf = ctypes.create_string_buffer(n.value + 1)
    _lib.check(call(buf, n.value + 1), "wost_kernel_source")
    return buf.value.decode()


def kernel_source_points(dirichletBoundary, dirichletBoundaryFunction=None, neumannBoundary=None, sigma=None,
                         alpha=None, *, n_charges: int, n_sources: int = 1, n_wavenumbers: int = 0,
                         sigma_bar: float | None = None, compat: str = "fixed",
                         dirichlet_tree: int | None = None) -> str:
    """HIP source of the walk kernel of a solver with ``n_charges`` point charges in
    ``n_sources`` source channels (set_point_sources; wost_kernel_source_points, no device
    needed). It depends on the counts only: positions and strengths are run-time data.
    dirichlet_tree: as kernel_source's (no wavenumbers then)."""
    dxy = np.asarray(_np(dirichletBoundary.points), dtype=np.float32).reshape(-1, 2)
    nxy = None if neumannBoundary is None else np.asarray(_np(neumannBoundary.points), dtype=np.float32).reshape(-1, 2)
    conv = _Converter(_bounds_of(dxy, nxy))
    g = conv(dirichletBoundaryFunction, "dirichletBoundaryFunction")
    s = conv(sigma, "sigma")
    a = conv(alpha, "alpha", is_alpha=True)
    if a is not None and a.is_constant():
        a = detach(a)
    if compat not in _lib.COMPAT:
        raise ValueError(f"compat must be one of {sorted(_lib.COMPAT)}")
    prob, keep = _problem(dxy, nxy, g, None, s, a, compat, 0, sigma_bar)
    n = ctypes.c_int64(0)
    call = lambda buf, cap: _lib.lib.wost_kernel_source_points(ctypes.byref(prob), int(n_charges), int(n_sources),
                                                                int(n_wavenumbers), buf, cap, ctypes.byref(n))
    if dirichlet_tree is not None:
        if n_wavenumbers:
            raise ValueError("dirichlet_tree: not together with wavenumbers")
        call = lambda buf, cap: _lib.lib.wost_kernel_source_dirichlet_tree(
            ctypes.byref(prob), int(dirichlet_tree), 0, int(n_charges), int(n_sources), buf, cap, ctypes.byref(n))
    _lib.check(call(None, 0), "wost_kernel_source_points")
    buf = ctypes.create_string_buffer(n.value + 1)
    _lib.check(call(buf, n.value + 1), "wost_kernel_source_points")
    return buf.value.decode()


def pack_point_charges(charges):
    """``charges``: a list of sources, each a list of ``(position, strength)`` pairs or an
    object with such a ``.charges`` list (survey.point_electrode / point_dipole) -> (ctypes
    array of wost_point_charge, n, n_sources). Raises ValueError for what
    wost_set_point_sources would refuse: more than WOST_MAX_POINT_CHARGES charges, a source
    without a charge, a non-finite position or strength."""
    rows = []
    srcs = list(charges)
    if not srcs:
        raise ValueError("point sources: need at least one source (None clears them)")
    for s, src in enumerate(srcs):
        lst = list(getattr(src, "charges", src))
        if not lst:
            raise ValueError(f"point sources: source {s} has no charge")
        for pos, q in lst:
            x, y = (float(v) for v in np.asarray(_np(pos), np.float64).ravel()[:2])
            if not (np.isfinite(x) and np.isfinite(y) and abs(float(q)) <= 3.4028234663852886e38):   # (finite as float32)
                raise ValueError(f"point sources: source {s} has a non-finite position or strength")
            rows.append((x, y, float(q), s))
    if len(rows) > _lib.WOST_MAX_POINT_CHARGES:
        raise ValueError(f"point sources: {len(rows)} charges exceed {_lib.WOST_MAX_POINT_CHARGES} per launch")
    arr = (_lib.WostPointCharge * len(rows))()
    for i, (x, y, q, s) in enumerate(rows):
        arr[i].x, arr[i].y, arr[i].strength, arr[i].source = x, y, q, s
    return arr, len(rows), len(srcs)


def is_point_source(src) -> bool:
    """A survey.PointSource-like source (an object with a ``charges`` list)."""
    return hasattr(src, "charges")


def _model_fields(conv, models) -> list:
    """WostSolver_2D.model_fields with the converter ``conv``."""
    out = []
    for m, pair in enumerate(models):
        try:
            sg, al = pair
        except (TypeError, ValueError):
            raise TypeError(f"models[{m}] must be a (sigma, alpha) pair") from None
        if sg is None and al is None:
            raise ValueError(f"models[{m}] has neither sigma nor alpha")
        s = conv(sg, f"models[{m}].sigma")
        a = conv(al, f"models[{m}].alpha", is_alpha=True)
        if a is not None and a.is_constant():
            a = detach(a)
        out.append((s, a))
    return out


class _Converter:
    """Coefficient arguments -> device fields: Fields and numbers as they are,
    Python callables traced into closed form or tabulated over the domain
    (dcrmontecarlo_amd.trace). Records how each one was converted."""

    def __init__(self, bounds, resolution: int = 513, trace: bool = True):
        self.bounds, self.resolution, self.trace = bounds, resolution, trace
        self.log = {}

    def __call__(self, obj, what: str, is_alpha: bool = False):
        if obj is None:
            return None
        from ..trace import field_from_callable

        c = field_from_callable(obj, self.bounds, what=what, is_alpha=is_alpha, resolution=self.resolution,
                                trace_first=self.trace)
        self.log[what] = c
        return c.field


class WostSolver_2D:
    """Walk-on-Stars solver for -div(alpha grad u) + sigma u = f with Dirichlet
    and (optionally) Neumann polyline boundaries, on a HIP device.

    Coefficients (dirichletBoundaryFunction, source, sigma, alpha) may be
    :mod:`dcrmontecarlo_amd.fields` fields, numbers, or the reference's Python
    callables ``fn(point)``: those are traced into closed-form device fields,
    or -- when they use something the tracer cannot express -- tabulated on a
    ``grid_resolution``-node grid over the domain with a warning
    (dcrmontecarlo_amd.trace). ``field_conversions`` records which."""

    def __init__(self, dirichletBoundary, dirichletBoundaryFunction=None, neumannBoundary=None,
                 source=None, sigma=None, alpha=None, *, compat: str = "reference", device: int | None = None,
                 sigma_bar: float | None = None, grid_resolution: int = 513, trace_callables: bool = True):
        self.dirichletBoundary = dirichletBoundary
        self.neumannBoundary = neumannBoundary
        dxy = np.asarray(_np(dirichletBoundary.points), dtype=np.float32).reshape(-1, 2)
        nxy = None if neumannBoundary is None else np.asarray(_np(neumannBoundary.points), dtype=np.float32).reshape(-1, 2)
        # solvers/WoStSolver.py:37-43
        self.domain_bounds = _bounds_of(dxy, nxy)
        self._conv = _Converter(self.domain_bounds, grid_resolution, trace_callables)
        self.field_conversions = self._conv.log
        self.boundaryDirichlet = self._conv(dirichletBoundaryFunction, "dirichletBoundaryFunction")
        self.source = self._conv(source, "source")
        self.use_delta_tracking = sigma is not None or alpha is not None     # :51-64
        self.sigma = self.alpha = None
        if self.use_delta_tracking:
            s = self._conv(sigma, "sigma")
            a = self._conv(alpha, "alpha", is_alpha=True)
            self.sigma = s if s is not None else const(0.0)                    # :55-56
            a = a if a is not None else const(1.0)                             # :57-58
            if a.is_constant():
                a = detach(a)   # autograd of a constant raises -> sigma/alpha (Q9)
            self.alpha = a
        if compat not in _lib.COMPAT:
            raise ValueError(f"compat must be one of {sorted(_lib.COMPAT)}")
        self.compat = compat
        if device is None:
            device = int(os.environ.get("WOST_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        self.device = int(device)

        prob, self._keep = _problem(dxy, nxy, self.boundaryDirichlet, self.source,
                                    self.sigma if sigma is not None else None,
                                    self.alpha if alpha is not None else None, compat, self.device, sigma_bar)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib.wost_create(ctypes.byref(prob), ctypes.byref(h)), "WostSolver_2D")
        self._h = h
        sb = ctypes.c_double(0.0)
        dt = ctypes.c_int32(0)
        _lib.check(_lib.lib.wost_get_info(self._h, ctypes.byref(sb), ctypes.byref(dt)), "wost_get_info")
        self.sigma_bar = float(sb.value) if self.use_delta_tracking else None
        self.last_timing = None
        self.last_point_sums = None   # (sum, sum^2, steps) per point of the last solve
        self.wavenumbers = None       # set_wavenumbers: the k of the handle's channels, or None
        self.point_sources = None     # set_point_sources: the sources' charge lists, or None
        self.models = None            # set_models: the models' (sigma, alpha) fields, or None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            _lib.lib.wost_destroy(h)
            self._h = None

    # ---- setters (solvers/WoStSolver.py:141-157) ------------------------------
    # the attribute changes only once libwost has accepted the field, so that it always
    # describes what the device solves
    def setBoundaryConditions(self, boundaryDirichlet):
        g = self._conv(boundaryDirichlet, "boundaryDirichlet")
        wf, keep = _lib.make_field(g)
        _lib.check(_lib.lib.wost_set_field(self._h, _lib.SLOT_BOUNDARY, ctypes.pointer(wf) if wf else None),
                   "setBoundaryConditions")
        self.boundaryDirichlet = g

    def setSourceTerm(self, source):
        f = self._conv(source, "source")
        wf, keep = _lib.make_field(f)
        _lib.check(_lib.lib.wost_set_field(self._h, _lib.SLOT_SOURCE, ctypes.pointer(wf) if wf else None),
                   "setSourceTerm")
        self.source = f

    # ---- sigma' as a callable, like the reference's attribute ----------------
    def sigma_prime(self, point):
        """sigma'(point) evaluated on the device (buildModifiedSigma's closure, :88-127)."""
        p = _points_np(point)
        out = self.eval_field("sigma_prime", p)[:, 0]
        return out[0] if np.asarray(_np(point)).ndim == 1 else out

    def eval_field(self, which: str, points) -> np.ndarray:
        """Device evaluation: which in {g, f, sigma, alpha, sigma_prime} -> [N, 4]
        (value, d/dx, d/dy, Laplacian; sigma_prime: sigma', alpha, sigma, 0)."""
        idx = {"g": 0, "f": 1, "sigma": 2, "alpha": 3, "sigma_prime": 4}[which]
        p = _points_np(points)
        out = np.empty((p.shape[0], 4), np.float32)
        _lib.check(_lib.lib.wost_eval_field(self._h, idx, _lib.fptr(p), p.shape[0], _lib.fptr(out)), "eval_field")
        return out

    def sampler_table(self) -> np.ndarray:
        t = np.empty(_lib.WOST_SAMPLER_TABLE_N, np.float32)
        _lib.check(_lib.lib.wost_sampler_table(self._h, _lib.fptr(t), t.shape[0]), "sampler_table")
        return t

    # ---- the hot path ----------------------------------------------------------
    def solve_blocks(self, solvePoints, nWalks: int, block_begin: int, block_end: int, maxSteps: int = 1000,
                     eps: float = 1e-4, seed: int = 0, walk_values: np.ndarray | None = None,
                     walk_steps: np.ndarray | None = None):
        """Run walk blocks [block_begin, block_end) (WOST_BLOCK_WALKS walks of one point
        each) and return their (sum, sum^2, steps) rows in block order. This is
        the unit of multi-GPU sharding (dcrmontecarlo_amd.distributed)."""
        p = _points_np(solvePoints)
        nb = int(block_end) - int(block_begin)
        bs = np.zeros((max(nb, 0), 3), np.float64)
        _lib.check(_lib.lib.wost_solve(self._h, _lib.fptr(p), p.shape[0], int(nWalks), int(block_begin),
                                       int(block_end), int(maxSteps), float(eps), _lib.seed64(seed),
                                       _lib.dptr(bs), None, _lib.fptr(walk_values), _lib.u32ptr(walk_steps)),
                   "WostSolver_2D.solve")
        self.last_timing = self.timing()
        return bs

    def solve_range(self, solvePoints, nWalks: int, walk_begin: int, walk_end: int, maxSteps: int = 1000,
                    eps: float = 1e-4, seed: int = 0, point_ids=None, walk_values: np.ndarray | None = None,
                    walk_steps: np.ndarray | None = None):
        """Walks [walk_begin, walk_end) of every point (block-aligned ends; wost_solve_range):
        the (sum, sum^2, steps) rows of its blocks, [N, blocks, 3] ([N, blocks, 2C+1] with C
        channels: sources x wavenumbers), each equal to the
        corresponding block of the full solve. The unit of dcrmontecarlo_amd.comm's sharding.

        point_ids (wost_solve_range_points): strictly ascending indices into ``solvePoints``;
        only these points are walked, with the ids -- and so the random streams and the bits
        -- they have in the solve of all points. The result then has len(point_ids) rows in
        list order, row r bitwise row point_ids[r] of the call without a list. Needs the
        field-specialised kernel (NotImplementedError after set_jit(False)); a bad list raises
        ValueError. walk_values / walk_steps: optional float32 [rows, walk_end - walk_begin, C]
        / uint32 [rows, walk_end - walk_begin] arrays that receive the per-walk results."""
        p = _points_np(solvePoints)
        n = p.shape[0]
        ids, rows, nbr = _range_layout(n, point_ids, walk_begin, walk_end)
        ns = self.num_channels()   # values per walk: models x wavenumbers x sources
        for a, dt, size in ((walk_values, np.float32, ns), (walk_steps, np.uint32, 1)):
            if a is not None and (a.dtype != dt or not a.flags.c_contiguous or
                                  a.size != rows * max(int(walk_end) - int(walk_begin), 0) * size):
                raise ValueError("walk_values / walk_steps: contiguous float32 [rows, walks, C] / uint32 [rows, walks]")
        bs = np.zeros((rows, max(nbr, 0), 2 * ns + 1), np.float64)
        if ids is None:
            rc = _lib.lib.wost_solve_range(self._h, _lib.fptr(p), n, int(nWalks), int(walk_begin), int(walk_end),
                                           int(maxSteps), float(eps), _lib.seed64(seed), _lib.dptr(bs), None,
                                           _lib.fptr(walk_values), _lib.u32ptr(walk_steps))
        else:
            rc = _lib.lib.wost_solve_range_points(self._h, _lib.fptr(p), n, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                  rows, int(nWalks), int(walk_begin), int(walk_end), int(maxSteps),
                                                  float(eps), _lib.seed64(seed), _lib.dptr(bs), None,
                                                  _lib.fptr(walk_values), _lib.u32ptr(walk_steps))
        _lib.check(rc, "WostSolver_2D.solve_range")
        self.last_timing = self.timing()
        return bs

    def solve_greens_map(self, solvePoints, grid, nWalks=1000, maxSteps=1000, eps=1e-4, *, seed: int = 0,
                         replicas: int = 8, quantum: float | None = None, walk_begin: int = 0,
                         walk_end: int | None = None, return_history: bool = False, return_walks: bool = False):
        """A solve that also tallies its walks' source samples on ``grid`` (a
        :class:`dcrmontecarlo_amd.greens_map.TallyGrid` or its six values x0, y0, dx, dy, nx,
        ny): a Monte-Carlo map of the Green's function G(x_p, .) of every query point, from
        the walks an ordinary solve takes (wost_solve_range_tally). The operator
        is self-adjoint, so row p is also the potential a unit point current at x_p produces
        everywhere on the grid. Returns a :class:`~dcrmontecarlo_amd.greens_map.GreensMap`.

        compat="fixed" only (NotImplementedError otherwise), one channel (no set_wavenumbers,
        set_models or set_point_sources in force), field-specialised kernel only. The walks,
        and ``u`` / ``stats`` of the result, are bit for bit those of solve_range with the
        solver's own source; a solver without a source gets the constant 0 for the call (the
        tally rides the source sample). Walk i of a point goes to replica row (i / 4096) mod
        ``replicas``; the rows give the standard errors. ``quantum`` = 2^-s is the value of one
        integer unit (rounded down to a power of two; None: chosen from a bound on one
        deposit); a deposit too large for it raises ValueError naming a quantum that fits.
        walk_begin / walk_end (block-aligned): a shard of the walks; shards add up
        (``map_a + map_b``) to the full solve's integers. A query point on the Neumann
        polyline starts as in every field-source solve.
        return_walks: also return (values float32 [N, walks], steps uint32 [N, walks])."""
        from ..greens_map import GreensMap, _c_grid, as_grid

        if return_history:
            raise NotImplementedError("solve_greens_map records no history: use solve(return_history=True)")
        if self.compat != "fixed":
            raise NotImplementedError("solve_greens_map needs compat=\"fixed\": the reference's source sample does not "
                                      "estimate the integral of G f (quirks Q3, Q13)")
        for what, on in (("wavenumbers (set_wavenumbers)", self.wavenumbers is not None),
                         ("models (set_models)", self.models is not None),
                         ("point sources (set_point_sources)", self.point_sources is not None)):
            if on:
                raise NotImplementedError(f"solve_greens_map tallies one channel: the solver has {what} set; clear "
                                          "them first")
        if self.num_channels() != 1:   # (sources_installed: installing the zero source below would drop them)
            raise NotImplementedError(f"solve_greens_map tallies one channel: the handle scores {self.num_channels()} "
                                      "(extra sources are installed)")
        p = _points_np(solvePoints)
        n = p.shape[0]
        nWalks = _walk_count(nWalks)
        w0, w1 = int(walk_begin), nWalks if walk_end is None else int(walk_end)
        R = int(replicas)
        g = as_grid(grid)
        cg = _c_grid(g)
        if R < 1:
            raise ValueError(f"replicas must be >= 1 (got {replicas})")
        if g.nx < 1 or g.ny < 1:
            raise ValueError("the grid needs nx, ny >= 1")
        bins = g.nx * g.ny + 1
        if n * R * bins * 8 > _lib.WOST_TALLY_MAX_BYTES:
            raise ValueError(f"a tally of {n} points x {R} replicas x {bins} bins exceeds "
                             f"{_lib.WOST_TALLY_MAX_BYTES} bytes: fewer points per call, replicas or cells")
        own = self.source

        @contextlib.contextmanager
        def zero_source():   # the tally rides the source sample: a constant 0 for the call
            wf, keep = _lib.make_field(const(0.0))
            _lib.check(_lib.lib.wost_set_field(self._h, _lib.SLOT_SOURCE, ctypes.pointer(wf)), "solve_greens_map")
            try:
                yield
            finally:
                _lib.check(_lib.lib.wost_set_field(self._h, _lib.SLOT_SOURCE, None), "solve_greens_map")

        with (zero_source() if own is None else contextlib.nullcontext()):
            if quantum is None:
                s = ctypes.c_int32(0)
                _lib.check(_lib.lib.wost_tally_default_scale(self._h, nWalks, w0, w1, R, int(maxSteps), ctypes.byref(s)),
                           "solve_greens_map")
                s = int(s.value)
            else:
                if not (quantum > 0 and np.isfinite(quantum)):
                    raise ValueError(f"quantum must be positive and finite (got {quantum})")
                s = -int(np.floor(np.log2(float(quantum))))
            tally = np.zeros((n, R, bins), np.int64)
            rows = np.zeros((n, R), np.int64)
            sums = np.zeros((n, 3), np.float64)
            nw = max(w1 - w0, 0)
            wv = np.empty((n, nw), np.float32) if return_walks else None
            ws = np.empty((n, nw), np.uint32) if return_walks else None
            i64 = ctypes.POINTER(ctypes.c_int64)
            _lib.check(_lib.lib.wost_solve_range_tally(
                self._h, _lib.fptr(p), n, nWalks, w0, w1, int(maxSteps), float(eps), _lib.seed64(seed), ctypes.byref(cg),
                R, s, None, _lib.dptr(sums), _lib.fptr(wv), _lib.u32ptr(ws), tally.ctypes.data_as(i64),
                rows.ctypes.data_as(i64)), "WostSolver_2D.solve_greens_map")
        self.last_timing = self.timing()
        self.last_point_sums = sums
        u = (sums[:, 0] / max(nw, 1)).astype(np.float32).reshape(n, 1)
        t = self.last_timing
        st = stats_from_sums(sums, max(nw, 1), t["total_steps"], t["walk_kernel_ms"], t["total_ms"])
        gm = GreensMap(tally[:, :, :-1].reshape(n, R, g.ny, g.nx).copy(), tally[:, :, -1].copy(), rows, 2.0 ** -s, g,
                       _like(u, solvePoints), st)
        return (gm, wv, ws) if return_walks else gm

    def _launch_greens_maps(self, p, grid, w, nWalks, w0, w1, maxSteps, eps, seed, R, s, want_walks):
        """One wost_solve_range_tally_channels launch: the maps of the rows ``w`` (float32
        [T <= 4, C]) at scale 2^s. Returns (tally int64 [N, R, T, bins], row_walks int64
        [N, R], point sums float64 [N, 2C+1], walk values float32 [N, walks, C] or None, walk
        steps uint32 [N, walks] or None)."""
        from ..greens_map import _c_grid

        n, (T, C) = p.shape[0], w.shape
        cg = _c_grid(grid)
        tally = np.zeros((n, R, T, grid.nx * grid.ny + 1), np.int64)
        rows = np.zeros((n, R), np.int64)
        sums = np.zeros((n, 2 * C + 1), np.float64)
        nw = max(w1 - w0, 0)
        wv = np.empty((n, nw, C), np.float32) if want_walks else None
        ws = np.empty((n, nw), np.uint32) if want_walks else None
        i64 = ctypes.POINTER(ctypes.c_int64)
        _lib.check(_lib.lib.wost_solve_range_tally_channels(
            self._h, _lib.fptr(p), n, nWalks, w0, w1, int(maxSteps), float(eps), _lib.seed64(seed), ctypes.byref(cg),
            R, s, _lib.fptr(w), T, None, _lib.dptr(sums), _lib.fptr(wv), _lib.u32ptr(ws), tally.ctypes.data_as(i64),
            rows.ctypes.data_as(i64)), "WostSolver_2D.solve_greens_maps")
        self.last_timing = self.timing()
        return tally, rows, sums, wv, ws

    def _default_tally_scale(self, nWalks, w0, w1, R, maxSteps) -> int:
        s = ctypes.c_int32(0)
        _lib.check(_lib.lib.wost_tally_default_scale(self._h, nWalks, w0, w1, R, int(maxSteps), ctypes.byref(s)),
                   "solve_greens_maps")
        return int(s.value)

    def solve_greens_maps(self, solvePoints, grid, weights, nWalks=1000, maxSteps=1000, eps=1e-4, *, seed: int = 0,
                          replicas: int = 8, quantum: float | None = None, walk_begin: int = 0,
                          walk_end: int | None = None, return_channels: bool = False, return_walks: bool = False):
        """``solve_greens_map`` for a solver with wavenumbers and / or models set
        (set_wavenumbers, set_models; wost_solve_range_tally_channels, DESIGN.md 7f "Channel
        maps"): a list of T :class:`~dcrmontecarlo_amd.greens_map.GreensMap`, map t the tally
        of the combination ``weights[t]`` of the C installed channels (c = m * K + j, model
        major), formed per deposit on the device. ``weights`` is [T, C] (a single row [C] is
        one map) and is **rounded to float32**: the kernel forms v_t = sum_c fl(w[t, c] * d_c)
        in float32, channels ascending, every product and sum rounded on its own, zero weights
        skipped -- a unit row gives, integer for integer, the solve_greens_map of that
        channel's own problem on this sigma_bar. No row may be all zero or hold a non-finite
        value.

        One launch keeps at most 4 maps; more rows are **chunked over launches of at most 4,
        and each chunk walks again** -- the same walks (same seed), so every row's integers
        are what a single launch would give, at the cost of one walk set per chunk
        (``last_timing`` is the last chunk's). ``quantum`` None: solve_greens_map's bound on
        one channel's deposit, over the smallest alpha of all installed models, times
        max_t sum_c |w[t, c]| (formed here, in the facade). Every map of the call shares the
        quantum. The maps' ``u`` / ``stats`` stay None: the channels' own solve --
        bit for bit solve_range's for the same solver -- comes with return_channels=True as
        (maps, u float32 [N, C], SolveStats with mean / stderr [N, C]); return_walks=True also
        appends (values float32 [N, walks, C], steps uint32 [N, walks]).
        compat="fixed" only, no point sources, no extra sources; replicas, walk_begin /
        walk_end and the Neumann start as in solve_greens_map."""
        from ..greens_map import GreensMap, as_grid

        if self.compat != "fixed":
            raise NotImplementedError("solve_greens_maps needs compat=\"fixed\": the reference's source sample does not "
                                      "estimate the integral of G f (quirks Q3, Q13)")
        if self.point_sources is not None:
            raise NotImplementedError("solve_greens_maps rides the source sample: the solver has point sources "
                                      "(set_point_sources) set; clear them first")
        C = self.num_channels()
        if C != max(self.num_models, 1) * (1 if self.wavenumbers is None else self.wavenumbers.size):
            raise NotImplementedError(f"solve_greens_maps takes one source: the handle scores {C} channels (extra "
                                      "sources are installed); the map does not depend on f")
        w = np.asarray(_np(weights), np.float64)
        with np.errstate(over="ignore"):   # (a weight beyond float32 becomes inf and is refused below)
            w = np.ascontiguousarray(np.atleast_2d(w).astype(np.float32))   # the kernel's weights: float32
        if w.ndim != 2 or w.shape[1] != C or w.shape[0] < 1:
            raise ValueError(f"weights must have shape [T, {C}] for the {C} installed channels, got {w.shape}")
        if not np.isfinite(w).all() or not (w != 0).any(axis=1).all():
            raise ValueError("weights: every value finite (as float32) and no row all zero")
        p = _points_np(solvePoints)
        n = p.shape[0]
        nWalks = _walk_count(nWalks)
        w0, w1 = int(walk_begin), nWalks if walk_end is None else int(walk_end)
        R = int(replicas)
        g = as_grid(grid)
        if R < 1:
            raise ValueError(f"replicas must be >= 1 (got {replicas})")
        if g.nx < 1 or g.ny < 1:
            raise ValueError("the grid needs nx, ny >= 1")
        bins = g.nx * g.ny + 1
        cap = _lib.WOST_TALLY_MAX_MAPS
        if n * R * min(w.shape[0], cap) * bins * 8 > _lib.WOST_TALLY_MAX_BYTES:
            raise ValueError(f"a tally of {n} points x {R} replicas x {min(w.shape[0], cap)} maps x {bins} bins exceeds "
                             f"{_lib.WOST_TALLY_MAX_BYTES} bytes: fewer points per call, replicas, rows or cells")

        @contextlib.contextmanager
        def zero_source():   # the tally rides the source sample: a constant 0 for the call
            wf, keep = _lib.make_field(const(0.0))
            _lib.check(_lib.lib.wost_set_field(self._h, _lib.SLOT_SOURCE, ctypes.pointer(wf)), "solve_greens_maps")
            try:
                yield
            finally:
                _lib.check(_lib.lib.wost_set_field(self._h, _lib.SLOT_SOURCE, None), "solve_greens_maps")

        maps, first = [], None
        with (zero_source() if self.source is None else contextlib.nullcontext()):
            if quantum is None:
                gain = float(np.abs(w.astype(np.float64)).sum(axis=1).max())
                s = self._default_tally_scale(nWalks, w0, w1, R, maxSteps) - int(np.ceil(np.log2(gain)))
                s = max(-100, min(100, s))
            else:
                if not (quantum > 0 and np.isfinite(quantum)):
                    raise ValueError(f"quantum must be positive and finite (got {quantum})")
                s = -int(np.floor(np.log2(float(quantum))))
            for t0 in range(0, w.shape[0], cap):   # every chunk walks again: the same walks
                tally, rows, sums, wv, ws = self._launch_greens_maps(p, g, np.ascontiguousarray(w[t0:t0 + cap]), nWalks,
                                                                      w0, w1, maxSteps, eps, seed, R, s,
                                                                      return_walks and first is None)
                if first is None:
                    first = (sums, wv, ws)
                for t in range(tally.shape[2]):
                    maps.append(GreensMap(tally[:, :, t, :-1].reshape(n, R, g.ny, g.nx).copy(),
                                          tally[:, :, t, -1].copy(), rows.copy(), 2.0 ** -s, g))
        sums, wv, ws = first
        self.last_point_sums = sums
        out = [maps]
        if return_channels:
            nw = max(w1 - w0, 1)
            mean, se, _ = tolerance_rule(sums, nw, 0.0, 0.0)   # [C, N]
            tm = self.last_timing
            out += [_like(np.ascontiguousarray(mean.T.astype(np.float32)), solvePoints),
                    SolveStats(mean=mean.T, stderr=se.T, mean_steps=sums[:, -1] / nw, walks=nw,
                               total_steps=int(tm["total_steps"]), kernel_ms=tm["walk_kernel_ms"],
                               total_ms=tm["total_ms"])]
        if return_walks:
            out += [wv, ws]
        return maps if len(out) == 1 else tuple(out)

    def _combination_weights(self, weights) -> np.ndarray:
        """``weights`` as contiguous float64 [L, C] for the C installed channels (ValueError
        on another width; the library checks L and the values)."""
        w = np.ascontiguousarray(np.atleast_2d(np.asarray(_np(weights), np.float64)))
        C = self.num_channels()
        if w.ndim != 2 or w.shape[1] != C:
            raise ValueError(f"weights must have shape [L, {C}] for the {C} installed channels, got {w.shape}")
        return w

    def solve_range_combinations(self, solvePoints, weights, nWalks: int, walk_begin: int, walk_end: int,
                                 maxSteps: int = 1000, eps: float = 1e-4, seed: int = 0, point_ids=None,
                                 point_sums: np.ndarray | None = None,
                                 channel_point_sums: np.ndarray | None = None):
        """``solve_range`` with L weighted combinations of the C installed channels reduced on
        the device (wost_solve_range_combined): ``weights`` [L, C]; walk i's
        combination l is sum_c weights[l, c] * value[i, c] in float64, product and sum rounded
        separately, zero weights skipped. Returns the block rows [rows, blocks, 2L+1] of
        (sum_l, sum^2_l, ..., steps); a unit row's entries are bit for bit that channel's of
        ``solve_range``. No per-walk value leaves the device. ``point_ids`` as in
        ``solve_range``. point_sums: an optional float64 [rows, 2L+1] array that receives the
        point rows (the block rows added in block order); channel_point_sums: an optional
        float64 [rows, 2C+1] array that receives the channels' own point rows (``solve_range``'s).
        ``last_combine_ms`` is the HIP-event time of the combine kernels."""
        p = _points_np(solvePoints)
        n = p.shape[0]
        w = self._combination_weights(weights)
        L, C = w.shape
        ids, rows, nbr = _range_layout(n, point_ids, walk_begin, walk_end)
        cps = channel_point_sums
        for a, width in ((point_sums, 2 * L + 1), (cps, 2 * C + 1)):
            if a is not None and (a.dtype != np.float64 or not a.flags.c_contiguous or a.size != rows * width):
                raise ValueError("point_sums / channel_point_sums: contiguous float64 [rows, 2L+1] / [rows, 2C+1]")
        bs = np.zeros((rows, max(nbr, 0), 2 * L + 1), np.float64)
        rc = _lib.lib.wost_solve_range_combined(
            self._h, _lib.fptr(p), n, None if ids is None else ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            rows if ids is not None else 0, int(nWalks), int(walk_begin), int(walk_end), int(maxSteps), float(eps),
            _lib.seed64(seed), _lib.dptr(w), L, _lib.dptr(bs), _lib.dptr(point_sums), _lib.dptr(cps))
        _lib.check(rc, "WostSolver_2D.solve_range_combinations")
        self.last_timing = self.timing()
        return bs

    @property
    def last_combine_ms(self) -> float:
        """HIP-event time of the combine kernels of the solver's last solve (wost_last_combine_ms):
        0.0 when that solve reduced no combinations, or before any solve."""
        ms = ctypes.c_double(0.0)
        _lib.check(_lib.lib.wost_last_combine_ms(self._h, ctypes.byref(ms)), "wost_last_combine_ms")
        return float(ms.value)

    def solve_combinations(self, solvePoints, weights, nWalks=1000, maxSteps=1000, eps=1e-4, *, seed: int = 0,
                           return_stats: bool = False):
        """Mean (float32 [L, N]) of L weighted combinations ``weights`` [L, C] of the C
        installed channels (sources, wavenumbers, models, point sources), and with
        ``return_stats`` a SolveStats whose mean and stderr are [L, N]. The channels share
        their walks, so the standard error comes from the per-walk combined values, formed and
        reduced on the device (``solve_range_combinations``); the point rows are the block
        rows added in block order and are kept in ``last_point_sums`` [N, 2L+1]."""
        p = _points_np(solvePoints)
        nWalks = _walk_count(nWalks)
        bs = self.solve_range_combinations(p, weights, nWalks, 0, nWalks, maxSteps, eps, seed)
        n, nbr, row = bs.shape
        sums = np.zeros((n, row), np.float64)
        for k in range(nbr):
            sums = sums + bs[:, k, :]
        self.last_point_sums = sums
        mean, se, _ = tolerance_rule(sums, nWalks, 0.0, 0.0)
        u = mean.astype(np.float32)
        if not return_stats:
            return u
        t = self.last_timing
        return u, SolveStats(mean=mean, stderr=se, mean_steps=sums[:, -1] / nWalks, walks=nWalks,
                             total_steps=int(t["total_steps"]), kernel_ms=t["walk_kernel_ms"], total_ms=t["total_ms"])

    def solve_models_differences(self, solvePoints, models, nWalks=1000, maxSteps=1000, eps=1e-4, *, sources=None,
                                 k=None, seed: int = 0):
        """Paired differences v_m - v_0 of models solved on shared paths, reduced on the
        device: (mean, stderr) of float64 [M-1, N] ([M-1, S, N], [M-1, K, N] or [M-1, K, S, N]
        with ``sources`` / ``k``), ``solve_models``' output shape without model 0, the
        standard error from the per-walk differences (``survey.paired_difference`` without the
        per-walk values on the host). All M*K*S channels must fit one launch
        (WOST_MAX_SOURCES; the (M-1)*K*S rows then fit too): ValueError otherwise -- use
        ``solve_models_walks`` with ``survey.paired_difference`` then. The solver's models,
        wavenumbers and source are restored afterwards."""
        from ..survey import difference_weights

        mods, fields, kk = self._models_request(models, sources, k, 2)
        M, S, K = len(mods), 1 if fields is None else len(fields), 1 if kk is None else kk.size
        cap = _lib.WOST_MAX_SOURCES
        if M * K * S > cap:   # (the (M - 1) K S rows then fit too)
            raise ValueError(f"{M} models x {K} wavenumbers x {S} sources are {M * K * S} channels, more than one "
                             f"launch's {cap}: use solve_models_walks with survey.paired_difference")
        w = difference_weights(M, K, S)
        with self.channels_installed(fields, mods, kk) as install:
            install(Launch((0, M), (0, K), (0, S)))
            _, st = self.solve_combinations(solvePoints, w, nWalks, maxSteps, eps, seed=seed, return_stats=True)
        n = st.mean.shape[1]
        shape = (M - 1,) + ((K,) if k is not None else ()) + ((S,) if sources is not None else ()) + (n,)
        return st.mean.reshape(shape), st.stderr.reshape(shape)

    def solve_to_tolerance(self, solvePoints, *, rel_tol: float = 0.0, abs_tol: float = 0.0, min_walks: int = 16384,
                           max_walks: int, maxSteps: int = 1000, eps: float = 1e-4, seed: int = 0,
                           combinations=None):
        """Solve each point to a target standard error instead of a fixed walk count: a point
        stops once stderr <= max(abs_tol, rel_tol * |mean|) in every channel, or at
        ``max_walks``. Walks run in rounds over the points still unconverged only (DESIGN.md
        7d): round 0 walks [0, n_0) of every point, n_0 = ``min_walks`` rounded up to whole
        blocks; round k walks [n_{k-1}, min(2 n_{k-1}, max_walks)). Every round launches the
        point-list kernel (solve_range(point_ids=...)), so the points keep their ids.

        The result is a prefix of the fixed solve: point p, stopped after n_p walks, holds bit
        for bit the sums of walks [0, n_p) of ``solve(..., nWalks=max_walks)`` -- with both
        tolerances 0 every point runs to ``max_walks`` and ``u`` is that solve's. It scores
        whatever channels are installed on the handle (inside sources_installed,
        point_sources_installed, models_installed, with set_wavenumbers).

        Stopping on an estimated error, looked at only at the doubling checkpoints, biases the
        estimate slightly: a point whose early walks happen to agree stops early, and the
        standard error it reports is the one that let it stop. ``min_walks`` is the guard --
        no point is judged on fewer walks. A channel whose walks all scored an exact 0 is not
        taken as converged to a relative tolerance (only with abs_tol > 0); NaN never converges.

        combinations: weights [L, C] (``solve_range_combinations``): the rule then acts on the L
        weighted combinations of the channels instead of the channels themselves -- in a 2.5-D
        solve the transformed potential (``wavenumber.transform_weights``), whose high
        wavenumbers are tiny and noisy and never meet a relative tolerance of their own. The
        rounds then reduce the combinations on the device, ``u`` is float32 [L, N] and the
        stats' ``sums`` are [N, 2L+1], bit for bit ``solve_range_combinations(0, n_p)``'s point
        rows. ``None`` (default): the channels, as above.

        Returns ``(u, stats)``: u float32 [N, 1] ([C, N] with C > 1 channels; a torch tensor if
        the points were one) and a :class:`ToleranceStats`. Needs the field-specialised kernel."""
        p = _points_np(solvePoints)
        n = p.shape[0]
        C = self.num_channels()
        cw = None if combinations is None else self._combination_weights(combinations)
        if cw is not None:
            C = cw.shape[0]   # (the rule's channels: the combinations)
        acc = {"steps": 0, "kernel_ms": 0.0, "total_ms": 0.0}

        def run_round(ids, w0, w1):
            if cw is None:
                bs = self.solve_range(p, int(max_walks), w0, w1, maxSteps, eps, seed, point_ids=ids)
            else:
                bs = self.solve_range_combinations(p, cw, int(max_walks), w0, w1, maxSteps, eps, seed, point_ids=ids)
            t = self.last_timing
            acc["steps"] += int(t["total_steps"])
            acc["kernel_ms"] += float(t["walk_kernel_ms"])
            acc["total_ms"] += float(t["total_ms"])
            return bs

        sums, walks, converged, rounds = run_to_tolerance(run_round, n, C, rel_tol=rel_tol, abs_tol=abs_tol,
                                                          min_walks=min_walks, max_walks=max_walks)
        mean, se, _ = tolerance_rule(sums, np.maximum(walks, 1), rel_tol, abs_tol)
        self.last_point_sums = sums
        if C == 1 and cw is None:
            mean, se = mean[0], se[0]
            u = _like(mean.astype(np.float32).reshape(n, 1), solvePoints)
        else:
            u = mean.astype(np.float32)
        return u, ToleranceStats(walks=walks, mean=mean, stderr=se, converged=converged, sums=sums, rounds=rounds,
                                 total_walks=int(walks.sum()), total_steps=acc["steps"], kernel_ms=acc["kernel_ms"],
                                 total_ms=acc["total_ms"])

    def set_jit(self, enable: bool):
        """Use the field-specialised (hiprtc) walk kernel (default) or the precompiled
        kernel that interprets the fields. Both give identical results."""
        _lib.check(_lib.lib.wost_set_jit(self._h, 1 if enable else 0), "wost_set_jit")

    def set_trig(self, mode: str = "auto"):
        """The walk direction's cos/sin (wost_set_trig): "exact" correctly rounded (the
        reference's torch values but for their own ulp errors), "fast" the hardware
        sin/cos, "auto" (default) exact when the Neumann polyline has >= 3 segments."""
        if mode not in _lib.WOST_TRIG:
            raise ValueError(f"trig mode must be one of {sorted(_lib.WOST_TRIG)}, got {mode!r}")
        _lib.check(_lib.lib.wost_set_trig(self._h, _lib.WOST_TRIG[mode]), "wost_set_trig")

    def set_fixed_step_check(self, enable: bool):
        """compat="fixed" delta tracking refuses (ValueError) a solve whose walks would all
        hit maxSteps (~d^2 sigma_bar / 4 steps from Dirichlet distance d at the median
        query point, wost_set_fixed_step_check); False lets such truncated solves run."""
        _lib.check(_lib.lib.wost_set_fixed_step_check(self._h, 1 if enable else 0), "wost_set_fixed_step_check")

    def set_segment_tree(self, min_segments: int = 64, leaf_segments: int = 0):
        """Route the Neumann closest-silhouette and ray queries through the segment
        tree when the Neumann polyline has >= min_segments segments (< 0: never,
        0: always). Results are bit-identical to the full scans."""
        _lib.check(_lib.lib.wost_set_segment_tree(self._h, int(min_segments), int(leaf_segments)),
                   "wost_set_segment_tree")

    def set_dirichlet_tree(self, min_segments: int | None = None, leaf_segments: int = 0):
        """Find each step's Dirichlet distance through a segment tree over the Dirichlet
        polyline when it has >= min_segments segments (< 0: never, 0: always, None: the
        library's default threshold), with leaf_segments segments per leaf (0 keeps the
        current value). Results are bit-identical to the full scan. Only the field-specialised
        kernel uses the tree, and only for a polyline that admits it (no zero-length segment,
        finite coordinates) and is too long to be compiled into the kernel; ``dirichlet_tree()``
        and ``last_timing["dirichlet_tree"]`` report what holds."""
        if min_segments is None:
            min_segments = _lib.WOST_DTREE_MIN_SEGMENTS_DEFAULT
        _lib.check(_lib.lib.wost_set_dirichlet_tree(self._h, int(min_segments), int(leaf_segments)),
                   "wost_set_dirichlet_tree")

    def dirichlet_tree(self) -> dict:
        """{"min_segments", "leaf_segments", "usable", "last_solve"} (wost_dirichlet_tree_info):
        the threshold and leaf size, whether the Dirichlet polyline admits the tree, and
        whether the last solve's walk kernel used it."""
        v = [ctypes.c_int32(0) for _ in range(4)]
        _lib.check(_lib.lib.wost_dirichlet_tree_info(self._h, *[ctypes.byref(x) for x in v]), "wost_dirichlet_tree_info")
        return {"min_segments": v[0].value, "leaf_segments": v[1].value, "usable": bool(v[2].value),
                "last_solve": bool(v[3].value)}

    def set_option(self, name: str, value):
        """A kernel or launch option of this handle (include/wost.h wost_set_option: the
        walk pools, LDS staging, work-queue chunks, tree hand-outs ...). None of them
        changes a walk's value or step count; unknown names and bad values raise
        ValueError, study-build-only names NotImplementedError."""
        _lib.check(_lib.lib.wost_set_option(self._h, str(name).encode(), float(value)), f"set_option({name!r})")

    def get_option(self, name: str) -> float:
        v = ctypes.c_double(0.0)
        _lib.check(_lib.lib.wost_get_option(self._h, str(name).encode(), ctypes.byref(v)), f"get_option({name!r})")
        return float(v.value)

    def options_report(self) -> dict:
        """{"build": "product"|"study", "non_default": {name: value}} (wost_options_report)."""
        return _lib.options_report(self._h)

    def num_blocks(self, n_points: int, nWalks: int) -> int:
        return int(_lib.lib.wost_num_blocks(int(n_points), int(nWalks)))

    def timing(self) -> dict:
        t = _lib.WostTiming()
        _lib.check(_lib.lib.wost_last_timing(self._h, ctypes.byref(t)), "wost_last_timing")
        out = {k: getattr(t, k) for k in _TIMING_FIELDS}
        out["dirichlet_tree"] = int(self.dirichlet_tree()["last_solve"])   # (wost_dirichlet_tree_info)
        return out

    def solve(self, solvePoints, nWalks=1000, maxSteps=1000, eps=1e-4, return_history=False, *,
              seed: int = 0, return_stats: bool = False):
        """Estimate u at each point (reference: solvers/WoStSolver.py:319-353).

        Returns ``[N, 1]`` float32 (torch tensor if ``solvePoints`` is one). With
        ``return_history=True`` returns ``(u, history)`` with the reference's
        structure (:335-350): per point a list of walk dicts with ``walk_id``,
        ``path`` (each step's point and Dirichlet / Neumann distances),
        ``contributions`` (each step's source sample and contribution, then the
        boundary term) and ``total_contribution`` (the running point total, :308),
        plus this walk's ``value`` and ``steps``. Points are torch tensors when
        ``solvePoints`` is one, numpy arrays otherwise. With ``return_stats=True``
        a :class:`SolveStats` is appended.
        """
        p = _points_np(solvePoints)
        n = p.shape[0]
        nWalks = _walk_count(nWalks)
        sums = np.zeros((n, 3), np.float64)
        if return_history:
            # the recorder keeps maxSteps + 1 records per walk on the host: refuse sizes the
            # host cannot hold before allocating (WOST_HISTORY_MAX_BYTES, default 8 GiB)
            rec_bytes = n * nWalks * (int(maxSteps) + 1) * _lib.REC_FLOATS * 4
            limit = int(os.environ.get("WOST_HISTORY_MAX_BYTES", str(8 << 30)))
            if rec_bytes > limit:
                raise ValueError(f"return_history needs {rec_bytes / 2**30:.1f} GiB of walk records "
                                 f"({n} points x {nWalks} walks x {int(maxSteps) + 1} records); lower maxSteps, "
                                 f"nWalks or the point count, or raise WOST_HISTORY_MAX_BYTES ({limit} bytes)")
            wv = np.empty(n * nWalks, np.float32)
            ws = np.empty(n * nWalks, np.uint32)
            stride = int(maxSteps) + 1
            rec = np.empty((n * nWalks, stride, _lib.REC_FLOATS), np.float32)
            _lib.check(_lib.lib.wost_solve_history(self._h, _lib.fptr(p), n, nWalks, int(maxSteps), float(eps),
                                                   _lib.seed64(seed), _lib.dptr(sums), _lib.fptr(wv),
                                                   _lib.u32ptr(ws), _lib.fptr(rec)),
                       "WostSolver_2D.solve")
        else:
            nb = self.num_blocks(n, nWalks)
            _lib.check(_lib.lib.wost_solve(self._h, _lib.addr(p), n, nWalks, 0, nb, int(maxSteps), float(eps),
                                           _lib.seed64(seed), None, _lib.addr(sums), None, None),
                       "WostSolver_2D.solve")
        self.last_timing = self.timing()
        self.last_point_sums = sums
        u = (sums[:, 0] / nWalks).astype(np.float32).reshape(n, 1)
        out = [_like(u, solvePoints)]
        if return_history:
            out.append(_history(rec, wv, ws, n, nWalks, self.neumannBoundary is not None, self.source is not None,
                                _is_torch(solvePoints)))
        if return_stats:
            t = self.last_timing
            out.append(stats_from_sums(sums, nWalks, t["total_steps"], t["walk_kernel_ms"], t["total_ms"]))
        return out[0] if len(out) == 1 else tuple(out)

    def solve_walks(self, solvePoints, nWalks=1000, maxSteps=1000, eps=1e-4, *, seed: int = 0):
        """Per-walk results without the paths: (values float32 [N, nWalks],
        steps uint32 [N, nWalks]) in walk order (walk j of point i has global id
        i * nWalks + j, as in return_history)."""
        p = _points_np(solvePoints)
        n = p.shape[0]
        nWalks = _walk_count(nWalks)
        wv = np.empty(n * nWalks, np.float32)
        ws = np.empty(n * nWalks, np.uint32)
        nb = self.num_blocks(n, nWalks)
        _lib.check(_lib.lib.wost_solve(self._h, _lib.fptr(p), n, nWalks, 0, nb, int(maxSteps), float(eps),
                                       _lib.seed64(seed), None, None, _lib.fptr(wv), _lib.u32ptr(ws)),
                   "WostSolver_2D.solve_walks")
        self.last_timing = self.timing()
        return wv.reshape(n, nWalks), ws.reshape(n, nWalks)

    # ---- multi-source batching -------------------------------
    def source_fields(self, sources) -> list:
        """The device fields of a list of sources (fields, numbers or callables; None = 0)."""
        srcs = list(sources)
        if not srcs:
            raise ValueError("sources must hold at least one source field")
        return [self._conv(0.0 if f is None else f, f"sources[{k}]") for k, f in enumerate(srcs)]

    @contextlib.contextmanager
    def sources_installed(self, fields):
        """Score up to WOST_MAX_SOURCES source fields per walk (wost_set_sources) inside
        the block; the solver's own (single) source is restored afterwards."""
        if not 1 <= len(fields) <= _lib.WOST_MAX_SOURCES:
            raise ValueError(f"1..{_lib.WOST_MAX_SOURCES} sources per launch, got {len(fields)}")
        arr, keep = _lib.pack_fields(fields)
        _lib.check(_lib.lib.wost_set_sources(self._h, arr, len(fields)), "WostSolver_2D.solve_sources")
        try:
            yield len(fields)
        finally:
            wf, keep = _lib.make_field(self.source)
            _lib.check(_lib.lib.wost_set_field(self._h, _lib.SLOT_SOURCE, ctypes.pointer(wf) if wf else None),
                       "WostSolver_2D.solve_sources")

    def prepare_sources(self, sources, n_points: int):
        """Compile (or fetch from the kernel caches) the kernel that solve_sources of
        ``n_points`` points with these ``sources`` launches, without solving or changing the
        handle (wost_prepare_sources). Thread-safe with other prepare_sources calls, also on
        this solver, but not with its solves: a survey prepares every group's kernel from a
        thread pool first, so that their compiles overlap in the compile helper."""
        fields = self.source_fields(sources)
        for c0 in range(0, len(fields), _lib.WOST_MAX_SOURCES):
            chunk = fields[c0:c0 + _lib.WOST_MAX_SOURCES]
            arr, keep = _lib.pack_fields(chunk)
            _lib.check(_lib.lib.wost_prepare_sources(self._h, arr, len(chunk), int(n_points)),
                       "WostSolver_2D.prepare_sources")

    # ---- channel batching: one launch, one installer, one runner ----------------
    def _launch(self, p, nWalks, n_blocks, C, maxSteps, eps, seed, want_walks, what):
        """All walks of the points ``p`` with the C channels the handle has installed
        (wost_solve_multi; the package's only call of it): (point rows [N, 2C+1], per-walk values
        float32 [N * nWalks * C] or None, steps uint32 [N * nWalks] or None, ``timing()``)."""
        n = p.shape[0]
        rows = np.zeros((n, 2 * C + 1), np.float64)
        wv = np.empty(n * nWalks * C, np.float32) if want_walks else None
        ws = np.empty(n * nWalks, np.uint32) if want_walks else None
        _lib.check(_lib.lib.wost_solve_multi(self._h, _lib.fptr(p), n, nWalks, 0, n_blocks, int(maxSteps), float(eps),
                                             _lib.seed64(seed), None, _lib.dptr(rows), _lib.fptr(wv), _lib.u32ptr(ws)),
                   what)
        return rows, wv, ws, self.timing()

    @contextlib.contextmanager
    def channels_installed(self, fields=None, models=None, k=None):
        """Bring the handle to channel sets of these axes and back: ``fields`` (source fields),
        ``models`` (model_fields) and ``k`` (wavenumbers), each ``None`` when the solve has no
        such axis. Yields ``install(launch, expect=None, mismatch=None)``, which installs a
        channels.Launch's slices: its source run (``fields[s0:s1]``, or the launch's point
        charges), then its models, then its wavenumbers; with ``expect`` it then raises
        ``mismatch(launch)`` unless ``num_channels() == expect``.

        On entry the solver's wavenumbers are cleared if the solve has wavenumbers or models,
        and its models if it has models: the setters check models x wavenumbers x sources. A
        solve of sources alone leaves both as they are. A source run stays installed for every
        following launch of the same run, and so do the models while run and models stay. When
        they change, and on exit, what was cleared on entry is cleared again, then the run's
        own source (sources_installed, point_sources_installed) comes back; on exit the
        solver's models, then its wavenumbers are set again."""
        clear_m = models is not None
        clear_k = clear_m or k is not None
        saved_k, saved_m = self.wavenumbers, self.models

        def clear():
            if clear_k:
                self.set_wavenumbers(None)
            if clear_m:
                self.set_models(None)

        at = [None, None]   # the installed launch's source run and models

        def install(launch, expect=None, mismatch=None):
            if at != [launch.s, launch.m]:
                under.close()
                if at[0] != launch.s:
                    run.close()
                    at[:] = launch.s, None
                    if launch.charges is not None:
                        run.enter_context(self.point_sources_installed(launch.charges))
                    elif fields is not None:
                        run.enter_context(self.sources_installed(fields[slice(*launch.s)]))
                at[1] = launch.m
                under.callback(clear)
                if models is not None:
                    self.set_models(models[slice(*launch.m)])
            if k is not None:
                self.set_wavenumbers(k[slice(*launch.k)])
            if expect is not None and self.num_channels() != expect:
                raise mismatch(launch)

        clear()
        try:
            with contextlib.ExitStack() as run, contextlib.ExitStack() as under:   # (under closes first)
                yield install
        finally:
            if clear_m:
                self.set_models(saved_m)
            if clear_k:
                self.set_wavenumbers(saved_k)

    def _run_plan(self, plan, shape, p, nWalks, maxSteps, eps, seed, want_walks, what, *, fields=None, models=None,
                  k=None, mismatch=None, sum_timings=True):
        """Run the launches ``plan`` (channels.plan_launches) of a request of ``shape`` = (M, K, S)
        channels and scatter their rows: a _Run of ``sums`` [M, K, S, N, 3] (sum, sum^2, steps),
        ``vals`` float32 [M, K, S, N, W] and ``steps`` uint32 [N, W] (``want_walks``; the paths do
        not depend on the channel, the steps are the last launch's), the launches' own
        ``timings`` and their point ``rows``. ``channels_installed`` moves the handle from
        launch to launch, and ``wavenumbers``, ``models`` and ``point_sources`` are afterwards
        what they were, whether the solve succeeded or not.

        What the callers differ in, on purpose:
        * solve_sources and solve_point_sources (no ``k``, no ``models``) leave the solver's
          wavenumbers and models installed and refuse -- ``mismatch``, a ValueError -- a handle
          that then scores more than one channel per source. The others clear them first and
          take a wrong channel count for a bug (RuntimeError).
        * ``sum_timings``: solve_wavenumbers and solve_models sum _SUMMED_TIMINGS over the
          launches into ``last_timing`` (the launch shape stays the last launch's);
          solve_sources and solve_point_sources keep the last launch's.
        * ``total_steps`` of the stats is the caller's: the first launch's step column
          (solve_sources, solve_point_sources, solve_wavenumbers: one walk set's, like
          ``mean_steps``) or the summed timing's (solve_models: every walk set that ran).
        Every launch gets the same seed, so that the launches share their walks."""
        M, K, S = shape
        n = p.shape[0]
        nb = self.num_blocks(n, nWalks)
        run = _Run(np.zeros((M, K, S, n, 3), np.float64),
                   np.empty((M, K, S, n, nWalks), np.float32) if want_walks else None, None, [], [])
        if mismatch is None:
            mismatch = lambda ln: RuntimeError(f"the handle scores {self.num_channels()} channels, expected {ln.channels}")
        with self.channels_installed(fields, models, k) as install:
            for ln in plan:
                (m0, m1), (k0, k1), (s0, s1) = ln.m, ln.k, ln.s
                C = ln.channels
                install(ln, C, mismatch)   # (the buffers below hold C values per walk)
                rows, wv, ws, t = self._launch(p, nWalks, nb, C, maxSteps, eps, seed, want_walks, what)
                run.timings.append(dict(t))
                run.rows.append(rows)
                if sum_timings and len(run.timings) > 1:
                    for key in _SUMMED_TIMINGS:
                        t[key] += self.last_timing[key]
                self.last_timing = t
                box = run.sums[m0:m1, k0:k1, s0:s1]
                box[..., :2] = rows[:, :2 * C].reshape((n,) + ln.shape + (2,)).transpose(1, 2, 3, 0, 4)
                box[..., 2] = rows[:, -1]
                if want_walks:
                    run.vals[m0:m1, k0:k1, s0:s1] = wv.reshape((n, nWalks) + ln.shape).transpose(2, 3, 4, 0, 1)
                    run = run._replace(steps=ws.reshape(n, nWalks))
        return run

    def _source_stats(self, run, nWalks, return_stats):
        """solve_sources' and solve_point_sources' result: u float32 [S, N] and the stacked stats."""
        st = stats_of_channels(run.rows, nWalks)
        st.kernel_ms, st.total_ms = self.last_timing["walk_kernel_ms"], self.last_timing["total_ms"]
        u = st.mean.astype(np.float32)
        return (u, st) if return_stats else u

    def _run_sources(self, solvePoints, sources, nWalks, maxSteps, eps, seed, want_walks):
        p, nWalks = _points_np(solvePoints), _walk_count(nWalks)
        fields = self.source_fields(sources)
        S, cap = len(fields), _lib.WOST_MAX_SOURCES
        refuse = lambda ln: ValueError(   # (wost_solve_multi would write rows of 2C+1, values [walks][C])
            f"solve_sources scores one value per source, but the solver scores "
            f"{self.num_channels() // ln.channels} channels per source: wavenumbers (set_wavenumbers) or models "
            "(set_models) are set. Use solve_wavenumbers(points, k, sources=...) or solve_models(points, models, "
            "sources=...), or clear them with set_wavenumbers(None) / set_models(None)")
        return self._run_plan(plan_launches(1, 1, S, cap, chunks=source_chunks(S, cap)), (1, 1, S), p, nWalks, maxSteps,
                              eps, seed, want_walks, "WostSolver_2D.solve_sources", fields=fields, mismatch=refuse,
                              sum_timings=False)

    def solve_sources(self, solvePoints, sources, nWalks=1000, maxSteps=1000, eps=1e-4, *, seed: int = 0,
                      return_stats: bool = False):
        """Multi-source batching (beyond the reference, which solves one source per
        solve): u[k] is the solve of this problem with source ``sources[k]``
        (fields, numbers or callables), all scored by the same walks. The walks
        do not depend on f (solvers/WoStSolver.py:242-258), so each u[k] is bit for
        bit ``setSourceTerm(sources[k]); solve(...)`` with the same seed, at about
        the cost of one solve (16 sources per launch; more are batched in groups).
        Returns float32 [S, N]; with ``return_stats`` also a SolveStats whose mean
        and stderr are [S, N]. The solver's own source is restored afterwards."""
        run = self._run_sources(solvePoints, sources, nWalks, maxSteps, eps, seed, False)
        return self._source_stats(run, nWalks, return_stats)

    def solve_sources_walks(self, solvePoints, sources, nWalks=1000, maxSteps=1000, eps=1e-4, *, seed: int = 0):
        """Per-walk values of every source, float32 [S, N, nWalks], and the walks'
        step counts, uint32 [N, nWalks] (shared by all sources)."""
        run = self._run_sources(solvePoints, sources, nWalks, maxSteps, eps, seed, True)
        return run.vals[0, 0], run.steps

    # ---- point sources (include/wost.h wost_set_point_sources) ----------------
    def set_point_sources(self, charges=None):
        """Score point charges instead of a source field (compat="fixed" only, a solver built
        without ``source``). ``charges``: a list of sources, each a list of
        ``(position, strength)`` -- the strength is the current that enters the 2-D domain --
        or of survey.point_electrode / point_dipole objects; ``None`` clears them. A walk
        scores every charge inside a step's ball and visible from its point exactly, with the
        ball's Green's function: no width, no sampling. ``solve`` / ``solve_walks`` (one
        source), ``solve_point_sources[_walks]``, ``solve_range`` and ``solve_wavenumbers``
        then score them; at most WOST_MAX_POINT_CHARGES charges and WOST_MAX_SOURCES channels
        (sources x wavenumbers) per launch. Positions are data, not code: one compiled kernel
        per (problem, charge count, source count, wavenumber count) serves every electrode set."""
        if charges is None:
            _lib.check(_lib.lib.wost_set_point_sources(self._h, None, 0, 0), "WostSolver_2D.set_point_sources")
            self.point_sources = None
            return
        arr, n, n_src = pack_point_charges(charges)
        _lib.check(_lib.lib.wost_set_point_sources(self._h, arr, n, n_src), "WostSolver_2D.set_point_sources")
        self.point_sources = charge_lists(charges)

    @contextlib.contextmanager
    def point_sources_installed(self, sources):
        """The point sources ``sources`` (one launch's worth) inside the block; the solver's
        own point sources (or none) are restored afterwards."""
        saved = self.point_sources
        self.set_point_sources(sources)
        try:
            yield len(sources)
        finally:
            self.set_point_sources(saved)

    def _run_point_sources(self, solvePoints, sources, nWalks, maxSteps, eps, seed, want_walks):
        p, nWalks = _points_np(solvePoints), _walk_count(nWalks)
        cap, n_k = _lib.WOST_MAX_SOURCES, 1 if self.wavenumbers is None else len(self.wavenumbers)
        runs = point_source_chunks(charge_lists(sources), cap // n_k, _lib.WOST_MAX_POINT_CHARGES)
        refuse = lambda ln: ValueError(
            "solve_point_sources scores one value per source, but the solver has wavenumbers or models set: use "
            "solve_wavenumbers(points, k, sources=...), or clear them with set_wavenumbers(None) / set_models(None)")
        S = sum(len(r) for r in runs)
        return self._run_plan(plan_launches(1, 1, S, cap, runs), (1, 1, S), p, nWalks, maxSteps, eps, seed, want_walks,
                              "WostSolver_2D.solve_point_sources", mismatch=refuse, sum_timings=False)

    def solve_point_sources(self, solvePoints, sources, nWalks=1000, maxSteps=1000, eps=1e-4, *, seed: int = 0,
                            return_stats: bool = False):
        """solve_sources for point sources: u[k] is the solve with the charges of
        ``sources[k]`` alone, all scored by the same walks, bit for bit. Returns float32
        [S, N]; with ``return_stats`` also a SolveStats whose mean and stderr are [S, N]."""
        run = self._run_point_sources(solvePoints, sources, nWalks, maxSteps, eps, seed, False)
        return self._source_stats(run, nWalks, return_stats)

    def solve_point_sources_walks(self, solvePoints, sources, nWalks=1000, maxSteps=1000, eps=1e-4, *, seed: int = 0):
        """Per-walk values of every point source, float32 [S, N, nWalks], and the walks' step
        counts, uint32 [N, nWalks]."""
        run = self._run_point_sources(solvePoints, sources, nWalks, maxSteps, eps, seed, True)
        return run.vals[0, 0], run.steps

    # ---- 2.5-D wavenumber batching (include/wost.h wost_set_wavenumbers) ---------
    def set_wavenumbers(self, k=None):
        """Score the screened problems div(alpha grad u) - k^2 alpha u = -f of the
        wavenumbers ``k`` (an array of k >= 0, not squared) with every walk, or none
        (``None`` or empty: the solver's own PDE). Needs delta tracking (alpha or sigma
        given; a constant alpha is enough) and at most WOST_MAX_SOURCES channels
        (wavenumbers x sources) per launch; ``solve_wavenumbers`` chunks larger requests.
        ``solve`` / ``solve_walks`` keep working with one wavenumber set. The collision
        weights are 1 - (sigma' + k^2)/sigma_bar: create the solver with
        ``sigma_bar >= max sigma' + max k^2`` (``wavenumber.sigma_bar_for``)."""
        kk = np.zeros(0) if k is None else np.atleast_1d(np.asarray(k, np.float64)).ravel()
        # (squaring would hide a negative k: it, and NaN, reach the library as invalid)
        k2 = np.ascontiguousarray(np.where(kk >= 0, kk * kk, -1.0), dtype=np.float64)
        _lib.check(_lib.lib.wost_set_wavenumbers(self._h, _lib.dptr(k2) if k2.size else None, int(k2.size)),
                   "WostSolver_2D.set_wavenumbers")
        self.wavenumbers = kk.copy() if kk.size else None

    def num_channels(self) -> int:
        n = ctypes.c_int32(1)
        _lib.check(_lib.lib.wost_num_channels(self._h, ctypes.byref(n)), "wost_num_channels")
        return int(n.value)

    def _run_wavenumbers(self, solvePoints, k, sources, nWalks, maxSteps, eps, seed, want_walks):
        p, nWalks = _points_np(solvePoints), _walk_count(nWalks)
        kk = _wavenumbers_of(k)
        if self.num_models:   # (wost_solve_multi would write rows of 2C+1 with the models' channels)
            raise ValueError(f"solve_wavenumbers scores one value per wavenumber and source, but the solver has "
                             f"{self.num_models} models set (set_models): use solve_models(points, models, k=..., "
                             "sources=...), or clear them with set_models(None)")
        points = sources is not None and len(sources) > 0 and all(is_point_source(s) or isinstance(s, (list, tuple))
                                                                 for s in sources)
        if sources is not None and not points and any(is_point_source(s) for s in sources):
            raise ValueError("sources mixes point sources and fields: one kind per solve")
        fields = None if sources is None or points else self.source_fields(sources)
        S, cap = 1 if sources is None else len(sources), _lib.WOST_MAX_SOURCES
        # point sources: runs of at most WOST_MAX_POINT_CHARGES charges, then as many wavenumbers as fit
        runs = point_source_chunks(charge_lists(sources), cap, _lib.WOST_MAX_POINT_CHARGES) if points else None
        plan = plan_launches(1, kk.size, S, cap, runs, None if points else source_chunks(S, cap))
        return self._run_plan(plan, (1, kk.size, S), p, nWalks, maxSteps, eps, seed, want_walks,
                              "WostSolver_2D.solve_wavenumbers", fields=fields, k=kk)

    def solve_wavenumbers(self, solvePoints, k, nWalks=1000, maxSteps=1000, eps=1e-4, *, sources=None,
                          seed: int = 0, return_stats: bool = False):
        """2.5-D wavenumber batching: u[j] solves div(alpha grad u) - k[j]^2 alpha u = -f
        (this solver's PDE with the absorption sigma + k^2 alpha), every wavenumber -- and
        with ``sources`` every source -- scored by the same walks: under delta tracking a
        walk's path depends only on sigma_bar. Each u[j] (u[j, s]) is bit for bit the single
        solve of (k[j], sources[s]) with the same seed. Returns float32 [K, N], or
        [K, S, N] with ``sources``; with ``return_stats`` also a SolveStats whose mean and
        stderr have that shape. More than WOST_MAX_SOURCES channels are solved in several
        launches, and ``last_timing`` / the stats' kernel_ms and total_ms then sum over them.
        The solver's wavenumbers and source are restored afterwards."""
        sums = self._run_wavenumbers(solvePoints, k, sources, nWalks, maxSteps, eps, seed, False).sums[0]
        K, S, n = sums.shape[:3]
        st = stats_from_sums(sums.reshape(K * S * n, 3), int(nWalks))
        shape = (K, n) if sources is None else (K, S, n)
        u = st.mean.astype(np.float32).reshape(shape)
        if not return_stats:
            return u
        t = self.last_timing
        return u, SolveStats(mean=st.mean.reshape(shape), stderr=st.stderr.reshape(shape),
                             mean_steps=sums[0, 0, :, 2] / int(nWalks), walks=int(nWalks),
                             total_steps=int(sums[0, 0, :, 2].sum()), kernel_ms=t["walk_kernel_ms"],
                             total_ms=t["total_ms"])

    def solve_wavenumbers_walks(self, solvePoints, k, nWalks=1000, maxSteps=1000, eps=1e-4, *, sources=None,
                                seed: int = 0):
        """Per-walk values of every wavenumber (and source), float32 [K, N, nWalks] or
        [K, S, N, nWalks], and the walks' step counts, uint32 [N, nWalks] (shared by all
        channels: the paths do not depend on them)."""
        run = self._run_wavenumbers(solvePoints, k, sources, nWalks, maxSteps, eps, seed, True)
        return (run.vals[0, :, 0] if sources is None else run.vals[0]), run.steps

    # ---- shared-path model batching (include/wost.h wost_set_models) ----------
    def model_fields(self, models) -> list:
        """The device fields of a list of models, each a ``(sigma, alpha)`` pair of fields,
        numbers or callables (``None``: sigma = 0 / alpha = 1, as the constructor's): a list
        of ``(sigma_field | None, alpha_field | None)``; a constant alpha is detached (Q9)."""
        return _model_fields(self._conv, models)

    def set_models(self, models=None):
        """Score the conductivity models ``models`` -- ``(sigma, alpha)`` pairs -- with every
        walk, or (``None`` or empty) the solver's own fields again. Under delta tracking a
        walk's path depends only on ``sigma_bar`` and the geometry, so one set of walks
        scores them all: channel ``(m, j, s)`` of model m, wavenumber j, source s is bit for
        bit the single solve of a solver created with model m's fields and this solver's
        ``sigma_bar``. ``sigma_bar`` stays the one fixed at construction: choose it >= the
        largest sigma' of any model (``survey.sigma_bar_for_models``). At most
        WOST_MAX_SOURCES channels (models x wavenumbers x sources) per launch;
        ``solve_models`` chunks larger requests. Needs delta tracking; several models cannot
        be combined with point sources."""
        fields = self.model_fields(models) if models is not None and len(models) else []
        if not fields:
            _lib.check(_lib.lib.wost_set_models(self._h, None, 0), "WostSolver_2D.set_models")
            self.models = None
            return
        arr, keep = _lib.pack_models(fields)
        _lib.check(_lib.lib.wost_set_models(self._h, arr, len(fields)), "WostSolver_2D.set_models")
        self.models = fields

    @property
    def num_models(self) -> int:
        """Models installed by ``set_models`` (0: none)."""
        n = ctypes.c_int32(0)
        _lib.check(_lib.lib.wost_models_info(self._h, ctypes.byref(n), None), "wost_models_info")
        return int(n.value)

    @contextlib.contextmanager
    def models_installed(self, models):
        """The models ``models`` (one launch's worth) inside the block; the solver's own models
        (or none) are restored afterwards."""
        saved = getattr(self, "models", None)
        self.set_models(models)
        try:
            yield len(models)
        finally:
            self.set_models(saved)

    def _models_request(self, models, sources, k, fewest: int = 1):
        """(model fields, source fields or None, wavenumbers or None) of a solve_models request."""
        mods = self.model_fields(models)
        if len(mods) < fewest:
            raise ValueError("models must hold at least one (sigma, alpha) pair" if fewest == 1
                             else "solve_models_differences needs at least two models")
        if sources is not None and any(is_point_source(s) for s in sources):
            raise NotImplementedError("solve_models scores source fields: point sources under several models are "
                                      "not supported")
        return mods, None if sources is None else self.source_fields(sources), None if k is None else _wavenumbers_of(k)

    def _run_models(self, solvePoints, models, sources, k, nWalks, maxSteps, eps, seed, want_walks):
        p, nWalks = _points_np(solvePoints), _walk_count(nWalks)
        mods, fields, kk = self._models_request(models, sources, k)
        shape = len(mods), 1 if kk is None else kk.size, 1 if fields is None else len(fields)
        return self._run_plan(plan_launches(*shape, _lib.WOST_MAX_SOURCES), shape, p, nWalks, maxSteps, eps, seed,
                              want_walks, "WostSolver_2D.solve_models", fields=fields, models=mods, k=kk)

    def solve_models(self, solvePoints, models, nWalks=1000, maxSteps=1000, eps=1e-4, *, sources=None, k=None,
                     seed: int = 0, return_stats: bool = False):
        """Shared-path model batching: u[m] is the solve of this problem with the conductivity
        model ``models[m] = (sigma, alpha)``, every model -- and with ``sources`` / ``k`` every
        source and wavenumber -- scored by the same walks (``set_models``). Each u[m] is bit
        for bit the solve of a solver created with that model's fields and
        ``sigma_bar=self.sigma_bar``, same seed. Returns float32 [M, N], [M, S, N], [M, K, N]
        or [M, K, S, N]; with ``return_stats`` also a SolveStats whose mean and stderr have
        that shape. More than WOST_MAX_SOURCES channels are solved in several launches, chosen
        to be as few as possible and, among those, to keep as many models together as fit
        (``_model_chunks``); every launch is a walk set of its own, ``last_timing`` sums over
        them, and the stats' ``total_steps`` counts every walk set that ran (``mean_steps`` is
        one walk set's). The solver's models, wavenumbers and source are restored afterwards."""
        sums = self._run_models(solvePoints, models, sources, k, nWalks, maxSteps, eps, seed, False).sums
        M, K, S, n = sums.shape[:4]
        st = stats_from_sums(sums.reshape(M * K * S * n, 3), int(nWalks))
        shape = (M,) + ((K,) if k is not None else ()) + ((S,) if sources is not None else ()) + (n,)
        u = st.mean.astype(np.float32).reshape(shape)
        if not return_stats:
            return u
        t = self.last_timing
        return u, SolveStats(mean=st.mean.reshape(shape), stderr=st.stderr.reshape(shape),
                             mean_steps=sums[0, 0, 0, :, 2] / int(nWalks), walks=int(nWalks),
                             total_steps=int(t["total_steps"]), kernel_ms=t["walk_kernel_ms"],
                             total_ms=t["total_ms"])

    def solve_models_walks(self, solvePoints, models, nWalks=1000, maxSteps=1000, eps=1e-4, *, sources=None,
                           k=None, seed: int = 0):
        """Per-walk values of every model (wavenumber, source), float32 [M, N, nWalks] (or
        [M, K, N, W], [M, S, N, W], [M, K, S, N, W]), and the walks' step counts, uint32
        [N, nWalks], shared by all channels: the paths do not depend on the model."""
        vals, steps = self._run_models(solvePoints, models, sources, k, nWalks, maxSteps, eps, seed, True)[1:3]
        if sources is None:
            vals = vals[:, :, 0]
        if k is None:
            vals = vals[:, 0]
        return vals, steps


def _history(rec, wv, ws, n, nWalks, has_neumann, has_source, as_torch):
    """The reference's history_dict (solvers/WoStSolver.py:180-309) from the recorder's
    records (include/wost.h, wost_solve_history)."""
    if as_torch:
        import torch

        pt = lambda x, y: torch.tensor([float(x), float(y)], dtype=torch.float32)
    else:
        pt = lambda x, y: np.array([x, y], np.float32)
    hist = {}
    for i in range(n):
        walks = []
        running = 0.0
        for j in range(nWalks):
            g = i * nWalks + j
            k = int(ws[g])
            r = rec[g]
            path = [{"point": pt(r[s, 0], r[s, 1]), "dirichlet_distance": float(r[s, 2]),
                     "neumann_distance": float(r[s, 3]) if has_neumann else None} for s in range(k)]
            contrib = []
            if has_source:
                contrib = [{"step": s, "type": "source", "point": pt(r[s, 4], r[s, 5]), "contribution": float(r[s, 6])}
                           for s in range(k)]
            contrib.append({"step": k, "type": "boundary", "point": pt(r[k, 0], r[k, 1]),
                            "contribution": float(r[k, 6])})
            running += float(wv[g])
            walks.append({"walk_id": j, "path": path, "contributions": contrib, "total_contribution": running,
                          "value": float(wv[g]), "steps": k})
        hist[i] = walks
    return hist


def _np(a):
    if _is_torch(a):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def _like(u: np.ndarray, ref):
    if _is_torch(ref):
        import torch

        return torch.from_numpy(u)
    return u
