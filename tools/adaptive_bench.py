#!/usr/bin/env python3
"""Solving to a target standard error against the fixed solve that reaches it.

1. dcr_dipole's 48 electrodes;
2. --tree: 64 points of wenner_topography (the segment-tree kernel).
A solve_to_tolerance run, then the fixed solve that reaches the same tolerance at every point:
nWalks = the adaptive run's largest n_p. Reports both runs' walk-steps, their wall times
around a device synchronise (median of --reps after a warm-up of each, the two alternating),
the walk-kernel times from libwost's HIP events, and the histogram of n_p. Prints one JSON
line per measurement. Honours WOST_LIB.
Usage: python tools/adaptive_bench.py [--rel-tol 0.05] [--abs-tol 0] [--min-walks 16384] [--max-walks 1048576]
       [--reps 3] [--tree] [--tree-points 64] [--tree-max-walks 131072]"""
import argparse
import collections
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcrmontecarlo_amd import scenarios as S  # noqa: E402

_hip = None


def _sync():
    """hipDeviceSynchronize through the HIP runtime libwost is linked with."""
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
    if _hip.hipDeviceSynchronize() != 0:
        raise RuntimeError("hipDeviceSynchronize failed")


def _wall(fn):
    _sync()
    t0 = time.perf_counter()
    out = fn()
    _sync()
    return 1e3 * (time.perf_counter() - t0), out


def compare(name, sc, pts, rel_tol, abs_tol, min_walks, max_walks, reps, seed=5):
    s = sc.solver()
    kw = dict(maxSteps=sc.max_steps, eps=sc.eps, seed=seed)
    adaptive = lambda: s.solve_to_tolerance(pts, rel_tol=rel_tol, abs_tol=abs_tol, min_walks=min_walks,
                                            max_walks=max_walks, **kw)
    _, st = adaptive()                                   # warm-up: compiles the point-list kernel
    n_fixed = int(st.walks.max())
    fixed = lambda: s.solve(pts, nWalks=n_fixed, return_stats=True, **kw)
    fixed()                                              # warm-up: compiles the plain kernel
    a_ms, f_ms, a_k, f_k = [], [], [], []
    for _ in range(reps):                                # alternating
        ms, (_, st) = _wall(adaptive)
        a_ms.append(ms)
        a_k.append(st.kernel_ms)
        ms, (_, fs) = _wall(fixed)
        f_ms.append(ms)
        f_k.append(fs.kernel_ms)
    hist = collections.Counter(int(n) for n in st.walks)
    rel = st.stderr / np.abs(st.mean)
    print(json.dumps({
        "measurement": name, "points": len(pts), "rel_tol": rel_tol, "abs_tol": abs_tol, "min_walks": min_walks,
        "max_walks": max_walks, "tree": s.last_timing["tree"], "rounds": st.rounds,
        "converged_points": int(st.converged.sum()), "n_p_histogram": {str(k): hist[k] for k in sorted(hist)},
        "adaptive_walks": st.total_walks, "adaptive_walk_steps": st.total_steps,
        "fixed_walks_per_point": n_fixed, "fixed_walks": n_fixed * len(pts), "fixed_walk_steps": fs.total_steps,
        "walk_steps_fixed_over_adaptive": fs.total_steps / max(st.total_steps, 1),
        "adaptive_wall_ms": statistics.median(a_ms), "adaptive_wall_runs_ms": [round(x, 3) for x in a_ms],
        "fixed_wall_ms": statistics.median(f_ms), "fixed_wall_runs_ms": [round(x, 3) for x in f_ms],
        "wall_fixed_over_adaptive": statistics.median(f_ms) / statistics.median(a_ms),
        "adaptive_kernel_ms": statistics.median(a_k), "fixed_kernel_ms": statistics.median(f_k),
        "largest_rel_stderr_of_converged": float(np.max(rel[st.converged])) if st.converged.any() else None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rel-tol", type=float, default=0.05)
    ap.add_argument("--abs-tol", type=float, default=0.0)
    ap.add_argument("--min-walks", type=int, default=16384)
    ap.add_argument("--max-walks", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tree", action="store_true", help="only the wenner_topography (segment-tree) measurement")
    ap.add_argument("--tree-points", type=int, default=64)
    ap.add_argument("--tree-max-walks", type=int, default=1 << 17)
    a = ap.parse_args()
    if a.tree:
        sc = S.wenner_topography()
        pts = np.ascontiguousarray(sc.points[::max(1, len(sc.points) // a.tree_points)][:a.tree_points])
        compare("wenner_topography", sc, pts, a.rel_tol, a.abs_tol, a.min_walks, a.tree_max_walks, a.reps)
    else:
        sc = S.dcr_dipole()
        compare("dcr_dipole", sc, sc.points, a.rel_tol, a.abs_tol, a.min_walks, a.max_walks, a.reps)


if __name__ == "__main__":
    main()
