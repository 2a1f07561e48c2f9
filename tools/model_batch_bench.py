#!/usr/bin/env python3
"""Shared-path model batching on one GPU.

1. dcr_dipole, model + homogeneous background: two solves on one sigma_bar and seed (what the
   surveys do without shared walks) against one launch that scores both models, and the cost
   of a batched walk-step relative to a single-model step.
2. --tree: the same for one wenner_topography launch (the segment-tree kernel, where the path
   dominates a step).
3. M = 4 and M = 8 models with a perturbed inclusion against 4 and 8 single solves.
Walk-kernel time from libwost's HIP events, median of --reps after a warm-up solve. Prints one
JSON line per measurement. Honours WOST_LIB.
Usage: python tools/model_batch_bench.py [--electrodes 48] [--walks 100000] [--reps 3] [--tree]
       [--tree-electrodes 64] [--tree-walks 2000]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcrmontecarlo_amd import fields as F  # noqa: E402
from dcrmontecarlo_amd import scenarios as S  # noqa: E402
from dcrmontecarlo_amd import survey  # noqa: E402


def timed(fn, reps):
    """(median walk-kernel ms, walk-steps, every run's ms) of fn() -> [(ms, steps), ...], after one warm-up."""
    fn()
    runs = []
    for _ in range(reps):
        parts = fn()
        runs.append((sum(p[0] for p in parts), sum(p[1] for p in parts)))
    return statistics.median(r[0] for r in runs), runs[0][1], [round(r[0], 3) for r in runs]


def compare(name, sc, models, walks, reps, seed=5):
    """One batched launch of `models` against one single solve per model, same sigma_bar and seed."""
    pts = sc.points
    kw = dict(nWalks=walks, maxSteps=sc.max_steps, eps=sc.eps, seed=seed)
    sb = survey.sigma_bar_for_models(sc.solver(), models)
    batched = sc.solver(sigma_bar=sb)
    singles = [dataclasses.replace(sc, sigma=m[0], alpha=m[1]).solver(sigma_bar=sb) for m in models]

    def run_batched():
        _, st = batched.solve_models(pts, models, return_stats=True, **kw)
        return [(batched.last_timing["walk_kernel_ms"], st.total_steps)]

    def run_singles():
        out = []
        for s1 in singles:
            _, st = s1.solve(pts, return_stats=True, **kw)
            out.append((s1.last_timing["walk_kernel_ms"], st.total_steps))
        return out

    b_ms, b_steps, b_runs = timed(run_batched, reps)
    s_ms, s_steps, s_runs = timed(run_singles, reps)
    one_ms = s_ms / len(models)
    print(json.dumps({
        "measurement": name, "models": len(models), "points": len(pts), "walks": walks, "sigma_bar": sb,
        "tree": batched.last_timing["tree"], "launches": batched.last_timing["n_launches"],
        "batched_ms": b_ms, "batched_runs_ms": b_runs, "walk_steps": b_steps,
        "singles_ms": s_ms, "singles_runs_ms": s_runs, "singles_walk_steps": s_steps,
        "singles_over_batched": s_ms / b_ms,
        # a batched walk-step against a single-model step: the same steps, so the times' ratio
        "batched_step_over_single_step": b_ms / one_ms,
        "batched_ns_per_step": 1e6 * b_ms / b_steps, "single_ns_per_step": 1e6 * one_ms / (s_steps / len(models))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--electrodes", type=int, default=48)
    ap.add_argument("--walks", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tree", action="store_true", help="only the wenner_topography (segment-tree) launch")
    ap.add_argument("--tree-electrodes", type=int, default=64)
    ap.add_argument("--tree-walks", type=int, default=2000)
    ap.add_argument("--tree-alpha-bg", type=float, default=0.01, help="the background conductivity of --tree")
    a = ap.parse_args()
    if a.tree:
        sc = S.wenner_topography(n_electrodes=a.tree_electrodes, n_walks=a.tree_walks)
        compare("wenner_topography model+background", sc, [(sc.sigma, sc.alpha), (sc.sigma, F.const(a.tree_alpha_bg))],
                a.tree_walks, a.reps)
        return
    sc = S.dcr_dipole(n_electrodes=a.electrodes)
    compare("dcr_dipole model+background", sc, [(None, sc.alpha), (None, F.const(100.0))], a.walks, a.reps)
    for m in (4, 8):
        models = [(None, S.dcr_alpha_geophysical(1.0 + 0.01 * k)) for k in range(m)]
        compare(f"dcr_dipole {m} perturbed inclusions", sc, models, a.walks, a.reps)


if __name__ == "__main__":
    main()
