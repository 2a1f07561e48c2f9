#!/usr/bin/env python3
"""2.5-D wavenumber batching on one GPU (DESIGN.md "2.5-D wavenumber batching").

1. dcr_dipole at a reduced size with K = 8 wavenumbers of wavenumber_quadrature: one batched
   solve (every wavenumber scored by the same walks) against 8 single solves with
   sigma = k^2 alpha and the same sigma_bar -- the only way to get these numbers without
   wost_set_wavenumbers -- and one wavenumber group against two (low k and high k, each with
   its own sigma_bar). Walk-kernel time from libwost's HIP events, after a warm-up solve.
2. --halfspace: the 2.5-D Wenner apparent resistivity of a homogeneous box against the true
   resistivity (run_wenner_survey_25d, compat="fixed"), for one and two groups.
Prints one JSON line per measurement. Honours WOST_LIB.
Usage: python tools/wavenumber_bench.py [--electrodes 16] [--walks 100000] [--reps 3] [--halfspace]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcrmontecarlo_amd import fields as F  # noqa: E402
from dcrmontecarlo_amd import scenarios as S  # noqa: E402
from dcrmontecarlo_amd import wavenumber as WN  # noqa: E402


def timed(fn, reps):
    """(median walk-kernel ms, walk-steps) of fn() -> [(ms, steps), ...] summed per call, after one warm-up."""
    fn()
    runs = []
    for _ in range(reps):
        parts = fn()
        runs.append((sum(p[0] for p in parts), sum(p[1] for p in parts)))
    ms = statistics.median(r[0] for r in runs)
    return ms, runs[0][1], [round(r[0], 3) for r in runs]


def dcr_bench(a):
    sc = S.dcr_dipole(n_electrodes=a.electrodes)
    pts = sc.points
    dx = float(pts[1, 0] - pts[0, 0])
    k, w = WN.wavenumber_quadrature(dx, 10.0 * dx, 8)
    probe = sc.solver()
    sp_max = WN.sigma_bar_for(probe, 0.0)
    kw = dict(nWalks=a.walks, maxSteps=sc.max_steps, eps=sc.eps, seed=5)

    def one_solver(idx):
        return sc.solver(sigma_bar=sp_max + float(k[idx].max()) ** 2)

    def batched(solver, idx):
        def run():
            _, st = solver.solve_wavenumbers(pts, k[idx], return_stats=True, **kw)
            return [(solver.last_timing["walk_kernel_ms"], st.total_steps)]
        return run

    every = np.arange(len(k))
    sb = one_solver(every)
    b_ms, b_steps, b_runs = timed(batched(sb, every), a.reps)
    # the 8 single solves: sigma = k^2 alpha as the sigma field, the same sigma_bar
    singles = [dataclasses.replace(sc, sigma=float(q * q) * sc.alpha).solver(sigma_bar=sb.sigma_bar) for q in k]

    def run_singles():
        out = []
        for s1 in singles:
            _, st = s1.solve(pts, return_stats=True, **kw)
            out.append((s1.last_timing["walk_kernel_ms"], st.total_steps))
        return out

    s_ms, s_steps, s_runs = timed(run_singles, a.reps)
    lo, hi = WN.wavenumber_groups(k, 2)
    g_lo, g_hi = one_solver(lo), one_solver(hi)
    r_lo, r_hi = batched(g_lo, lo), batched(g_hi, hi)
    g_ms, g_steps, g_runs = timed(lambda: r_lo() + r_hi(), a.reps)
    rate = lambda steps, ms: steps / (ms * 1e-3)
    print(json.dumps({
        "measurement": "dcr_dipole K=8", "electrodes": a.electrodes, "walks": a.walks, "k": [round(float(x), 5) for x in k],
        "sigma_bar": sb.sigma_bar, "sigma_bar_groups": [g_lo.sigma_bar, g_hi.sigma_bar],
        "batched_ms": b_ms, "batched_runs_ms": b_runs, "batched_walk_steps": b_steps,
        "batched_walk_steps_per_s": rate(b_steps, b_ms),
        "singles_ms": s_ms, "singles_runs_ms": s_runs, "singles_walk_steps": s_steps,
        "singles_walk_steps_per_s": rate(s_steps, s_ms), "singles_over_batched": s_ms / b_ms,
        "two_groups_ms": g_ms, "two_groups_runs_ms": g_runs, "two_groups_walk_steps": g_steps,
        "two_groups_walk_steps_per_s": rate(g_steps, g_ms), "one_group_over_two_groups": b_ms / g_ms}))


def halfspace(a):
    """Wenner over the homogeneous box [-10, 10] x [-10, 0] (Neumann top): electrode spacing
    0.1, so that the box is large against 1 / k_min = 2 (k from 0.1 / 0.2 to 4 / 0.1)."""
    a0, dx, n_el = 2.0, 0.1, 6
    D = np.array([[-10, 0], [-10, -10], [10, -10], [10, 0]], np.float32)
    N = np.array([[10, 0], [-10, 0]], np.float32)
    x = (np.arange(n_el) - 0.5 * (n_el - 1)) * dx
    pts = np.stack([x, np.zeros_like(x)], axis=1).astype(np.float32)
    sc = S.Scenario("halfspace_box", D, N, g=F.const(0.0), f=F.const(0.0), alpha=F.const(a0), points=pts,
                    max_steps=a.halfspace_steps, eps=1e-4)
    for groups in (1, 2):
        r = WN.run_wenner_survey_25d(sc, a.halfspace_walks, a=1, width=0.01, groups=groups, seed=3)
        ratio = r.rho_a * a0   # rho_true = 1 / a0
        se = r.rho_a_se * a0
        # the quadripoles share receiver electrodes: report each, and the mean with the
        # (conservative, fully correlated) mean of their standard errors
        print(json.dumps({"measurement": "halfspace Wenner", "groups": groups, "k": [round(float(v), 4) for v in r.k],
                          "w": [round(float(v), 5) for v in r.w], "sigma_bar": r.sigma_bar,
                          "rho_a_over_rho": [round(float(v), 4) for v in ratio],
                          "stderr": [round(float(v), 4) for v in se], "mean_ratio": float(ratio.mean()),
                          "mean_ratio_stderr": float(se.mean()), "walks": a.halfspace_walks,
                          "walk_steps": r.walk_steps, "kernel_ms": r.kernel_ms, "launches": r.launches}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--electrodes", type=int, default=16)
    ap.add_argument("--walks", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--halfspace", action="store_true", help="only the homogeneous-box Wenner survey")
    ap.add_argument("--halfspace-walks", type=int, default=40_000)
    ap.add_argument("--halfspace-steps", type=int, default=100_000)
    a = ap.parse_args()
    if a.halfspace:
        halfspace(a)
    else:
        dcr_bench(a)


if __name__ == "__main__":
    main()
