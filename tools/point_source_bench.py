#!/usr/bin/env python3
"""Point electrodes against Gaussian electrodes on one GPU.

1. The end-to-end 2.5-D Wenner case of DESIGN.md 7a -- homogeneous box [-10, 10] x [-10, 0],
   alpha = 2, six electrodes 0.1 apart, 40,000 walks per electrode, n = 4 wavenumbers -- with
   electrodes="point" against Gaussian electrodes of width 0.01, for one wavenumber group and
   for two: rho_a / rho, its standard error, walk-kernel ms and the number of kernels compiled
   (launches whose kernel was in no cache, jit_ms > 0, with a fresh kernel cache directory),
   for the survey and then for the same survey with its electrodes moved by half a spacing.
2. --dcr: the 16-electrode dcr_dipole batched case (8 wavenumbers x 2 dipoles = 16 channels
   per launch), point dipoles against Gaussian dipoles: walk-kernel ms and walk-steps/s.
Medians of --reps runs after a warm-up. Prints one JSON line per measurement. Honours WOST_LIB.
Usage: python tools/point_source_bench.py [--dcr] [--reps 3] [--walks 40000]"""
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
from dcrmontecarlo_amd import survey  # noqa: E402
from dcrmontecarlo_amd import wavenumber as WN  # noqa: E402


def wenner(a):
    a0, dx, n_el = 2.0, 0.1, 6
    D = np.array([[-10, 0], [-10, -10], [10, -10], [10, 0]], np.float32)
    N = np.array([[10, 0], [-10, 0]], np.float32)
    x = (np.arange(n_el) - 0.5 * (n_el - 1)) * dx
    pts = np.stack([x, np.zeros_like(x)], axis=1).astype(np.float32)
    sc = S.Scenario("halfspace_box", D, N, g=F.const(0.0), f=F.const(0.0), alpha=F.const(a0), points=pts,
                    max_steps=a.steps, eps=1e-4)
    for electrodes in ("point", "gaussian"):
        for groups in (1, 2):
            k, _ = WN.wavenumber_quadrature(dx, 2 * dx, 4)
            solvers, _ = WN._solvers_25d(sc, k, groups, "fixed", None, None, electrodes)
            compiled = 0
            runs = []
            for rep in range(a.reps + 1):   # (the first is the warm-up: its compiles are counted, its time is not)
                r = WN.run_wenner_survey_25d(sc, a.walks, a=1, width=0.01, groups=groups, seed=3, solvers=solvers,
                                             electrodes=electrodes)
                if rep == 0:
                    compiled = sum(1 for s in solvers if s.last_timing["jit_ms"] > 0)
                else:
                    runs.append(r.kernel_ms)
            ratio, se = r.rho_a * a0, r.rho_a_se * a0
            moved = dataclasses.replace(sc, points=(pts + np.float32([0.5 * dx, 0.0])).astype(np.float32))
            WN.run_wenner_survey_25d(moved, 4096, a=1, width=0.01, groups=groups, seed=3, solvers=solvers,
                                     electrodes=electrodes)
            compiled_moved = sum(1 for s in solvers if s.last_timing["jit_ms"] > 0)
            print(json.dumps({"measurement": "halfspace Wenner", "electrodes": electrodes, "groups": groups,
                              "k": [round(float(v), 4) for v in r.k], "sigma_bar": r.sigma_bar,
                              "rho_a_over_rho": [round(float(v), 4) for v in ratio],
                              "stderr": [round(float(v), 4) for v in se], "mean_ratio": float(ratio.mean()),
                              "mean_ratio_stderr": float(se.mean()), "walks": a.walks, "walk_steps": r.walk_steps,
                              "kernel_ms": statistics.median(runs), "kernel_ms_runs": [round(v, 2) for v in runs],
                              "launches": r.launches, "kernels_compiled": compiled,
                              "kernels_compiled_for_moved_electrodes": compiled_moved}))


def dcr(a):
    sc = S.dcr_dipole(n_electrodes=16)
    pts = sc.points
    e = np.asarray(pts, np.float64)
    dx = float(e[1, 0] - e[0, 0])
    k, _ = WN.wavenumber_quadrature(dx, 10.0 * dx, 8)
    sb = WN.sigma_bar_for(sc.solver(), float(k.max()))
    kw = dict(nWalks=a.dcr_walks, maxSteps=sc.max_steps, eps=sc.eps, seed=5)
    cases = {
        "point": (dataclasses.replace(sc, f=None), [survey.point_dipole(e[7], e[8], surface=False),
                                                    survey.point_dipole(e[3], e[12], surface=False)]),
        "gaussian": (sc, [survey.dipole_source(e[7], e[8], 1.5), survey.dipole_source(e[3], e[12], 1.5)]),
    }
    for name, (scn, srcs) in cases.items():
        s = scn.solver(compat="fixed", sigma_bar=sb)
        s.set_fixed_step_check(False)
        runs = []
        for rep in range(a.reps + 1):
            _, st = s.solve_wavenumbers(pts, k, sources=srcs, return_stats=True, **kw)
            if rep:
                runs.append((s.last_timing["walk_kernel_ms"], st.total_steps))
        ms = statistics.median(r[0] for r in runs)
        print(json.dumps({"measurement": "dcr_dipole 16 electrodes, 8 wavenumbers x 2 dipoles", "sources": name,
                          "walks": a.dcr_walks, "sigma_bar": s.sigma_bar, "kernel_ms": ms,
                          "kernel_ms_runs": [round(r[0], 3) for r in runs], "walk_steps": runs[0][1],
                          "walk_steps_per_s": runs[0][1] / (ms * 1e-3), "jit": s.last_timing["jit"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dcr", action="store_true", help="only the dcr_dipole batched case")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--walks", type=int, default=40_000)
    ap.add_argument("--steps", type=int, default=100_000)
    ap.add_argument("--dcr-walks", type=int, default=100_000)
    a = ap.parse_args()
    if "WOST_JIT_CACHE" not in os.environ:   # a fresh kernel cache: every compile is seen
        import tempfile

        os.environ["WOST_JIT_CACHE"] = tempfile.mkdtemp(prefix="wost_jit_")
    if a.dcr:
        dcr(a)
    else:
        wenner(a)


if __name__ == "__main__":
    main()
