#!/usr/bin/env python3
"""Kernel time of a tally solve (solve_greens_map) against the same handle's plain
solve_range: dcr_dipole (compat="fixed", sigma_bar 0.02) and poisson_square, grids of 32 x 16 and
256 x 128 cells over the domain and, as the case of the most contention, of one cell; R = 1 and 8.
A solve whose deposits do not fit the default quantum is repeated with the quantum its error
message names (dcr_dipole at sigma_bar 0.02: its weights are signed and huge); the
timing does not depend on the quantum, since every deposit is added whatever it rounds to. After one warm-up of each, the two solves
alternate; the medians of --repeats walk-kernel times (HIP events around the walk launches) are
reported, with the walk-steps per second of both. Every step of a walk deposits once unless its
sample is clipped, so the tally's walk-steps per second bound its deposits (64-bit integer
atomic adds) per second from above.

Usage: python tools/tally_bench.py [--walks 16384] [--steps 200] [--repeats 3] [--json out.json]"""
import argparse
import dataclasses
import json
import os
import re
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def cases(walks):
    from dcrmontecarlo_amd import scenarios as S

    dd = S.dcr_dipole(48, n_walks=walks)
    sq = S.poisson_square(64, n_walks=walks)
    return [("dcr_dipole", dd, 0.02, (-100.0, -100.0, 200.0, 200.0)),
            ("poisson_square", sq, None, (-2.0, -2.0, 4.0, 4.0))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from dcrmontecarlo_amd.greens_map import TallyGrid

    rows = []
    for name, sc, sigma_bar, (x0, y0, wx, wy) in cases(a.walks):
        sc = dataclasses.replace(sc, max_steps=a.steps)
        s = sc.solver(compat="fixed", device=0, sigma_bar=sigma_bar)
        s.set_fixed_step_check(False)
        s.set_option("jit_race", 0)
        pts = np.ascontiguousarray(sc.points, np.float32)
        kw = dict(maxSteps=a.steps, eps=sc.eps, seed=7)
        for nx, ny in ((32, 16), (256, 128), (1, 1)):
            grid = TallyGrid(x0, y0, wx / nx, wy / ny, nx, ny)
            for R in (1, 8):
                quantum = None
                try:
                    s.solve_greens_map(pts, grid, nWalks=a.walks, replicas=R, **kw)
                except ValueError as e:   # the deposits do not fit the default quantum: the one the solve names
                    m = re.search(r"scale_log2 (-?\d+)", str(e))
                    if m is None:
                        print(f"{name:15s} {nx:3d}x{ny:<3d} R={R}: not measured: {e}", flush=True)
                        continue
                    quantum = 2.0 ** -int(m.group(1))

                def plain():
                    s.solve_range(pts, a.walks, 0, a.walks, **kw)
                    return s.last_timing

                def tally():
                    gm = s.solve_greens_map(pts, grid, nWalks=a.walks, replicas=R, quantum=quantum, **kw)
                    return s.last_timing, gm

                plain(), tally()   # warm-up: both kernels compiled, buffers sized
                tp, tt, gm = [], [], None
                for _ in range(a.repeats):
                    tp.append(plain())
                    t, gm = tally()
                    tt.append(t)
                mp = statistics.median(t["walk_kernel_ms"] for t in tp)
                mt = statistics.median(t["walk_kernel_ms"] for t in tt)
                steps = tt[-1]["total_steps"]
                row = {"problem": name, "grid": f"{nx}x{ny}", "replicas": R, "points": len(pts), "walks": a.walks,
                       "plain_ms": mp, "tally_ms": mt, "ratio": mt / mp, "steps": int(steps),
                       "plain_steps_per_s": steps / (mp * 1e-3), "tally_steps_per_s": steps / (mt * 1e-3),
                       "cells_hit": int((gm.sums.sum(axis=(0, 1)) != 0).sum()), "quantum_log2": int(np.log2(gm.quantum)),
                       "plain_all_ms": [t["walk_kernel_ms"] for t in tp], "tally_all_ms": [t["walk_kernel_ms"] for t in tt]}
                rows.append(row)
                print(f"{name:15s} {nx:3d}x{ny:<3d} R={R}: plain {mp:8.3f} ms, tally {mt:8.3f} ms (x{mt / mp:.3f}); "
                      f"{steps:.3e} steps: {row['plain_steps_per_s']:.3e} -> {row['tally_steps_per_s']:.3e} steps/s; "
                      f"{row['cells_hit']} of {nx * ny} cells hit", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
