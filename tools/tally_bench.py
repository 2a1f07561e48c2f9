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

--channels (channel maps, DESIGN.md 7f "Channel maps"): dcr_dipole with --electrodes points, K = 8
wavenumbers of wavenumber_quadrature(3, 30) at sigma_bar_for(k_max), grids of 32 x 16 and 256 x 128
cells, R = 8. Four routes to the 2.5-D section alternate after a warm-up of each: the plain
solve_wavenumbers launch (no map), one combined row w / 2 (one launch), the 8 unit rows (two
launches of 4 maps) and the route without channel maps, 8 one-channel solve_greens_map calls on
solvers with the explicit sigma = k^2 alpha. Medians of --repeats walk-kernel times, summed over a
route's launches.

Usage: python tools/tally_bench.py [--channels [--electrodes 16]] [--walks 16384] [--steps 200] [--repeats 3]
       [--json out.json]"""
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


def _fitting(call):
    """call(quantum) with the default quantum, or with the one its error message names."""
    try:
        call(None)
        return None
    except ValueError as e:
        m = re.search(r"scale_log2 (-?\d+)", str(e))
        if m is None:
            raise
        return 2.0 ** -int(m.group(1))


def channel_mode(a):
    from dcrmontecarlo_amd import scenarios as S
    from dcrmontecarlo_amd import wavenumber as WN
    from dcrmontecarlo_amd.greens_map import TallyGrid

    sc = dataclasses.replace(S.dcr_dipole(a.electrodes, n_walks=a.walks), max_steps=a.steps)
    k, w = WN.wavenumber_quadrature(3.0, 30.0, 8)
    sb = WN.sigma_bar_for(sc, float(k.max()))
    pts = np.ascontiguousarray(sc.points, np.float32)
    kw = dict(maxSteps=a.steps, eps=sc.eps, seed=7)

    def make(scn):
        s = scn.solver(compat="fixed", device=0, sigma_bar=sb)
        s.set_fixed_step_check(False)
        s.set_option("jit_race", 0)
        return s

    multi = make(sc)
    multi.set_wavenumbers(k)
    singles = [make(dataclasses.replace(sc, sigma=sc.alpha * float(kj * kj))) for kj in k]
    rows = []
    for nx, ny in ((32, 16), (256, 128)):
        grid = TallyGrid(-100.0, -100.0, 200.0 / nx, 200.0 / ny, nx, ny)
        R = 8
        q1 = _fitting(lambda q: multi.solve_greens_maps(pts, grid, w / 2.0, nWalks=a.walks, replicas=R, quantum=q, **kw))
        q8 = _fitting(lambda q: multi.solve_greens_maps(pts, grid, np.eye(8), nWalks=a.walks, replicas=R, quantum=q, **kw))
        qs = [_fitting(lambda q: s.solve_greens_map(pts, grid, nWalks=a.walks, replicas=R, quantum=q, **kw))
              for s in singles]

        def plain():
            multi.solve_range(pts, a.walks, 0, a.walks, **kw)
            return multi.last_timing["walk_kernel_ms"], multi.last_timing["total_steps"]

        def combined():
            multi.solve_greens_maps(pts, grid, w / 2.0, nWalks=a.walks, replicas=R, quantum=q1, **kw)
            return multi.last_timing["walk_kernel_ms"]

        def units():   # (solve_greens_maps keeps the last launch's timing: one launch per call here)
            ms = 0.0
            for t0 in (0, 4):
                multi.solve_greens_maps(pts, grid, np.eye(8)[t0:t0 + 4], nWalks=a.walks, replicas=R, quantum=q8, **kw)
                ms += multi.last_timing["walk_kernel_ms"]
            return ms

        def separate():
            ms = 0.0
            for s, q in zip(singles, qs):
                s.solve_greens_map(pts, grid, nWalks=a.walks, replicas=R, quantum=q, **kw)
                ms += s.last_timing["walk_kernel_ms"]
            return ms

        plain(), combined(), units(), separate()   # warm-up: every kernel compiled, buffers sized
        t = {"plain": [], "combined": [], "units": [], "separate": []}
        steps = 0
        for _ in range(a.repeats):
            ms, steps = plain()
            t["plain"].append(ms)
            t["combined"].append(combined())
            t["units"].append(units())
            t["separate"].append(separate())
        med = {n: statistics.median(v) for n, v in t.items()}
        rows.append({"problem": "dcr_dipole", "grid": f"{nx}x{ny}", "replicas": R, "points": len(pts), "walks": a.walks,
                     "wavenumbers": 8, "sigma_bar": sb, "steps": int(steps), **{f"{n}_ms": v for n, v in med.items()},
                     **{f"{n}_all_ms": v for n, v in t.items()}, "combined_over_separate": med["combined"] / med["separate"],
                     "units_over_separate": med["units"] / med["separate"], "combined_over_plain": med["combined"] / med["plain"]})
        print(f"dcr_dipole K=8 {nx:3d}x{ny:<3d} R={R}: plain {med['plain']:8.3f} ms, combined row {med['combined']:8.3f} ms, "
              f"8 unit rows {med['units']:8.3f} ms, 8 one-channel solves {med['separate']:8.3f} ms; {steps:.3e} steps per "
              f"walk set", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--channels", action="store_true", help="the channel-map routes to a 2.5-D section")
    ap.add_argument("--electrodes", type=int, default=16, help="--channels: query points")
    a = ap.parse_args()
    if a.channels:
        rows = channel_mode(a)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows, f, indent=1)
                f.write("\n")
        return
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
