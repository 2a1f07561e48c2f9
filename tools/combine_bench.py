#!/usr/bin/env python3
"""Weighted channel combinations on the device against the host path.

The 2.5-D case of README: dcr_dipole with 16 electrodes, 100k walks, the 8 wavenumbers of
wavenumber_quadrature x 2 transmitter dipoles = 16 channels in one launch, compat="fixed" (its
step-count refusal off: the walks of this box end at maxSteps, which is fine for a timing).
wavenumber.transformed_potentials end to end, wall clock: the host path copies the per-walk
values [8, 2, 16, W] to the host and combines them in numpy; device_reduce=True reduces the
per-walk weighted sums on the device (wost_block_combine). The two paths alternate; median of
--reps runs each after a warm-up of both. Also the HIP-event time of the combine kernel
(wost_last_combine_ms), the bytes it reads (walks x channels x 4) and that time's ratio to the
floor at 6.3 TB/s. Prints one JSON line. Honours WOST_LIB.
Usage: python tools/combine_bench.py [--electrodes 16] [--walks 100000] [--reps 3] [--compat fixed]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcrmontecarlo_amd import scenarios as S  # noqa: E402
from dcrmontecarlo_amd import survey  # noqa: E402
from dcrmontecarlo_amd import wavenumber as WN  # noqa: E402

HBM_BYTES_PER_S = 6.3e12   # the achievable HBM rate the floor is taken at


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--electrodes", type=int, default=16)
    ap.add_argument("--walks", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--compat", default="fixed")
    a = ap.parse_args()

    sc = S.dcr_dipole(n_electrodes=a.electrodes)
    pts = sc.points
    e = np.asarray(pts, np.float64)
    dx = float(pts[1, 0] - pts[0, 0])
    k, w = WN.wavenumber_quadrature(dx, 10.0 * dx, 8)
    srcs = [survey.dipole_source(e[0], e[1], 0.5), survey.dipole_source(e[2], e[3], 0.5)]
    sc = dataclasses.replace(sc, f=srcs[0])
    solver = sc.solver(compat=a.compat, sigma_bar=WN.sigma_bar_for(sc.solver(), float(k.max())))
    if a.compat == "fixed":
        solver.set_fixed_step_check(False)
    groups = [np.arange(len(k))]
    C = len(k) * len(srcs)

    def run(device_reduce):
        t0 = time.perf_counter()
        tr = WN.transformed_potentials([solver], groups, pts, srcs, k, w, a.walks, sc.max_steps, sc.eps, seed=5,
                                       device_reduce=device_reduce)
        return (time.perf_counter() - t0) * 1e3, tr

    run(False), run(True)   # warm-up: the kernels compiled, the buffers allocated
    host_ms, dev_ms, comb_ms, kern_ms = [], [], [], []
    for _ in range(a.reps):
        t, tr_h = run(False)
        host_ms.append(t)
        t, tr_d = run(True)
        dev_ms.append(t)
        comb_ms.append(solver.last_combine_ms)
        kern_ms.append(tr_d.kernel_ms)
    scale = np.abs(tr_h.mean).max()
    nbytes = len(pts) * a.walks * C * 4
    floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
    cm = statistics.median(comb_ms)
    print(json.dumps({
        "measurement": "transformed_potentials, host combination against device_reduce", "electrodes": a.electrodes,
        "walks": a.walks, "channels": C, "combinations": len(srcs), "compat": a.compat, "sigma_bar": solver.sigma_bar,
        "host_path_ms": statistics.median(host_ms), "host_path_runs_ms": [round(t, 2) for t in host_ms],
        "device_reduce_ms": statistics.median(dev_ms), "device_reduce_runs_ms": [round(t, 2) for t in dev_ms],
        "host_over_device": statistics.median(host_ms) / statistics.median(dev_ms),
        "walk_kernel_ms": statistics.median(kern_ms), "combine_kernel_ms": cm,
        "combine_kernel_runs_ms": [round(t, 4) for t in comb_ms], "combine_bytes_read": nbytes,
        "combine_floor_ms_at_6.3TBps": floor_ms, "floor_over_combine": floor_ms / cm if cm > 0 else None,
        "max_abs_mean_difference_over_scale": float(np.abs(tr_d.mean - tr_h.mean).max() / scale),
        "max_rel_stderr_difference": float(np.max(np.abs(tr_d.stderr - tr_h.stderr)[tr_h.stderr > 0]
                                                  / tr_h.stderr[tr_h.stderr > 0], initial=0.0))}))


if __name__ == "__main__":
    main()
