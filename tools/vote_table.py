#!/usr/bin/env python3
"""How often the walk kernel's wave votes take their slow side (study build, GPU).

Each vote of wost_device.h / wost_walk.h guards an exact fallback that a wave runs only
when one of its lanes needs it. With option vote_stats the field-specialised kernel counts,
per site, the times the vote ran, the times some lane needed the slow side, and the lanes
that needed it (WOST_VOTE; the waves add their counts once, at their ends). This prints,
per scenario, a table: votes and slow-side entries per wave-step, the share of votes that
enter, and the mean number of lanes that needed the slow side when a wave entered.

Usage (GPU box, after `make -C dcrmontecarlo_amd/csrc study`):
    WOST_LIB=build/libwost_study.so python tools/vote_table.py [--walks-scale 0.1] [--only a,b]
"""
import argparse
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# site ids of WOST_VOTE(site, ...), and the static VALU count of each slow side where known
SITES = ["walk-step (lanes stepping)", "sqrt_rn: x outside [2^-96, inf)", "norm_greater: band above b2",
         "fv_exp_quad_diag: exp needed", "fv_sigmoid_radial: unsaturated", "fj_exp_quad_diag: exp needed",
         "fj_sigmoid_radial: unsaturated", "sigma_prime_from: acp != ac", "poly_distance_const: redo",
         "ray test: tiny t", "unit_direction: !fast", "ray test: candidate body (IEEE division)",
         "generated alpha_jet: not saturated", "delta update: a colliding lane needs sigma'"]
SIZES = {"dcr_dipole": ("C4", 48, 1_000_000), "variable_coefficients": ("C3", 256, 100_000)}


def run_one(name, scale):
    sys.path.insert(0, REPO)
    from dcrmontecarlo_amd import scenarios as S

    _, n, W = SIZES[name]
    sc = S.ALL[name]()
    s = sc.solver(device=0)
    s.set_option("jit_race", 0)      # the specialised kernel from the first launch on
    s.set_option("vote_stats", 1)    # study builds only
    _, st = s.solve_walks(sc.points[:n], nWalks=max(64, int(W * scale)), maxSteps=sc.max_steps, eps=sc.eps, seed=7)
    print("lane_steps:", int(st.sum()))


def table(name, words, lane_steps):
    tag = SIZES[name][0]
    runs0, _, lanes0 = words[0:3]
    out = [f"{tag} ({name}): {lane_steps} lane-steps, {runs0} wave-steps, {lanes0 / max(runs0, 1):.1f} lanes stepping per wave-step",
           "", "| Site | votes per wave-step | entries per wave-step | share of votes that enter | mean lanes needing it |",
           "|---|---|---|---|---|"]
    for i, label in enumerate(SITES):
        if i == 0:
            continue
        runs, ent, lanes = words[3 * i:3 * i + 3]
        if runs == 0:
            out.append(f"| {label} | 0 | — | — | — |")
            continue
        out.append(f"| {label} | {runs / runs0:.3f} | {ent / runs0:.4f} | {100.0 * ent / runs:.2f}% | "
                   + (f"{lanes / ent:.2f}" if ent else "—") + " |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--walks-scale", type=float, default=0.1, help="fraction of the bench's walks per point")
    ap.add_argument("--only", default=",".join(SIZES))
    a = ap.parse_args()
    if a.one:
        run_one(a.one, a.walks_scale)
        return 0
    for name in a.only.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--walks-scale", str(a.walks_scale)],
                           capture_output=True, text=True)
        votes = [l for l in r.stderr.splitlines() if l.startswith("vote_stats:")]
        steps = [l for l in r.stdout.splitlines() if l.startswith("lane_steps:")]
        if r.returncode != 0 or not votes or not steps:
            sys.stderr.write(r.stderr[-2000:])
            print(f"{name}: no vote_stats line (needs the study build: WOST_LIB=build/libwost_study.so)")
            return 1
        words = [0] * 48
        for l in votes:   # one line per solve
            for i, v in enumerate(l.split()[1:]):
                words[i] += int(v)
        lane_steps = int(steps[0].split()[1])
        if words[2] != lane_steps:
            print(f"{name}: counted {words[2]} stepping lanes, the kernel reports {lane_steps} walk-steps")
            return 1
        print(table(name, words, lane_steps))
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
