#!/usr/bin/env python3
"""Offline ISA of a scenario's field-specialised walk kernel (no GPU needed).

Generates the kernel source libwost would hand to hiprtc (wost_kernel_source),
compiles it with hipcc for gfx950 with hiprtc's options, and prints the
kernel's resource usage and an instruction histogram (static counts).
Usage: python tools/jit_isa.py dcr_dipole [--out build/jit] [--show] [--votes] [--wavenumbers NK] [--sources NS]
       [--point-charges PC]   (point sources: PC charges in NS sources, compat="fixed")
       [--models M]           (set_models: the scenario's fields, a constant background, then perturbed copies)
       [--point-list]         (the kernel of solve_range(point_ids=...) / solve_to_tolerance: WOST_POINT_LIST)
       [--tally]              (the kernel of solve_greens_map: WOST_TALLY; compat="fixed", the scenario's own source)
       [--tally-maps T]       (the kernel of solve_greens_maps with T maps: WOST_TALLY_MAPS; compat="fixed", with
                               --wavenumbers / --models)
       [--compat fixed]       (the plain kernel under compat="fixed": what --tally is compared with)"""
import argparse
import collections
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

_CND = re.compile(r"^v_cndmask_b32(?:_e32|_e64)?\s+(v\d+),\s*0,\s*1(?:,\s*(?:vcc|s\[\d+:\d+\]))?$")
_CMP = re.compile(r"^v_cmp_ne_u32(?:_e32|_e64)?\s+(?:vcc|s\[\d+:\d+\]),\s*0,\s*(v\d+)$")


def instructions(body):
    """(line number, text, in a loop) of every instruction of a function body."""
    out, in_loop = [], False
    for n, line in enumerate(body.splitlines(), 1):
        code, _, note = line.partition(";")
        s = code.strip()
        if s.endswith(":") or (not s and note.lstrip().startswith("%bb.")):   # a block starts
            in_loop = "in Loop:" in note or "Loop Header:" in note
        if not s or s.startswith((".", "//")) or s.endswith(":"):
            continue
        out.append((n, s, in_loop))
    return out


def round_trips(body):
    """The wave votes that send a lane mask through a VGPR and back: a v_cndmask_b32 vN, 0, 1, <mask>
    whose vN is next read by a v_cmp_ne_u32 <mask>, 0, vN. (The 0/1 selects of the walk-id arithmetic
    are read by other instructions.) Returns [(line, select, line, compare)]."""
    ins = instructions(body)
    found = []
    for i, (n, s, _) in enumerate(ins):
        m = _CND.match(s)
        if not m:
            continue
        reg = re.compile(r"\b" + m.group(1) + r"\b")
        for n2, s2, _ in ins[i + 1:]:
            if reg.search(s2):
                m2 = _CMP.match(s2)
                if m2 and m2.group(1) == m.group(1):
                    found.append((n, s, n2, s2))
                break
    return found


def loop_valu(body):
    """Static count of the VALU instructions inside the function's loops."""
    return sum(1 for _, s, in_loop in instructions(body) if in_loop and s.startswith("v_"))


def assemble(hip):
    """Compiles a generated kernel source to gfx950 assembly with hiprtc's options (next to it, .s);
    returns the assembly and the body of wost_walk_jit."""
    asm = os.path.splitext(hip)[0] + ".s"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--offload-device-only", "-S", "-O3", "-std=c++17",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-ffp-contract=fast-honor-pragmas",
           *([] if os.environ.get("WOST_JIT_SLP") == "1" else ["-fno-slp-vectorize"]),
           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "dcrmontecarlo_amd", "csrc"), hip, "-o", asm]
    subprocess.run(cmd, check=True)
    text = open(asm).read()
    return text, text.split("wost_walk_jit:", 1)[1].split(".Lfunc_end", 1)[0]


def resources(text):
    """The kernel's resource usage from the assembly's metadata."""
    keys = ("vgpr_count", "sgpr_count", "lds_size", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
    found = {k: re.search(rf"\.{k}:\s+(\d+)", text) for k in keys}
    return {k: int(m.group(1)) for k, m in found.items() if m}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenario")
    ap.add_argument("--out", default=os.path.join(REPO, "build", "jit"))
    ap.add_argument("--show", action="store_true", help="print the ISA")
    ap.add_argument("--votes", action="store_true",
                    help="list the wave votes that still go through a VGPR (v_cndmask 0/1, v_cmp_ne), by body line")
    ap.add_argument("--waves", default=None, help="WOST_JIT_WAVES for the generator")
    ap.add_argument("--wavenumbers", type=int, default=0, help="NK: wavenumbers per walk (set_wavenumbers; 0: none)")
    ap.add_argument("--sources", type=int, default=0, help="NS: copies of the scenario's source (solve_sources; 0: its own)")
    ap.add_argument("--point-charges", type=int, default=0,
                    help="PC: point charges (set_point_sources) in --sources sources, instead of the source field")
    ap.add_argument("--models", type=int, default=0,
                    help="NM: conductivity models per walk (set_models; 0: none): the scenario's own fields, a "
                         "constant-alpha background, then copies with a scaled conductivity")
    ap.add_argument("--point-list", action="store_true",
                    help="the point-list kernel (solve_range(point_ids=...), solve_to_tolerance); not with --point-charges")
    ap.add_argument("--tally", action="store_true",
                    help="the tally kernel (solve_greens_map; compat=\"fixed\"); not with the channel options")
    ap.add_argument("--tally-maps", type=int, default=0,
                    help="T: the channel-map kernel (solve_greens_maps; compat=\"fixed\"); with --wavenumbers / --models")
    ap.add_argument("--compat", default="reference", choices=("reference", "fixed"), help="the kernel's estimators")
    a = ap.parse_args()
    if a.point_list and a.point_charges:
        ap.error("--point-list: not together with --point-charges")
    if a.tally and (a.point_list or a.point_charges or a.sources or a.wavenumbers or a.models):
        ap.error("--tally: one channel only")
    if a.tally_maps and (a.tally or a.point_list or a.point_charges or a.sources):
        ap.error("--tally-maps: with --wavenumbers and --models only")
    if a.waves:
        os.environ["WOST_JIT_WAVES"] = a.waves
    from dcrmontecarlo_amd import scenarios as S

    kw = {"n_walks": 1}
    sc = S.ALL[a.scenario](**({"n_electrodes": 4} if a.scenario in ("dcr_dipole", "wenner_topography") else {}), **kw) \
        if a.scenario in ("dcr_dipole", "wenner_topography") else S.ALL[a.scenario]()
    models = None
    if a.models:
        from dcrmontecarlo_amd import fields as F

        dcr = a.scenario == "dcr_dipole"
        models = [(sc.sigma, sc.alpha), (sc.sigma, F.const(100.0 if dcr else 1.0))]
        models += [(sc.sigma, S.dcr_alpha_geophysical(1.0 + 0.01 * k) if dcr else sc.alpha * (1.0 + 0.01 * k))
                   for k in range(1, a.models - 1)]
        models = models[:a.models]
    if a.tally:
        src = sc.kernel_source(compat="fixed", tally=True)
    elif a.point_charges:
        src = sc.kernel_source_points(a.point_charges, max(a.sources, 1), n_wavenumbers=a.wavenumbers)
    else:
        src = sc.kernel_source(n_wavenumbers=a.wavenumbers, **({"sources": [sc.f * (1.0 + k) for k in range(a.sources)]}
                                                               if a.sources else {}),
                               **({"models": models} if models else {}), point_list=a.point_list,
                               compat="fixed" if a.tally_maps else a.compat, tally_maps=a.tally_maps)
    os.makedirs(a.out, exist_ok=True)
    tag = a.scenario + (f"_nk{a.wavenumbers}" if a.wavenumbers else "") + (f"_ns{a.sources}" if a.sources else "") + (
        f"_pc{a.point_charges}" if a.point_charges else "") + (f"_nm{a.models}" if a.models else "") + (
        "_list" if a.point_list else "") + (
        "_tally" if a.tally else f"_maps{a.tally_maps}" if a.tally_maps else "_fixed" if a.compat == "fixed" else "")
    hip = os.path.join(a.out, f"{tag}.hip")
    with open(hip, "w") as f:
        f.write(src)
    text, body = assemble(hip)
    hist = collections.Counter()
    n = 0
    for line in body.splitlines():
        s = line.strip()
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        hist[op] += 1
        n += 1
    print(f"{a.scenario}: {n} instructions;", ", ".join(f"{k}={v}" for k, v in resources(text).items()))
    for pre in ("v_", "s_", "ds_", "global_", "buffer_", "scratch_"):
        print(f"  {pre}*: {sum(c for o, c in hist.items() if o.startswith(pre))}")
    trans = [o for o in hist if re.match(r"v_(exp|log|rcp|rsq|sqrt|sin|cos)_f32", o)]
    print("  transcendental:", {o: hist[o] for o in trans})
    print("  top:", hist.most_common(25))
    if a.votes:
        trips = round_trips(body)
        print(f"  VALU in loops: {loop_valu(body)}; wave votes through a VGPR: {len(trips)}")
        for n1, s1, n2, s2 in trips:
            print(f"    {n1}: {s1}\n    {n2}: {s2}")
    if a.show:
        print(body)


if __name__ == "__main__":
    main()
