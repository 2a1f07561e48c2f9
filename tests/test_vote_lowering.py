"""The walk kernels' wave votes test scalar lane masks (wost_device.h WaveMask): none of the
restated votes sends its mask through a VGPR and back. Checked offline on the generated
kernels' gfx950 assembly (tools/jit_isa.py: the source libwost would hand to hiprtc, compiled
with hiprtc's options); no GPU is needed.

A round trip is a `v_cndmask_b32 vN, 0, 1, <mask>` whose vN is next read by a
`v_cmp_ne_u32 <mask>, 0, vN` (tools/jit_isa.py round_trips). PARENT holds the figures the same
functions gave on the parent commit bf91a09; RESTATED is the number of restated vote sites each
scenario's kernel contains, of
  the loop head's idle-lane ballot, the refill test's any(active), the loop's exit vote, the
  refill round's ballot, poly_distance_const's redo, unit_direction's !fast, norm_greater's band,
  the generated alpha jet's whole-field saturation vote and the flat-sigma' vote:
  * dcr_dipole (C4): all nine, and the four votes of its jet's unsaturated side: 13 of 13;
  * variable_coefficients (C3, detached alpha: no jet shortcut, sigma != 0): the first seven;
  * poisson_square (C2: no Neumann polyline, no delta tracking): the loop's four, redo, band;
  * wenner_topography (C5, tree kernel: the refill test's vote is compiled out, the Dirichlet
    square is compiled in): the other eight.
A kernel's count is at most the parent's less its restated sites; registers, SGPR spills and
scratch do not exceed the parent's."""
import importlib.util
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

from dcrmontecarlo_amd import scenarios as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# parent commit bf91a09: round trips, VALU instructions in the kernel's loops (static), resources
PARENT = {
    "dcr_dipole": dict(round_trips=13, loop_valu=990, vgpr_count=67, sgpr_spill_count=9, private_segment_fixed_size=0),
    "variable_coefficients": dict(round_trips=7, loop_valu=1647, vgpr_count=72, sgpr_spill_count=11,
                                  private_segment_fixed_size=0),
    "poisson_square": dict(round_trips=6, loop_valu=542, vgpr_count=42, sgpr_spill_count=0, private_segment_fixed_size=0),
    "wenner_topography": dict(round_trips=27, loop_valu=2883, vgpr_count=96, sgpr_spill_count=47,
                              private_segment_fixed_size=56),
}
RESTATED = {"dcr_dipole": 13, "variable_coefficients": 7, "poisson_square": 6, "wenner_topography": 8}


def _tool():
    spec = importlib.util.spec_from_file_location("jit_isa", os.path.join(REPO, "tools", "jit_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """Each scenario's generated kernel, compiled once: (assembly, body of wost_walk_jit)."""
    J = _tool()
    d = tmp_path_factory.mktemp("vote_isa")
    paths = {}
    for name in PARENT:
        sc = (S.ALL[name](n_electrodes=4, n_walks=1) if name in ("dcr_dipole", "wenner_topography") else S.ALL[name]())
        paths[name] = str(d / (name + ".hip"))
        with open(paths[name], "w") as f:
            f.write(sc.kernel_source())
    with ThreadPoolExecutor(len(paths)) as ex:
        out = dict(zip(paths, ex.map(J.assemble, paths.values())))
    return J, out


def test_the_counter_finds_a_round_trip_and_skips_the_integer_selects():
    J = _tool()
    body = "\n".join([
        "\tv_cndmask_b32_e64 v0, 0, 1, s[66:67]",
        "\ts_nop 1",
        "\tv_cmp_ne_u32_e32 vcc, 0, v0",                # a vote through v0
        "\tv_cndmask_b32_e64 v5, 0, 1, vcc",
        "\tv_add_u32_e32 v6, v5, v7",                   # an integer use of the 0/1: not a vote
        "\tv_cmp_ne_u32_e32 vcc, 0, v5",
        ".LBB0_3:                                ;   in Loop: Header=BB0_2 Depth=1",
        "\tv_cndmask_b32_e64 v9, 0, 1, s[4:5]",
        "\tv_cmp_ne_u32_e64 s[4:5], 0, v9",
        "\tv_cndmask_b32_e64 v8, 1.0, 0, s[8:9]",       # another select
        "\tv_cmp_ne_u32_e32 vcc, 0, v8",
    ])
    trips = J.round_trips(body)
    assert [(a, b) for a, _, b, _ in trips] == [(1, 3), (8, 9)]
    assert J.loop_valu(body) == 4


@pytest.mark.parametrize("name", list(PARENT))
def test_votes_do_not_go_through_a_vgpr(kernels, name):
    J, out = kernels
    text, body = out[name]
    trips = J.round_trips(body)
    res = J.resources(text)
    par = PARENT[name]
    print(f"{name}: round trips {par['round_trips']} -> {len(trips)}; VALU in loops (static) "
          f"{par['loop_valu']} -> {J.loop_valu(body)}; "
          + ", ".join(f"{k} {par[k]} -> {res[k]}" for k in ("vgpr_count", "sgpr_spill_count", "private_segment_fixed_size")))
    for n1, s1, n2, s2 in trips:
        print(f"    {n1}: {s1} / {n2}: {s2}")
    if name == "dcr_dipole":
        assert len(trips) == 0
    assert len(trips) <= par["round_trips"] - RESTATED[name]
    for k in ("vgpr_count", "sgpr_spill_count", "private_segment_fixed_size"):
        assert res[k] <= par[k], k
