"""The field interpreter (wost_device.h fj_*, jet_mul, field_jet, field_value,
sigma_prime_from, sat_*) against float64 torch autograd on the field zoo
(tests/field_zoo.py, which derives the tolerances), on a host build of the header: libm is
IEEE there, so the bounds hold with room. The device runs the same header against the same
reference in tests/test_gpu_field_zoo.py.

Mutation check, carried out by hand on this test: deleting the ``2.0f * (a.gx * b.gx +
a.gy * b.gy)`` cross term of jet_mul fails test_jets_match_the_reference and the sigma' test
for trig_product, three_factors and grid (the fields whose terms multiply two factors with
a gradient); flipping the sign of ``-s * a`` in fj_cos_lin fails both for trig_product (the
zoo's other cosine, cos(Y) in grid, has a = 0).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import field_zoo as Z
from dcrmontecarlo_amd import fields as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

# wost_device.h's alignas(16) records
DTERM = np.dtype([("coef", "<f4"), ("first", "<i4"), ("nf", "<i4"), ("pad", "<i4")])
DFACTOR = np.dtype([("kind", "<i4"), ("pad", "<i4", (3,)), ("p", "<f4", (8,))])
DFIELD = np.dtype([("n_terms", "<i4"), ("first_term", "<i4"), ("flags", "<i4"), ("present", "<i4")])
KIND_NAME = {F.FK_MONO: "mono", F.FK_SIN_LIN: "sin_lin", F.FK_COS_LIN: "cos_lin", F.FK_SIGMOID_LIN: "sigmoid_lin",
             F.FK_SIGMOID_RADIAL: "sigmoid_radial", F.FK_IND_BOX: "ind_box", F.FK_IND_DISK: "ind_disk",
             F.FK_GRID: "grid"}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("field_jet") / "libfield_jet_check.so")
    # host build of the __host__ __device__ header, every operation rounded on its own
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950",
                    "-ffp-contract=off", "-I" + os.path.join(REPO, "include"), "-x", "hip",
                    os.path.join(HERE, "native", "field_jet_check.cpp"), "-o", out], check=True)
    so = ctypes.CDLL(out)
    so.field_jet_check.restype = ctypes.c_int
    so.field_jet_check.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    sizes = np.zeros(3, np.float32)
    assert so.field_jet_check(None, None, None, None, None, 0, 4, sizes.ctypes.data) == 0
    assert [int(s) for s in sizes] == [DTERM.itemsize, DFACTOR.itemsize, DFIELD.itemsize] == [16, 48, 16]
    return so


def pack(fields):
    """The records of one program holding `fields` (None: an absent field): terms, factors
    and grid values one after another, with absolute indices as the device's program has."""
    terms, factors, grids, recs = [], [], [], np.zeros(len(fields), DFIELD)
    n_grid = 0
    for i, fld in enumerate(fields):
        if fld is None:
            continue
        t, f = fld.pack()
        recs[i] = (len(t), len(terms), fld.flags, 1)
        base = len(factors)
        for kind, p in f:
            p = list(p)
            if kind == F.FK_GRID:
                p[6] += n_grid
            factors.append((kind, (0, 0, 0), tuple(np.float32(v) for v in p)))
        terms += [(np.float32(c), base + first, n, 0) for c, first, n in t]
        g = fld.grid_values()
        grids.append(g)
        n_grid += g.size
    T = np.array(terms, DTERM) if terms else np.zeros(1, DTERM)
    Fa = np.array(factors, DFACTOR) if factors else np.zeros(1, DFACTOR)
    G = np.ascontiguousarray(np.concatenate(grids + [np.zeros(1, np.float32)]), np.float32)
    return T, Fa, G, recs


def run(lib, fields, pts, mode, width):
    T, Fa, G, recs = pack(fields)
    p = np.ascontiguousarray(pts, np.float32)
    out = np.full((len(p), width), np.nan, np.float32)
    assert lib.field_jet_check(T.ctypes.data, Fa.ctypes.data, G.ctypes.data, recs.ctypes.data, p.ctypes.data, len(p),
                               mode, out.ctypes.data) == 0
    return out


def jet(lib, field, pts):
    return run(lib, [field], pts, 1, 4)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("name", list(Z.ZOO))
def test_jets_match_the_reference(lib, name, positive):
    field = (Z.POSITIVE if positive else Z.ZOO)[name]
    pts = Z.points_for(name)
    got = jet(lib, field, pts)
    ratios = Z.compare(got, name, positive)
    print(f"{name}{' (positive)' if positive else ''}: largest error / tolerance per component {np.round(ratios, 3)}")
    assert np.all(ratios <= 1.0), ratios


@pytest.mark.parametrize("name", list(Z.ZOO))
def test_field_value_is_the_jets_value_bit_for_bit(lib, name):
    """field_value against field_jet's value on every point of every zoo field: the generated
    whole-field saturated return takes the one for the other, and a walk uses alpha's value
    and its jet at the same point. This failed for sigmoid_radial_neg, sigmoid_radial_pos and
    sharp while fv_sigmoid_radial took the distance as sqrt(d2) and fj_sigmoid_radial as
    d2 * rsq(d2): on the host build 122 of 300, 109 of 300 and 12 of 621 values differed
    inside a radial factor's band, by at most 1.2e-7, 1.2e-7 and 1.4e-6. Both now form the
    distance the same way."""
    field = Z.ZOO[name]
    pts = Z.points_for(name)
    v, j = run(lib, [field], pts, 0, 1)[:, 0], jet(lib, field, pts)[:, 0]
    diff = _bits(v) != _bits(j)
    print(f"{name}: {diff.sum()} of {len(pts)} values differ, largest |difference| "
          f"{np.abs(v.astype(np.float64) - j)[diff].max(initial=0.0):.3g}")
    np.testing.assert_array_equal(_bits(v), _bits(j))


@pytest.mark.parametrize("detached", [False, True])
@pytest.mark.parametrize("sigma_key", list(Z.SIGMAS))
@pytest.mark.parametrize("name", list(Z.ZOO))
def test_sigma_prime_matches_the_reference_formula(lib, name, sigma_key, detached):
    alpha = Z.POSITIVE[name]
    pts = Z.points_for(name)
    got = run(lib, [F.detach(alpha) if detached else alpha, Z.SIGMAS[sigma_key]], pts, 2, 1)[:, 0]
    ratio = Z.compare_sigma_prime(got, name, sigma_key, detached)
    print(f"sigma'({name}, sigma={sigma_key}, detached={detached}): largest error / tolerance {ratio:.3f}")
    assert ratio <= 1.0


def test_grid_at_its_nodes_and_outside(lib):
    """The cases the uniform points leave out: at a node the value is the node's (t = 0: the
    weights are exactly 0, 1, 0, 0); outside the grid every derivative is exactly zero and
    the value that of the nearest edge point."""
    tab = Z._tab()
    nodes, values = Z.grid_nodes()
    np.testing.assert_array_equal(jet(lib, tab, nodes)[:, 0], values)
    out = Z.special_points("outside_grid")
    assert np.all(Z.grid_outside(out))
    both = out[(np.abs(out[:, 0]) > 0.9375) & (np.abs(out[:, 1]) > 1.0)]
    assert len(both) >= 2
    j = jet(lib, tab, both)
    np.testing.assert_array_equal(j[:, 1:], np.zeros((len(both), 3), np.float32))
    # outside in x only: d/dx is zero, and the Laplacian is the y part alone
    j = jet(lib, tab, out)
    ref = Z.reference_jet(tab, out)
    outx = np.abs(out[:, 0]) > 0.9375
    assert outx.any() and np.all(j[outx, 1] == 0) and np.all(ref[outx, 1] == 0)
    outy = np.abs(out[:, 1]) > 1.0
    assert outy.any() and np.all(j[outy, 2] == 0) and np.all(ref[outy, 2] == 0)
    clamped = np.clip(out, [-0.9375, -1.0], [0.9375, 1.0]).astype(np.float32)
    np.testing.assert_array_equal(_bits(j[:, 0]), _bits(jet(lib, tab, clamped)[:, 0]))


def test_indicator_edges_belong(lib):
    box = jet(lib, F.indicator_box(*Z.IND_BOX), Z.special_points("box_edge"))
    disk = jet(lib, F.indicator_disk(Z.IND_DISK_C, Z.IND_DISK_R), Z.special_points("disk_edge"))
    assert np.all(box[:, 0] == 1) and np.all(disk[:, 0] == 1) and np.all(box[:, 1:] == 0) and np.all(disk[:, 1:] == 0)
    outside = Z.special_points("just_outside")
    assert jet(lib, F.indicator_box(*Z.IND_BOX), outside[:1])[0, 0] == 0
    assert jet(lib, F.indicator_disk(Z.IND_DISK_C, Z.IND_DISK_R), outside[1:])[0, 0] == 0
    # (the zoo's `indicators` is compared at these points in test_jets_match_the_reference)
    edge = Z.special_points("box_edge", "disk_edge", "just_outside")
    assert all(np.any(np.all(Z.points_for("indicators") == e, axis=1)) for e in edge)


def _single_factor_fields(field):
    """One Field per factor of `field`, in the order of pack(): the factor alone."""
    out = []
    for t in field.terms:
        if t.mono != (0, 0):
            out.append((F.FK_MONO, F.Field([F._Term(1.0, t.mono)])))
        out += [(f.kind, F.Field([F._Term(1.0, (0, 0), [f])])) for f in t.factors]
    return out


def test_saturation_predicates_and_what_the_shortcut_rests_on(lib):
    """Where a factor's sat_* predicate holds, its full fj_* jet is exactly 0 or 1 (sigmoids)
    or exactly 0 (Gaussians) with every derivative exactly +-0 -- the claim the generated
    whole-field return {value, 0, 0, 0} rests on -- and NaN derivatives at a radial centre
    inside the inner band."""
    sharp = Z.ZOO["sharp"]
    regions = Z.sharp_regions()
    assert len(regions) == 10 and all(len(p) >= 32 for p in regions.values())
    pts = Z.points_for("sharp")
    factors = _single_factor_fields(sharp)
    nf = len(factors)
    sat = run(lib, [sharp], pts, 3, nf)
    with_predicate = [j for j in range(nf) if factors[j][0] not in (F.FK_IND_DISK, F.FK_IND_BOX, F.FK_MONO)]
    assert len(with_predicate) == 4 and np.all(sat[:, [j for j in range(nf) if j not in with_predicate]] == -1)
    # the numpy predicate that selects the regions (and the walks' positions on the device)
    mine = Z.factor_saturation(sharp, pts)
    assert [n for n, _ in mine] == ["sat_sigmoid_radial", "sat_sigmoid_lin", "sat_exp_quad_diag", "sat_exp_quad"]
    centre = np.all(pts == np.float32(Z.SHARP_C1), axis=1)
    assert centre.sum() == 1
    for (name, state), j in zip(mine, with_predicate):
        holds = (sat[:, j].astype(int) & 1) == 1
        np.testing.assert_array_equal(holds, state != 0, err_msg=name)
        assert holds.sum() >= 64 and (~holds).sum() >= 32, name
        kind, alone = factors[j]
        full = jet(lib, alone, pts)
        at_centre = holds & centre if kind == F.FK_SIGMOID_RADIAL else np.zeros(len(pts), bool)
        if kind == F.FK_SIGMOID_RADIAL:
            assert at_centre.sum() == 1 and sat[at_centre, j] == 3 and np.all(sat[~centre, j] < 2)
            assert full[at_centre, 0] == 1 and np.all(np.isnan(full[at_centre, 1:]))
        h = holds & ~at_centre
        want = np.where(state[h] > 0, 1.0, 0.0).astype(np.float32)
        np.testing.assert_array_equal(full[h, 0], want, err_msg=name)
        np.testing.assert_array_equal(full[h, 1:], np.zeros((h.sum(), 3), np.float32), err_msg=name)
        if kind == F.FK_EXP_QUAD:
            assert np.all(state <= 0)
        # the band is a band: some unsaturated point has a derivative that is not zero
        assert np.any(full[~holds, 1:] != 0), name
    whole = Z.field_saturated(sharp, pts)
    assert whole.sum() >= 6 * 32 and (~whole).sum() >= 4 * 32
    # the whole field where it is saturated: the derivatives of the full jet are exactly zero
    full = jet(lib, sharp, pts)
    np.testing.assert_array_equal(full[whole & ~centre, 1:], np.zeros(((whole & ~centre).sum(), 3), np.float32))
    # ... and its value the bits of field_value, which the generated return takes in its place
    np.testing.assert_array_equal(_bits(full[whole, 0]), _bits(run(lib, [sharp], pts, 0, 1)[whole, 0]))


@pytest.mark.parametrize("name", list(Z.SIGMA_BAR))
def test_oracle_self_agreement_is_what_the_floors_assume(name):
    """The share of the zoo problem's walks that the oracle keeps under a 1-ulp change of the
    step directions is the recorded one (to 1e-4: one walk of 8192 is 1.2e-4), from which
    tests/test_gpu_field_zoo.py takes the device's floor."""
    share = Z.oracle_self_agreement(name)
    print(f"{name}: {share:.5f} (recorded {Z.SELF_AGREEMENT[name]:.5f}, floor {Z.floor(name):.5f})")
    assert share >= Z.SELF_AGREEMENT[name] - 1e-4
    assert Z.floor(name) >= 0.95


# ---- the generated text ----------------------------------------------------------------------
def _call(kind, p, pre):
    if kind == F.FK_EXP_QUAD:
        diag = all(np.float32(v) == 0 for v in p[4:8])
        return re.escape(pre + ("exp_quad_diag(" if diag else "exp_quad(")) + r"[^;]*?\)"
    return re.escape(pre + KIND_NAME[kind] + "(") + r"[^;]*?\)"


def _term_patterns(field, jet_form):
    """One regular expression per term, in term order: the per-kind calls in the order
    field_jet / field_value makes them."""
    terms, factors = field.pack()
    out = []
    for coef, first, n in terms:
        fs = factors[first:first + n]
        if jet_form:
            if n == 0:
                out.append(r"acc = wost::jet_add\(acc, wost::jet_const\([^;]*\)\);")
                continue
            s = r"\{ wost::Jet t = wost::jet_scale\([^,;]*, " + _call(*fs[0], "wost::fj_") + r"\);"
            for f in fs[1:]:
                s += r" t = wost::jet_mul\(t, " + _call(*f, "wost::fj_") + r"\);"
            out.append(s + r" acc = wost::jet_add\(acc, t\); \}")
        else:
            s = r"\{ float t = [^;]*;"
            for f in fs:
                s += r" t = t \* " + _call(*f, "wost::fv_") + ";"
            out.append(s + r" acc = acc \+ t; \}")
    return out


def _body(src, head):
    i = src.index(head)
    return src[i:src.index("\n    }\n", i)]     # (the member function's own closing brace)


def _zoo_source(name, **kw):
    from dcrmontecarlo_amd.geometry import PolyLinesSimple
    from dcrmontecarlo_amd.solvers.WoStSolver import kernel_source

    b = Z.BOX
    sq = np.array([[-b, -b], [b, -b], [b, b], [-b, b], [-b, -b]], np.float32)
    return kernel_source(PolyLinesSimple(sq), Z.ZOO[name], None, source=Z.ZOO[name], sigma=Z.POSITIVE[name],
                         alpha=Z.POSITIVE[name], sigma_bar=1.0, **kw)


@pytest.mark.parametrize("name", list(Z.ZOO))
def test_generated_text_calls_the_kinds_in_the_interpreters_order(name):
    src = _zoo_source(name)
    bodies = {"g": (_body(src, "float g(float x, float y"), Z.ZOO[name], False),
              "alpha": (_body(src, "float alpha(float x, float y"), Z.POSITIVE[name], False)}
    jet_head = "wost::Jet alpha_jet(float x, float y" + (", bool& flat)" if "bool& flat" in src else ")")
    bodies["alpha_jet"] = (_body(src, jet_head), Z.POSITIVE[name], True)
    for what, (body, field, jet_form) in bodies.items():
        pos = 0
        pats = _term_patterns(field, jet_form)
        assert len(pats) == len(field.terms)
        for k, pat in enumerate(pats):
            m = re.compile(pat).search(body, pos)
            assert m is not None, f"{name}.{what}: term {k} not found in order:\n{pat}\n{body}"
            pos = m.end()
        n_acc = body.count("acc = acc + t;") if not jet_form else body.count("wost::jet_add(acc")
        assert n_acc == len(pats), f"{name}.{what}: {n_acc} accumulations for {len(pats)} terms"


def test_sharp_alpha_carries_the_four_predicates():
    src = _zoo_source("sharp")
    for pred in ("sat_sigmoid_radial", "sat_sigmoid_lin", "sat_exp_quad_diag", "sat_exp_quad"):
        assert f"wost::{pred}(x, y, " in src, pred
    assert "if (WOST_SAT_ALL(sat))" in src
    # no other zoo alpha has a predicate for every factor
    for name in Z.ZOO:
        if name not in ("sharp", "sigmoid_lin", "sigmoid_radial_neg", "sigmoid_radial_pos", "exp_general",
                        "exp_general_det0", "exp_diag", "exp_linear"):
            assert "WOST_SAT_ALL(sat)" not in _zoo_source(name), name
