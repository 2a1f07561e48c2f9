"""The walk's sigma' shortcut at a flat alpha jet (wost_device.h flat_alpha_min, option
flat_sigma_prime): a kernel whose sigma is the constant 0 skips sigma_prime_from on the
wave-steps where every colliding lane's jet is the whole-field saturated {alpha, 0, 0, 0}
with alpha at or above the bound, because the collision weight 1 - sigma'/sigma_bar is then
1.0f bit for bit. Host checks: the arithmetic over the floats (a host build of the header),
and which generated kernels carry the shortcut."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
MARK = "#define WOST_FLAT_SIGMA_PRIME 1"
CALL = "flat = wost::flat_lane(z);"


def test_flat_weight_is_one_bit_for_bit(tmp_path):
    out = str(tmp_path / "libflat_sigma_check.so")
    # host build of the __host__ __device__ header; every operation rounded on its own (the
    # check forms the fused variants itself)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950",
                    "-ffp-contract=off", "-pthread", "-I" + os.path.join(REPO, "include"), "-x", "hip",
                    os.path.join(HERE, "native", "flat_sigma_check.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    c = (ctypes.c_long * 5)()
    assert lib.flat_sigma_check(c) == 0
    bad, alphas, evals, pred_bad, pred_n = list(c)
    print(f"alphas {alphas}, evaluations {evals}, mismatches {bad}; predicate checks {pred_n}, wrong {pred_bad}")
    # per 1/sigma_bar: at least the two whole binades above the bound's own, ulp by ulp
    assert alphas >= 6 * 2 * (1 << 23)
    assert evals == 13 * alphas
    assert pred_n >= 6 * 14 + 3 + 5 * 5
    assert pred_bad == 0
    assert bad == 0


def _dcr():
    from dcrmontecarlo_amd import scenarios as S

    return S.dcr_dipole(n_electrodes=4, n_walks=1)


def test_sigma_free_kernels_carry_the_shortcut():
    from dcrmontecarlo_amd import scenarios as S

    for sc in (_dcr(), S.notebook_dcr(), S.wenner_topography(n_electrodes=8, n_walks=1)):
        src = sc.kernel_source()
        assert MARK in src and CALL in src, sc.name
        assert "alpha_jet(float x, float y, bool& flat)" in src
        assert src.index(MARK) < src.index('#include "wost_walk.h"')
    fixed = _dcr().kernel_source(compat="fixed")
    assert MARK in fixed and CALL in fixed
    from dcrmontecarlo_amd import fields as F

    multi = _dcr().kernel_source(sources=[S.dcr_source_geophysical(), 2.0 * F.gaussian((0.0, -5.0), 0.5)])
    assert MARK in multi and "f_multi" in multi


def test_other_kernels_do_not():
    from dcrmontecarlo_amd import scenarios as S

    c3 = S.variable_coefficients().kernel_source()          # sigma != 0, alpha detached
    assert MARK not in c3 and CALL not in c3 and "bool& flat" not in c3
    nk = _dcr().kernel_source(n_wavenumbers=2)              # sc reads k2[j]
    assert "#define WOST_WAVENUMBERS 1" in nk
    assert MARK not in nk and CALL not in nk
    nm = _dcr().kernel_source(models=[(None, S.dcr_alpha_geophysical()), (None, S.dcr_alpha_geophysical(1.01))])
    assert "alpha_jet_multi" in nm
    assert MARK not in nm and CALL not in nm
    c2 = S.poisson_square().kernel_source()                 # no delta tracking
    assert MARK not in c2 and CALL not in c2


def test_option_zero_generates_the_kernel_without_it():
    sc = _dcr()
    off = sc.kernel_source(options={"flat_sigma_prime": 0})
    on = sc.kernel_source(options={"flat_sigma_prime": 1})
    assert on == sc.kernel_source()
    assert MARK not in off and CALL not in off and "bool& flat" not in off
    # the rest of the source is the same text: the jet's body is emitted once, with the flag
    head = "    __device__ __forceinline__ wost::Jet alpha_jet(float x, float y"
    wrapper = head + ") const {\n        bool flat;\n        return alpha_jet(x, y, flat);\n    }\n"
    assert on.count(wrapper) == 1 and on.count("wost::sat_sigmoid_radial(x, y, ") == 2
    stripped = (on.replace(MARK + "\n", "").replace(wrapper, "")
                .replace(head + ", bool& flat) const {\n        flat = false;\n", head + ") const {\n")
                .replace("                flat = wost::flat_lane(z);\n", ""))
    assert stripped == off


def test_option_is_a_product_option_with_default_one():
    import pytest

    from dcrmontecarlo_amd import _lib

    assert _lib.options_report() == {"build": "product", "non_default": {}}
    with pytest.raises(ValueError):
        _dcr().kernel_source(options={"flat_sigma_prime": 2})
    with pytest.raises(ValueError):
        _dcr().kernel_source(options={"no_such_option": 1})
