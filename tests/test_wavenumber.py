"""2.5-D wavenumber batching, the parts that need no device: the inverse transform's
quadrature against scipy's K0, the point-electrode geometric factors on the exact
half-space potential, the C ABI's new entry points, and the generated multi-wavenumber
kernels, which must name their NK and compile for gfx950 (wost_jit_compile)."""
import ctypes
import math

import numpy as np
import pytest

from dcrmontecarlo_amd import _lib
from dcrmontecarlo_amd import scenarios as S


def test_quadrature_k0_identity():
    """r * sum_j w_j K0(k_j r) = 1 on [r_min, r_max]: n = 8 wavenumbers at r_max / r_min =
    100 reach 1.1e-3; the bound leaves 9x room."""
    from scipy.special import k0

    from dcrmontecarlo_amd.wavenumber import wavenumber_quadrature

    k, w = wavenumber_quadrature(1.0, 100.0, 8)
    assert k.shape == (8,) and w.shape == (8,)
    np.testing.assert_allclose(k[0], 0.1 / 100.0, rtol=1e-12)
    np.testing.assert_allclose(k[-1], 4.0 / 1.0, rtol=1e-12)
    np.testing.assert_allclose(np.diff(np.log(k)), np.log(k[1] / k[0]), rtol=1e-9)   # log-spaced
    r = np.geomspace(1.0, 100.0, 1013)
    err = np.abs(r * (k0(np.outer(r, k)) @ w) - 1.0)
    print("max relative error", err.max(), "smallest weight", w.min())
    assert err.max() <= 1e-2


def test_bessel_k0_matches_scipy():
    from scipy.special import k0

    from dcrmontecarlo_amd.wavenumber import bessel_k0

    x = np.geomspace(1e-4, 60.0, 4000)
    assert np.max(np.abs(bessel_k0(x) - k0(x)) / k0(x)) < 1e-6


def test_geometric_factors_on_the_half_space():
    """rho_a = K dV / I reproduces rho on the exact potential rho I / (2 pi r)."""
    from dcrmontecarlo_amd import wavenumber as WN

    rho, cur = 37.5, 2.0
    V = lambda r: WN.halfspace_potential(rho, cur, r)
    for a in (0.5, 3.0):
        # Wenner A M N B at 0, a, 2a, 3a; A +I, B -I; dV = V_M - V_N
        vm = V(a) - V(2 * a)
        vn = V(2 * a) - V(a)
        assert math.isclose(WN.wenner_geometric_factor(a) * (vm - vn) / cur, rho, rel_tol=1e-12)
        for n in (1, 2, 5):
            # dipole-dipole A B M N at 0, a, (n+1) a, (n+2) a; dV = V_N - V_M
            vm = V((n + 1) * a) - V(n * a)
            vn = V((n + 2) * a) - V((n + 1) * a)
            assert math.isclose(WN.dipole_dipole_geometric_factor(a, n) * (vn - vm) / cur, rho, rel_tol=1e-12)


def test_new_entry_points_are_declared_and_exported():
    names = _lib.declared_symbols()
    for n in ("wost_set_wavenumbers", "wost_num_channels", "wost_kernel_source_channels"):
        assert n in names
        assert hasattr(_lib.lib, n), f"libwost.so does not export {n}"
    assert _lib.lib.wost_version() == 6   # additive: the ABI version stays


def _compiles(src: str):
    n, used = ctypes.c_int64(), ctypes.c_int32(-1)
    rc = _lib.lib.wost_jit_compile(src.encode(), b"gfx950", 0, None, 0, ctypes.byref(n), ctypes.byref(used))
    assert rc == 0, _lib.lib.wost_last_error().decode()
    assert n.value > 1000


def test_multi_wavenumber_kernels_name_their_nk_and_compile():
    vc = S.variable_coefficients()
    src = vc.kernel_source(n_wavenumbers=3)
    assert "#define WOST_WAVENUMBERS 1" in src
    assert "walk_body<true, true, true, false, false, 1, false, false, 3>" in src
    _compiles(src)
    dd = S.dcr_dipole()
    src2 = dd.kernel_source(sources=[dd.f, 2.0 * dd.f], n_wavenumbers=2)
    assert "walk_body<true, true, true, false, false, 2, false, false, 2>" in src2
    assert "f_multi" in src2
    _compiles(src2)
    # without wavenumbers the kernel is the one the handle always ran: no k2 read
    plain = dd.kernel_source()
    assert "WOST_WAVENUMBERS" not in plain and plain == dd.kernel_source(n_wavenumbers=0)


def test_kernel_source_channels_checks_its_arguments():
    with pytest.raises(ValueError):                       # 17 channels
        S.variable_coefficients().kernel_source(n_wavenumbers=17)
    dd = S.dcr_dipole()
    with pytest.raises(ValueError):                       # 9 sources x 2 wavenumbers
        dd.kernel_source(sources=[dd.f] * 9, n_wavenumbers=2)
    with pytest.raises(NotImplementedError, match="constant alpha"):   # no delta tracking
        S.poisson_square().kernel_source(n_wavenumbers=2)


def test_wavenumber_groups_split_low_from_high():
    from dcrmontecarlo_amd.wavenumber import wavenumber_groups

    k = np.array([4.0, 0.1, 1.0, 0.3])
    g = wavenumber_groups(k, 2)
    assert [sorted(k[i]) for i in g] == [[0.1, 0.3], [1.0, 4.0]]
    assert len(wavenumber_groups(k, 1)) == 1 and len(wavenumber_groups(k, 9)) == 4
