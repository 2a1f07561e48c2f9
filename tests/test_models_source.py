"""Shared-path model batching, the parts that need no device: the generated
kernel sources -- with no model, or one, they are byte for byte the sources of today's
handles; with several they name their count and compile for gfx950 -- the new entry points,
their argument checks, and KernelVariant::n_models in the kernel cache's comparison."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from dcrmontecarlo_amd import _lib
from dcrmontecarlo_amd import fields as F
from dcrmontecarlo_amd import scenarios as S

HERE = os.path.dirname(os.path.abspath(__file__))
SB = 12.0   # (an explicit sigma_bar: a handle's stays its own whatever the models are)


def _scenario(name):
    return S.dcr_dipole(6) if name == "dcr_dipole" else S.variable_coefficients(6)


def _second_model(sc):
    """A model other than the scenario's own: (sigma, alpha)."""
    if sc.name == "dcr_dipole":
        return (None, F.const(100.0))
    return (0.5 + 0.25 * F.sin(S.X) * F.cos(S.Y), 0.8 + 0.4 * F.exp(-1.0 * (S.X**2 + S.Y**2)))


def _with_fields(sc, model):
    return S.Scenario(sc.name, sc.dirichlet, sc.neumann, g=sc.g, f=sc.f, sigma=model[0], alpha=model[1])


def _compiles(src: str):
    n, used = ctypes.c_int64(), ctypes.c_int32(-1)
    rc = _lib.lib.wost_jit_compile(src.encode(), b"gfx950", 0, None, 0, ctypes.byref(n), ctypes.byref(used))
    assert rc == 0, _lib.lib.wost_last_error().decode()
    assert n.value > 1000


def test_new_entry_points_are_declared_and_exported():
    names = _lib.declared_symbols()
    for n in ("wost_set_models", "wost_models_info", "wost_kernel_source_models"):
        assert n in names
        assert hasattr(_lib.lib, n), f"libwost.so does not export {n}"
    assert _lib.lib.wost_version() == 6   # additive: the ABI version stays
    assert ctypes.sizeof(_lib.WostModel) == 2 * ctypes.sizeof(ctypes.c_void_p)


@pytest.mark.parametrize("name", ["dcr_dipole", "variable_coefficients"])
def test_no_model_and_one_model_are_todays_sources(name):
    sc = _scenario(name)
    srcs = [sc.f, 2.0 * sc.f]
    for kw in ({}, {"n_wavenumbers": 2}, {"sources": srcs}, {"sources": srcs, "n_wavenumbers": 2}):
        plain = sc.kernel_source(sigma_bar=SB, **kw)
        assert sc.kernel_source(sigma_bar=SB, models=[], **kw) == plain
        # one model: the source of a problem that carries that model's fields
        other = _second_model(sc)
        one = sc.kernel_source(sigma_bar=SB, models=[other], **kw)
        assert one == _with_fields(sc, other).kernel_source(sigma_bar=SB, **kw)
        assert one != plain
        assert "models" not in one.splitlines()[[l.startswith("// generated") for l in one.splitlines()].index(True)]
        # ... and the scenario's own fields as the one model: the plain source again
        assert sc.kernel_source(sigma_bar=SB, models=[(sc.sigma, sc.alpha)], **kw) == plain


def _models(sc, m):
    if sc.name == "dcr_dipole":
        return [(None, sc.alpha), (None, F.const(100.0))] + [
            (None, S.dcr_alpha_geophysical(1.0 + 0.01 * k)) for k in range(1, m - 1)]
    a = sc.alpha
    return [(sc.sigma, a), _second_model(sc)] + [(sc.sigma * (1.0 + 0.01 * k), a) for k in range(1, m - 1)]


@pytest.mark.parametrize("m", [2, 4])
def test_multi_model_kernels_name_their_count_and_compile(m):
    sc = _scenario("dcr_dipole")
    src = sc.kernel_source(sigma_bar=SB, models=_models(sc, m))
    head = [l for l in src.splitlines() if l.startswith("// generated")][0]
    assert head.endswith(f"neumann+source+delta, {m} models")
    assert f"walk_body<true, true, true, false, false, 1, false, false, 1, 0, {m}>" in src
    assert f"point_alpha_multi_body<{m}>" in src
    for fn in ("alpha_multi", "alpha_jet_multi", "sigma_multi", "detached_multi", f"alpha_jet_m{m - 1}"):
        assert fn in src
    assert "WOST_WAVENUMBERS" not in src
    _compiles(src)


def test_two_models_with_sources_and_wavenumbers_compile():
    sc = _scenario("variable_coefficients")
    src = sc.kernel_source(sigma_bar=SB, models=_models(sc, 2), sources=[sc.f, 2.0 * sc.f], n_wavenumbers=2)
    assert "walk_body<true, true, true, false, false, 2, false, false, 2, 0, 2>" in src
    assert "#define WOST_WAVENUMBERS 1" in src and "f_multi" in src
    # one differentiable alpha and one detached one (Q9) in the same kernel
    assert "const bool d[2] = {true, false};" in src
    _compiles(src)


def test_two_models_compile_for_a_tree_variant():
    sc = S.wenner_topography(n_electrodes=4, n_walks=1, n_segments=200)
    src = sc.kernel_source(models=[(sc.sigma, sc.alpha), (sc.sigma, F.const(0.01))])
    head = [l for l in src.splitlines() if l.startswith("// generated")][0]
    assert "+tree" in head and head.endswith(", 2 models")
    _compiles(src)


def test_kernel_source_models_checks_its_arguments():
    dd = _scenario("dcr_dipole")
    with pytest.raises(ValueError, match="neither"):                  # both fields NULL
        dd.kernel_source(models=[(None, dd.alpha), (None, None)])
    with pytest.raises(ValueError, match="channels"):                 # 9 models x 2 sources
        dd.kernel_source(models=[(None, dd.alpha)] * 9, sources=[dd.f, dd.f])
    with pytest.raises(ValueError, match="channels"):                 # 3 x 3 x 2
        dd.kernel_source(models=[(None, dd.alpha)] * 3, sources=[dd.f, dd.f], n_wavenumbers=3)
    with pytest.raises(NotImplementedError, match="delta tracking"):  # no delta tracking
        S.poisson_square().kernel_source(models=[(None, F.const(2.0))])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_variants_that_differ_in_n_models_compare_unequal(tmp_path):
    """tests/native/variant_models_check.cpp, built stand-alone with the address and
    undefined-behaviour sanitizers when the compiler has them (host code only)."""
    src = os.path.join(HERE, "native", "variant_models_check.cpp")
    exe = str(tmp_path / "variant_models_check")
    san = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", src, "-o", exe])
    if san.returncode != 0:
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "variant_models_check: 0 failed checks" in r.stdout


def test_paired_difference_is_the_mean_and_stderr_of_per_walk_differences():
    from dcrmontecarlo_amd import survey

    rng = np.random.default_rng(3)
    common = rng.normal(size=(1, 4, 1000))                     # the shared part of the noise
    v = (common + np.array([0.0, 0.5, -0.25]).reshape(3, 1, 1) + 1e-3 * rng.normal(size=(3, 4, 1000))).astype(np.float32)
    mean, se = survey.paired_difference(v)
    assert mean.shape == se.shape == (3, 4)
    assert np.all(mean[0] == 0.0) and np.all(se[0] == 0.0)
    d = v.astype(np.float64)[1] - v.astype(np.float64)[0]
    np.testing.assert_allclose(mean[1], d.mean(axis=1), rtol=1e-12)
    np.testing.assert_allclose(se[1], d.std(axis=1, ddof=1) / np.sqrt(1000), rtol=1e-12)
    # the common noise cancels: far below the unpaired error of two independent solves
    unpaired = np.sqrt(2.0) * v.astype(np.float64)[0].std(axis=1, ddof=1) / np.sqrt(1000)
    assert np.all(se[1] < 0.01 * unpaired)
    with pytest.raises(ValueError):
        survey.paired_difference(v[0])


def test_model_chunks_keep_models_together_at_the_fewest_launches():
    from dcrmontecarlo_amd.solvers.WoStSolver import _model_chunks

    launches = lambda M, S, K: (lambda m, s, k: -(-M // m) * -(-S // s) * -(-K // k))(*_model_chunks(M, S, K, 16))
    assert _model_chunks(2, 1, 1, 16) == (2, 1, 1)
    assert _model_chunks(2, 8, 1, 16) == (2, 8, 1) and launches(2, 8, 1) == 1
    assert _model_chunks(2, 9, 1, 16) == (2, 8, 1) and launches(2, 9, 1) == 2      # the two separate solves' count
    assert _model_chunks(2, 47, 1, 16) == (2, 8, 1) and launches(2, 47, 1) == 6    # = 2 * ceil(47 / 16)
    assert _model_chunks(3, 2, 2, 16) == (3, 2, 2)
    assert _model_chunks(9, 2, 1, 16) == (9, 1, 1) and launches(9, 2, 1) == 2
    assert _model_chunks(20, 1, 1, 16)[0] <= 16 and launches(20, 1, 1) == 2
    for M in range(1, 20):
        for S in (1, 2, 5, 9, 17):
            for K in (1, 3, 8):
                m, s, k = _model_chunks(M, S, K, 16)
                assert 1 <= m * s * k <= 16 and launches(M, S, K) >= -(-(M * S * K) // 16)
