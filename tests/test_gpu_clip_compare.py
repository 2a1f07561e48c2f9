"""The source sample's clip test decided by the ratio a2/b2 (wost_device.h norm_greater)
leaves every walk as it was: small solves' per-walk values and step counts are compared
bit for bit with tests/golden/clip_compare_parent.npz, recorded on an MI355X from the
build of the commit before the change (SHA-256 of each array's bytes, and the first 64
walks in clear for diagnosis). A walk's result depends only on its id and the seed.

The cases cover the kernels that share the clip lines of walk_body: the specialised
kernel in reference mode with and without delta tracking's sigma, the tree kernel,
compat="fixed" delta tracking with a Neumann side, and the precompiled kernel.

Recording (on the GPU, with WOST_LIB pointing at the other build's libwost.so):
    python tests/test_gpu_clip_compare.py tests/golden/clip_compare_parent.npz
"""
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "clip_compare_parent.npz")
HEAD = 64
CASES = ["dcr_dipole", "variable_coefficients", "notebook_dcr", "wenner_topography", "fixed_mixed_delta",
         "dcr_dipole_precompiled"]


def _run(case):
    """(values float32 [N, W], steps uint32 [N, W], last_timing) of one case."""
    from dcrmontecarlo_amd import scenarios as S

    if case == "fixed_mixed_delta":
        if HERE not in sys.path:
            sys.path.insert(0, HERE)
        import test_gpu_fixed as TF

        u, alpha, sigma, f, pts, _ = TF._mixed_problem()
        s = TF._solver(TF.UNIT_U, u, TF.UNIT_TOP, f=f, sigma=sigma, alpha=alpha, compat="fixed")
        s.set_option("jit_race", 0)
        v, st = s.solve_walks(pts[:4], nWalks=2048, maxSteps=4000, eps=1e-4, seed=23)
        return v, st, s.last_timing
    name, pick, W, seed = {
        "dcr_dipole": ("dcr_dipole", lambda p: p[20:24], 4096, 7),
        "dcr_dipole_precompiled": ("dcr_dipole", lambda p: p[20:24], 4096, 7),
        "variable_coefficients": ("variable_coefficients", lambda p: p[:8], 2048, 8),
        "notebook_dcr": ("notebook_dcr", lambda p: p[::5][:4], 2048, 9),
        "wenner_topography": ("wenner_topography", lambda p: p[32::64][:4], 512, 10),
    }[case]
    sc = S.ALL[name]()
    s = sc.solver(device=0)
    s.set_option("jit_race", 0)
    if case == "dcr_dipole_precompiled":
        s.set_jit(False)
    v, st = s.solve_walks(pick(sc.points), nWalks=W, maxSteps=sc.max_steps, eps=sc.eps, seed=seed)
    return v, st, s.last_timing


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def record(path):
    out = {}
    for case in CASES:
        v, st, t = _run(case)
        out[case + "_shape"] = np.array(v.shape, np.int64)
        out[case + "_v_sha"], out[case + "_s_sha"] = _sha(v), _sha(st)
        out[case + "_v_head"] = v.ravel()[:HEAD].view(np.uint32).copy()
        out[case + "_s_head"] = st.ravel()[:HEAD].copy()
        print(case, v.shape, "jit", t["jit"], "tree", t["tree"], "mean steps", float(st.mean()))
    np.savez(path, **out)


@pytest.mark.parametrize("case", CASES)
def test_walks_equal_the_parent_builds(gpu_available, case):
    fx = np.load(FIXTURE, allow_pickle=False)
    v, st, t = _run(case)
    assert t["jit"] == (0 if case == "dcr_dipole_precompiled" else 1)
    assert t["tree"] == (1 if case == "wenner_topography" else 0)
    assert list(v.shape) == list(fx[case + "_shape"]) and v.dtype == np.float32 and st.dtype == np.uint32
    # the first walks in clear first: a difference then shows which walks and by how much
    np.testing.assert_array_equal(st.ravel()[:HEAD], fx[case + "_s_head"])
    np.testing.assert_array_equal(v.ravel()[:HEAD].view(np.uint32), fx[case + "_v_head"])
    assert bytes(_sha(st)) == bytes(fx[case + "_s_sha"]), "step counts differ from the parent build's"
    assert bytes(_sha(v)) == bytes(fx[case + "_v_sha"]), "walk values differ from the parent build's"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    record(sys.argv[1])
