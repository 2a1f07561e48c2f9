"""A handle keeps the one field-specialised kernel it looked up last, keyed by the kernel's
variant (dcrmontecarlo_amd/csrc/wost_variant.h KernelVariant) and the program's version. A
wrong hit there would run a solve on another variant's kernel, so one handle goes through
solves that need different variants -- the trig choice, the walk recorder, two sources -- and
back, and every result must be, bit for bit, that of a fresh handle configured that way from
the start."""
import numpy as np
import pytest

from dcrmontecarlo_amd import _lib
from dcrmontecarlo_amd.fields import X, Y
from dcrmontecarlo_amd.geometry import PolyLinesSimple
from dcrmontecarlo_amd.solvers import WostSolver_2D

pytestmark = pytest.mark.gpu

W, MAX_STEPS, EPS, SEED = 256, 200, 1e-3, 7
PTS = np.array([[0.5, 0.5], [0.25, 0.75], [0.8, 0.9], [0.1, 0.2]], np.float32)
SOURCES = [1.0 + X * Y, 2.0 - X]


def _solver():
    """The unit square: Dirichlet on three sides (g = x), one Neumann segment on top, a source."""
    D = PolyLinesSimple(np.array([[0, 1], [0, 0], [1, 0], [1, 1]], np.float32))
    N = PolyLinesSimple(np.array([[1, 1], [0, 1]], np.float32))
    return WostSolver_2D(D, X, N, source=SOURCES[0])


def _plain(s):
    v, k = s.solve_walks(PTS, nWalks=W, maxSteps=MAX_STEPS, eps=EPS, seed=SEED)
    assert s.last_timing["jit"] == 1
    return v, k


def _history(s):
    n = len(PTS)
    sums = np.zeros((n, 3), np.float64)
    v = np.empty(n * W, np.float32)
    k = np.empty(n * W, np.uint32)
    rec = np.empty((n * W, MAX_STEPS + 1, _lib.REC_FLOATS), np.float32)
    _lib.check(_lib.lib.wost_solve_history(s._h, _lib.fptr(PTS), n, W, MAX_STEPS, EPS, SEED, _lib.dptr(sums),
                                           _lib.fptr(v), _lib.u32ptr(k), _lib.fptr(rec)), "wost_solve_history")
    assert s.timing()["jit"] == 1
    # what the recorder writes: every field of a walk's step records, and of its end record
    # (index steps) the point, the boundary term and the total (wost_walk.h RecField)
    idx = np.arange(MAX_STEPS + 1)[None, :, None]
    end_fields = np.isin(np.arange(_lib.REC_FLOATS), [0, 1, 6, 7])[None, None, :]
    written = (idx < k[:, None, None]) | ((idx == k[:, None, None]) & end_fields)
    return v, k, np.where(written, rec, np.float32(0))


def _two_sources(s):
    v, k = s.solve_sources_walks(PTS, SOURCES, nWalks=W, maxSteps=MAX_STEPS, eps=EPS, seed=SEED)
    assert s.last_timing["jit"] == 1
    return v, k


def _same(a, b):
    return len(a) == len(b) and all(
        x.shape == y.shape and x.dtype == y.dtype and np.array_equal(np.ascontiguousarray(x).view(np.uint32),
                                                                     np.ascontiguousarray(y).view(np.uint32))
        for x, y in zip(a, b))


def test_one_handle_through_several_variants(gpu_available):
    s = _solver()
    plain = _plain(s)
    assert _same(plain, _plain(_solver()))

    def fresh_fast():
        f = _solver()
        f.set_trig("fast")
        return f

    s.set_trig("fast")
    assert _same(_plain(s), _plain(fresh_fast()))

    assert _same(_history(s), _history(fresh_fast()))
    assert _same(_plain(s), plain)   # (one Neumann segment: "auto" chooses the fast directions too)

    assert _same(_two_sources(s), _two_sources(fresh_fast()))
    assert _same(_plain(s), plain)   # the single-source kernel again
