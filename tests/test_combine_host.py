"""Weighted channel combinations on the host (csrc/wost_combine.h, wost_combine.cpp).

wost_combine_blocks_host restates wost_block_combine op for op: walk i's combination l is
v = 0.0, then for c ascending v = v + w[l][c] * (double)val[i][c] with product and sum rounded
separately and a zero weight skipped; thread t of 256 takes walks lo + t, lo + t + 256, ... of
a block (s += v, q = fma(v, v, q): the device's `q += v * v` is one v_fma_f64), and a halving
tree 256 -> 128 -> ... -> 1 adds the threads' partial sums. Here that order is written out in
numpy and must give the same bits. The fused multiply-add is math.fma where Python has it,
else exact rational arithmetic rounded once.
"""
import ctypes
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from dcrmontecarlo_amd import _lib
from dcrmontecarlo_amd import survey
from dcrmontecarlo_amd import wavenumber as wn
from dcrmontecarlo_amd.solvers.WoStSolver import run_to_tolerance, tolerance_rule, tolerance_schedule

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "dcrmontecarlo_amd", "csrc")
B = 4096
# a full block, a 904-walk block, a block shorter than 256 walks, a 1-walk block
BEGIN = np.array([0, 4096, 5000, 5100, 5101], np.int64)


def combine_host(values, begin, weights):
    """wost_combine_blocks_host: rows [blocks, 2L] of values [walks, C] under weights [L, C]."""
    values = np.ascontiguousarray(values, np.float32)
    begin = np.ascontiguousarray(begin, np.int64)
    w = np.ascontiguousarray(weights, np.float64)
    out = np.zeros((len(begin) - 1, 2 * w.shape[0]), np.float64)
    rc = _lib.lib.wost_combine_blocks_host(_lib.fptr(values), begin.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                           len(begin) - 1, values.shape[1], _lib.dptr(w), w.shape[0], _lib.dptr(out))
    _lib.check(rc, "wost_combine_blocks_host")
    return out


def _fma(a, b, c):
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))   # (one rounding: Fraction -> float is exact-rounded)


def numpy_rows(values, begin, weights):
    """The order written out: per-walk combinations with separately rounded ops, the 16
    strided passes of the 256 threads, then the halving tree."""
    x = np.asarray(values, np.float32).astype(np.float64)
    L, C = weights.shape
    out = np.zeros((len(begin) - 1, 2 * L))
    for b in range(len(begin) - 1):
        lo, hi = int(begin[b]), int(begin[b + 1])
        for l in range(L):
            v = np.zeros(hi - lo)
            for c in range(C):
                if weights[l, c] != 0.0:
                    p = weights[l, c] * x[lo:hi, c]   # rounded
                    v = v + p                         # rounded
            s, q = np.zeros(256), np.zeros(256)
            for r in range(-(-(hi - lo) // 256)):     # (16 passes of a full block)
                part = v[r * 256:(r + 1) * 256]
                s[:len(part)] = s[:len(part)] + part
                q[:len(part)] = [_fma(float(a), float(a), float(c)) for a, c in zip(part, q[:len(part)])]
            h = 128
            while h > 0:
                s[:h] = s[:h] + s[h:2 * h]
                q[:h] = q[:h] + q[h:2 * h]
                h //= 2
            out[b, 2 * l], out[b, 2 * l + 1] = s[0], q[0]
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("L", [1, 3, 16])
@pytest.mark.parametrize("C", [1, 6, 15, 16])
def test_host_rows_are_the_numpy_restatement_bit_for_bit(C, L):
    rng = np.random.default_rng(100 * C + L)
    vals = (rng.standard_normal((int(BEGIN[-1]), C)) * 10.0 ** rng.integers(-3, 4, size=C)).astype(np.float32)
    w = rng.standard_normal((L, C))
    w[rng.random((L, C)) < 0.3] = 0.0   # some sparse entries
    got = combine_host(vals, BEGIN, w)
    np.testing.assert_array_equal(_bits(got), _bits(numpy_rows(vals, BEGIN, w)))


def test_unit_rows_give_the_plain_channel_sums():
    rng = np.random.default_rng(7)
    C = 6
    vals = rng.standard_normal((int(BEGIN[-1]), C)).astype(np.float32)
    got = combine_host(vals, BEGIN, np.eye(C))
    for c in range(C):
        one = combine_host(vals[:, c:c + 1], BEGIN, np.ones((1, 1)))
        np.testing.assert_array_equal(_bits(got[:, 2 * c:2 * c + 2]), _bits(one))
        # ... which are the ordinary reduce's: double sums of the float values in that order
        np.testing.assert_array_equal(_bits(one), _bits(numpy_rows(vals[:, c:c + 1], BEGIN, np.ones((1, 1)))))
    # a 1-walk block: the value and its square
    np.testing.assert_array_equal(got[3, 0::2], vals[5100].astype(np.float64))
    np.testing.assert_array_equal(got[3, 1::2], vals[5100].astype(np.float64) ** 2)


def test_a_zero_weight_skips_a_non_finite_value():
    vals = np.array([[1.0, np.nan, np.inf], [2.0, np.inf, np.nan], [4.0, -np.inf, 3.0]], np.float32)
    w = np.array([[1.0, 0.0, 0.0], [0.5, 0.0, -0.0], [0.0, 1.0, 0.0]])
    got = combine_host(vals, np.array([0, 3], np.int64), w)
    np.testing.assert_array_equal(got[0, :4], [7.0, 21.0, 3.5, 5.25])
    assert not np.isfinite(got[0, 4])   # (the row that does weigh the bad channel sees it)


def test_refusals():
    vals = np.zeros((4, 2), np.float32)
    begin = np.array([0, 4], np.int64)
    out = np.zeros(64)
    f, bp = _lib.fptr(vals), begin.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    good = np.ones((1, 2))
    call = lambda w, L, C=2: _lib.lib.wost_combine_blocks_host(f, bp, 1, C, None if w is None else _lib.dptr(w), L,
                                                             _lib.dptr(out))
    assert call(good, 1) == _lib.WOST_OK
    assert call(good, 0) == _lib.WOST_ERR_INVALID_ARG
    assert call(np.ones((17, 2)), _lib.WOST_MAX_SOURCES + 1) == _lib.WOST_ERR_INVALID_ARG
    assert call(None, 1) == _lib.WOST_ERR_INVALID_ARG
    for bad in (np.nan, np.inf, -np.inf):
        assert call(np.array([[1.0, bad]]), 1) == _lib.WOST_ERR_INVALID_ARG
        assert b"not finite" in _lib.lib.wost_last_error()
    assert call(good, 1, C=0) == _lib.WOST_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        combine_host(vals, begin, np.array([[np.nan, 1.0]]))


def test_transform_weights():
    np.testing.assert_array_equal(wn.transform_weights([0.5, -2.0, 3.0], 2),
                                  [[0.5, 0.0, -2.0, 0.0, 3.0, 0.0], [0.0, 0.5, 0.0, -2.0, 0.0, 3.0]])
    np.testing.assert_array_equal(wn.transform_weights([1.5, 2.5]), [[1.5, 2.5]])
    assert wn.transform_weights(np.arange(8.0), 2).shape == (2, 16)
    with pytest.raises(ValueError):
        wn.transform_weights([], 1)


def test_difference_weights():
    np.testing.assert_array_equal(survey.difference_weights(3), [[-1, 1, 0], [-1, 0, 1]])
    # M = 2, K = 1, S = 2: channels (m, s) = 00 01 10 11
    np.testing.assert_array_equal(survey.difference_weights(2, 1, 2), [[-1, 0, 1, 0], [0, -1, 0, 1]])
    # M = 3, K = 2, S = 1: channel m * 2 + j
    np.testing.assert_array_equal(survey.difference_weights(3, 2, 1),
                                  [[-1, 0, 1, 0, 0, 0], [0, -1, 0, 1, 0, 0], [-1, 0, 0, 0, 1, 0], [0, -1, 0, 0, 0, 1]])
    assert survey.difference_weights(2, 2, 3).shape == (6, 12)
    with pytest.raises(ValueError):
        survey.difference_weights(1)


def test_the_tolerance_rule_acts_on_combined_rows():
    """run_to_tolerance with rounds that return combined rows [ids, blocks, 2L+1]: channel 0 is
    accurate, channel 1 small and noisy (a high wavenumber); the rule on the combination
    w0 v0 + w1 v1 stops where the rule on the channels never does."""
    rng = np.random.default_rng(3)
    N, W, C = 3, 4 * B + 100, 2
    vals = np.empty((N, W, C), np.float32)
    vals[:, :, 0] = 1.0 + 0.5 * rng.standard_normal((N, W))
    vals[:, :, 1] = 1e-3 * rng.standard_normal((N, W)) * (1 + 50 * (rng.random((N, W)) < 0.01))
    vals[2, :, 0] = 0.01 + 3.0 * rng.standard_normal(W)   # a point that converges late or never
    w = np.array([[1.0, 0.7]])
    steps = rng.integers(1, 50, size=(N, W)).astype(np.float64)

    def rows(weights, ids, w0, w1):
        begin = np.array(list(range(0, w1 - w0, B)) + [w1 - w0], np.int64)
        out = np.zeros((len(ids), len(begin) - 1, 2 * weights.shape[0] + 1))
        for r, p in enumerate(ids):
            out[r, :, :-1] = combine_host(vals[p, w0:w1], begin, weights)
            out[r, :, -1] = [steps[p, w0 + a:w0 + b].sum() for a, b in zip(begin[:-1], begin[1:])]
        return out

    calls = []

    def run_round(ids, w0, w1):
        calls.append((ids.tolist(), w0, w1))
        return rows(w, ids, w0, w1)

    rel = 0.01
    sums, walks, conv, rounds = run_to_tolerance(run_round, N, 1, rel_tol=rel, min_walks=B, max_walks=W)
    assert sums.shape == (N, 3) and rounds == len(calls)
    assert conv[0] and conv[1] and len(set(walks.tolist())) >= 2 and walks[2] == W
    assert all(b in tolerance_schedule(B, W) for b in walks)
    for p in range(N):   # a prefix of the full range's rows, added in block order
        full = rows(w, [p], 0, int(walks[p]))[0]
        acc = np.zeros(3)
        for k in range(full.shape[0]):
            acc = acc + full[k]
        np.testing.assert_array_equal(sums[p], acc)
    mean, se, ok = tolerance_rule(sums, walks, rel, 0.0)
    np.testing.assert_array_equal(ok, conv)
    assert mean.shape == (1, N)
    for p in range(2):   # the combination's mean: the per-walk weighted sums'
        want = (vals[p, :int(walks[p])].astype(np.float64) @ w[0]).mean()
        assert abs(mean[0, p] - want) <= 1e-12 * abs(want)
    # the channels themselves (unit rows): channel 1 never meets the relative tolerance
    s2, w2, c2, _ = run_to_tolerance(lambda ids, a, b: rows(np.eye(2), ids, a, b), N, 2, rel_tol=rel, min_walks=B,
                                     max_walks=W)
    assert s2.shape == (N, 5) and not c2.any() and np.all(w2 == W)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_native_check_under_sanitizers(tmp_path):
    """tests/native/combine_check.cpp: a stand-alone program around wost_combine.cpp, built with
    the address and undefined-behaviour sanitizers and run directly."""
    exe = str(tmp_path / "combine_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "native", "combine_check.cpp"),
                    os.path.join(CSRC, "wost_combine.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "combine_check: 0 failed checks" in r.stdout
