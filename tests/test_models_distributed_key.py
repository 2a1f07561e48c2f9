"""The agreement of a distributed solve with models. wost_solve_distributed
hands wost_distributed_run a key of ten values: wost_dist_solve_key's six, the point charges'
checksum in two 32-bit halves, and the models' checksum (wost_models_info) in two more. Here
that protocol runs on the host with two thread ranks and synthetic block rows: ranks whose
keys agree merge their sums, and ranks that differ only in one half of the models' checksum
-- key[8] or key[9] -- refuse on every rank."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dcrmontecarlo_amd import distributed as D  # noqa: E402

B = 4096
N, W, ROW = 3, 2 * B, 7          # three points, two blocks per point, C = 3 model channels


def _key(pts, models_checksum):
    k = np.zeros(10)
    k[:6] = D.solve_key(11, 1e-3, 200, pts)
    k[8] = float(models_checksum & 0xFFFFFFFF)
    k[9] = float(models_checksum >> 32)
    return k


def _run(checksums):
    from rank_threads import RankThreads

    rng = np.random.default_rng(2)
    pts = rng.uniform(-1, 1, size=(N, 2)).astype(np.float32)
    full = rng.integers(0, 1000, size=(N, W // B, ROW)).astype(np.float64)

    def shard(w0, w1):
        return full[:, w0 // B:-(-w1 // B)]

    R = len(checksums)
    res = RankThreads(R).run(lambda r, ar, ag: D.run_protocol(R, r, N, W, ROW, shard, ar, ag,
                                                              key=_key(pts, checksums[r])))
    return res, full.sum(axis=1)


def test_ranks_with_the_same_models_merge():
    chk = 0x9E3779B97F4A7C15
    res, want = _run([chk, chk])
    for r in res:
        assert not isinstance(r, Exception), r
        np.testing.assert_array_equal(r[0], want)


@pytest.mark.parametrize("other", [0x9E3779B97F4A7C15 ^ 1, 0x9E3779B97F4A7C15 ^ (1 << 40), 0])
def test_ranks_with_different_models_refuse_to_merge(other):
    """A difference in the low half (key[8]), in the high half (key[9]), and models on one
    rank only (checksum 0 on the other)."""
    res, _ = _run([0x9E3779B97F4A7C15, other])
    for r in res:
        assert isinstance(r, ValueError) and "disagree" in str(r), r
