"""Channel batching without ctypes or a device: which channels each launch scores, and the
statistics of the rows the launches return.

A walk scores C = models x wavenumbers x sources channels, at most ``cap`` (WOST_MAX_SOURCES)
per launch. A request of M x K x S channels is a box; ``plan_launches`` tiles it with
launches, in the order WostSolver_2D's runner (``_run_plan``) walks them: source runs
outermost -- a run stays installed on the handle for every launch under it --, then model
chunks, then wavenumber chunks. The chunk sizes are the models' (``_model_chunks``: the fewest
launches) or the sources' (``source_chunks``: whole source runs, then as many wavenumbers as
fit), and point sources bring their own runs (``point_source_chunks``: the charge cap splits
them too)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class SolveStats:
    """Per-point Monte-Carlo statistics of one solve."""

    mean: np.ndarray        # [N] float64: sum / nWalks
    stderr: np.ndarray      # [N] float64: sample std / sqrt(nWalks)
    mean_steps: np.ndarray  # [N] float64
    walks: int              # walks per point
    total_steps: int
    kernel_ms: float        # walk-kernel time (HIP events)
    total_ms: float         # device time of the whole solve


def stats_from_sums(sums: np.ndarray, n_walks: int, total_steps=None, kernel_ms=0.0, total_ms=0.0) -> SolveStats:
    s, q, st = sums[:, 0], sums[:, 1], sums[:, 2]
    mean = s / n_walks
    var = np.maximum(q / n_walks - mean * mean, 0.0) * (n_walks / max(n_walks - 1, 1))
    return SolveStats(mean=mean, stderr=np.sqrt(var / n_walks), mean_steps=st / n_walks, walks=n_walks,
                      total_steps=int(st.sum()) if total_steps is None else int(total_steps),
                      kernel_ms=float(kernel_ms), total_ms=float(total_ms))


def _stats_of_multi(sums: np.ndarray, n_walks: int):
    """SolveStats of each source from [N, 2S+1] wost_solve_multi rows."""
    S = (sums.shape[1] - 1) // 2
    return [stats_from_sums(np.stack([sums[:, 2 * k], sums[:, 2 * k + 1], sums[:, -1]], axis=1), n_walks)
            for k in range(S)]


def stats_of_channels(rows_list, n_walks: int, total_steps=None, kernel_ms=0.0, total_ms=0.0) -> SolveStats:
    """One SolveStats of all the channels of ``rows_list``, point rows [N, 2C+1] of one launch
    each: mean and stderr are [sum of C, N] in launch and channel order, ``mean_steps`` is the
    first launch's (every launch walks the same paths), and so is ``total_steps`` unless given."""
    stats = [st for rows in rows_list for st in _stats_of_multi(rows, int(n_walks))]
    return SolveStats(mean=np.stack([st.mean for st in stats]), stderr=np.stack([st.stderr for st in stats]),
                      mean_steps=stats[0].mean_steps, walks=int(n_walks),
                      total_steps=stats[0].total_steps if total_steps is None else int(total_steps),
                      kernel_ms=float(kernel_ms), total_ms=float(total_ms))


@dataclass(frozen=True)
class Launch:
    """The channels one launch scores: half-open slices of the model, wavenumber and source
    axes; ``charges``: the charge lists of its sources when they are point sources."""

    m: tuple
    k: tuple
    s: tuple
    charges: tuple | None = None

    @property
    def shape(self) -> tuple:
        return self.m[1] - self.m[0], self.k[1] - self.k[0], self.s[1] - self.s[0]

    @property
    def channels(self) -> int:
        dm, dk, ds = self.shape
        return dm * dk * ds


def _model_chunks(M: int, S: int, K: int, cap: int):
    """(models, sources, wavenumbers) per launch of solve_models for M x S x K channels at
    most ``cap`` per launch: the split with the fewest launches -- every launch walks the
    paths once -- and among those the one that keeps the most models together (then sources),
    so that a model and its background share a walk set whenever that saves one."""
    best = None
    for m in range(1, min(M, cap) + 1):
        for s in range(1, min(S, cap // m) + 1):
            k = min(K, cap // (m * s))
            launches = -(-M // m) * -(-S // s) * -(-K // k)
            key = (launches, -m, -s)
            if best is None or key < best[0]:
                best = (key, (m, s, k))
    return best[1]


def source_chunks(S: int, cap: int):
    """(models, sources, wavenumbers) per launch of solve_sources and solve_wavenumbers: runs
    of up to ``cap`` sources, each with as many wavenumbers as then fit."""
    s = min(S, cap)
    return 1, s, max(1, cap // s)


def charge_lists(sources) -> list:
    """The ``(position, strength)`` list of each point source (a list, or an object with
    ``.charges``: survey.point_electrode / point_dipole)."""
    return [list(getattr(s, "charges", s)) for s in sources]


def point_source_chunks(lists, s_max: int, charge_cap: int) -> list:
    """Runs of the point sources ``lists`` (a charge list each) that fit one launch: at most
    ``charge_cap`` charges and ``s_max`` sources."""
    s_max = max(1, s_max)
    chunks, cur, cnt = [], [], 0
    for lst in lists:
        if len(lst) > charge_cap:
            raise ValueError(f"a point source of {len(lst)} charges exceeds {charge_cap} per launch")
        if cur and (cnt + len(lst) > charge_cap or len(cur) >= s_max):
            chunks.append(cur)
            cur, cnt = [], 0
        cur.append(lst)
        cnt += len(lst)
    if cur:
        chunks.append(cur)
    return chunks


def plan_launches(M: int, K: int, S: int, cap: int, point_runs=None, chunks=None) -> list:
    """The launches of M models x K wavenumbers x S sources, in order. ``chunks``: the
    (models, sources, wavenumbers) per launch, by default ``_model_chunks``'. ``point_runs``
    (point_source_chunks, S sources in all): the source runs are these instead, each with the
    wavenumbers that fit beside it."""
    if point_runs is None:
        m_chunk, s_chunk, k_chunk = chunks or _model_chunks(M, S, K, cap)
        runs = [((s0, min(S, s0 + s_chunk)), None) for s0 in range(0, S, s_chunk)]
    else:   # (several models do not combine with point sources: M == 1)
        m_chunk, ends = 1, np.cumsum([len(r) for r in point_runs]).tolist()
        runs = [((s1 - len(r), s1), tuple(r)) for r, s1 in zip(point_runs, ends)]
    plan = []
    for s, charges in runs:
        if charges is not None:
            k_chunk = max(1, cap // (s[1] - s[0]))
        for m0 in range(0, M, m_chunk):
            for k0 in range(0, K, k_chunk):
                plan.append(Launch((m0, min(M, m0 + m_chunk)), (k0, min(K, k0 + k_chunk)), s, charges))
    return plan
