"""Green's function maps: the grid of a tally solve, the library's cell rule
and fixed-point conversion on the host, and the result of WostSolver_2D.solve_greens_map.

A tally solve adds, for every step of every walk from a query point x, the weight that the
source sample y would multiply f(y) by to the grid cell of y -- as integers, so that the sums
do not depend on the launch shape or the order in which the deposits arrive. The sums of one
point, times the quantum and divided by the walks, are the integrals of G(x, .) over the cells.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import _lib


class TallyGrid(NamedTuple):
    """nx x ny cells from the lower left corner (x0, y0), widths (dx, dy): wost_tally_grid.
    The values are taken as float32; the edges are :func:`tally_edges`."""
    x0: float
    y0: float
    dx: float
    dy: float
    nx: int
    ny: int


def as_grid(grid) -> TallyGrid:
    g = TallyGrid(**grid) if isinstance(grid, dict) else TallyGrid(*grid)
    return TallyGrid(float(np.float32(g.x0)), float(np.float32(g.y0)), float(np.float32(g.dx)), float(np.float32(g.dy)),
                     int(g.nx), int(g.ny))


def _c_grid(grid) -> _lib.WostTallyGrid:
    g = as_grid(grid)
    return _lib.WostTallyGrid(g.x0, g.y0, g.dx, g.dy, g.nx, g.ny)


def tally_edges(grid):
    """The float32 cell edges (x edges [nx + 1], y edges [ny + 1]) of a grid: e_i = fl(fl(i *
    d) + origin), two roundings -- the numbers the kernels compare a sample against. Cell i is
    the half-open interval [e_i, e_{i+1})."""
    g = as_grid(grid)
    ex = np.arange(g.nx + 1, dtype=np.float32) * np.float32(g.dx) + np.float32(g.x0)
    ey = np.arange(g.ny + 1, dtype=np.float32) * np.float32(g.dy) + np.float32(g.y0)
    return ex.astype(np.float32), ey.astype(np.float32)


def tally_cell(grid, points) -> np.ndarray:
    """wost_tally_cell: the bin of each point [N, 2] as the kernels find it, iy * nx + ix, or
    nx * ny for the outside bin (outside every cell, or NaN). ValueError for a grid the
    library does not accept (include/wost.h)."""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 2))
    out = np.empty(p.shape[0], np.int32)
    cg = _c_grid(grid)
    _lib.check(_lib.lib.wost_tally_cell(ctypes.byref(cg), _lib.fptr(p), p.shape[0],
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "tally_cell")
    return out


def tally_quantize(d, scale_log2: int, limit: int):
    """wost_tally_quantize: (q int64, ok bool) of the deposits d (float32): q =
    round-to-nearest-even(d * 2^scale_log2), ok = |q| < limit (q = 0 where not)."""
    d = np.ascontiguousarray(np.asarray(d, np.float32).ravel())
    q = np.empty(d.shape[0], np.int64)
    ok = np.empty(d.shape[0], np.uint8)
    _lib.check(_lib.lib.wost_tally_quantize(_lib.fptr(d), d.shape[0], int(scale_log2), int(limit),
                                            q.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                            ok.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "tally_quantize")
    return q, ok.astype(bool)


def tally_limit(nWalks: int, walk_begin: int, walk_end: int, replicas: int, maxSteps: int) -> int:
    """wost_tally_limit: the power of two a quantised deposit must stay below."""
    L = ctypes.c_int64(0)
    _lib.check(_lib.lib.wost_tally_limit(int(nWalks), int(walk_begin), int(walk_end), int(replicas), int(maxSteps),
                                         ctypes.byref(L)), "tally_limit")
    return int(L.value)


@dataclass
class GreensMap:
    """The tally of one solve_greens_map call over N points, R replica rows and a grid of
    ny x nx cells.

    sums      int64 [N, R, ny, nx]: the fixed-point deposits of each row's walks per cell
    outside   int64 [N, R]: ... of the samples outside the grid
    row_walks int64 [N, R]: the walks that went to each row
    quantum   the value of one unit of ``sums``
    grid      the TallyGrid
    u, stats  the ordinary result of the solve with the solver's own source: float32 [N, 1]
              and its SolveStats

    Rows merge by integer addition: ``a + b`` is the map of the two walk ranges together
    (same points, grid, quantum and replicas)."""
    sums: np.ndarray
    outside: np.ndarray
    row_walks: np.ndarray
    quantum: float
    grid: TallyGrid
    u: np.ndarray | None = None
    stats: object | None = None

    @property
    def cell_area(self) -> float:
        return float(self.grid.dx) * float(self.grid.dy)

    def _row_means(self) -> np.ndarray:
        """Each row's own estimate of the cell integrals of G, float64 [N, R, ny, nx] (NaN for
        a row without walks)."""
        w = self.row_walks.astype(np.float64)[:, :, None, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.sums.astype(np.float64) * self.quantum / w

    @property
    def mean(self) -> np.ndarray:
        """Cell averages of G(x_p, .), float64 [N, ny, nx]: sums * quantum / walks / cell area,
        the integer rows added first (exact)."""
        tot = self.sums.sum(axis=1, dtype=np.int64).astype(np.float64)
        walks = self.row_walks.sum(axis=1).astype(np.float64)[:, None, None]
        return tot * self.quantum / walks / self.cell_area

    @property
    def stderr(self) -> np.ndarray:
        """Standard error of ``mean`` by batch means over the replica rows, float64 [N, ny,
        nx]: the rows weighted by their walks; NaN for R = 1."""
        return _batch_stderr(self._row_means() / self.cell_area, self.row_walks)

    def potential(self, f_cells):
        """u(x_p) = sum over the cells of f_c * (integral of G over cell c), for a source that
        is the constant f_c on cell c (float [ny, nx]) and 0 outside the grid; the boundary
        term is not part of it. Returns (u [N], stderr [N]). The cells of one walk set are
        correlated, so the combination is formed per replica row first and the standard error
        taken over the rows' values (NaN for R = 1)."""
        f = np.asarray(f_cells, np.float64)
        if f.shape != self.sums.shape[2:]:
            raise ValueError(f"f_cells must have the grid's shape {self.sums.shape[2:]}, got {f.shape}")
        per_row = (self._row_means() * f[None, None]).sum(axis=(2, 3))   # [N, R]
        tot = (self.sums.astype(np.float64) * f[None, None]).sum(axis=(1, 2, 3)) * self.quantum
        u = tot / self.row_walks.sum(axis=1).astype(np.float64)
        return u, _batch_stderr(per_row[:, :, None, None], self.row_walks)[:, 0, 0]

    def __add__(self, other: "GreensMap") -> "GreensMap":
        if (self.grid != other.grid or self.quantum != other.quantum or self.sums.shape != other.sums.shape):
            raise ValueError("maps merge only with the same points, grid, quantum and replicas")
        return GreensMap(self.sums + other.sums, self.outside + other.outside, self.row_walks + other.row_walks,
                         self.quantum, self.grid)


def _batch_stderr(rows: np.ndarray, row_walks: np.ndarray) -> np.ndarray:
    """Batch-means standard error of the walk-weighted mean of rows [N, R, ...] with weights
    row_walks [N, R]: sqrt(sum_r w_r (m_r - m)^2 / ((R' - 1) sum_r w_r)) over the R' rows that
    have walks; NaN when R' < 2."""
    w = row_walks.astype(np.float64)[:, :, None, None]
    used = w > 0
    n_used = used.sum(axis=1)
    m = np.where(used, rows, 0.0)
    wsum = w.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (w * m).sum(axis=1) / wsum
        var = (w * np.where(used, (m - mean[:, None]) ** 2, 0.0)).sum(axis=1) / ((n_used - 1) * wsum)
    return np.where(n_used >= 2, np.sqrt(var), np.nan)
