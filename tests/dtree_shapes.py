"""Polylines and query points shared by tests/test_dirichlet_tree.py (host) and
tests/test_gpu_dirichlet_tree.py (device). float32 arrays [n, 2]."""
import numpy as np


def ngon(nv, r=1.0, centre=(0.0, 0.0)):
    """Closed regular polygon with nv vertices (the last repeats the first), as
    tests/test_gpu_long_polylines.py builds its circle."""
    t = np.linspace(0.0, 2.0 * np.pi, nv, dtype=np.float64)
    p = np.stack([centre[0] + r * np.cos(t), centre[1] + r * np.sin(t)], axis=1).astype(np.float32)
    p[-1] = p[0]
    return p


def zigzag(nv=257):
    x = np.linspace(-2.0, 3.0, nv)
    y = np.where(np.arange(nv) % 2 == 0, 0.0, 0.37) + 0.05 * x
    return np.stack([x, y], axis=1).astype(np.float32)


def sine(nseg=1000):
    """Open polyline sampled from a function, like the reference's funcToPolyline."""
    x = np.linspace(0.0, 10.0, nseg + 1)
    return np.stack([x, 0.8 * np.sin(1.7 * x) + 0.1 * x], axis=1).astype(np.float32)


def resample(corners, nseg):
    """The closed or open polyline through `corners`, its sides cut into nseg equal parts in all
    (nseg a multiple of the side count), corner to corner."""
    corners = np.asarray(corners, np.float64)
    sides = len(corners) - 1
    assert nseg % sides == 0
    k = nseg // sides
    out = [corners[:1]]
    for a, b in zip(corners[:-1], corners[1:]):
        t = np.arange(1, k + 1)[:, None] / k
        out.append(a + t * (b - a))
    p = np.concatenate(out).astype(np.float32)
    p[-1] = corners[-1]
    return p


def thin_rectangle(nseg=2048):
    """100:1 rectangle: boxes that prune badly."""
    return resample([[0, 0], [100, 0], [100, 1], [0, 1], [0, 0]], nseg)


def random_polylines(n=60, seed=20):
    rng = np.random.default_rng(seed)
    return [(0.1 + 15.9 * rng.random((int(rng.integers(5, 401)), 2))).astype(np.float32) for _ in range(n)]


def ulp_neighbours(p):
    """p and the points one ulp either side of it in each coordinate."""
    inf = np.float32(np.inf)
    return np.concatenate([p, np.nextafter(p, -inf), np.nextafter(p, inf)])


def query_points(verts, rng, n_uniform=10_000):
    """The host fuzz's query points for one polyline."""
    v = verts.astype(np.float32)
    mid = ((v[:-1].astype(np.float64) + v[1:]) * 0.5).astype(np.float32)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    c, half = 0.5 * (lo + hi), (hi - lo)            # twice the bounding box
    uni = c + (rng.random((n_uniform, 2)) * 2.0 - 1.0) * half
    # points 1e-7 and 1e6 from the boundary: off segment midpoints along the normal
    i = rng.integers(0, len(v) - 1, 256)
    u = v[i + 1].astype(np.float64) - v[i]
    nrm = np.stack([-u[:, 1], u[:, 0]], 1) / np.maximum(np.hypot(u[:, 0], u[:, 1]), 1e-30)[:, None]
    near = np.concatenate([mid[i] + s * 1e-7 * nrm for s in (1, -1)])
    far = np.concatenate([mid[i] + s * 1e6 * nrm for s in (1, -1)])
    nan, inf = np.nan, np.inf
    odd = np.array([[nan, 0.0], [0.0, nan], [nan, nan], [inf, 0.0], [0.0, -inf], [inf, inf], [-inf, inf],
                    [3e38, -3e38], [1e30, 1e30], [2.0**61, 0.0]])
    centre = v[:-1].astype(np.float64).mean(0, keepdims=True)   # an n-gon's centre: every segment ties
    pts = np.concatenate([v, ulp_neighbours(mid), centre, np.array([[0.0, 0.0]]), uni, near, far, odd])
    return np.ascontiguousarray(pts, np.float32)
