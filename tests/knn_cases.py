"""Clouds and the float64 brute-force oracle shared by the k-NN tests."""

import functools

import numpy as np

NS = (1, 5, 63, 64, 65, 257, 4099)
KS = (1, 4, 5, 16, 32)
CLOUDS = ("uniform", "lattice", "cluster", "line", "plane", "identical")


@functools.lru_cache(maxsize=None)
def cloud(name, N):
    """float32 [N, 3].  lattice: N points of an integer lattice scaled by 0.25
    (the full 9 x 9 x 9 at N = 729): exact distance ties, points on cell planes.
    cluster: points within 1e-3 of the origin and up to 8 outliers at distance
    1e3 (1,000 + 8 at N = 1008).  line / plane: no extent on two axes / one."""
    g = np.random.default_rng(N * 7 + len(name))
    if name == "uniform":
        p = g.random((N, 3))
    elif name == "lattice":
        s = int(np.ceil(N ** (1 / 3) - 1e-9))
        p = np.stack(np.meshgrid(*[np.arange(s)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.25
        p = p[g.permutation(len(p))[:N]]
    elif name == "cluster":
        n_out = min(8, N // 2)
        d = g.standard_normal((n_out, 3))
        p = np.concatenate([(g.random((N - n_out, 3)) - 0.5) * 1e-3,
                            1e3 * d / np.linalg.norm(d, axis=1, keepdims=True)])
    elif name == "line":
        p = np.stack([g.random(N), np.full(N, 0.5), np.full(N, -2.0)], 1)
    elif name == "plane":
        p = np.concatenate([g.random((N, 2)), np.full((N, 1), 3.0)], 1)
    else:
        p = np.tile(np.float32([[0.3, -1.7, 2.5]]), (N, 1))
    return np.ascontiguousarray(p, dtype=np.float32)


def oracle(points, queries, k):
    """(d2 [M, k] float64, idx [M, k]): per query the k first points by
    (d2, index), d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float64.  A stable sort
    by d2 of columns in index order is np.lexsort((index, d2)) of every row."""
    p, q = points.astype(np.float64), queries.astype(np.float64)
    d2s, ids = [], []
    for b in range(0, len(q), 512):
        dx, dy, dz = (q[b:b + 512, None, a] - p[None, :, a] for a in range(3))
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        sel = np.argsort(d2, axis=1, kind="stable")[:, :k]
        d2s.append(np.take_along_axis(d2, sel, 1))
        ids.append(sel)
    return np.concatenate(d2s), np.concatenate(ids)


@functools.lru_cache(maxsize=None)
def self_oracle(name, N):
    """oracle(cloud, cloud, min(32, N)): the first k columns answer any k."""
    p = cloud(name, N)
    return oracle(p, p, min(32, N))
