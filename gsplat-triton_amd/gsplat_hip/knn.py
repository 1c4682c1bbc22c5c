"""Exact k-nearest neighbours of a 3-D point cloud, backed by libgsplat_hip.so
(csrc/knn.hip): the reference's `knn` (examples/utils.py:141-151, sklearn
NearestNeighbors), which sets every Gaussian's initial scale from its SfM
neighbours (examples/simple_trainer.py:221-224), as a device operation that
outlier removal, normals and density estimates can start from as well.

The order is defined exactly: row i holds the k points with the smallest
(d2, index), d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float64 on the float32
coordinates, the lower index first on a tie, and dists = float32(sqrt(d2)).
The device search, the CPU path and a brute-force float64 search therefore
agree index for index, and two calls give the same bits.

Points are data: there is no autograd.  On the device every launch goes on
torch's current stream; with validate=False the host reads nothing and the
call can be captured.  CPU tensors take a host path (a k-d tree for the
candidates when scipy imports, chunked brute force otherwise).
"""

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._wrapper import _aligned16, _ptr, _stream

MAX_K = 32


def _check(name, t):
    if not isinstance(t, Tensor) or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"knn: {name} [*, 3] expected, got "
                         f"{list(t.shape) if isinstance(t, Tensor) else type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"knn: {name} must be float32, got {t.dtype}")
    if t.requires_grad:
        raise NotImplementedError(f"knn: no autograd; {name} requires grad")


def _d2(q, p):
    """The rule's d2 of queries q [B,3] against points p [N,3] (float64)."""
    dx, dy, dz = (q[:, None, a] - p[None, :, a] for a in range(3))
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def _order(d2, ids, k):
    """The k first of every row by (d2, id): a stable sort of rows already in
    ascending id."""
    by_id = np.argsort(ids, axis=1, kind="stable")
    d2, ids = np.take_along_axis(d2, by_id, 1), np.take_along_axis(ids, by_id, 1)
    sel = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d2, sel, 1), np.take_along_axis(ids, sel, 1)


def _host_brute(p, q, k, chunk=1 << 22):
    N = p.shape[0]
    rows = max(1, chunk // N)
    d2o, ido = np.empty((len(q), k)), np.empty((len(q), k), dtype=np.int64)
    ids = np.arange(N, dtype=np.int64)[None]
    for b in range(0, len(q), rows):
        d2 = _d2(q[b:b + rows], p)
        d2o[b:b + rows], ido[b:b + rows] = _order(d2, np.broadcast_to(ids, d2.shape), k)
    return d2o, ido


def _host_tree(p, q, k):
    """k + 8 candidates per query from a k-d tree, ordered by the rule; a row
    is settled when its k-th d2 lies clearly below its last candidate's (the
    tree's own distances round differently), the others (ties beyond the
    candidates) go to the brute-force search."""
    from scipy.spatial import cKDTree
    N = p.shape[0]
    kc = min(N, k + 8)
    _, cand = cKDTree(p).query(q, k=kc, workers=-1)
    cand = cand.reshape(len(q), kc).astype(np.int64)
    pc = p[cand]
    dx, dy, dz = (q[:, None, a] - pc[:, :, a] for a in range(3))
    d2, ids = _order(((dx * dx) + (dy * dy)) + (dz * dz), cand, kc)
    if kc < N:
        open_rows = np.nonzero(~(d2[:, k - 1] < d2[:, -1] * (1.0 - 1e-12)))[0]
        if open_rows.size:
            d2[open_rows, :k], ids[open_rows, :k] = _host_brute(p, q[open_rows], k)
    return d2[:, :k], ids[:, :k]


def _host(points, queries, k):
    p = points.detach().double().numpy()
    q = p if queries is None else queries.detach().double().numpy()
    try:
        d2, ids = _host_tree(p, q, k)
    except ImportError:
        d2, ids = _host_brute(p, q, k)
    return torch.from_numpy(np.sqrt(d2)).float(), torch.from_numpy(np.ascontiguousarray(ids))


def knn(points: Tensor, k: int, queries: Tensor = None, return_indices: bool = True,
        validate: bool = True):
    """The k nearest of `points` [N, 3] float32 for every row of `queries`
    [M, 3] float32 (None: the points themselves, each among its own neighbours
    at distance 0): dists [M, k] float32 ascending and, with return_indices,
    idx [M, k] int64.  1 <= k <= min(32, N).  validate=True makes one host read
    and raises ValueError on a non-finite coordinate; validate=False reads
    nothing (non-finite input then gives unspecified neighbours with indices
    in range)."""
    _check("points", points)
    if queries is not None:
        _check("queries", queries)
        if queries.device != points.device:
            raise ValueError(f"knn: points on {points.device}, queries on {queries.device}")
    N, k = points.shape[0], int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"knn: k {k} outside [1, {MAX_K}]")
    if k > N:
        raise ValueError(f"knn: k {k} > N {N}")
    if validate:
        ok = torch.isfinite(points).all()
        if queries is not None:
            ok = ok & torch.isfinite(queries).all()
        if not bool(ok):  # the one host read
            raise ValueError("knn: non-finite coordinates")
    M = N if queries is None else queries.shape[0]
    if not points.is_cuda:
        if M > 0:
            dists, idx = _host(points, queries, k)
        else:
            dists, idx = torch.empty(0, k), torch.empty(0, k, dtype=torch.int64)
    else:
        p = _aligned16(points.contiguous())
        q = None if queries is None else _aligned16(queries.contiguous())
        dists = torch.empty(M, k, dtype=torch.float32, device=p.device)
        idx = torch.empty(M, k, dtype=torch.int64, device=p.device)
        if M > 0:
            nbytes = _lib.query("gsplat_hip_knn_workspace_bytes", N, 0 if q is None else M)
            if nbytes <= 0:
                raise ValueError(f"knn: N {N} / M {M} beyond 2^30")
            ws = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.float64, device=p.device)
            with torch.cuda.device(p.device):
                _lib.call("gsplat_hip_knn", N, _ptr(p), M, _ptr(q), k, _ptr(dists), _ptr(idx),
                          _ptr(ws), _stream())
    return (dists, idx) if return_indices else dists
