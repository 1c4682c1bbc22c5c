"""gsplat_hip.knn (csrc/knn.hip) against the float64 brute-force oracle of
tests/knn_cases.py: indices exactly, distances to one float32 rounding step,
two calls bit for bit; and Trainer(init="sfm", init_knn="hip") against the
host search."""

import numpy as np
import pytest
import torch

import knn_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 2.0 ** -23


def _check(got_d, got_i, d2, idx):
    assert got_i.dtype == torch.int64 and got_d.dtype == torch.float32
    np.testing.assert_array_equal(got_i.cpu().numpy(), idx)
    np.testing.assert_allclose(got_d.cpu().numpy(), np.sqrt(d2).astype(np.float32), rtol=RTOL,
                               atol=0)


CASES = [(c, n, k) for c in C.CLOUDS for n in C.NS for k in C.KS if k <= n]
# the clouds as the sizes they are named for: 9 x 9 x 9, and 1,000 + 8
CASES += [("lattice", 729, k) for k in C.KS] + [("cluster", 1008, k) for k in C.KS]


@pytest.mark.parametrize("name,N,k", CASES)
def test_knn_matches_the_oracle(name, N, k):
    """Both search paths are reached.  LDS-staged: `identical`, where every
    lane sits in cell 0 of level 0, so the union of the blocks is 2 x 2 x 2
    cells; and the outliers of `cluster`, which climb to level 20, one cell.
    Direct: `uniform` at N = 4099, k = 1, where every lane starts at level 0
    (its own cell holds itself) and the finest cells of 256 random points span
    far more than the 512 cells looked up cooperatively."""
    import gsplat_hip
    p = torch.from_numpy(C.cloud(name, N)).to(DEV)
    d2, idx = C.self_oracle(name, N)
    d, i = gsplat_hip.knn(p, k)
    assert d.shape == i.shape == (N, k)
    _check(d, i, d2[:, :k], idx[:, :k])
    d_again, i_again = gsplat_hip.knn(p, k, validate=False)
    assert torch.equal(i, i_again) and torch.equal(d.view(torch.int32), d_again.view(torch.int32))


@pytest.mark.parametrize("M", [1, 65, 300])
@pytest.mark.parametrize("name,k", [("uniform", 4), ("uniform", 32), ("lattice", 5)])
def test_separate_queries(name, k, M):
    """Queries inside the points' box, outside it on every side (their cells
    are clamped to the border) and equal to some points, in turn."""
    import gsplat_hip
    pts = C.cloud(name, 4099)
    g = np.random.default_rng(M)
    lo, hi = pts.min(0), pts.max(0)
    inside = lo + g.random((M, 3)) * (hi - lo)
    # every axis pushed past one face or the other
    outside = np.where(g.random((M, 3)) < 0.5, lo - g.random((M, 3)), hi + g.random((M, 3)))
    equal = pts[g.integers(0, len(pts), M)]
    q = np.stack([inside, outside, equal], 1).reshape(-1, 3)[:M].astype(np.float32)
    d2, idx = C.oracle(pts, q, k)
    d, i = gsplat_hip.knn(torch.from_numpy(pts).to(DEV), k, queries=torch.from_numpy(q).to(DEV))
    _check(d, i, d2, idx)
    only_d = gsplat_hip.knn(torch.from_numpy(pts).to(DEV), k, torch.from_numpy(q).to(DEV),
                            return_indices=False)
    assert torch.equal(only_d, d)


def test_trainer_sfm_init_on_the_device():
    """scales: both sides start from float64 distances and differ by the
    float32 rounding of the distances and of a logarithm of magnitude below 16
    (one ulp there is 9.5e-7).  Everything else does not depend on the search."""
    from gsplat_hip.train_step import Trainer
    g = torch.Generator().manual_seed(3)
    pts = torch.from_numpy(C.cloud("uniform", 4099).copy()) * 4.0
    rgbs = torch.rand(4099, 3, generator=g)
    vm, K = torch.eye(4)[None], torch.tensor([[[40.0, 0, 16], [0, 40.0, 16], [0, 0, 1]]])
    tr = {m: Trainer(pts, rgbs, vm, K, 32, 32, device=DEV, init="sfm", init_knn=m)
          for m in ("host", "hip")}
    for name, want in tr["host"].params.items():
        got, want = tr["hip"].params[name].detach(), want.detach()
        if name == "scales":
            assert float((got - want).abs().max()) <= 2e-6
        else:
            assert torch.equal(got, want), name
