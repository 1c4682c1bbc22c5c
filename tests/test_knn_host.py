"""gsplat_hip.knn without a GPU: the refusals, the CPU path against the float64
brute-force oracle of tests/knn_cases.py, and the `init_knn` switch's host
side."""

import numpy as np
import pytest
import torch

import knn_cases as C


@pytest.mark.parametrize("bad,error", [
    (lambda: (torch.zeros(5, 2), 1), ValueError),
    (lambda: (torch.zeros(5, 3, 1), 1), ValueError),
    (lambda: (torch.zeros(5, 3, dtype=torch.float64), 1), ValueError),
    (lambda: (torch.zeros(5, 3), 0), ValueError),
    (lambda: (torch.zeros(40, 3), 33), ValueError),
    (lambda: (torch.zeros(5, 3), 6), ValueError),
    (lambda: (torch.tensor([[0.0, 1.0, float("nan")]] * 4), 1), ValueError),
    (lambda: (torch.tensor([[0.0, float("inf"), 1.0]] * 4), 1), ValueError),
    (lambda: (torch.zeros(5, 3, requires_grad=True), 1), NotImplementedError),
])
def test_refusals(bad, error):
    import gsplat_hip
    assert "knn" in gsplat_hip.__all__
    points, k = bad()
    with pytest.raises(error, match="knn"):
        gsplat_hip.knn(points, k)


def test_queries_are_checked_like_the_points():
    import gsplat_hip
    p = torch.rand(8, 3)
    for q in (torch.zeros(2, 4), torch.zeros(2, 3, dtype=torch.float16),
              torch.tensor([[0.0, float("nan"), 0.0]])):
        with pytest.raises(ValueError, match="queries|non-finite"):
            gsplat_hip.knn(p, 2, queries=q)
    with pytest.raises(NotImplementedError, match="queries"):
        gsplat_hip.knn(p, 2, queries=torch.zeros(2, 3, requires_grad=True))
    assert gsplat_hip.knn(p, 2, queries=torch.zeros(0, 3))[1].shape == (0, 2)


@pytest.mark.parametrize("name,N", [("lattice", 729), ("cluster", 1008)])
@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("tree", [True, False])
def test_cpu_path_matches_the_oracle(name, N, k, tree, monkeypatch):
    import gsplat_hip
    import sys
    knn_mod = sys.modules["gsplat_hip.knn"]  # (the package's `knn` is the function)
    if not tree:  # what a machine without scipy runs
        def no_scipy(*a):
            raise ImportError("scipy")
        monkeypatch.setattr(knn_mod, "_host_tree", no_scipy)
    p = C.cloud(name, N)
    d2, idx = C.self_oracle(name, N)
    d, i = gsplat_hip.knn(torch.from_numpy(p.copy()), k)
    np.testing.assert_array_equal(i.numpy(), idx[:, :k])
    np.testing.assert_allclose(d.numpy(), np.sqrt(d2[:, :k]).astype(np.float32), rtol=2.0 ** -23,
                               atol=0)
    q = torch.from_numpy(p[::7] + np.float32(0.125))
    d2q, idxq = C.oracle(p, q.numpy(), k)
    assert np.array_equal(gsplat_hip.knn(torch.from_numpy(p.copy()), k, queries=q)[1].numpy(), idxq)


def test_knn_log_scales_host_is_unchanged():
    from scipy.spatial import cKDTree
    from gsplat_hip.train_step import knn_log_scales
    points = torch.from_numpy(C.cloud("uniform", 4099).copy())
    pts = points.double().numpy()
    d, _ = cKDTree(pts).query(pts, k=4, workers=-1)
    want = torch.log(torch.sqrt(torch.from_numpy((d[:, 1:] ** 2).mean(-1)).float()) * 0.5)
    want = want.unsqueeze(-1).repeat(1, 3)
    assert torch.equal(knn_log_scales(points, 0.5), want)
    assert torch.equal(knn_log_scales(points, 0.5, backend="host"), want)
    # the same formula over the CPU path of knn
    assert float((knn_log_scales(points, 0.5, backend="hip") - want).abs().max()) <= 2e-6
    with pytest.raises(ValueError, match="backend"):
        knn_log_scales(points, backend="tree")


def test_trainer_refuses_the_device_search_on_a_cpu_device():
    from gsplat_hip.train_step import Trainer
    pts = torch.from_numpy(C.cloud("uniform", 63).copy())
    with pytest.raises(NotImplementedError, match="init_knn='hip'"):
        Trainer(pts, pts, torch.eye(4)[None], torch.eye(3)[None], 8, 8, device="cpu", init="sfm",
                init_knn="hip")
    with pytest.raises(ValueError, match="init_knn"):
        Trainer(pts, pts, torch.eye(4)[None], torch.eye(3)[None], 8, 8, device="cpu",
                init_knn="tree")
