"""GPU: splat compression -- the HIP k-means kernels (csrc/compress.hip)
against the float64 oracles of compression_oracle.py, PngCompression end to end
on the device, and Trainer.evaluate_compressed.

Assignment bar: every point's chosen centroid is optimal to rounding,
d64[i, label_i] <= dmin64[i] * (1 + 1e-5) + 1e-6 (the fp32 sum of D <= 72
non-negative terms errs by about D * 2^-24 relative, on each of the two
distances compared).  Shapes: not multiples of a wave (64), a workgroup's
points (512), a centroid tile (128) or a centroid group (4), those sizes +- 1,
and every compiled row length (9, 24, 45 exact; 8, 16, 32, 48, 64, 72 padded).
File bars: those of test_compression_host.py (compression_oracle.half_step)."""

import json
import os

import numpy as np
import pytest
import torch

import compression_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def _data(N, K, D, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + N * 31 + K * 7 + D)
    return torch.randn(N, D, generator=g), torch.randn(K, D, generator=g)


def _check_assignment(x, c, labels, dist, rows=None):
    """labels / dist (numpy) of the points `rows` of x against the oracle."""
    xs = x if rows is None else x[rows]
    d64 = O.l1_distances(xs.numpy(), c.numpy())
    if rows is not None:
        labels, dist = labels[rows], dist[rows]
    assert labels.min() >= 0 and labels.max() < len(c)
    chosen = d64[np.arange(len(xs)), labels]
    bar = O.optimality_bar(d64.min(1))
    worst = float((chosen - d64.min(1)).max())
    print(f"N={len(xs)} K={len(c)} D={x.shape[1]}: worst excess over the optimum {worst:.3e}, "
          f"labels differing from argmin {int((labels != d64.argmin(1)).sum())}")
    assert (chosen <= bar).all()
    assert (np.abs(dist - chosen) <= O.optimality_bar(chosen) - chosen).all()


ASSIGN_SHAPES = [
    (1, 1, 9), (67, 5, 24), (1000, 257, 45), (4099, 1024, 45),
    # the kernel's own tile sizes +- 1: 512 points, 128-centroid tile, groups of 4, a wave
    (511, 127, 9), (512, 128, 24), (513, 129, 45), (63, 3, 45), (65, 4, 9), (1025, 255, 24),
    # the padded row lengths and their edges
    (130, 9, 1), (130, 9, 5), (130, 9, 8), (130, 9, 13), (130, 9, 16), (130, 9, 30),
    (130, 9, 32), (130, 9, 47), (130, 9, 48), (130, 9, 60), (130, 9, 64), (130, 9, 72),
]


@pytest.mark.parametrize("N,K,D", ASSIGN_SHAPES)
def test_assign_matches_the_oracle(N, K, D):
    from gsplat_hip import compression as C
    x, c = _data(N, K, D)
    dist = torch.full((N,), -1.0, device=DEV)
    labels = C.kmeans_assign(x.to(DEV), c.to(DEV), dist=dist)
    assert labels.dtype == torch.int32 and labels.shape == (N,)
    _check_assignment(x, c, labels.cpu().numpy(), dist.cpu().numpy())


def test_assign_tie_goes_to_the_lowest_index():
    from gsplat_hip import compression as C
    x, c = _data(700, 300, 45, seed=1)
    c[290] = c[17]     # a later tile holds the copy
    c[18] = c[17]      # the same group
    c[140] = c[3]
    # points that do choose the duplicated centroids: at them, and close by
    x[:50] = c[17] + 0.01 * x[:50]
    x[50:100] = c[3] + 0.01 * x[50:100]
    x[100], x[101] = c[17], c[3]
    labels = C.kmeans_assign(x.to(DEV), c.to(DEV)).cpu().numpy()
    assert not np.isin(labels, [290, 18, 140]).any()
    assert (labels[:50] == 17).all() and (labels[50:100] == 3).all()
    assert labels[100] == 17 and labels[101] == 3
    # exact ties everywhere: identical centroids
    same = c[:1].repeat(130, 1)
    assert (C.kmeans_assign(x.to(DEV), same.to(DEV)) == 0).all()


def test_changed_counter():
    from gsplat_hip import compression as C
    x, c = _data(1500, 40, 24, seed=2)
    xd, cd = x.to(DEV), c.to(DEV)
    truth = C.kmeans_assign(xd, cd)
    g = torch.Generator().manual_seed(5)
    prev = truth.clone()
    flip = torch.randperm(1500, generator=g)[:333].to(DEV)
    prev[flip] = (prev[flip] + 1) % 40
    counter = torch.full((1,), 12345, dtype=torch.int32, device=DEV)
    out = C.kmeans_assign(xd, cd, prev, n_changed=counter)
    assert out is prev and torch.equal(prev, truth)
    assert int(counter) == 333
    C.kmeans_assign(xd, cd, prev, n_changed=counter)
    assert int(counter) == 0
    fresh = torch.full((1500,), -1, dtype=torch.int32, device=DEV)
    C.kmeans_assign(xd, cd, fresh, n_changed=counter)
    assert int(counter) == 1500


def test_label_range_edge():
    """K = 65,536 (the last label is 65,535), N a little more, D = 9."""
    from gsplat_hip import compression as C
    N, K, D = 65573, 65536, 9
    x, c = _data(N, K, D, seed=3)
    dist = torch.empty(N, device=DEV)
    labels = C.kmeans_assign(x.to(DEV), c.to(DEV), dist=dist).cpu().numpy()
    assert labels.min() >= 0 and labels.max() <= 65535
    rows = np.random.default_rng(0).choice(N, 256, replace=False)
    _check_assignment(x, c, labels, dist.cpu().numpy(), rows=rows)
    # the centroids themselves as points: each is its own nearest, the last included
    own = C.kmeans_assign(c[-600:].contiguous().to(DEV), c.to(DEV)).cpu().numpy()
    assert np.array_equal(own, np.arange(K - 600, K))
    with pytest.raises(ValueError):
        C.kmeans_l1(x[:100].to(DEV), n_clusters=65537)


UPDATE_SHAPES = [(1, 1, 9), (67, 5, 24), (1000, 257, 45), (4099, 256, 45), (513, 2, 72),
                 (3000, 1000, 65), (300, 3, 1), ((1 << 20) + 3, 300, 9)]


@pytest.mark.parametrize("N,K,D", UPDATE_SHAPES)
def test_update_matches_the_oracle(N, K, D):
    from gsplat_hip import compression as C
    x, c = _data(N, K, D, seed=4)
    g = torch.Generator().manual_seed(N + K)
    labels = torch.randint(0, K, (N,), generator=g, dtype=torch.int32)
    if K > 4:  # some centroids without members, the first and the last among them
        empty = torch.tensor([0, K // 2, K - 1], dtype=torch.int32)
        labels[torch.isin(labels, empty)] = 1
    want, counts = O.update_means(x.numpy(), labels.numpy().astype(np.int64), c.numpy())
    xd, ld = x.to(DEV), labels.to(DEV)
    runs = []
    for _ in range(2):
        cd = c.to(DEV).clone()
        got_counts = C.kmeans_update(xd, ld, cd)
        runs.append((cd.cpu(), got_counts.cpu()))
    got, got_counts = runs[0]
    assert np.array_equal(got_counts.numpy(), counts)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-6, atol=0)
    has = torch.from_numpy(counts > 0)
    assert torch.equal(got[~has], c[~has])  # empty centroids keep their value, bit for bit
    if K > 4:
        assert (~has).sum() >= 3
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def _planted(seed=0):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-10, 10, (8, 9))
    while min(np.abs(a - b).sum() for i, a in enumerate(centres) for b in centres[:i]) < 20:
        centres = rng.uniform(-10, 10, (8, 9))
    member = rng.integers(0, 8, 2000)
    x = centres[member] + rng.normal(scale=0.05, size=(2000, 9))
    init = centres + rng.normal(scale=1.0, size=centres.shape)
    return (torch.from_numpy(x).float(), torch.from_numpy(init).float(), member)


def test_lloyd_loop_matches_the_oracle():
    from gsplat_hip import compression as C
    x, init, member = _planted()
    want_c, want_l, want_it = O.lloyd(x.numpy(), init.numpy(), 10, 1e-4)
    assert want_it < 10  # the oracle stops early at tol
    cents, labels, iters = C.lloyd(x.to(DEV), init.to(DEV).clone(), 10, 1e-4)
    assert iters == want_it
    assert np.array_equal(labels.cpu().numpy(), want_l)
    assert np.array_equal(want_l, member)  # and these are the planted clusters
    np.testing.assert_allclose(cents.cpu().numpy(), want_c, rtol=0, atol=1e-5)
    # max_iters cuts the loop short of that
    _, _, one = C.lloyd(x.to(DEV), init.to(DEV).clone(), 1, 1e-4)
    assert one == 1
    c2, l2 = C.kmeans_l1(x.to(DEV), 8, init=init.to(DEV))
    assert l2.dtype == torch.int64 and torch.equal(l2, labels.long()) and torch.equal(c2, cents)


def test_kmeans_l1_is_deterministic_and_seeded():
    from gsplat_hip import compression as C
    x, _ = _data(3000, 1, 24, seed=6)
    xd = x.to(DEV)
    a = C.kmeans_l1(xd, 100, seed=3)
    b = C.kmeans_l1(xd, 100, seed=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].shape == (100, 24) and a[1].shape == (3000,) and a[1].dtype == torch.int64
    # the initial centroids are the documented rows of x
    perm = torch.randperm(3000, generator=torch.Generator().manual_seed(3))[:100]
    c0, _ = C.kmeans_l1(xd, 100, max_iters=0, seed=3)
    assert torch.equal(c0.cpu(), x[perm])
    # K = min(n_clusters, N)
    few = C.kmeans_l1(xd[:40].contiguous(), 65536)
    assert few[0].shape == (40, 24) and torch.equal(few[1].sort().values.cpu(), torch.arange(40))
    from gsplat_hip import _lib
    with pytest.raises(_lib.GsplatHipError):
        C.kmeans_l1(x)


# ---------------------------------------------------------- PngCompression
def _splats(N, seed=0, device=DEV):
    g = torch.Generator().manual_seed(seed)
    sp = {"means": torch.randn(N, 3, generator=g) * 3, "scales": torch.randn(N, 3, generator=g),
          "quats": torch.randn(N, 4, generator=g), "opacities": torch.randn(N, generator=g),
          "sh0": torch.randn(N, 1, 3, generator=g) * 0.5,
          "shN": torch.randn(N, 15, 3, generator=g) * 0.1}
    return {k: v.to(device) for k, v in sp.items()}


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_png_compression_end_to_end(tmp_path):
    from gsplat_hip import PngCompression
    from gsplat_hip import compression as C
    sp = _splats(2030)  # n = 45: 5 Gaussians are dropped
    before = {k: v.clone() for k, v in sp.items()}
    comp = PngCompression(verbose=False, n_clusters=256)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    comp.compress(d1, sp)
    comp.compress(d2, sp)
    assert all(torch.equal(sp[k], before[k]) for k in sp) and list(sp) == list(before)
    f1, f2 = _files(d1), _files(d2)
    assert list(f1) == sorted(["means_l.png", "means_u.png", "scales.png", "quats.png",
                               "opacities.png", "sh0.png", "shN.npz", "meta.json"])
    assert f1 == f2  # byte-identical
    meta = json.load(open(os.path.join(d1, "meta.json")))
    assert list(meta) == list(sp) and meta["shN"]["quantization"] == 6
    out = comp.decompress(d1)
    assert all(v.shape[0] == 45 * 45 and v.dtype == torch.float32 for v in out.values())

    ordered = {k: v.cpu().numpy() for k, v in comp.prepare(sp).items()}
    raw = C.read_arrays(d1)
    for k, bits in (("means", 16), ("scales", 8), ("quats", 8), ("opacities", 8), ("sh0", 8)):
        bar = O.half_step(meta[k]["mins"], meta[k]["maxs"], bits)
        err = np.abs(raw[k].astype(np.float64) - ordered[k]).reshape(2025, -1)
        assert (err <= bar).all(), (k, err.max(0), bar)
    # shN: each row is the dequantised centroid of its label, and the label is
    # an optimal one for the stored centroids' originals
    cents, labels = C.kmeans_l1(torch.from_numpy(ordered["shN"]).reshape(2025, 45).to(DEV), 256)
    with np.load(os.path.join(d1, "shN.npz")) as z:
        assert np.array_equal(z["labels"], labels.cpu().numpy())
        assert z["centroids"].shape == (256, 45)
    bar = O.half_step(meta["shN"]["mins"], meta["shN"]["maxs"], 6)
    err = np.abs(raw["shN"].reshape(2025, 45) - cents.cpu().numpy()[labels.cpu().numpy()])
    assert (err <= bar).all()
    # the means came back through the inverse log transform
    torch.testing.assert_close(out["means"],
                               C.inverse_log_transform(torch.from_numpy(raw["means"])))


def test_use_sort_false_keeps_the_order(tmp_path):
    from gsplat_hip import PngCompression
    sp = _splats(1024, seed=1)  # square: nothing dropped
    d = str(tmp_path / "c")
    PngCompression(use_sort=False, verbose=False, n_clusters=64).compress(d, sp)
    out = PngCompression().decompress(d)
    meta = json.load(open(os.path.join(d, "meta.json")))
    for k in ("scales", "opacities", "sh0"):
        bar = O.half_step(meta[k]["mins"], meta[k]["maxs"], 8)
        err = np.abs(out[k].numpy().astype(np.float64) - sp[k].cpu().numpy()).reshape(1024, -1)
        assert (err <= bar).all(), k
    ds = str(tmp_path / "s")
    PngCompression(use_sort=True, verbose=False, n_clusters=64).compress(ds, sp)
    srt = PngCompression().decompress(ds)
    assert not torch.equal(srt["opacities"], out["opacities"])
    torch.testing.assert_close(srt["opacities"].sort().values, out["opacities"].sort().values)


# ------------------------------------------------------ evaluate_compressed
def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


@pytest.mark.parametrize("model,graph", [("3dgs", False), ("2dgs", False), ("3dgs", True)],
                         ids=["3dgs", "2dgs", "3dgs-graph"])
def test_evaluate_compressed(tmp_path, model, graph):
    from gsplat_hip import PngCompression, rasterization, rasterization_2dgs
    from gsplat_hip.losses import ssim_and_l1
    from gsplat_hip.train_step import Trainer
    from test_gpu_trainer_pose import _trainer_scene
    means, rgbs, vm, K, W, H = _trainer_scene()
    tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, model=model, graph=graph)
    for it in range(3):
        tr.step(it)
    tr.sync()
    assert (tr._graph is not None) == graph, tr.graph_fallback
    params = {k: p.detach().clone() for k, p in tr.params.items()}
    moms = {k: [m.clone() for m in mv] for k, mv in tr.moments().items()}
    plain = tr.evaluate()
    d = str(tmp_path / "c")
    comp = PngCompression(verbose=False, n_clusters=512)
    got = tr.evaluate_compressed(d, compression=comp)
    print(f"{model}: PSNR {plain['psnr']:.3f} -> {got['psnr']:.3f}, SSIM {plain['ssim']:.4f} -> "
          f"{got['ssim']:.4f}, {got['num_GS']} of {len(means)} Gaussians in "
          f"{got['compressed_bytes']} B ({got['compressed_bytes'] / got['num_GS']:.1f} B each)")
    n = int(len(means) ** 0.5)
    assert got["num_GS"] == n * n and got["num_images"] == 4
    assert got["compressed_bytes"] == _dir_bytes(d)
    assert set(got) == set(plain) | {"num_GS", "compressed_bytes"}

    sp = {k: v.to(DEV) for k, v in comp.decompress(d).items()}
    ps, ss = [], []
    with torch.no_grad():
        for ci in range(4):
            args = (sp["means"], sp["quats"], torch.exp(sp["scales"]),
                    torch.sigmoid(sp["opacities"]), torch.cat([sp["sh0"], sp["shN"]], 1),
                    tr.viewmats[ci:ci + 1], tr.Ks[ci:ci + 1], W, H)
            kw = dict(sh_degree=3, near_plane=0.01, far_plane=1e10, packed=False)
            if model == "3dgs":
                c = rasterization(*args, **kw)[0]
            else:
                c = rasterization_2dgs(*args, render_mode="RGB+D", **kw)[0][..., :3]
            c = c.clamp(0, 1)
            gt = tr.targets[ci:ci + 1]
            ps.append(float(-10 * torch.log10(((c - gt) ** 2).mean())))
            ss.append(float(ssim_and_l1(c.contiguous(), gt)[0]))
    assert abs(got["psnr"] - sum(ps) / 4) < 1e-4 and abs(got["ssim"] - sum(ss) / 4) < 1e-5, \
        (got, ps, ss)

    # the trainer is untouched, and goes on
    assert list(tr.params) == list(params)
    for k in params:
        assert isinstance(tr.params[k], torch.nn.Parameter) and torch.equal(tr.params[k], params[k])
    now = tr.moments()
    for k in moms:
        assert all(torch.equal(a, b) for a, b in zip(now[k], moms[k])), k
    again = tr.evaluate()
    assert again == pytest.approx(plain, abs=1e-5)
    loss = float(tr.step(3).detach())
    tr.sync()
    assert np.isfinite(loss)
    assert (tr._graph is not None) == graph, tr.graph_fallback  # still replaying
    tr.release_graph()


def test_evaluate_compressed_app_opt(tmp_path):
    """app_opt: `features` / `colors` go to NPZ (lossless), there is no shN to
    cluster, and the evaluation uses the zero embedding as evaluate() does."""
    from gsplat_hip.train_step import Trainer
    from test_gpu_trainer_pose import _trainer_scene
    means, rgbs, vm, K, W, H = _trainer_scene()
    tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, app_opt=True)
    for it in range(2):
        tr.step(it)
    tr.sync()
    params = {k: p.detach().clone() for k, p in tr.params.items()}
    plain = tr.evaluate()
    d = str(tmp_path / "c")
    got = tr.evaluate_compressed(d)
    print(f"app_opt: PSNR {plain['psnr']:.3f} -> {got['psnr']:.3f}, {got['compressed_bytes']} B")
    assert sorted(os.listdir(d)) == sorted(
        ["means_l.png", "means_u.png", "scales.png", "quats.png", "opacities.png",
         "features.npz", "colors.npz", "meta.json"])
    n = int(len(means) ** 0.5)
    assert got["num_GS"] == n * n and got["compressed_bytes"] == _dir_bytes(d)
    assert np.isfinite(got["psnr"]) and np.isfinite(got["ssim"])
    assert all(torch.equal(tr.params[k], params[k]) for k in params)
    assert np.isfinite(float(tr.step(2).detach()))
    tr.sync()


def test_evaluate_compressed_refuses_a_sharded_trainer(tmp_path):
    from gsplat_hip.train_step import Trainer
    from test_gpu_trainer_pose import _trainer_scene
    means, rgbs, vm, K, W, H = _trainer_scene()
    tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, gaussian_shard=True)
    with pytest.raises(NotImplementedError, match="compression.*gaussian_shard"):
        tr.evaluate_compressed(str(tmp_path / "c"))
    assert not os.path.exists(str(tmp_path / "c"))
