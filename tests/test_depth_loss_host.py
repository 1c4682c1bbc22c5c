"""CPU: the host side of sparse depth supervision -- the new ABI entries, the
argument checks of gsplat_hip.sparse_depth_loss, the Trainer constructor's
gating and tables, and colmap.Dataset(load_depths=True) against a numpy
restatement of the reference's projection (examples/datasets/colmap.py:394-415)."""

import os

import numpy as np
import pytest
import torch


def test_abi_entries_and_version():
    from gsplat_hip import _lib
    for name in ("gsplat_hip_depth_loss_fwd", "gsplat_hip_depth_loss_bwd",
                 "gsplat_hip_depth_loss_workspace_bytes"):
        assert name in _lib.EXPORTED
    assert _lib.ABI_VERSION == 38
    assert _lib.load().gsplat_hip_abi_version() == 38
    q = _lib.query
    # a 16-B header (the ticket) and one partial per 256-point workgroup
    assert q("gsplat_hip_depth_loss_workspace_bytes", 0) == 16 + 4
    assert q("gsplat_hip_depth_loss_workspace_bytes", 256) == 16 + 4
    assert q("gsplat_hip_depth_loss_workspace_bytes", 257) == 16 + 8
    assert q("gsplat_hip_depth_loss_workspace_bytes", 32768) == 16 + 4 * 128


def test_sparse_depth_loss_is_exported():
    import gsplat_hip
    assert "sparse_depth_loss" in gsplat_hip.__all__
    assert callable(gsplat_hip.sparse_depth_loss)


BAD_ARGS = {
    "depths rank": dict(depths=torch.zeros(4, 4, 1)),
    "points rank": dict(points=torch.zeros(3, 2)),
    "points last dim": dict(points=torch.zeros(2, 3, 3)),
    "points cameras": dict(points=torch.zeros(1, 3, 2)),
    "depths_gt shape": dict(depths_gt=torch.ones(2, 4)),
    "alphas shape": dict(alphas=torch.ones(2, 4, 4, 4)),
    "channel": dict(channel=4),
    "negative channel": dict(channel=-5),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_sparse_depth_loss_argument_checks(name):
    import gsplat_hip
    kw = dict(depths=torch.zeros(2, 4, 4, 4), points=torch.zeros(2, 3, 2),
              depths_gt=torch.ones(2, 3), alphas=torch.ones(2, 4, 4, 1), channel=-1)
    kw.update(BAD_ARGS[name])
    with pytest.raises(ValueError):
        gsplat_hip.sparse_depth_loss(kw["depths"], kw["points"], kw["depths_gt"], kw["alphas"],
                                     channel=kw["channel"])


def test_sparse_depth_loss_refuses_cpu_tensors():
    import gsplat_hip
    from gsplat_hip._lib import GsplatHipError
    with pytest.raises(GsplatHipError):  # no CPU fall-back
        gsplat_hip.sparse_depth_loss(torch.zeros(1, 4, 4, 1), torch.zeros(1, 3, 2),
                                     torch.ones(1, 3))
    with pytest.raises(GsplatHipError):
        gsplat_hip.sparse_depth_loss(torch.zeros(1, 4, 4, 4), torch.zeros(1, 0, 2),
                                     torch.ones(1, 0), torch.ones(1, 4, 4, 1))


# ------------------------------------------------------------------ Trainer
def _points(counts, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(m, 2, generator=g) * 15, torch.rand(m, generator=g) + 1.0)
            for m in counts]


def _trainer(**kw):
    from gsplat_hip.train_step import Trainer
    g = torch.Generator().manual_seed(0)
    pts, rgbs = torch.rand(8, 3, generator=g), torch.rand(8, 3, generator=g)
    vm, K = torch.eye(4)[None].repeat(3, 1, 1), torch.eye(3)[None].repeat(3, 1, 1)
    return Trainer(pts, rgbs, vm, K, 16, 16, device="cpu", **kw)


UNSUPPORTED = {
    "model='2dgs'": dict(model="2dgs"),
    "packed": dict(packed=True),
    "sparse_grad": dict(packed=True, sparse_grad=True),
    "visible_adam": dict(visible_adam=True),
    "gaussian_shard": dict(gaussian_shard=True, world_size=2),
    "sharded_optimizer": dict(sharded_optimizer=True),
    "world_size": dict(world_size=2),
    "fused=False": dict(fused=False),
}


@pytest.mark.parametrize("name", sorted(UNSUPPORTED))
def test_trainer_refuses_unsupported_combinations(name):
    """Checked before anything touches the device; the message names the option."""
    with pytest.raises(NotImplementedError, match=name.split("=")[0]):
        _trainer(depth_loss=True, depth_points=_points([3, 0, 2]), **UNSUPPORTED[name])


def test_trainer_needs_one_entry_per_image():
    with pytest.raises(ValueError, match="depth_points"):
        _trainer(depth_loss=True)
    with pytest.raises(ValueError, match="depth_points"):
        _trainer(depth_loss=True, depth_points=_points([3, 2]))
    with pytest.raises(ValueError, match="depth_points"):
        _trainer(depth_loss=True, depth_points=_points([3, 2, 1, 0]))
    with pytest.raises(ValueError):  # 4 points, 3 depths
        _trainer(depth_loss=True, depth_points=[(torch.zeros(4, 2), torch.ones(3))] * 3)


def test_trainer_tables():
    """CSR tables built once: offsets int32 [n + 1], rows (x, y, d_gt); empty
    entries allowed.  A trainer without the option holds none and is unchanged."""
    pts = _points([5, 0, 2])
    tr = _trainer(depth_loss=True, depth_lambda=0.5, depth_points=pts)
    tab = tr.depth_table
    assert tab.offsets.dtype == torch.int32 and tab.offsets.tolist() == [0, 5, 5, 7]
    assert tab.max_points == 5 and tab.n_images == 3 and tab.counts == [5, 0, 2]
    rows = tab.points[:7]
    assert torch.equal(rows[:5, :2], pts[0][0]) and torch.equal(rows[:5, 2], pts[0][1])
    assert torch.equal(rows[5:, :2], pts[2][0]) and torch.equal(rows[5:, 2], pts[2][1])
    assert tr.depth_loss and tr.depth_lambda == 0.5
    # numpy arrays, as a dataset's items converted by the caller
    tr2 = _trainer(depth_loss=True, depth_points=[(p.numpy(), d.numpy()) for p, d in pts])
    assert torch.equal(tr2.depth_table.points, tab.points)
    assert tr2.depth_lambda == 1e-2  # the reference's default
    plain, off = _trainer(), _trainer(depth_loss=False, depth_points=pts)
    for t in (plain, off):
        assert not t.depth_loss and not hasattr(t, "depth_table")
    for k in plain.params:
        assert torch.equal(plain.params[k], tr.params[k]), k


# ------------------------------------------------------------------ Dataset
W, H, F_ = 32, 24, 30.0


def _model(tmp):
    """Three images of one 32 x 24 pinhole camera.  b.png observes a handful of
    points: ordinary ones, one behind the camera, one projecting outside the
    image and one at x in (W - 1, W); c.png some of them from a shifted and
    rotated pose; a.png observes none."""
    from PIL import Image as PILImage
    from gsplat_hip import colmap as M
    cams = {1: M.Camera(1, "PINHOLE", W, H, [F_, F_, W / 2, H / 2])}
    th = 0.05
    q_rot = np.array([np.cos(th / 2), 0.0, np.sin(th / 2), 0.0])  # about y
    poses = {1: ("a.png", np.array([1.0, 0, 0, 0]), np.zeros(3)),
             2: ("b.png", np.array([1.0, 0, 0, 0]), np.zeros(3)),
             3: ("c.png", q_rot, np.array([0.1, -0.05, 0.2]))}
    xyz = {
        1: [0.0, 0.0, 2.0],                     # the image centre
        2: [-0.9, 0.5, 2.5],
        3: [0.7, -0.6, 3.0],
        4: [0.2, 0.1, -1.0],                    # behind the camera
        5: [3.0, 0.0, 2.0],                     # projects to x = 61: outside
        6: [(W - 0.5 - W / 2) / F_ * 2.0, 0.3, 2.0],   # x = W - 0.5, in (W - 1, W)
        7: [0.1, (H - 0.25 - H / 2) / F_ * 4.0, 4.0],  # y = H - 0.25, in (H - 1, H)
        8: [-0.3, -0.2, 1.5],
    }
    seen = {2: [1, 2, 3, 4, 5, 6, 7, 8], 3: [1, 2, 3, 6, 8], 1: []}
    ims = {}
    for i, (name, q, t) in poses.items():
        ids = np.array(seen[i], np.int64)
        ims[i] = M.Image(i, q, t, 1, name, np.zeros((len(ids), 2)), ids)
    pts = {}
    for p, x in xyz.items():
        who = [i for i in ims if p in seen[i]]
        pts[p] = M.Point3D(p, np.array(x), np.array([1, 2, 3]), 0.5, who,
                           [seen[i].index(p) for i in who])
    M.write_model_bin(str(tmp / "sparse" / "0"), cams, ims, pts)
    os.makedirs(tmp / "images", exist_ok=True)
    for name, _, _ in poses.values():
        PILImage.new("RGB", (W, H), (10, 20, 30)).save(tmp / "images" / name)
    return M.Parser(str(tmp), factor=1, normalize=False, test_every=2)


def _reference_points(P, index, K, width, height):
    """examples/datasets/colmap.py:396-413 restated."""
    worldtocams = np.linalg.inv(P.camtoworlds[index])
    point_indices = P.point_indices.get(P.image_names[index], np.zeros(0, np.int32))
    points_world = P.points[point_indices]
    points_cam = (worldtocams[:3, :3] @ points_world.T + worldtocams[:3, 3:4]).T
    points_proj = (K @ points_cam.T).T
    with np.errstate(divide="ignore", invalid="ignore"):
        points = points_proj[:, :2] / points_proj[:, 2:3]
    depths = points_cam[:, 2]
    selector = ((points[:, 0] >= 0) & (points[:, 0] < width) & (points[:, 1] >= 0)
                & (points[:, 1] < height) & (depths > 0))
    return points[selector].astype(np.float32), depths[selector].astype(np.float32)


@pytest.mark.parametrize("patch", [None, 16], ids=["full", "patch16"])
def test_dataset_load_depths(tmp_path, patch):
    from gsplat_hip import colmap as M
    P = _model(tmp_path)
    assert P.image_names == ["a.png", "b.png", "c.png"]
    assert "a.png" not in P.point_indices
    counts = {}
    for split in ("val", "train"):  # val: a.png, c.png; train: b.png
        ds = M.Dataset(P, split, patch_size=patch, load_depths=True)
        for item in range(len(ds)):
            index = int(ds.indices[item])
            np.random.seed(100 + index)
            data = ds[item]
            K = P.Ks_dict[1].copy()
            w, h = W, H
            if patch is not None:  # the dataset's own draws, in its order
                np.random.seed(100 + index)
                x = np.random.randint(0, max(W - patch, 1))
                y = np.random.randint(0, max(H - patch, 1))
                K[0, 2] -= x
                K[1, 2] -= y
                w = h = patch
            np.testing.assert_array_equal(data["K"].numpy(), K.astype(np.float32))
            assert data["image"].shape[:2] == (h, w)
            pts, dep = _reference_points(P, index, K, w, h)
            assert data["points"].dtype == torch.float32 and data["depths"].dtype == torch.float32
            assert data["points"].shape == (len(dep), 2) and data["depths"].shape == (len(dep),)
            np.testing.assert_array_equal(data["points"].numpy(), pts)
            np.testing.assert_array_equal(data["depths"].numpy(), dep)
            counts[P.image_names[index]] = len(dep)
    assert counts["a.png"] == 0
    if patch is None:
        # b.png: 8 observed, minus the one behind and the one outside
        assert counts["b.png"] == 6 and 0 < counts["c.png"] <= 5, counts
        b = M.Dataset(P, "train", load_depths=True)[0]
        xs, ys = b["points"][:, 0], b["points"][:, 1]
        assert float(xs.max()) == pytest.approx(W - 0.5, abs=1e-4)  # kept: x < W
        assert float(ys.max()) == pytest.approx(H - 0.25, abs=1e-4)
        assert float(b["depths"].min()) > 0
    # off by default: the items are what they were
    plain = M.Dataset(P, "train")[0]
    assert "points" not in plain and "depths" not in plain
