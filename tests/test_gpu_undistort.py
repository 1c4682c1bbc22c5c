"""GPU checks of image undistortion (csrc/undistort.hip through
gsplat_hip.undistort, and gsplat_hip.colmap's Dataset(device=...) and
scene_tensors on top of it).

The truth is the float64 oracle of tests/undistort_cases.py.  The bound is the
project's bar convention (tests/test_gpu_covar.py): err <= max(4 x bar,
1e-6 x 255 x scale), where bar is the error against the oracle of the same
computation with the map evaluated in float32, computed on the CPU and
printed.  The kernel evaluates the map in float64 and rounds it to float32,
so it should sit well inside."""

import numpy as np
import pytest
import torch

import undistort_cases as UC
from test_undistort_host import scene

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401  (fails loudly if the .so is missing)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True)).to(DEV)  # the cached cases stay read-only
    return t if dtype is None else t.to(dtype)


def _analytic(name, scale=1.0, out=None, B=2):
    from gsplat_hip import undistort_images
    case, g = UC.CASES[name], UC.geometry(name)
    return undistort_images(_dev(UC.images(name, B)), UC.K3(case.K), case.params, UC.K3(g.K_new),
                            g.roi, case.camtype, scale=scale, out=out)


def _check(what, got, want, bound):
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max())
    print(f"{what}: err {err:.3e}  bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


# ------------------------------------------------------ 1 the analytic map
@pytest.mark.parametrize("scale", [1.0, 1.0 / 255.0])
@pytest.mark.parametrize("name", UC.ALL)
def test_analytic_kernel_vs_float64_oracle(name, scale):
    g = UC.geometry(name)
    out = _analytic(name, scale)
    assert out.shape == (2, g.roi[3], g.roi[2], 3) and out.dtype == torch.float32
    print(f"{name}: bar {UC.bar(name):.3e} levels")
    _check(f"{name} scale {scale:.4g}", out, UC.oracle(name) * scale, UC.bound(name, scale))
    assert not torch.equal(out[0], out[1])  # two different images


# ---------------------------------------------------- 2 the table-driven form
@pytest.mark.parametrize("name", UC.ALL)
def test_table_remap_vs_oracle_and_analytic(name):
    from gsplat_hip import remap_bilinear
    g = UC.geometry(name)
    mapx, mapy = g.sx.astype(np.float32), g.sy.astype(np.float32)
    out = remap_bilinear(_dev(UC.images(name)), _dev(mapx), _dev(mapy), scale=1.0 / 255.0)
    bound = UC.bound(name, 1.0 / 255.0)
    _check(f"{name} table", out, UC.oracle(name) / 255.0, bound)
    ana = _analytic(name, 1.0 / 255.0)
    _check(f"{name} table vs analytic", out, ana.cpu().numpy().astype(np.float64), bound)


def test_table_remap_border_contributes_zero():
    """Coordinates below 0, beyond W - 1 / H - 1, exactly on integers, far
    away and not finite: the oracle's remap of the same float32 map, so only
    the fp32 blend separates the two (the floor of the bound)."""
    from gsplat_hip import remap_bilinear
    name = "P1"
    imgs = UC.images(name)
    W, H = UC.CASES[name].size
    rng = np.random.default_rng(5)
    h, w = 37, 53
    mapx = rng.uniform(-3.0, W + 2.0, size=(h, w)).astype(np.float32)
    mapy = rng.uniform(-3.0, H + 2.0, size=(h, w)).astype(np.float32)
    mapx[0, :12] = [-1.0, -0.5, 0.0, W - 1.0, W - 0.5, W, 5.0, 7.0, 1e30, -1e30, np.nan, np.inf]
    mapy[0, :12] = [3.0, 3.0, 0.0, H - 1.0, H - 0.5, 3.0, -0.25, 9.0, 3.0, 3.0, 3.0, -np.inf]
    mapx[1], mapy[1] = np.arange(w), 4.0  # integers: the source pixels themselves
    out = remap_bilinear(_dev(imgs), _dev(mapx), _dev(mapy))
    want = UC.remap(imgs, mapx.astype(np.float64), mapy.astype(np.float64))
    # four terms of three fp32 roundings each and three additions, of values <= 255
    _check("border", out, want, 1e-6 * 255.0 + 16 * 255.0 * 2.0 ** -24)
    o = out.cpu().numpy()
    np.testing.assert_array_equal(o[:, 1], imgs[:, 4, :w].astype(np.float32))
    for j in (0, 5, 8, 9, 10, 11):
        assert not o[:, 0, j].any()
    np.testing.assert_array_equal(o[:, 0, 2], imgs[:, 0, 0].astype(np.float32))
    np.testing.assert_array_equal(o[:, 0, 3], imgs[:, H - 1, W - 1].astype(np.float32))
    np.testing.assert_allclose(o[:, 0, 4], imgs[:, H - 1, W - 1] * 0.25, rtol=1e-6)
    outside = (mapx <= -1) | (mapx >= W) | (mapy <= -1) | (mapy >= H)
    assert outside.sum() > 50 and not o[:, outside].any()


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 2), (1, 1, 5), (2, 2, 3), (1, 3, 2)])
def test_table_remap_tiny_sources(shape):
    """Source buffers of 3 to 36 bytes: below 16 bytes the kernel reads byte by
    byte, from 16 on with 12-B loads whose start is pulled back at the end of
    the buffer.  Every pixel centre, the midpoints between them and a ring
    outside are sampled."""
    from gsplat_hip import remap_bilinear
    B, H, W = shape
    rng = np.random.default_rng(B * 100 + H * 10 + W)
    imgs = rng.integers(1, 256, size=(B, H, W, 3), dtype=np.uint8)
    xs, ys = np.arange(-1.5, W + 1.0, 0.5), np.arange(-1.5, H + 1.0, 0.5)
    mapx, mapy = (m.astype(np.float32) for m in np.meshgrid(xs, ys))
    out = remap_bilinear(_dev(imgs), _dev(mapx), _dev(mapy))
    want = UC.remap(imgs, mapx.astype(np.float64), mapy.astype(np.float64))
    # weights in {0, 1/4, 1/2, 1}: every product and sum is exact in fp32
    np.testing.assert_array_equal(out.cpu().numpy().astype(np.float64), want)


# ------------------------------------------------------------------- 3 out=
def test_out_slice_of_a_larger_tensor():
    name = "F1"  # odd w (93) and h*w*3: the slice starts 4 B off a 16-B boundary
    g = UC.geometry(name)
    h, w = g.roi[3], g.roi[2]
    assert (h * w * 3) % 4 != 0
    targets = torch.full((4, h, w, 3), -7.0, device=DEV)
    ret = _analytic(name, 1.0 / 255.0, out=targets[1:3])
    assert ret.data_ptr() == targets[1].data_ptr()
    fresh = _analytic(name, 1.0 / 255.0)
    assert torch.equal(targets[1:3], fresh)
    assert (targets[0] == -7.0).all() and (targets[3] == -7.0).all()


# ---------------------------------------------------------- 4 determinism
@pytest.mark.parametrize("name", ["P3", "F2"])
def test_two_runs_are_bit_identical(name):
    a, b = _analytic(name), _analytic(name)
    assert torch.equal(a, b)


# ----------------------------------------------------------- 5 end to end
def test_scene_to_trainer(tmp_path):
    from gsplat_hip import colmap as M
    from gsplat_hip.train_step import Trainer
    scene(tmp_path, "P1", n_img=5, mixed=False)
    P = M.Parser(str(tmp_path), test_every=100)
    t = M.scene_tensors(P, "train", device=DEV, load_depths=True)
    ds, dsg = M.Dataset(P, "train"), M.Dataset(P, "train", device=DEV)
    n, (w, h) = len(ds), P.imsize_dict[2]
    assert t["targets"].shape == (n, h, w, 3) and t["targets"].is_cuda
    assert (t["width"], t["height"]) == (w, h) and t["masks"] is None
    assert len(t["depth_points"]) == n and t["viewmats"].shape == (n, 4, 4)
    bound = UC.bound("P1", 1.0)  # the same camera and the same family of images
    for j in range(n):
        item, gitem = ds[j], dsg[j]
        assert gitem["image"].is_cuda and gitem["image"].shape == item["image"].shape
        host = item["image"].numpy().astype(np.float64)
        _check(f"targets[{j}]", t["targets"][j], host / 255.0, bound / 255.0)
        _check(f"Dataset(device)[{j}]", gitem["image"], host, bound)
        np.testing.assert_allclose(t["Ks"][j].numpy(), item["K"].numpy(), rtol=1e-6)
        np.testing.assert_allclose(t["viewmats"][j].numpy() @ item["camtoworld"].numpy(),
                                   np.eye(4), atol=1e-5)
    masks = t.pop("masks")
    t.pop("depth_points")
    tr = Trainer(t.pop("points"), t.pop("rgbs"), **t, init="sfm")
    losses = [float(tr.step(it).detach()) for it in range(2)]
    print("losses", losses)
    assert all(np.isfinite(v) for v in losses) and masks is None


def test_scene_tensors_refuses_mixed_sizes_and_returns_masks(tmp_path):
    from gsplat_hip import colmap as M
    scene(tmp_path / "mixed", "P1", n_img=4, mixed=True)
    with pytest.raises(ValueError, match="one width and height"):
        M.scene_tensors(M.Parser(str(tmp_path / "mixed"), test_every=100), device=DEV)
    scene(tmp_path / "fish", "F2", n_img=3, mixed=False)
    P = M.Parser(str(tmp_path / "fish"), test_every=100)
    t = M.scene_tensors(P, device=DEV)
    g = UC.geometry("F2")
    assert t["masks"].shape == (2, g.roi[3], g.roi[2]) and t["masks"].dtype == torch.bool
    np.testing.assert_array_equal(t["masks"][0].cpu().numpy(), g.mask)
    item = M.Dataset(P, "train")[0]
    _check("fisheye targets", t["targets"][0], item["image"].numpy().astype(np.float64) / 255.0,
           UC.bound("F2", 1.0 / 255.0))
