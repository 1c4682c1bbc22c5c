"""Host side of the undistortion of COLMAP scenes (gsplat_hip.colmap:
undistort_points, optimal_new_camera_matrix, undistort_maps, fisheye_roi,
undistort_host, Parser / Dataset) and the refusals of gsplat_hip.undistort.
CPU only.  The cases and the independent float64 oracle are in
tests/undistort_cases.py."""

import os

import numpy as np
import pytest
import torch

import undistort_cases as UC


def _geo(name):
    """colmap.py's own geometry of a case: K_new, roi, K_undist-shifted, maps, mask."""
    from gsplat_hip import colmap as M
    case = UC.CASES[name]
    K = UC.K3(case.K)
    if case.camtype == "perspective":
        K_new, roi = M.optimal_new_camera_matrix(K, case.params, case.size)
        mapx, mapy = M.undistort_maps(K, case.params, K_new, case.size, "perspective")
        mask = None
    else:
        K_new = K
        mapx, mapy = M.undistort_maps(K, case.params, K_new, case.size, "fisheye")
        roi, mask = M.fisheye_roi(mapx, mapy, case.size)
    return K, K_new, roi, mapx, mapy, mask


# ------------------------------------------------------------ 1 round trip
@pytest.mark.parametrize("name", ["P1", "P2", "P3"])
def test_undistort_points_round_trip(name):
    """Forward-distorted normalised points over |x|, |y| <= 0.6 come back
    within 1e-3 (normalised, i.e. 1e-3 of the focal length in pixels) after
    OpenCV's 5 fixed-point iterations, which do not reach machine precision."""
    from gsplat_hip import colmap as M
    case = UC.CASES[name]
    fx, fy, cx, cy = case.K
    k1, k2, p1, p2 = case.params
    x, y = (a.ravel() for a in np.meshgrid(np.linspace(-0.6, 0.6, 25), np.linspace(-0.6, 0.6, 25)))
    r2 = x * x + y * y
    kr = 1 + (k2 * r2 + k1) * r2
    xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    pix = np.stack([fx * xd + cx, fy * yd + cy], -1)
    back = M.undistort_points(pix, UC.K3(case.K), case.params)
    assert back.shape == (x.size, 2) and back.dtype == np.float64
    res = np.abs(back - np.stack([x, y], -1)).max()
    print(f"{name}: residual after 5 iterations {res:.3e} (normalised), "
          f"{res * max(fx, fy):.3e} px")
    assert res < 1e-3
    # more iterations converge further: the residual is the iteration's, not a bug's
    res20 = np.abs(M.undistort_points(pix, UC.K3(case.K), case.params, iters=20)
                   - np.stack([x, y], -1)).max()
    assert res20 < res * 1e-2 or res20 < 1e-12


# ---------------------------------------------- 2 optimal_new_camera_matrix
# From a numpy prototype of the same algorithm (the issue's), not from cv2:
# OpenCV is not available to pin these against.
NEW_K = {"P1": (76.184, 78.594, 47.222, 31.141),
         "P2": (83.368, 83.371, 47.340, 31.075),
         "P3": (77.689, 77.291, 49.914, 29.104)}


@pytest.mark.parametrize("name", ["P1", "P2", "P3"])
def test_optimal_new_camera_matrix_values(name):
    K, K_new, roi, *_ = _geo(name)
    got = (K_new[0, 0], K_new[1, 1], K_new[0, 2], K_new[1, 2])
    print(name, got, roi)
    np.testing.assert_allclose(got, NEW_K[name], rtol=0, atol=2e-3)
    assert tuple(roi) == (0, 0, 96, 60)
    assert K_new[0, 1] == 0 and K_new[1, 0] == 0 and K_new[2].tolist() == [0, 0, 1]
    # the independent restatement agrees to rounding
    g = UC.geometry(name)
    np.testing.assert_allclose(got, g.K_new, rtol=1e-12)
    assert tuple(roi) == tuple(g.roi)


@pytest.mark.parametrize("name", UC.PERSPECTIVE)
def test_roi_sources_lie_inside_the_image(name):
    """alpha = 0: every ROI pixel's source coordinate lies in
    [-0.5, W - 0.5] x [-0.5, H - 0.5]."""
    _, _, roi, mapx, mapy, _ = _geo(name)
    W, H = UC.CASES[name].size
    x, y, w, h = roi
    sx, sy = mapx[y:y + h, x:x + w], mapy[y:y + h, x:x + w]
    print(f"{name}: roi {roi} sx [{sx.min():.3f}, {sx.max():.3f}] sy [{sy.min():.3f}, {sy.max():.3f}]")
    assert w > 0 and h > 0
    assert sx.min() >= -0.5 and sx.max() <= W - 0.5
    assert sy.min() >= -0.5 and sy.max() <= H - 0.5


@pytest.mark.parametrize("name", UC.ALL)
def test_maps_match_the_independent_oracle(name):
    """float32 maps [H, W] of the full frame = the oracle's float64 map of the
    ROI, rounded."""
    _, K_new, roi, mapx, mapy, _ = _geo(name)
    W, H = UC.CASES[name].size
    g = UC.geometry(name)
    assert mapx.shape == (H, W) and mapx.dtype == np.float32 and mapy.dtype == np.float32
    assert tuple(roi) == tuple(g.roi)
    x, y, w, h = roi
    # a few ulp of the float64 evaluation around the rounding, i.e. 1 fp32 ulp at most
    tol = float(np.spacing(np.float32(max(W, H))))
    assert np.abs(mapx[y:y + h, x:x + w] - g.sx).max() <= tol
    assert np.abs(mapy[y:y + h, x:x + w] - g.sy).max() <= tol


# --------------------------------------------- 3 geometry vs analytic truth
@pytest.mark.parametrize("name", UC.ALL)
def test_undistort_host_against_the_analytic_image(name):
    """The source image is g sampled on the pixel grid, so the undistorted
    image must be g(mapx, mapy) within 0.5 + A (wx^2 + wy^2) / 8 levels per
    channel (uint8 rounding + bilinear interpolation, UC.interp_bound),
    wherever the four neighbours lie inside the source (elsewhere the zero
    border enters).  A half-pixel shift, a transposed map, a swapped channel
    or an unshifted ROI break this bound."""
    from gsplat_hip import colmap as M
    _, _, roi, mapx, mapy, _ = _geo(name)
    W, H = UC.CASES[name].size
    imgs = UC.images(name)
    x, y, w, h = roi
    sx = mapx[y:y + h, x:x + w].astype(np.float64)
    sy = mapy[y:y + h, x:x + w].astype(np.float64)
    inner = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
    assert inner.mean() > 0.9, inner.mean()
    for b in range(imgs.shape[0]):
        out = M.undistort_host(imgs[b], mapx, mapy, roi)
        assert out.shape == (h, w, 3) and out.dtype == np.float32
        for c in range(3):
            err = np.abs(out[..., c] - UC.pattern(c, b, sx, sy))[inner].max()
            print(f"{name} image {b} channel {c}: {err:.3f} levels, bound {UC.interp_bound(c):.3f}")
            assert err <= UC.interp_bound(c)
        # and against the oracle's remap: float32 maps and blend vs float64
        o = UC.oracle(name)[b]
        assert np.abs(out - o).max() <= UC.bound(name, 1.0)
    # the sensitivity the docstring claims, on the first image
    out = M.undistort_host(imgs[0], mapx, mapy, roi)
    truth = np.stack([UC.pattern(c, 0, sx, sy) for c in range(3)], -1)
    bounds = np.array([UC.interp_bound(c) for c in range(3)])

    def breaks(o):
        return (np.abs(o - truth)[inner].reshape(-1, 3).max(0) > bounds).any()
    assert not breaks(out)
    assert breaks(M.undistort_host(imgs[0], mapx + np.float32(0.5), mapy, roi))
    assert breaks(out[..., [1, 0, 2]])
    if x or y:
        assert breaks(M.undistort_host(imgs[0], mapx, mapy, (0, 0, w, h)))


def test_undistort_host_border_is_zero():
    from gsplat_hip import colmap as M
    img = np.full((3, 4, 3), 200, np.uint8)
    mapx = np.array([[-1.0, -0.5, 0.0, 3.0, 3.5, 4.0, np.nan, 1.25]], np.float32)
    mapy = np.array([[1.0, 1.0, 0.0, 2.0, 2.5, 1.0, 1.0, -0.25]], np.float32)
    out = M.undistort_host(img, mapx, mapy, (0, 0, 8, 1))
    np.testing.assert_allclose(out[0, :, 0], [0, 100, 200, 200, 50, 0, 0, 150], atol=1e-4)


# ---------------------------------------------------------------- 4 fisheye
@pytest.mark.parametrize("name", UC.FISHEYE)
def test_fisheye_mask_and_roi(name):
    """Mask and ROI against a direct evaluation of the reference's formula
    (colmap.py:281-316), written out here."""
    case = UC.CASES[name]
    W, H = case.size
    fx, fy, cx, cy = case.K
    k = case.params
    _, K_new, roi, mapx, mapy, mask = _geo(name)
    gx, gy = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x1, y1 = (gx - cx) / fx, (gy - cy) / fy
    theta = np.sqrt(x1 ** 2 + y1 ** 2)
    r = 1.0 + k[0] * theta ** 2 + k[1] * theta ** 4 + k[2] * theta ** 6 + k[3] * theta ** 8
    mx = (fx * x1 * r + W // 2).astype(np.float32)
    my = (fy * y1 * r + H // 2).astype(np.float32)
    m = (mx > 0) & (my > 0) & (mx < W - 1) & (my < H - 1)
    ys, xs = np.nonzero(m)
    want = (xs.min(), ys.min(), xs.max() + 1 - xs.min(), ys.max() + 1 - ys.min())
    print(f"{name}: roi {roi}, {mask.mean():.3%} of it inside the mask")
    assert tuple(roi) == tuple(int(v) for v in want)
    np.testing.assert_array_equal(mask, m[want[1]:want[1] + want[3], want[0]:want[0] + want[2]])
    assert mask.dtype == bool and mask.shape == (roi[3], roi[2])
    assert roi[0] > 0 and roi[1] > 0  # the origin these cases are there for
    assert np.abs(mapx - mx).max() <= np.spacing(np.float32(W))
    assert np.abs(mapy - my).max() <= np.spacing(np.float32(W))
    g = UC.geometry(name)
    assert tuple(roi) == tuple(g.roi)
    np.testing.assert_array_equal(mask, g.mask)


# ------------------------------------------------------- 5 Parser / Dataset
def scene(tmp, case_name="P1", n_img=6, n_pts=60, seed=0, mixed=True):
    """A synthetic scene directory: camera 1 PINHOLE 64x48, camera 2 the
    case's distorted camera, images alternating between them (PNGs of the
    cases' smooth pattern; `mixed=False`: every image from camera 2), points in
    front of every camera."""
    from PIL import Image as PILImage
    from gsplat_hip import colmap as M
    case = UC.CASES[case_name]
    W, H = case.size
    rng = np.random.default_rng(seed)
    cams = {1: M.Camera(1, "PINHOLE", 64, 48, [70.0, 71.0, 31.0, 25.0]),
            2: M.Camera(2, case.model, W, H, UC.colmap_params(case))}
    xyz = rng.uniform(-1, 1, size=(n_pts, 3)) * [1.0, 0.7, 0.5]
    ims = {}
    for i in range(1, n_img + 1):
        a = 0.05 * (i - n_img / 2)
        q = np.array([np.cos(a / 2), 0.0, np.sin(a / 2), 0.0])  # a small turn about y
        ids = np.arange(1, n_pts + 1)
        ims[i] = M.Image(i, q, np.array([0.05 * i, 0.0, 4.0]), 1 if mixed and i % 3 == 0 else 2,
                         f"img_{i:03d}.png", rng.random((n_pts, 2)) * 50, ids)
    pts = {p: M.Point3D(p, xyz[p - 1], rng.integers(0, 255, 3), 0.5, list(ims),
                        [p - 1] * len(ims)) for p in range(1, n_pts + 1)}
    M.write_model_bin(os.path.join(str(tmp), "sparse", "0"), cams, ims, pts)
    os.makedirs(os.path.join(str(tmp), "images"), exist_ok=True)
    frames = {}
    for i, im in ims.items():
        c = cams[im.camera_id]
        x, y = np.meshgrid(np.arange(c.width, dtype=np.float64),
                           np.arange(c.height, dtype=np.float64))
        f = np.rint(np.stack([UC.pattern(ch, i, x, y) for ch in range(3)], -1)).astype(np.uint8)
        PILImage.fromarray(f).save(os.path.join(str(tmp), "images", im.name))
        frames[im.name] = f
    return cams, ims, pts, frames


def test_parser_and_dataset_undistort(tmp_path):
    from gsplat_hip import colmap as M
    case = UC.CASES["P1"]
    cams, ims, pts, frames = scene(tmp_path)
    P = M.Parser(str(tmp_path), test_every=100)  # everything but image 0 trains
    g = UC.geometry("P1")
    # the pinhole camera is what it was: its own K and size, no map entries
    np.testing.assert_array_equal(P.Ks_dict[1], [[70.0, 0, 31.0], [0, 71.0, 25.0], [0, 0, 1]])
    assert P.imsize_dict[1] == (64, 48) and len(P.params_dict[1]) == 0
    assert P.mask_dict[1] is None
    for d in (P.mapx_dict, P.mapy_dict, P.roi_undist_dict):
        assert list(d) == [2]
    # the distorted camera: undistorted K (shifted by the ROI origin), ROI size
    roi = P.roi_undist_dict[2]
    assert tuple(roi) == tuple(g.roi) and P.imsize_dict[2] == (roi[2], roi[3])
    K2 = P.Ks_dict[2]
    np.testing.assert_allclose([K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2]], g.K_undist, rtol=1e-6)
    np.testing.assert_allclose(P.Ks_dist_dict[2], UC.K3(case.K))
    assert P.mapx_dict[2].shape == (case.size[1], case.size[0])
    assert P.mask_dict[2] is None and P.camtype_dict[2] == "perspective"

    ds = M.Dataset(P, "train", load_depths=True)
    seen = set()
    for j in range(len(ds)):
        item = ds[j]  # NotImplementedError before undistortion was there
        name = P.image_names[ds.indices[j]]
        cid = P.camera_ids[ds.indices[j]]
        seen.add(cid)
        w, h = P.imsize_dict[cid]
        assert item["image"].shape == (h, w, 3) and item["image"].dtype == torch.float32
        np.testing.assert_allclose(item["K"].numpy(), P.Ks_dict[cid], rtol=1e-6)
        assert "mask" not in item
        if cid == 1:
            np.testing.assert_array_equal(item["image"].numpy(), frames[name].astype(np.float32))
        else:
            want = M.undistort_host(frames[name], P.mapx_dict[2], P.mapy_dict[2], roi)
            np.testing.assert_array_equal(item["image"].numpy(), want)
            assert want.max() > 200 and want.min() < 60  # an image, not a blank
        p, d = item["points"].numpy(), item["depths"].numpy()
        assert len(p) > 10 and len(p) == len(d) and (d > 0).all()
        assert (p[:, 0] >= 0).all() and (p[:, 0] < w).all()
        assert (p[:, 1] >= 0).all() and (p[:, 1] < h).all()
    assert seen == {1, 2}

    # patch_size crops the undistorted image and shifts the undistorted K
    np.random.seed(3)
    item = M.Dataset(P, "train", patch_size=32)[0]
    assert item["image"].shape == (32, 32, 3)
    cid = P.camera_ids[M.Dataset(P, "train").indices[0]]
    assert float(item["K"][0, 2]) <= P.Ks_dict[cid][0, 2]
    assert float(item["K"][0, 0]) == float(np.float32(P.Ks_dict[cid][0, 0]))


def test_parser_chooses_the_camera_type_per_camera(tmp_path):
    """A fisheye camera after a perspective one: each gets its own type, its
    own mask and ROI (the reference applies one type to all)."""
    from gsplat_hip import colmap as M
    cams, ims, pts, frames = scene(tmp_path, "F2")
    cams[1] = M.Camera(1, "OPENCV", 97, 61, UC.colmap_params(UC.CASES["P3"]))
    M.write_model_bin(os.path.join(str(tmp_path), "sparse", "0"), cams, ims, pts)
    os.rename(tmp_path / "images", tmp_path / "unused")  # sizes differ now: no image check
    P = M.Parser(str(tmp_path))
    assert P.camtype_dict == {1: "perspective", 2: "fisheye"}
    gp, gf = UC.geometry("P3"), UC.geometry("F2")
    assert tuple(P.roi_undist_dict[1]) == tuple(gp.roi) and P.mask_dict[1] is None
    assert tuple(P.roi_undist_dict[2]) == tuple(gf.roi)
    np.testing.assert_array_equal(P.mask_dict[2], gf.mask)
    K2 = P.Ks_dict[2]  # the fisheye K, shifted by the ROI origin
    np.testing.assert_allclose([K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2]], gf.K_undist, rtol=1e-6)
    assert P.imsize_dict[2] == (gf.roi[2], gf.roi[3])


def test_dataset_returns_the_fisheye_mask(tmp_path):
    from gsplat_hip import colmap as M
    scene(tmp_path, "F1")
    P = M.Parser(str(tmp_path), test_every=100)
    ds = M.Dataset(P, "train")
    j = [P.camera_ids[i] for i in ds.indices].index(2)
    item = ds[j]
    w, h = P.imsize_dict[2]
    assert item["mask"].dtype == torch.bool and item["mask"].shape == (h, w)
    assert item["image"].shape == (h, w, 3)
    np.testing.assert_array_equal(item["mask"].numpy(), UC.geometry("F1").mask)


# -------------------------------------------------- 6 refusals and exports
def test_exports_and_abi():
    import gsplat_hip
    from gsplat_hip import _lib
    for name in ("undistort_images", "remap_bilinear"):
        assert name in gsplat_hip.__all__ and callable(getattr(gsplat_hip, name))
    for name in ("gsplat_hip_undistort_u8_f32", "gsplat_hip_remap_u8_f32"):
        assert name in _lib.EXPORTED
    assert _lib.ABI_VERSION == 38


def test_ops_refuse_before_any_device_work():
    from gsplat_hip import remap_bilinear, undistort_images
    from gsplat_hip._lib import GsplatHipError
    K = UC.K3((80.0, 80.0, 47.3, 31.1))
    k = [-0.12, 0, 0, 0]
    roi = (0, 0, 8, 6)
    img = torch.zeros(2, 6, 8, 3, dtype=torch.uint8)
    mx = torch.zeros(6, 8)
    with pytest.raises(GsplatHipError, match="GPU only"):
        undistort_images(img, K, k, K, roi)
    with pytest.raises(GsplatHipError, match="GPU only"):
        remap_bilinear(img, mx, mx)
    for bad in (img.float(), img[0], img[..., :2], img.permute(0, 2, 1, 3)):
        with pytest.raises(GsplatHipError, match="images must"):
            undistort_images(bad, K, k, K, roi)
        with pytest.raises(GsplatHipError, match="images must"):
            remap_bilinear(bad, mx, mx)
    with pytest.raises(GsplatHipError):
        remap_bilinear(img, mx.double(), mx)
    with pytest.raises(GsplatHipError):
        remap_bilinear(img, mx, mx[:5])
    with pytest.raises(GsplatHipError):
        remap_bilinear(img, mx[None], mx[None])
    with pytest.raises(GsplatHipError):
        undistort_images(img, K, k[:3], K, roi)
    with pytest.raises(GsplatHipError):
        undistort_images(img, K, k, K, (0, 0, 8))
    with pytest.raises(GsplatHipError):
        undistort_images(img, K, k, K, roi, out=torch.zeros(2, 6, 8, 3, dtype=torch.float64))
    with pytest.raises(GsplatHipError):
        undistort_images(img, K, k, K, roi, out=torch.zeros(2, 6, 9, 3))
    with pytest.raises(ValueError):
        undistort_images(img, K, k, K, roi, camtype="equirect")
