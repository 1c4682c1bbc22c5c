"""COLMAP scenes for the trainer counterpart.

The reference trainer reads its scenes with `pycolmap.SceneManager`
(examples/datasets/colmap.py:59-333, a git-URL dependency pinned in
examples/requirements.txt:4 and absent here) and normalises the world with
examples/datasets/normalize.py.  This module restates both on numpy:

  read_model(dir)    cameras / images / points3D from COLMAP's binary
                     (`*.bin`) or text (`*.txt`) model files, in the formats
                     COLMAP documents (src/colmap/scene/reconstruction_io)
  similarity_from_cameras, align_principle_axes, transform_points,
  transform_cameras  normalize.py:4-143, same algebra and order
  Parser             colmap.py:59-333: world-to-camera matrices from the
                     image quaternions, K / factor per camera, images sorted
                     by name, optional normalisation, the per-image point
                     indices, the actual-image-size K rescale and scene_scale
  Dataset            colmap.py:336-440: the every-`test_every`-th split and
                     the per-item dict (K, camtoworld, image, image_id)
  scene_tensors      Parser -> Trainer: the split's images undistorted on the
                     device into one `targets` table, with the cameras

Undistortion (colmap.py:258-325, 366-374).  The reference calls OpenCV; here
OpenCV's published algorithms are restated on numpy in float64
(`undistort_points`, `optimal_new_camera_matrix` = getOptimalNewCameraMatrix
at alpha 0, `undistort_maps` = initUndistortRectifyMap with R = I, and the
reference's own fisheye formula), and the remap itself is a HIP kernel
(gsplat_hip.undistort) with `undistort_host` as its numpy counterpart.
Deviations, all deliberate:
  * the bilinear weights are fp32 at the unquantised coordinate (cv2.remap
    quantises them to 5 bits);
  * the result stays float32 in [0, 255], it is not rounded back to uint8;
  * the stored K of a perspective camera is shifted by the ROI origin, like a
    fisheye camera's (the reference crops the image and keeps K);
  * the camera type is chosen per camera (the reference applies the last
    camera's type to all).
Camera models 6-10 are parsed; `Camera.distortion()` raises for them.
"""

import os
import struct
from typing import Dict, List, Optional

import numpy as np

# model id -> (name, number of parameters)  (COLMAP's camera models)
CAMERA_MODELS = {
    0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5),
    4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5),
    8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12),
}
MODEL_IDS = {name: i for i, (name, _) in CAMERA_MODELS.items()}


class Camera:
    def __init__(self, camera_id, model, width, height, params):
        self.id, self.model = int(camera_id), str(model)
        self.width, self.height = int(width), int(height)
        self.params = np.asarray(params, dtype=np.float64)

    def intrinsics(self):
        """(fx, fy, cx, cy) as pycolmap's Camera exposes them."""
        p, m = self.params, self.model
        if m in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE",
                 "RADIAL_FISHEYE", "FOV"):
            return p[0], p[0], p[1], p[2]
        return p[0], p[1], p[2], p[3]

    def distortion(self):
        """[k1, k2, p1|k3, p2|k4] as colmap.py:111-129 builds them; empty for
        pinhole cameras."""
        p, m = self.params, self.model
        if m in ("SIMPLE_PINHOLE", "PINHOLE"):
            return np.empty(0, np.float32)
        if m == "SIMPLE_RADIAL":
            return np.array([p[3], 0, 0, 0], np.float32)
        if m == "RADIAL":
            return np.array([p[3], p[4], 0, 0], np.float32)
        if m in ("OPENCV", "OPENCV_FISHEYE"):
            return np.array(p[4:8], np.float32)
        raise NotImplementedError(f"camera model {m} (colmap.py:111-133 supports models 0-5)")


class Image:
    def __init__(self, image_id, qvec, tvec, camera_id, name, xys, point3D_ids):
        self.id, self.camera_id, self.name = int(image_id), int(camera_id), str(name)
        self.qvec = np.asarray(qvec, np.float64)  # (w, x, y, z), world -> camera
        self.tvec = np.asarray(tvec, np.float64)
        self.xys = np.asarray(xys, np.float64).reshape(-1, 2)
        self.point3D_ids = np.asarray(point3D_ids, np.int64)

    def R(self):
        w, x, y, z = self.qvec
        return np.array([
            [1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
            [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
            [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


class Point3D:
    def __init__(self, point_id, xyz, rgb, error, image_ids, point2D_idxs):
        self.id = int(point_id)
        self.xyz = np.asarray(xyz, np.float64)
        self.rgb = np.asarray(rgb, np.uint8)
        self.error = float(error)
        self.image_ids = np.asarray(image_ids, np.int64)
        self.point2D_idxs = np.asarray(point2D_idxs, np.int64)


# ----------------------------------------------------------------- readers
def _read(f, fmt):
    n = struct.calcsize(fmt)
    return struct.unpack(fmt, f.read(n))


def _read_cameras_bin(path):
    cams = {}
    with open(path, "rb") as f:
        (n,) = _read(f, "<Q")
        for _ in range(n):
            cid, mid, w, h = _read(f, "<iiQQ")
            name, npar = CAMERA_MODELS[mid]
            cams[cid] = Camera(cid, name, w, h, _read(f, "<" + "d" * npar))
    return cams


def _read_images_bin(path):
    ims = {}
    with open(path, "rb") as f:
        (n,) = _read(f, "<Q")
        for _ in range(n):
            iid, qw, qx, qy, qz, tx, ty, tz, cid = _read(f, "<idddddddi")
            name = b""
            while True:
                ch = f.read(1)
                if ch in (b"\x00", b""):
                    break
                name += ch
            (n2,) = _read(f, "<Q")
            data = np.frombuffer(f.read(24 * n2), dtype=np.dtype([("x", "<f8"), ("y", "<f8"),
                                                                  ("p", "<i8")]))
            ims[iid] = Image(iid, (qw, qx, qy, qz), (tx, ty, tz), cid, name.decode(),
                             np.stack([data["x"], data["y"]], -1), data["p"])
    return ims


def _read_points_bin(path):
    pts = {}
    with open(path, "rb") as f:
        (n,) = _read(f, "<Q")
        for _ in range(n):
            pid, x, y, z, r, g, b, err, tl = _read(f, "<QdddBBBdQ")
            track = np.frombuffer(f.read(8 * tl), dtype="<i4").reshape(-1, 2)
            pts[pid] = Point3D(pid, (x, y, z), (r, g, b), err, track[:, 0], track[:, 1])
    return pts


def _lines(path):
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line and not line.startswith("#"):
                yield line


def _read_cameras_txt(path):
    cams = {}
    for line in _lines(path):
        el = line.split()
        cid, model, w, h = int(el[0]), el[1], int(el[2]), int(el[3])
        cams[cid] = Camera(cid, model, w, h, [float(x) for x in el[4:]])
    return cams


def _read_images_txt(path):
    # two lines per image; the second (its 2D points) may be empty
    with open(path) as f:
        rows = [ln.rstrip("\n") for ln in f if not ln.startswith("#")]
    while rows and not rows[-1].strip() and len(rows) % 2:
        rows.pop()
    ims = {}
    for k in range(0, len(rows) - 1, 2):
        el = rows[k].split()
        if not el:
            continue
        iid = int(el[0])
        q = [float(x) for x in el[1:5]]
        t = [float(x) for x in el[5:8]]
        cid, name = int(el[8]), " ".join(el[9:])
        pts = rows[k + 1].split()
        xys = np.array([[float(pts[i]), float(pts[i + 1])] for i in range(0, len(pts), 3)])
        ids = np.array([int(pts[i + 2]) for i in range(0, len(pts), 3)], np.int64)
        ims[iid] = Image(iid, q, t, cid, name, xys.reshape(-1, 2), ids)
    return ims


def _read_points_txt(path):
    pts = {}
    for line in _lines(path):
        el = line.split()
        pid = int(el[0])
        track = np.array([int(x) for x in el[8:]], np.int64).reshape(-1, 2)
        pts[pid] = Point3D(pid, [float(x) for x in el[1:4]], [int(x) for x in el[4:7]],
                           float(el[7]), track[:, 0], track[:, 1])
    return pts


def read_model(path: str):
    """(cameras, images, points3D) dicts keyed by id, from `path`'s
    cameras/images/points3D .bin files (or .txt when no .bin exists)."""
    if os.path.exists(os.path.join(path, "cameras.bin")):
        return (_read_cameras_bin(os.path.join(path, "cameras.bin")),
                _read_images_bin(os.path.join(path, "images.bin")),
                _read_points_bin(os.path.join(path, "points3D.bin")))
    return (_read_cameras_txt(os.path.join(path, "cameras.txt")),
            _read_images_txt(os.path.join(path, "images.txt")),
            _read_points_txt(os.path.join(path, "points3D.txt")))


def write_model_bin(path: str, cameras, images, points3D):
    """COLMAP binary model writer (the inverse of read_model; tests and tools)."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cameras)))
        for c in cameras.values():
            f.write(struct.pack("<iiQQ", c.id, MODEL_IDS[c.model], c.width, c.height))
            f.write(struct.pack("<" + "d" * len(c.params), *c.params))
    with open(os.path.join(path, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(images)))
        for im in images.values():
            f.write(struct.pack("<idddddddi", im.id, *im.qvec, *im.tvec, im.camera_id))
            f.write(im.name.encode() + b"\x00")
            f.write(struct.pack("<Q", len(im.point3D_ids)))
            for (x, y), p in zip(im.xys, im.point3D_ids):
                f.write(struct.pack("<ddq", x, y, p))
    with open(os.path.join(path, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(points3D)))
        for p in points3D.values():
            f.write(struct.pack("<QdddBBBdQ", p.id, *p.xyz, *[int(v) for v in p.rgb], p.error,
                                len(p.image_ids)))
            for i, j in zip(p.image_ids, p.point2D_idxs):
                f.write(struct.pack("<ii", i, j))


# ----------------------------------------------------------- normalisation
def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def similarity_from_cameras(c2w, strict_scaling=False, center_method="focus"):
    """normalize.py:4-69 restated: rotate the world so the cameras' mean up
    direction (their -y axes) becomes (0, -1, 0), recentre on the median of
    the points nearest the origin along the cameras' optical axes ("focus")
    or on the median camera position ("poses"), and scale so the median (max
    with strict_scaling) camera distance is 1."""
    pos, rot = c2w[:, :3, 3], c2w[:, :3, :3]
    cam_up = np.array([0.0, -1.0, 0.0])
    up = (-rot[:, :, 1]).mean(axis=0)  # each camera's -y axis in world space
    up = up / np.linalg.norm(up)
    cos = float(cam_up @ up)
    if cos > -1:  # Rodrigues rotation taking `up` onto cam_up
        k = _skew(np.cross(up, cam_up))
        r_align = np.eye(3) + k + (k @ k) / (1 + cos)
    else:  # exactly opposite: half turn about x
        r_align = np.diag([-1.0, 1.0, 1.0])
    axes = (r_align @ rot)[:, :, 2]  # optical axes after the rotation
    pos = pos @ r_align.T
    if center_method == "focus":
        foot = pos - (axes * pos).sum(-1, keepdims=True) * axes
        shift = -np.median(foot, axis=0)
    elif center_method == "poses":
        shift = -np.median(pos, axis=0)
    else:
        raise ValueError(f"Unknown center_method {center_method}")
    dist = np.linalg.norm(pos + shift, axis=-1)
    scale = 1.0 / (dist.max() if strict_scaling else np.median(dist))
    out = np.eye(4)
    out[:3, :3] = r_align * scale
    out[:3, 3] = shift * scale
    return out


def align_principle_axes(point_cloud):
    """normalize.py:72-104 restated: a rigid transform to the median-centred
    principal axes of the points, the largest variance on x and the smallest
    on z, kept right-handed."""
    centre = np.median(point_cloud, axis=0)
    evals, evecs = np.linalg.eigh(np.cov(point_cloud - centre, rowvar=False))
    basis = evecs[:, np.argsort(evals)[::-1]]
    if np.linalg.det(basis) < 0:
        basis[:, 0] = -basis[:, 0]
    out = np.eye(4)
    out[:3, :3] = basis.T
    out[:3, 3] = -basis.T @ centre
    return out


def transform_points(matrix, points):
    """normalize.py:107-119: x -> A x + b for an affine 4x4."""
    assert matrix.shape == (4, 4) and points.ndim == 2 and points.shape[1] == 3
    return points @ matrix[:3, :3].T + matrix[:3, 3]


def transform_cameras(matrix, camtoworlds):
    """normalize.py:122-136: left-multiply every camera-to-world matrix by the
    similarity, then divide the scale back out of the rotation block."""
    assert matrix.shape == (4, 4) and camtoworlds.ndim == 3 and camtoworlds.shape[1:] == (4, 4)
    out = matrix[None] @ camtoworlds
    norm = np.linalg.norm(out[:, 0, :3], axis=1)
    out[:, :3, :3] /= norm[:, None, None]
    return out


def _rel_paths(d):
    out = []
    for dp, _, fn in os.walk(d):
        out += [os.path.relpath(os.path.join(dp, f), d) for f in fn]
    return out


# ------------------------------------------------------------ undistortion
def _k4(K):
    K = np.asarray(K, np.float64)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def _p4(params):
    p = np.asarray(params, np.float64).reshape(-1)
    assert p.size == 4, f"4 distortion parameters, got {p.size}"
    return p


def undistort_points(pts, K, params, iters=5):
    """OpenCV's undistortPoints for the radial-tangential model
    `params` = [k1, k2, p1, p2], without a new camera matrix: distorted pixels
    `pts` [N, 2] -> undistorted normalised coordinates [N, 2], float64.  The
    inverse is OpenCV's fixed-point iteration from x0 = (u - cx) / fx, `iters`
    rounds (OpenCV: 5), which does not converge to machine precision."""
    fx, fy, cx, cy = _k4(K)
    k1, k2, p1, p2 = _p4(params)
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    x0, y0 = (pts[:, 0] - cx) / fx, (pts[:, 1] - cy) / fy
    x, y = x0.copy(), y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icd = 1.0 / (1.0 + (k2 * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return np.stack([x, y], -1)


def _inner_rect(gx, gy):
    """The largest axis-aligned rectangle inside the image of a 9x9 pixel
    grid ([row, column] arrays): (x, y, w, h)."""
    left, right = gx[:, 0].max(), gx[:, -1].min()
    top, bottom = gy[0, :].max(), gy[-1, :].min()
    return left, top, right - left, bottom - top


def optimal_new_camera_matrix(K, params, size):
    """cv2.getOptimalNewCameraMatrix(K, params, (w, h), 0): alpha 0, the same
    output size, the principal point not centred.  Returns (K_undist [3, 3],
    roi (x, y, w, h)): the camera whose H x W frame shows only valid pixels
    of the undistorted image, and the rectangle of those pixels."""
    w, h = int(size[0]), int(size[1])
    gx, gy = np.meshgrid(np.arange(9) * (w - 1) / 8.0, np.arange(9) * (h - 1) / 8.0)
    n = undistort_points(np.stack([gx.ravel(), gy.ravel()], -1), K, params)
    nx, ny = n[:, 0].reshape(9, 9), n[:, 1].reshape(9, 9)
    ix, iy, iw, ih = _inner_rect(nx, ny)
    fx, fy = (w - 1) / iw, (h - 1) / ih
    cx, cy = -fx * ix, -fy * iy
    K_undist = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    rx, ry, rw, rh = _inner_rect(fx * nx + cx, fy * ny + cy)
    x0, y0 = int(np.ceil(rx)), int(np.ceil(ry))
    x1, y1 = x0 + int(np.floor(rw)), y0 + int(np.floor(rh))
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
    roi = (x0, y0, x1 - x0, y1 - y0) if x1 > x0 and y1 > y0 else (0, 0, 0, 0)
    return K_undist, roi


def undistort_maps(K, params, K_undist, size, camtype="perspective"):
    """mapx, mapy [h, w] float32: the source pixel of every pixel of the
    undistorted full frame, evaluated in float64 and stored as float32.
    "perspective": cv2.initUndistortRectifyMap(K, params, None, K_undist,
    (w, h), CV_32FC1), params = [k1, k2, p1, p2].  "fisheye": the reference's
    own formula (colmap.py:281-316), params = [k1, k2, k3, k4], K_undist = K,
    the map centred on (w // 2, h // 2)."""
    w, h = int(size[0]), int(size[1])
    fx, fy, cx, cy = _k4(K)
    nfx, nfy, ncx, ncy = _k4(K_undist)
    k = _p4(params)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x, y = (u - ncx) / nfx, (v - ncy) / nfy
    r2 = x * x + y * y
    if camtype == "perspective":
        kr = 1.0 + (k[1] * r2 + k[0]) * r2
        xy = x * y
        xd = x * kr + 2.0 * k[2] * xy + k[3] * (r2 + 2.0 * (x * x))
        yd = y * kr + k[2] * (r2 + 2.0 * (y * y)) + 2.0 * k[3] * xy
        mapx, mapy = fx * xd + cx, fy * yd + cy
    elif camtype == "fisheye":
        r4 = r2 * r2
        r = 1.0 + k[0] * r2 + k[1] * r4 + k[2] * (r4 * r2) + k[3] * (r4 * r4)
        mapx, mapy = fx * x * r + float(w // 2), fy * y * r + float(h // 2)
    else:
        raise ValueError(f"Unsupported camtype: {camtype!r}")
    return mapx.astype(np.float32), mapy.astype(np.float32)


def fisheye_roi(mapx, mapy, size):
    """colmap.py:304-316: the mask 0 < map < size - 1 (compared in float32),
    its bounding box as the ROI (x, y, w, h), and the mask cropped to it."""
    w, h = int(size[0]), int(size[1])
    mask = ((mapx > np.float32(0)) & (mapy > np.float32(0))
            & (mapx < np.float32(w - 1)) & (mapy < np.float32(h - 1)))
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        raise ValueError("fisheye undistortion: no pixel of the map lies inside the image")
    x0, x1, y0, y1 = int(xs.min()), int(xs.max()) + 1, int(ys.min()), int(ys.max()) + 1
    return (x0, y0, x1 - x0, y1 - y0), np.ascontiguousarray(mask[y0:y1, x0:x1])


def undistort_host(image_u8, mapx, mapy, roi):
    """numpy counterpart of the kernel (gsplat_hip.undistort): the bilinear
    remap of `image_u8` [H, W, C] through the full-frame maps with a constant
    0 border, cropped to `roi` (x, y, w, h): float32 [h, w, C] in [0, 255].
    Unlike cv2.remap(..., INTER_LINEAR) the weights are fp32 at the
    unquantised coordinate (cv2: 5-bit fixed point) and the result is not
    rounded back to uint8."""
    img = np.asarray(image_u8)
    assert img.ndim == 3 and img.dtype == np.uint8, (img.shape, img.dtype)
    H, W = img.shape[:2]
    x, y, w, h = (int(v) for v in roi)
    sx = np.asarray(mapx, np.float32)[y:y + h, x:x + w]
    sy = np.asarray(mapy, np.float32)[y:y + h, x:x + w]
    with np.errstate(invalid="ignore"):
        near = (sx > -1) & (sx < W) & (sy > -1) & (sy < H)  # false for NaN
    sx, sy = np.where(near, sx, np.float32(-1)), np.where(near, sy, np.float32(-1))
    x0f, y0f = np.floor(sx), np.floor(sy)
    wx, wy = sx - x0f, sy - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    one = np.float32(1)

    def tap(xi, yi, wgt):
        ok = near & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        px = img[np.where(ok, yi, 0), np.where(ok, xi, 0)].astype(np.float32)
        return np.where(ok, wgt, np.float32(0))[..., None] * px

    top = tap(x0, y0, (one - wx) * (one - wy)) + tap(x0 + 1, y0, wx * (one - wy))
    bot = tap(x0, y0 + 1, (one - wx) * wy) + tap(x0 + 1, y0 + 1, wx * wy)
    return np.ascontiguousarray(top + bot, dtype=np.float32)


# ------------------------------------------------------------------ parser
class Parser:
    """colmap.py:59-333 on read_model (no pycolmap, no OpenCV).

    For every camera with distortion parameters (models 2-5) the parser also
    holds, as the reference's does, `mapx_dict` / `mapy_dict` (full-frame
    float32 maps), `roi_undist_dict`, `mask_dict` (fisheye only), the
    undistorted K in `Ks_dict` and the ROI size in `imsize_dict`; the camera
    type is chosen per camera ("fisheye" for OPENCV_FISHEYE, "perspective"
    otherwise; the reference applies one type to every camera).  The stored K
    has its principal point shifted by the ROI origin, for perspective cameras
    too, so it is the K of the cropped image that Dataset returns (the
    reference crops a perspective image without shifting K).  `Ks_dist_dict`
    keeps the distorted camera's K and `Ks_new_dict` the undistorted K of the
    full frame, the two matrices the kernel takes.  Pinhole cameras have no
    entry in the map dicts and keep their K and size."""

    def __init__(self, data_dir: str, factor: int = 1, normalize: bool = False,
                 test_every: int = 8):
        self.data_dir, self.factor = data_dir, factor
        self.normalize, self.test_every = normalize, test_every
        colmap_dir = os.path.join(data_dir, "sparse/0/")
        if not os.path.exists(colmap_dir):
            colmap_dir = os.path.join(data_dir, "sparse")
        assert os.path.exists(colmap_dir), f"COLMAP directory {colmap_dir} does not exist."
        cameras, images, points3D = read_model(colmap_dir)
        if len(images) == 0:
            raise ValueError("No images found in COLMAP.")

        bottom = np.array([0, 0, 0, 1.0]).reshape(1, 4)
        w2c, camera_ids, names = [], [], []
        Ks, params, imsize, masks = {}, {}, {}, {}
        for k in images:  # the model's order, then sorted by name below
            im = images[k]
            w2c.append(np.concatenate([np.concatenate([im.R(), im.tvec.reshape(3, 1)], 1),
                                       bottom], 0))
            camera_ids.append(im.camera_id)
            names.append(im.name)
            cam = cameras[im.camera_id]
            fx, fy, cx, cy = cam.intrinsics()
            K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
            K[:2, :] /= factor
            Ks[im.camera_id] = K
            params[im.camera_id] = cam.distortion()
            imsize[im.camera_id] = (cam.width // factor, cam.height // factor)
            masks[im.camera_id] = None
        camtoworlds = np.linalg.inv(np.stack(w2c, 0))
        inds = np.argsort(names)
        names = [names[i] for i in inds]
        camtoworlds = camtoworlds[inds]
        camera_ids = [camera_ids[i] for i in inds]

        # images (the `images_<factor>` folder mapped to COLMAP's by sorted order)
        suffix = f"_{factor}" if factor > 1 else ""
        colmap_image_dir = os.path.join(data_dir, "images")
        image_dir = os.path.join(data_dir, "images" + suffix)
        self.image_paths = []
        if os.path.exists(image_dir) and os.path.exists(colmap_image_dir):
            mapping = dict(zip(sorted(_rel_paths(colmap_image_dir)),
                               sorted(_rel_paths(image_dir))))
            self.image_paths = [os.path.join(image_dir, mapping[n]) for n in names]

        ordered = sorted(points3D)
        idx_of = {pid: i for i, pid in enumerate(ordered)}
        points = np.array([points3D[p].xyz for p in ordered], np.float32).reshape(-1, 3)
        points_err = np.array([points3D[p].error for p in ordered], np.float32)
        points_rgb = np.array([points3D[p].rgb for p in ordered], np.uint8).reshape(-1, 3)
        name_of = {im.id: im.name for im in images.values()}
        point_indices: Dict[str, List[int]] = {}
        for p in ordered:
            for iid in points3D[p].image_ids:
                point_indices.setdefault(name_of[int(iid)], []).append(idx_of[p])
        self.point_indices = {k: np.array(v, np.int32) for k, v in point_indices.items()}

        if normalize:
            T1 = similarity_from_cameras(camtoworlds)
            camtoworlds = transform_cameras(T1, camtoworlds)
            points = transform_points(T1, points)
            T2 = align_principle_axes(points)
            camtoworlds = transform_cameras(T2, camtoworlds)
            points = transform_points(T2, points)
            transform = T2 @ T1
        else:
            transform = np.eye(4)

        self.image_names, self.camtoworlds, self.camera_ids = names, camtoworlds, camera_ids
        self.Ks_dict, self.params_dict, self.imsize_dict = Ks, params, imsize
        self.mask_dict = masks
        self.points, self.points_err, self.points_rgb = points, points_err, points_rgb
        self.transform = transform

        # actual image size vs COLMAP's (colmap.py:237-247)
        if self.image_paths:
            from PIL import Image as PILImage
            with PILImage.open(self.image_paths[0]) as img:
                aw, ah = img.size
            cw, ch = self.imsize_dict[self.camera_ids[0]]
            sw, sh = aw / cw, ah / ch
            for cid, K in self.Ks_dict.items():
                K[0, :] *= sw
                K[1, :] *= sh
                w, h = self.imsize_dict[cid]
                self.imsize_dict[cid] = (int(w * sw), int(h * sh))

        # undistortion (colmap.py:258-325), the camera type per camera
        self.mapx_dict, self.mapy_dict, self.roi_undist_dict = {}, {}, {}
        self.camtype_dict, self.Ks_dist_dict, self.Ks_new_dict = {}, {}, {}
        for cid, par in self.params_dict.items():
            if len(par) == 0:
                continue  # no distortion
            K, size = self.Ks_dict[cid], self.imsize_dict[cid]
            camtype = "fisheye" if cameras[cid].model == "OPENCV_FISHEYE" else "perspective"
            if camtype == "perspective":
                K_new, roi = optimal_new_camera_matrix(K, par, size)
                mapx, mapy = undistort_maps(K, par, K_new, size, camtype)
                mask = None
            else:
                K_new = K.copy()
                mapx, mapy = undistort_maps(K, par, K_new, size, camtype)
                roi, mask = fisheye_roi(mapx, mapy, size)
            if roi[2] <= 0 or roi[3] <= 0:
                raise ValueError(f"camera {cid}: the undistorted image has no valid pixel")
            K_undist = K_new.copy()
            K_undist[0, 2] -= roi[0]
            K_undist[1, 2] -= roi[1]
            self.camtype_dict[cid] = camtype
            self.Ks_dist_dict[cid], self.Ks_new_dict[cid] = K, K_new
            self.mapx_dict[cid], self.mapy_dict[cid] = mapx, mapy
            self.roi_undist_dict[cid] = roi
            self.Ks_dict[cid] = K_undist
            self.imsize_dict[cid] = (roi[2], roi[3])
            self.mask_dict[cid] = mask

        locs = camtoworlds[:, :3, 3]
        self.scene_scale = float(np.max(np.linalg.norm(locs - locs.mean(0), axis=1)))


class Dataset:
    """colmap.py:336-440: every `test_every`-th image is a test image.
    `load_depths` (colmap.py:342-347, 394-415): items also hold the image's
    SfM points projected into it, "points" [M, 2] (pixels) and "depths" [M]
    (camera z) -- Trainer(depth_points=...)'s input.
    An image of a distorted camera is undistorted and cropped to the ROI
    (colmap.py:366-374): float32 in [0, 255], not rounded back to uint8, with
    the undistorted K; `patch_size` and `load_depths` work on that image and K.
    A fisheye camera's items also hold "mask" (the ROI-sized validity mask).
    `device`: a cuda device undistorts with the kernel (gsplat_hip.undistort)
    and returns "image" on that device; None is the numpy path."""

    def __init__(self, parser: Parser, split: str = "train", patch_size: Optional[int] = None,
                 load_depths: bool = False, device=None):
        self.parser, self.split, self.patch_size = parser, split, patch_size
        self.load_depths = bool(load_depths)
        self.device = device
        idx = np.arange(len(parser.image_names))
        self.indices = idx[idx % parser.test_every != 0] if split == "train" else \
            idx[idx % parser.test_every == 0]

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, item: int):
        import torch
        from PIL import Image as PILImage
        index = self.indices[item]
        cid = self.parser.camera_ids[index]
        P = self.parser
        with PILImage.open(P.image_paths[index]) as img:
            image = np.array(img.convert("RGB"))
        on_gpu = self.device is not None and torch.device(self.device).type == "cuda"
        if on_gpu:
            image = torch.from_numpy(image).to(self.device)
        K = P.Ks_dict[cid].copy()  # the undistorted K of the ROI-sized image
        if len(P.params_dict[cid]) > 0:
            # colmap.py:366-374: remap, then crop to the ROI
            if on_gpu:
                from .undistort import undistort_images
                image = undistort_images(image[None], P.Ks_dist_dict[cid], P.params_dict[cid],
                                         P.Ks_new_dict[cid], P.roi_undist_dict[cid],
                                         P.camtype_dict[cid])[0]
            else:
                image = undistort_host(image, P.mapx_dict[cid], P.mapy_dict[cid],
                                       P.roi_undist_dict[cid])
        if self.patch_size is not None:
            h, w = image.shape[:2]
            x = np.random.randint(0, max(w - self.patch_size, 1))
            y = np.random.randint(0, max(h - self.patch_size, 1))
            image = image[y:y + self.patch_size, x:x + self.patch_size]
            K[0, 2] -= x
            K[1, 2] -= y
        camtoworld = P.camtoworlds[index]
        if not on_gpu:
            image = torch.from_numpy(np.ascontiguousarray(image))
        data = {"K": torch.from_numpy(K).float(),
                "camtoworld": torch.from_numpy(camtoworld).float(),
                "image": image.float().contiguous(),
                "image_id": item}
        if P.mask_dict[cid] is not None:
            data["mask"] = torch.from_numpy(P.mask_dict[cid]).bool()
        if self.load_depths:
            points, depths = _depth_points(P, index, K, image.shape[1], image.shape[0])
            data["points"] = torch.from_numpy(points).float().reshape(-1, 2)
            data["depths"] = torch.from_numpy(depths).float()
        return data


def _depth_points(parser, index, K, width, height):
    """The image's SfM points in its camera frame, projected with the
    (undistorted, crop-shifted) K; kept inside the image and in front of the
    camera (colmap.py:394-415)."""
    w2c = np.linalg.inv(parser.camtoworlds[index])
    ids = parser.point_indices.get(parser.image_names[index], np.zeros(0, np.int32))
    cam = (w2c[:3, :3] @ parser.points[ids].T + w2c[:3, 3:4]).T
    proj = (K @ cam.T).T
    with np.errstate(divide="ignore", invalid="ignore"):
        points = proj[:, :2] / proj[:, 2:3]
    depths = cam[:, 2]
    keep = ((points[:, 0] >= 0) & (points[:, 0] < width) & (points[:, 1] >= 0)
            & (points[:, 1] < height) & (depths > 0))
    return points[keep], depths[keep]


def scene_tensors(parser: Parser, split: str = "train", device="cuda", load_depths: bool = False,
                  batch: int = 8):
    """A parsed scene as the tensors `Trainer` takes (the reference trainer's
    Parser -> Dataset -> DataLoader path, done once): the split's images are
    decoded on the host, uploaded as uint8 and undistorted on the device
    (gsplat_hip.undistort), `batch` images of one camera at a time, straight
    into the `targets` table.  Returns a dict:

        viewmats [n, 4, 4], Ks [n, 3, 3]   world-to-camera, undistorted K
        targets [n, h, w, 3]               float32 in [0, 1], on `device`
        width, height                      the images' (undistorted) size
        masks [n, h, w] bool or None       fisheye validity masks (all true for
                                           the other cameras): what
                                           `Trainer(masks=...)` takes
        depth_points                       with `load_depths`: one (points
                                           [M, 2], depths [M]) per image
        points [N, 3], rgbs [N, 3]         the SfM points, colours in [0, 1]
        scene_scale

    so that `Trainer(t.pop("points"), t.pop("rgbs"), **t)` trains on the scene,
    the render zeroed outside each image's mask before the loss.  `Trainer` has
    one width and height: images that do not all end at one size raise
    ValueError."""
    import torch
    from PIL import Image as PILImage
    from .undistort import undistort_images
    ds = Dataset(parser, split)
    idx = [int(i) for i in ds.indices]
    if not idx:
        raise ValueError(f"scene_tensors: the {split!r} split is empty")
    cids = [parser.camera_ids[i] for i in idx]
    sizes = sorted({parser.imsize_dict[c] for c in cids})
    if len(sizes) != 1:
        raise ValueError("scene_tensors: Trainer has one width and height, the split's images "
                         f"end at {sizes} (after undistortion)")
    w, h = sizes[0]
    n = len(idx)
    targets = torch.empty((n, h, w, 3), dtype=torch.float32, device=device)
    k = 0
    while k < n:  # runs of consecutive images of one camera, at most `batch` long
        e = k + 1
        while e < n and e - k < batch and cids[e] == cids[k]:
            e += 1
        frames = []
        for i in idx[k:e]:
            with PILImage.open(parser.image_paths[i]) as img:
                frames.append(np.array(img.convert("RGB")))
        if len({f.shape for f in frames}) != 1:
            raise ValueError(f"scene_tensors: images of camera {cids[k]} differ in size")
        u8 = torch.from_numpy(np.stack(frames)).to(device)
        c = cids[k]
        if len(parser.params_dict[c]) > 0:
            undistort_images(u8, parser.Ks_dist_dict[c], parser.params_dict[c],
                             parser.Ks_new_dict[c], parser.roi_undist_dict[c],
                             parser.camtype_dict[c], scale=1.0 / 255.0, out=targets[k:e])
        else:
            # a pinhole camera: the identity map of the same kernel (integer
            # source coordinates, weights 0 and 1: the exact uint8 -> float scaling)
            if tuple(u8.shape[1:3]) != (h, w):
                raise ValueError(f"scene_tensors: camera {c}'s images are "
                                 f"{u8.shape[2]}x{u8.shape[1]}, the parser says {w}x{h}")
            undistort_images(u8, parser.Ks_dict[c], [0.0] * 4, parser.Ks_dict[c], (0, 0, w, h),
                             "perspective", scale=1.0 / 255.0, out=targets[k:e])
        k = e
    masks = None
    if any(parser.mask_dict[c] is not None for c in cids):
        masks = torch.ones((n, h, w), dtype=torch.bool)
        for j, c in enumerate(cids):
            if parser.mask_dict[c] is not None:
                masks[j] = torch.from_numpy(parser.mask_dict[c])
        masks = masks.to(device)
    c2w = parser.camtoworlds[idx]
    out = {"viewmats": torch.from_numpy(np.linalg.inv(c2w)).float(),
           "Ks": torch.from_numpy(np.stack([parser.Ks_dict[c] for c in cids])).float(),
           "targets": targets, "width": int(w), "height": int(h), "masks": masks,
           "points": torch.from_numpy(parser.points).float(),
           "rgbs": torch.from_numpy(parser.points_rgb.astype(np.float32) / 255.0),
           "scene_scale": float(parser.scene_scale)}
    if load_depths:
        dp = []
        for i, c in zip(idx, cids):
            p, d = _depth_points(parser, i, parser.Ks_dict[c], w, h)
            dp.append((torch.from_numpy(p).float().reshape(-1, 2), torch.from_numpy(d).float()))
        out["depth_points"] = dp
    return out
