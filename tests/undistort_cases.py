"""Cases and an independent float64 oracle for image undistortion
(tests/test_undistort_host.py on the CPU, tests/test_gpu_undistort.py on the
GPU).  A helper, not a conftest: no tests, and nothing of the HIP package is
imported here.  The geometry below (new camera matrix, ROI, fisheye mask, the
per-pixel map, the bilinear remap) is written on its own, with scalar loops
where gsplat_hip.colmap is vectorised, so the two check each other.

Every case is non-square with an off-centre principal point and a width that
is no multiple of 4.  P4 is a strip whose fp32 source coordinates reach 4000.
The images are smooth: channel c of image b is

    g(x, y) = 127.5 + 100 sin(wx x + phase) cos(wy y + phase')

with its own (wx, wy) <= 0.21 rad/px per channel, rounded to uint8.  A smooth
image makes the result a differentiable function of the source coordinate, so
a coordinate error of e px costs at most 100 * 0.21 * sqrt(2) * e levels, and
the bilinear blend of the samples is within A (wx^2 + wy^2) / 8 of g itself.
"""

import functools
import math
from types import SimpleNamespace

import numpy as np

AMP = 100.0
FREQS = ((0.21, 0.17), (0.13, 0.19), (0.20, 0.11))  # (wx, wy) per channel, rad/px

#        name   model             (W, H)      (fx, fy, cx, cy)            params
_CASES = [
    ("P1", "SIMPLE_RADIAL", (97, 61), (80.0, 80.0, 47.3, 31.1), (-0.12, 0.0, 0.0, 0.0)),
    ("P2", "RADIAL", (97, 61), (80.0, 80.0, 47.3, 31.1), (0.08, 0.02, 0.0, 0.0)),
    ("P3", "OPENCV", (97, 61), (82.0, 79.0, 50.0, 29.0), (-0.15, 0.03, 0.004, -0.003)),
    ("P4", "OPENCV", (4000, 24), (3000.0, 2990.0, 2010.0, 12.0), (-0.15, 0.03, 0.004, -0.003)),
    ("F1", "OPENCV_FISHEYE", (97, 61), (60.0, 60.0, 47.3, 31.1), (0.05, 0.01, 0.002, 0.0005)),
    ("F2", "OPENCV_FISHEYE", (97, 61), (60.0, 60.0, 47.3, 31.1), (0.3, 0.1, 0.02, 0.005)),
]
CASES = {n: SimpleNamespace(name=n, model=m, size=s, K=k, params=p,
                            camtype="fisheye" if m == "OPENCV_FISHEYE" else "perspective")
         for n, m, s, k, p in _CASES}
PERSPECTIVE = ("P1", "P2", "P3", "P4")
FISHEYE = ("F1", "F2")
ALL = PERSPECTIVE + FISHEYE


def colmap_params(case):
    """The case as a COLMAP camera's parameter list."""
    fx, fy, cx, cy = case.K
    k = case.params
    return {"SIMPLE_RADIAL": [fx, cx, cy, k[0]], "RADIAL": [fx, cx, cy, k[0], k[1]],
            "OPENCV": [fx, fy, cx, cy, *k], "OPENCV_FISHEYE": [fx, fy, cx, cy, *k]}[case.model]


def K3(k4):
    fx, fy, cx, cy = k4
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


# ------------------------------------------------------------------ images
def pattern(c, b, x, y):
    """g of channel c, image b, at (x, y) (arrays or scalars), float64."""
    wx, wy = FREQS[c]
    return 127.5 + AMP * np.sin(wx * x + 0.3 + 0.9 * c + 0.7 * b) * np.cos(wy * y + 0.5 * c - 0.4 * b)


def interp_bound(c):
    """|bilinear blend of the uint8 samples - g|: the uint8 rounding of the
    samples (0.5, a convex combination keeps it) plus the bilinear
    interpolation error of a C2 function on a unit cell,
    (max |g_xx| + max |g_yy|) / 8 = A (wx^2 + wy^2) / 8."""
    wx, wy = FREQS[c]
    return 0.5 + AMP * (wx * wx + wy * wy) / 8.0


@functools.lru_cache(maxsize=None)
def images(name, B=2):
    """[B, H, W, 3] uint8, read-only."""
    W, H = CASES[name].size
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    img = np.stack([np.stack([pattern(c, b, x, y) for c in range(3)], -1) for b in range(B)])
    img = np.rint(img).astype(np.uint8)
    img.setflags(write=False)
    return img


# ---------------------------------------------------------------- geometry
def _undistort_point(u, v, K, k, iters=5):
    fx, fy, cx, cy = K
    k1, k2, p1, p2 = k
    x0, y0 = (u - cx) / fx, (v - cy) / fy
    x, y = x0, y0
    for _ in range(iters):
        r2 = x * x + y * y
        icd = 1.0 / (1.0 + (k2 * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return x, y


def _inner(pts):
    """pts[j][i] = (x, y) of grid row j, column i -> (x, y, w, h)."""
    left = max(pts[j][0][0] for j in range(9))
    right = min(pts[j][8][0] for j in range(9))
    top = max(pts[0][i][1] for i in range(9))
    bottom = min(pts[8][i][1] for i in range(9))
    return left, top, right - left, bottom - top


def _new_camera(case):
    """getOptimalNewCameraMatrix at alpha 0 on a 9x9 grid: ((fx', fy', cx', cy'), roi)."""
    W, H = case.size
    n = [[_undistort_point(i * (W - 1) / 8.0, j * (H - 1) / 8.0, case.K, case.params)
          for i in range(9)] for j in range(9)]
    ix, iy, iw, ih = _inner(n)
    fx, fy = (W - 1) / iw, (H - 1) / ih
    cx, cy = -fx * ix, -fy * iy
    rx, ry, rw, rh = _inner([[(fx * x + cx, fy * y + cy) for x, y in row] for row in n])
    x0, y0 = math.ceil(rx), math.ceil(ry)
    x1, y1 = min(x0 + math.floor(rw), W), min(y0 + math.floor(rh), H)
    x0, y0 = max(x0, 0), max(y0, 0)
    return (fx, fy, cx, cy), (x0, y0, x1 - x0, y1 - y0)


def source_coords(case, K_new, roi, dtype):
    """The source pixel (sx, sy) of every ROI pixel, every operation in
    `dtype`: float64 is the oracle's map, float32 the restatement whose error
    is the bar."""
    f = dtype
    W, H = case.size
    fx, fy, cx, cy = (f(v) for v in case.K)
    nfx, nfy, ncx, ncy = (f(v) for v in K_new)
    k = [f(v) for v in case.params]
    rx, ry, w, h = roi
    u, v = np.meshgrid(np.arange(rx, rx + w).astype(f), np.arange(ry, ry + h).astype(f))
    x, y = (u - ncx) / nfx, (v - ncy) / nfy
    r2 = x * x + y * y
    if case.camtype == "perspective":
        kr = f(1) + (k[1] * r2 + k[0]) * r2
        xd = x * kr + f(2) * k[2] * x * y + k[3] * (r2 + f(2) * x * x)
        yd = y * kr + k[2] * (r2 + f(2) * y * y) + f(2) * k[3] * x * y
        sx, sy = fx * xd + cx, fy * yd + cy
    else:
        th = np.sqrt(r2)
        r = f(1) + k[0] * th ** 2 + k[1] * th ** 4 + k[2] * th ** 6 + k[3] * th ** 8
        sx, sy = fx * x * r + f(W // 2), fy * y * r + f(H // 2)
    assert sx.dtype == np.dtype(f)
    return sx, sy


@functools.lru_cache(maxsize=None)
def geometry(name):
    """K_new (the undistorted camera of the full frame), roi (x, y, w, h),
    K_undist (K_new shifted by the ROI origin), mask (fisheye) and the
    float64 map of the ROI's pixels."""
    case = CASES[name]
    W, H = case.size
    if case.camtype == "perspective":
        K_new, roi = _new_camera(case)
        mask = None
    else:
        K_new = case.K
        fx, fy = source_coords(case, K_new, (0, 0, W, H), np.float64)
        fx, fy = fx.astype(np.float32), fy.astype(np.float32)
        inside = np.zeros((H, W), bool)
        for v in range(H):
            for u in range(W):
                inside[v, u] = 0 < fx[v, u] < np.float32(W - 1) and 0 < fy[v, u] < np.float32(H - 1)
        cols, rows = np.nonzero(inside.any(0))[0], np.nonzero(inside.any(1))[0]
        roi = (int(cols[0]), int(rows[0]), int(cols[-1] - cols[0] + 1), int(rows[-1] - rows[0] + 1))
        mask = inside[roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]].copy()
    sx, sy = source_coords(case, K_new, roi, np.float64)
    for a in (sx, sy):
        a.setflags(write=False)
    K_undist = (K_new[0], K_new[1], K_new[2] - roi[0], K_new[3] - roi[1])
    return SimpleNamespace(K_new=K_new, roi=roi, K_undist=K_undist, mask=mask, sx=sx, sy=sy)


# ------------------------------------------------------------------- remap
def remap(imgs, sx, sy, dtype=np.float64):
    """Bilinear remap with a constant 0 border: imgs [B, H, W, 3] uint8 and
    coordinates [h, w] -> [B, h, w, 3] in `dtype`.  A coordinate that is not
    finite, or whose four neighbours all lie outside, gives 0."""
    f = dtype
    B, H, W, _ = imgs.shape
    sx, sy = np.asarray(sx, f), np.asarray(sy, f)
    fin = np.isfinite(sx) & np.isfinite(sy)
    sx = np.clip(np.where(fin, sx, f(-8)), f(-8), f(W + 8))
    sy = np.clip(np.where(fin, sy, f(-8)), f(-8), f(H + 8))
    x0, y0 = np.floor(sx), np.floor(sy)
    wx, wy = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    out = np.zeros((B,) + sx.shape + (3,), f)
    for dy, dx, wgt in ((0, 0, (f(1) - wx) * (f(1) - wy)), (0, 1, wx * (f(1) - wy)),
                        (1, 0, (f(1) - wx) * wy), (1, 1, wx * wy)):
        xi, yi = x0 + dx, y0 + dy
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        px = imgs[:, np.where(ok, yi, 0), np.where(ok, xi, 0)].astype(f)
        out += (np.where(ok, wgt, f(0))[None, ..., None] * px).astype(f)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, B=2):
    """The float64 truth at scale 1: [B, h, w, 3], read-only."""
    g = geometry(name)
    out = remap(images(name, B), g.sx, g.sy, np.float64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bar(name, B=2):
    """The bar at scale 1 (levels): the maximum error against the oracle of
    the same computation with the map and the blend evaluated in float32."""
    case, g = CASES[name], geometry(name)
    sx, sy = source_coords(case, g.K_new, g.roi, np.float32)
    return float(np.abs(remap(images(name, B), sx, sy, np.float32).astype(np.float64)
                        - oracle(name, B)).max())


def bound(name, scale, B=2):
    """max(4 x bar, 1e-6 of the value range) at `scale`."""
    return max(4.0 * bar(name, B) * scale, 1e-6 * 255.0 * scale)
