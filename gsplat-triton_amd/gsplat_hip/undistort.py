"""Image undistortion on the device, backed by libgsplat_hip.so
(csrc/undistort.hip): what the reference's dataset does per image with
`cv2.remap(image, mapx, mapy, cv2.INTER_LINEAR)` and the ROI crop
(examples/datasets/colmap.py:366-374), for a batch of uint8 images that share
one camera.

    undistort_images   the map is evaluated in the kernel from the camera
                       (K, the four distortion parameters, the undistorted K)
    remap_bilinear     the map is given as mapx / mapy tensors

Both return float32 [B, h, w, 3] = scale * the bilinear blend, with a constant
0 border.  They differ from cv2.remap in two documented ways: the weights are
fp32 at the unquantised coordinate (cv2 quantises to 1/32 px), and the result
is not rounded back to uint8.  Images are data: there is no autograd.  Every
launch goes on torch's current stream; there is no CPU or torch fallback.
"""

from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _lib
from ._wrapper import _dev_check, _ptr, _stream

CAMTYPES = {"perspective": 0, "fisheye": 1}


def _err(msg):
    raise _lib.GsplatHipError(msg)


def _check_images(name, images):
    if not isinstance(images, Tensor) or images.dim() != 4 or images.shape[-1] != 3:
        _err(f"{name}: images must be a [B, H, W, 3] tensor, got "
             f"{tuple(images.shape) if isinstance(images, Tensor) else type(images).__name__}")
    if images.dtype != torch.uint8:
        _err(f"{name}: images must be uint8, got {images.dtype}")
    if not images.is_contiguous():
        _err(f"{name}: images must be contiguous")


def _check_out(name, out, shape, like):
    if out is None:
        return
    if not isinstance(out, Tensor) or tuple(out.shape) != tuple(shape):
        _err(f"{name}: out must have the result's shape {tuple(shape)}, got "
             f"{tuple(out.shape) if isinstance(out, Tensor) else type(out).__name__}")
    if out.dtype != torch.float32 or not out.is_contiguous():
        _err(f"{name}: out must be a contiguous float32 tensor")
    if out.device != like.device:
        _err(f"{name}: out is on {out.device}, the images on {like.device}")


def _result(out, shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device) if out is None else out


def _k4(name, what, K):
    """(fx, fy, cx, cy) as Python floats from a 3x3 matrix or four numbers
    (host values: a device tensor would cost a synchronisation)."""
    if isinstance(K, Tensor):
        if K.is_cuda:
            _err(f"{name}: {what} is read on the host; pass a CPU tensor, an array or numbers")
        K = K.tolist()
    elif hasattr(K, "tolist"):
        K = K.tolist()
    K = list(K)
    if len(K) == 3 and all(hasattr(r, "__len__") and len(r) == 3 for r in K):
        return float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    if len(K) == 4 and not any(hasattr(v, "__len__") for v in K):
        return tuple(float(v) for v in K)
    _err(f"{name}: {what} must be a 3x3 matrix or (fx, fy, cx, cy)")


def undistort_images(images: Tensor, K, params: Sequence[float], K_undist, roi: Sequence[int],
                     camtype: str = "perspective", scale: float = 1.0,
                     out: Optional[Tensor] = None) -> Tensor:
    """Undistorts `images` [B, H, W, 3] (uint8, contiguous, on the GPU), all
    taken by one camera, into float32 [B, h, w, 3].

    K:         the distorted camera, 3x3 or (fx, fy, cx, cy), host values
    params:    [k1, k2, p1, p2] ("perspective") or [k1, k2, k3, k4] ("fisheye")
    K_undist:  the undistorted camera of the full H x W frame, before the ROI
               crop: `optimal_new_camera_matrix`'s first result, or K for a
               fisheye camera (Parser.Ks_new_dict)
    roi:       (x, y, w, h): the result is the full undistorted frame cropped
               to this rectangle (Parser.roi_undist_dict)
    scale:     multiplies the result (1 / 255 for images in [0, 1])
    out:       optionally the contiguous float32 [B, h, w, 3] tensor to write,
               e.g. a slice `targets[i:i + B]`

    The source coordinate of each output pixel is evaluated in the kernel in
    float64 and rounded to float32, as `colmap.undistort_maps` stores it."""
    name = "undistort_images"
    if camtype not in CAMTYPES:
        raise ValueError(f"Unsupported camtype: {camtype!r} (one of {sorted(CAMTYPES)})")
    _check_images(name, images)
    fx, fy, cx, cy = _k4(name, "K", K)
    nfx, nfy, ncx, ncy = _k4(name, "K_undist", K_undist)
    k = [float(v) for v in (params.tolist() if hasattr(params, "tolist") else params)]
    if len(k) != 4:
        _err(f"{name}: params must hold 4 values, got {len(k)}")
    r = [int(v) for v in roi]
    if len(r) != 4 or r[2] < 0 or r[3] < 0:
        _err(f"{name}: roi must be (x, y, w, h) with w, h >= 0, got {tuple(roi)!r}")
    B, H, W, _ = images.shape
    _check_out(name, out, (B, r[3], r[2], 3), images)
    _dev_check(images, out)  # after every shape and dtype check, before any device work
    out = _result(out, (B, r[3], r[2], 3), images)
    with torch.cuda.device(images.device):
        _lib.call("gsplat_hip_undistort_u8_f32", B, H, W, _ptr(images), fx, fy, cx, cy, *k,
                  nfx, nfy, ncx, ncy, r[0], r[1], r[2], r[3], CAMTYPES[camtype], float(scale),
                  _ptr(out), _stream())
    return out


def remap_bilinear(images: Tensor, mapx: Tensor, mapy: Tensor, scale: float = 1.0,
                   out: Optional[Tensor] = None) -> Tensor:
    """`cv2.remap(image, mapx, mapy, cv2.INTER_LINEAR)` with a constant 0
    border for `images` [B, H, W, 3] (uint8) and maps [h, w] (float32), all
    contiguous and on the GPU: float32 [B, h, w, 3], out[b, v, u] = scale * the
    blend of images[b] at (mapx[v, u], mapy[v, u]).  `out` as in
    `undistort_images`."""
    name = "remap_bilinear"
    _check_images(name, images)
    for what, m in (("mapx", mapx), ("mapy", mapy)):
        if not isinstance(m, Tensor) or m.dim() != 2:
            _err(f"{name}: {what} must be a [h, w] tensor")
        if m.dtype != torch.float32 or not m.is_contiguous():
            _err(f"{name}: {what} must be a contiguous float32 tensor")
    if mapx.shape != mapy.shape:
        _err(f"{name}: mapx {tuple(mapx.shape)} and mapy {tuple(mapy.shape)} differ")
    if mapx.device != images.device or mapy.device != images.device:
        _err(f"{name}: the maps and the images are on different devices")
    B, H, W, _ = images.shape
    h, w = mapx.shape
    _check_out(name, out, (B, h, w, 3), images)
    _dev_check(images, mapx, mapy, out)
    out = _result(out, (B, h, w, 3), images)
    with torch.cuda.device(images.device):
        _lib.call("gsplat_hip_remap_u8_f32", B, H, W, _ptr(images), _ptr(mapx), _ptr(mapy), w, h,
                  float(scale), _ptr(out), _stream())
    return out
