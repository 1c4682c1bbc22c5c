"""The projection stage for Gaussians given by covariances, backed by
libgsplat_hip.so (csrc/projection_covar.hip):

    fully_fused_projection(covars=[N,6])   gsplat/cuda/_wrapper.py:209-345
                                           (dense :780-905, packed :998-1190)
    world_to_cam                           gsplat/cuda/_wrapper.py:19-53 (:628-676)
    proj                                   gsplat/cuda/_wrapper.py:176-206 (:679-760)

`fully_fused_projection` in _wrapper.py dispatches here when `covars` is
given.  Every op runs through the HIP C ABI on torch's current stream; there
is no CPU or torch fallback.
"""

from typing import Tuple

import torch
from torch import Tensor

from . import _lib
from ._wrapper import _dev_check, _f32c, _ptr, _stream

CAMERA_MODELS = {"pinhole": 0, "ortho": 1, "fisheye": 2}


def _aligned(t: Tensor, n: int) -> Tensor:
    return t if t.data_ptr() % n == 0 else t.clone()


def _g(t, shape, dev):
    return torch.zeros(shape, device=dev) if t is None else _f32c(t)


class _FullyFusedProjectionCovar(torch.autograd.Function):
    """Projects Gaussians given by covars [N,6] to 2D, dense [C,N] outputs."""

    @staticmethod
    def forward(ctx, means, covars, viewmats, Ks, width, height, eps2d, near_plane, far_plane,
                radius_clip, calc_compensations):
        ctx.set_materialize_grads(False)
        means, covars, viewmats, Ks = (_f32c(x) for x in (means, covars, viewmats, Ks))
        covars = _aligned(covars, 8)
        _dev_check(means, covars, viewmats, Ks)
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device
        radii = torch.empty((C, N), dtype=torch.int32, device=dev)
        means2d = torch.empty((C, N, 2), dtype=torch.float32, device=dev)
        depths = torch.empty((C, N), dtype=torch.float32, device=dev)
        conics = torch.empty((C, N, 3), dtype=torch.float32, device=dev)
        comps = torch.empty((C, N), dtype=torch.float32, device=dev) if calc_compensations else None
        _lib.call("gsplat_hip_projection_covar_fwd", C, N, _ptr(means), _ptr(covars),
                  _ptr(viewmats), _ptr(Ks), int(width), int(height), float(eps2d),
                  float(near_plane), float(far_plane), float(radius_clip), _ptr(radii),
                  _ptr(means2d), _ptr(depths), _ptr(conics), _ptr(comps), _stream())
        ctx.save_for_backward(means, covars, viewmats, Ks, radii, conics, comps)
        ctx.width, ctx.height, ctx.eps2d = int(width), int(height), float(eps2d)
        ctx.mark_non_differentiable(radii)
        return radii, means2d, depths, conics, comps

    @staticmethod
    def backward(ctx, v_radii, v_means2d, v_depths, v_conics, v_compensations):
        means, covars, viewmats, Ks, radii, conics, comps = ctx.saved_tensors
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device
        v_means2d = _g(v_means2d, (C, N, 2), dev)
        v_depths = None if v_depths is None else _f32c(v_depths)  # null = zeros in the kernel
        v_conics = _g(v_conics, (C, N, 3), dev)
        v_comps = _g(v_compensations, (C, N), dev) if comps is not None else None
        v_means = torch.empty((N, 3), device=dev)
        v_covars = torch.empty((N, 6), device=dev)
        v_viewmats = torch.empty((C, 4, 4), device=dev) if ctx.needs_input_grad[2] else None
        _lib.call("gsplat_hip_projection_covar_bwd", C, N, _ptr(means), _ptr(covars),
                  _ptr(viewmats), _ptr(Ks), ctx.width, ctx.height, ctx.eps2d, _ptr(radii),
                  _ptr(conics), _ptr(comps), _ptr(v_means2d), _ptr(v_depths), _ptr(v_conics),
                  _ptr(v_comps), _ptr(v_means), _ptr(v_covars), _ptr(v_viewmats), _stream())
        return (v_means if ctx.needs_input_grad[0] else None,
                v_covars if ctx.needs_input_grad[1] else None,
                v_viewmats, None, None, None, None, None, None, None, None)


class _FullyFusedProjectionCovarPacked(torch.autograd.Function):
    """Projects Gaussians given by covars [N,6] to 2D, packed [nnz] outputs in
    (camera, Gaussian) order.  One host read of nnz."""

    @staticmethod
    def forward(ctx, means, covars, viewmats, Ks, width, height, eps2d, near_plane, far_plane,
                radius_clip, sparse_grad, calc_compensations):
        means, covars, viewmats, Ks = (_f32c(x) for x in (means, covars, viewmats, Ks))
        covars = _aligned(covars, 8)
        _dev_check(means, covars, viewmats, Ks)
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device
        ws = torch.empty(max(int(_lib.query("gsplat_hip_projection_packed_workspace_bytes", C, N))
                             // 8, 1), dtype=torch.int64, device=dev)
        nnz_dev = torch.empty(1, dtype=torch.int64, device=dev)
        args = (_ptr(means), _ptr(covars), _ptr(viewmats), _ptr(Ks), int(width), int(height),
                float(eps2d), float(near_plane), float(far_plane), float(radius_clip))
        _lib.call("gsplat_hip_projection_covar_packed_count", C, N, *args, _ptr(ws),
                  _ptr(nnz_dev), _stream())
        nnz = int(nnz_dev.item())
        camera_ids = torch.empty(nnz, dtype=torch.int64, device=dev)
        gaussian_ids = torch.empty(nnz, dtype=torch.int64, device=dev)
        radii = torch.empty(nnz, dtype=torch.int32, device=dev)
        means2d = torch.empty((nnz, 2), device=dev)
        depths = torch.empty(nnz, device=dev)
        conics = torch.empty((nnz, 3), device=dev)
        comps = torch.empty(nnz, device=dev) if calc_compensations else None
        if nnz > 0:
            _lib.call("gsplat_hip_projection_covar_packed_fwd", C, N, *args, _ptr(ws),
                      _ptr(camera_ids), _ptr(gaussian_ids), _ptr(radii), _ptr(means2d),
                      _ptr(depths), _ptr(conics), _ptr(comps), _stream())
        ctx.save_for_backward(camera_ids, gaussian_ids, means, covars, viewmats, Ks, conics, comps)
        ctx.width, ctx.height, ctx.eps2d = int(width), int(height), float(eps2d)
        ctx.sparse_grad = sparse_grad
        ctx.mark_non_differentiable(camera_ids, gaussian_ids, radii)
        return camera_ids, gaussian_ids, radii, means2d, depths, conics, comps

    @staticmethod
    def backward(ctx, v_camera_ids, v_gaussian_ids, v_radii, v_means2d, v_depths, v_conics,
                 v_compensations):
        camera_ids, gaussian_ids, means, covars, viewmats, Ks, conics, comps = ctx.saved_tensors
        C, N, nnz = viewmats.shape[0], means.shape[0], camera_ids.numel()
        dev = means.device
        v_means2d = _g(v_means2d, (nnz, 2), dev)
        v_conics = _g(v_conics, (nnz, 3), dev)
        v_depths = None if v_depths is None else _f32c(v_depths)
        v_comps = _g(v_compensations, (nnz,), dev) if comps is not None else None
        rows = nnz if ctx.sparse_grad else N
        v_means = torch.empty((rows, 3), device=dev)
        v_covars = torch.empty((rows, 6), device=dev)
        v_viewmats = torch.empty((C, 4, 4), device=dev) if ctx.needs_input_grad[2] else None
        _lib.call("gsplat_hip_projection_covar_packed_bwd", C, N, nnz, _ptr(means), _ptr(covars),
                  _ptr(viewmats), _ptr(Ks), ctx.width, ctx.height, ctx.eps2d, _ptr(camera_ids),
                  _ptr(gaussian_ids), _ptr(conics), _ptr(comps), _ptr(v_means2d), _ptr(v_depths),
                  _ptr(v_conics), _ptr(v_comps), int(bool(ctx.sparse_grad)), _ptr(v_means),
                  _ptr(v_covars), _ptr(v_viewmats), _stream())
        if ctx.sparse_grad:  # COO gradients (gsplat/cuda/_wrapper.py:1127-1170)
            def coo(v, like):
                return torch.sparse_coo_tensor(indices=gaussian_ids[None], values=v,
                                               size=like.size(), is_coalesced=C == 1)
            v_means, v_covars = coo(v_means, means), coo(v_covars, covars)
        return (v_means if ctx.needs_input_grad[0] else None,
                v_covars if ctx.needs_input_grad[1] else None,
                v_viewmats, None, None, None, None, None, None, None, None, None)


# ============================================================ world_to_cam ==
class _WorldToCam(torch.autograd.Function):
    """Transforms Gaussians from world to camera space
    (gsplat/cuda/_wrapper.py:628-676)."""

    @staticmethod
    def forward(ctx, means, covars, viewmats):
        ctx.set_materialize_grads(False)
        means, covars, viewmats = (_f32c(x) for x in (means, covars, viewmats))
        _dev_check(means, covars, viewmats)
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device
        means_c = torch.empty((C, N, 3), device=dev)
        covars_c = torch.empty((C, N, 3, 3), device=dev)
        _lib.call("gsplat_hip_world_to_cam_fwd", C, N, _ptr(means), _ptr(covars), _ptr(viewmats),
                  _ptr(means_c), _ptr(covars_c), _stream())
        ctx.save_for_backward(means, covars, viewmats)
        return means_c, covars_c

    @staticmethod
    def backward(ctx, v_means_c, v_covars_c):
        means, covars, viewmats = ctx.saved_tensors
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device
        v_means_c = None if v_means_c is None else _f32c(v_means_c)  # null = zeros in the kernel
        v_covars_c = None if v_covars_c is None else _f32c(v_covars_c)
        need = ctx.needs_input_grad
        v_means = torch.empty((N, 3), device=dev) if need[0] else None
        v_covars = torch.empty((N, 3, 3), device=dev) if need[1] else None
        v_viewmats = torch.empty((C, 4, 4), device=dev) if need[2] else None
        _lib.call("gsplat_hip_world_to_cam_bwd", C, N, _ptr(means), _ptr(covars), _ptr(viewmats),
                  _ptr(v_means_c), _ptr(v_covars_c), _ptr(v_means), _ptr(v_covars),
                  _ptr(v_viewmats), _stream())
        return v_means, v_covars, v_viewmats


def world_to_cam(
    means: Tensor,  # [N, 3]
    covars: Tensor,  # [N, 3, 3]
    viewmats: Tensor,  # [C, 4, 4]
) -> Tuple[Tensor, Tensor]:
    """Transforms Gaussians from world to camera space
    (gsplat/cuda/_wrapper.py:19-53): means_c [C,N,3] = R m + t and
    covars_c [C,N,3,3] = R S R^T.  Differentiable in all three inputs; each
    gradient is computed only when its input requires it."""
    C = viewmats.size(0)
    N = means.size(0)
    assert means.size() == (N, 3), means.size()
    assert covars.size() == (N, 3, 3), covars.size()
    assert viewmats.size() == (C, 4, 4), viewmats.size()
    return _WorldToCam.apply(means.contiguous(), covars.contiguous(), viewmats.contiguous())


# ==================================================================== proj ==
class _Proj(torch.autograd.Function):
    """Projects Gaussians in camera space to the image
    (gsplat/cuda/_wrapper.py:679-760)."""

    @staticmethod
    def forward(ctx, means, covars, Ks, width, height, camera_model):
        ctx.set_materialize_grads(False)
        means, covars, Ks = (_f32c(x) for x in (means, covars, Ks))
        _dev_check(means, covars, Ks)
        C, N = means.shape[0], means.shape[1]
        dev = means.device
        means2d = torch.empty((C, N, 2), device=dev)
        covars2d = torch.empty((C, N, 2, 2), device=dev)
        _lib.call("gsplat_hip_proj_fwd", C, N, CAMERA_MODELS[camera_model], _ptr(means),
                  _ptr(covars), _ptr(Ks), int(width), int(height), _ptr(means2d),
                  _ptr(covars2d), _stream())
        ctx.save_for_backward(means, covars, Ks)
        ctx.width, ctx.height, ctx.model = int(width), int(height), CAMERA_MODELS[camera_model]
        return means2d, covars2d

    @staticmethod
    def backward(ctx, v_means2d, v_covars2d):
        means, covars, Ks = ctx.saved_tensors
        C, N = means.shape[0], means.shape[1]
        dev = means.device
        # null = zeros in the kernel; freshly made contiguous tensors are 16-B aligned
        v_means2d = None if v_means2d is None else _aligned(_f32c(v_means2d), 8)
        v_covars2d = None if v_covars2d is None else _aligned(_f32c(v_covars2d), 16)
        v_means = torch.empty((C, N, 3), device=dev) if ctx.needs_input_grad[0] else None
        v_covars = torch.empty((C, N, 3, 3), device=dev) if ctx.needs_input_grad[1] else None
        _lib.call("gsplat_hip_proj_bwd", C, N, ctx.model, _ptr(means), _ptr(covars), _ptr(Ks),
                  ctx.width, ctx.height, _ptr(v_means2d), _ptr(v_covars2d), _ptr(v_means),
                  _ptr(v_covars), _stream())
        return v_means, v_covars, None, None, None, None


def proj(
    means: Tensor,  # [C, N, 3]
    covars: Tensor,  # [C, N, 3, 3]
    Ks: Tensor,  # [C, 3, 3]
    width: int,
    height: int,
    camera_model: str = "pinhole",
) -> Tuple[Tensor, Tensor]:
    """Projects Gaussians in camera space (gsplat/cuda/_wrapper.py:176-206):
    means2d [C,N,2] and covars2d [C,N,2,2] = J S J^T, for the "pinhole" (with
    the 15 % screen-margin clamp of the fused projection), "ortho" and
    "fisheye" models.  No culling and no blur.  Differentiable in means and
    covars (the covars2d cotangent may be any 2x2 matrix); Ks gets no
    gradient."""
    if camera_model not in CAMERA_MODELS:
        raise ValueError(f"Unsupported camera model: {camera_model!r} "
                         f"(one of {sorted(CAMERA_MODELS)})")
    assert means.dim() == 3, means.size()
    C, N, _ = means.shape
    assert means.shape == (C, N, 3), means.size()
    assert covars.shape == (C, N, 3, 3), covars.size()
    assert Ks.shape == (C, 3, 3), Ks.size()
    return _Proj.apply(means.contiguous(), covars.contiguous(), Ks.contiguous(), width, height,
                       camera_model)
