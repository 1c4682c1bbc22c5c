"""Fused photometric loss and multi-tensor Adam for the training step.

`l1_ssim_loss` = (1 - lam) * mean|render - gt| + lam * (1 - SSIM_valid),
the loss of examples/simple_trainer.py:642-646 with fused_ssim
(rahul-goel/fused-ssim, padding="valid") restated in HIP (csrc/ssim.hip).
`FusedAdam` applies torch.optim.Adam's update to all Gaussian parameter
groups in one kernel (csrc/adam.hip).
"""

import ctypes
import math
import os

import torch

from . import _lib
from ._wrapper import _dev_check, _f32c, _ptr, _stream


class _L1SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, gt):
        assert img.dim() == 4 and img.shape == gt.shape, (img.shape, gt.shape)
        img = img.contiguous().float()
        gt = gt.contiguous().float()
        B, H, W, C = img.shape
        ws = torch.empty(max(int(_lib.query("gsplat_hip_ssim_workspace_bytes", B, H, W, C)), 4),
                         dtype=torch.uint8, device=img.device)
        sums = torch.empty(2, device=img.device)
        _lib.call("gsplat_hip_ssim_l1_fwd", B, H, W, C, _ptr(img), _ptr(gt), _ptr(sums),
                  _ptr(ws), _stream())
        ctx.save_for_backward(img, gt, ws)
        n_map = B * C * (H - 10) * (W - 10)
        n_img = B * C * H * W
        return sums[0] / n_map, sums[1] / n_img  # mean SSIM, mean L1

    @staticmethod
    def backward(ctx, g_ssim, g_l1):
        img, gt, ws = ctx.saved_tensors
        B, H, W, C = img.shape
        dloss = torch.stack([g_ssim.reshape(()), g_l1.reshape(())]).float().contiguous()
        grad = torch.empty_like(img)
        _lib.call("gsplat_hip_ssim_l1_bwd", B, H, W, C, _ptr(img), _ptr(gt), _ptr(ws),
                  _ptr(dloss), _ptr(grad), _stream())
        return grad, None


def ssim_and_l1(img, gt):
    """(mean SSIM over the valid region, mean L1) of [B,H,W,C] images."""
    return _L1SSIM.apply(img, gt)


class _L1SSIMLoss(torch.autograd.Function):
    """The whole loss in one forward and one backward launch pair: the scalar
    arithmetic is folded into the reduction / gradient kernels."""

    @staticmethod
    def forward(ctx, img, gt, lam):
        assert img.dim() == 4 and img.shape == gt.shape, (img.shape, gt.shape)
        img = img.contiguous().float()
        gt = gt.contiguous().float()
        B, H, W, C = img.shape
        ws = torch.empty(max(int(_lib.query("gsplat_hip_ssim_workspace_bytes", B, H, W, C)), 4),
                         dtype=torch.uint8, device=img.device)
        out = torch.empty(3, device=img.device)
        _lib.call("gsplat_hip_l1_ssim_loss_fwd", B, H, W, C, _ptr(img), _ptr(gt),
                  ctypes.c_float(lam), _ptr(out), _ptr(ws), _stream())
        ctx.save_for_backward(img, gt, ws)
        ctx.lam = float(lam)
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        img, gt, ws = ctx.saved_tensors
        B, H, W, C = img.shape
        g_loss = g_loss.float().contiguous()
        grad = torch.empty_like(img)
        _lib.call("gsplat_hip_l1_ssim_loss_bwd", B, H, W, C, _ptr(img), _ptr(gt), _ptr(ws),
                  ctypes.c_float(ctx.lam), _ptr(g_loss), _ptr(grad), _stream())
        return grad, None, None


class _L1SSIMLossFused(torch.autograd.Function):
    """The same loss with dloss/dimg computed in the forward launch
    (csrc/ssim.hip fused_kernel); the backward scales it by the incoming
    gradient.  The training path: no per-pixel SSIM partials through HBM."""

    @staticmethod
    def forward(ctx, img, gt, lam, gt_index=None, out_ring=None, channels=None):
        # gt_index: device int64 [1]; gt is then a stack [n, H, W, C] of
        # single-image targets and gt[gt_index] is this image's target.
        # out_ring: (ring float32 [R], seq int64 [1], both on the device): the
        # loss also goes to ring[(seq - 1) % R] (gsplat_hip_l1_ssim_loss_fused_fwd_ring)
        # channels: the loss reads the first `channels` of img's XS channels
        # (an RGB+D render in place); its gradient is img-shaped, zero in the rest
        XS = img.shape[-1]
        C = XS if channels is None else int(channels)
        if gt_index is None:
            assert img.dim() == 4 and img.shape[:3] == gt.shape[:3] and gt.shape[3] == C, \
                (img.shape, gt.shape)
        else:
            assert img.dim() == 4 and img.shape[0] == 1 and gt.shape[1:3] == img.shape[1:3] \
                and gt.shape[3] == C, (img.shape, gt.shape)
            assert gt_index.dtype == torch.int64 and gt_index.is_cuda and gt.is_contiguous()
        img = img.contiguous().float()
        gt = gt.contiguous().float()
        B, H, W, _ = img.shape
        ws = torch.empty(max(int(_lib.query("gsplat_hip_l1_ssim_loss_fused_workspace_bytes",
                                            B, H, W, C)), 4),
                         dtype=torch.uint8, device=img.device)
        out = torch.empty(3, device=img.device)
        unit = torch.empty_like(img)
        if out_ring is None:
            _lib.call("gsplat_hip_l1_ssim_loss_fused_fwd", B, H, W, C, XS, _ptr(img), _ptr(gt),
                      _ptr(gt_index), ctypes.c_float(lam), _ptr(out), _ptr(unit), _ptr(ws),
                      _stream())
        else:
            ring, seq = out_ring
            assert ring.dtype == torch.float32 and ring.is_cuda and seq.dtype == torch.int64
            _lib.call("gsplat_hip_l1_ssim_loss_fused_fwd_ring", B, H, W, C, XS, _ptr(img), _ptr(gt),
                      _ptr(gt_index), ctypes.c_float(lam), _ptr(out), _ptr(unit), _ptr(ws),
                      _ptr(ring), ring.numel(), _ptr(seq), _stream())
        ctx.save_for_backward(unit)
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        (unit,) = ctx.saved_tensors
        if g_loss is ONE_GRAD:  # the trainer's constant 1.0 seed: the unit gradient as is
            return unit, None, None, None, None, None
        g_loss = g_loss.float().contiguous()
        grad = torch.empty_like(unit)
        _lib.call("gsplat_hip_l1_ssim_loss_fused_bwd", unit.numel(), _ptr(unit), _ptr(g_loss),
                  _ptr(grad), _stream())
        return grad, None, None, None, None, None


class _L1SSIMLossMasked(torch.autograd.Function):
    """_L1SSIMLossFused on the masked render over a background colour,
    x = (masks ? img : 0) + backgrounds * (1 - alphas), composed in the loss
    kernel's window load (csrc/ssim.hip fused_masked_kernel): no composed image
    and no select / composite backward through HBM.  Gradients for img
    (zero under the mask) and alphas; arguments checked by l1_ssim_loss."""

    @staticmethod
    def forward(ctx, img, gt, lam, gt_index, out_ring, masks, alphas, backgrounds):
        img = img.contiguous().float()
        gt = gt.contiguous().float()
        B, H, W, C = img.shape
        ws = torch.empty(max(int(_lib.query("gsplat_hip_l1_ssim_loss_fused_workspace_bytes",
                                            B, H, W, C)), 4),
                         dtype=torch.uint8, device=img.device)
        out = torch.empty(3, device=img.device)
        unit = torch.empty_like(img)
        a_unit = None if backgrounds is None else torch.empty_like(alphas)
        ring, seq = (None, None) if out_ring is None else out_ring
        if ring is not None:
            assert ring.dtype == torch.float32 and ring.is_cuda and seq.dtype == torch.int64
        _lib.call("gsplat_hip_l1_ssim_loss_masked_fwd", B, H, W, C, _ptr(img), _ptr(gt),
                  _ptr(gt_index), _ptr(masks), _ptr(alphas if backgrounds is not None else None),
                  _ptr(backgrounds), ctypes.c_float(lam), _ptr(out), _ptr(unit), _ptr(a_unit),
                  _ptr(ws), _ptr(ring), 0 if ring is None else ring.numel(), _ptr(seq), _stream())
        ctx.save_for_backward(unit, a_unit)
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        unit, a_unit = ctx.saved_tensors
        if g_loss is ONE_GRAD:  # the trainer's constant 1.0 seed: the unit gradients as they are
            return unit, None, None, None, None, None, a_unit, None
        g_loss = g_loss.float().contiguous()
        grad = torch.empty_like(unit)
        g_alpha = None if a_unit is None else torch.empty_like(a_unit)
        _lib.call("gsplat_hip_l1_ssim_loss_masked_bwd", unit.numel(), _ptr(unit),
                  0 if a_unit is None else a_unit.numel(), _ptr(a_unit), _ptr(g_loss), _ptr(grad),
                  _ptr(g_alpha), _stream())
        return grad, None, None, None, None, None, g_alpha, None


# A constant scalar 1.0 the trainer seeds loss.backward() with (never written):
# seen as the incoming gradient, the fused loss's backward returns its stored
# unit gradient without the scaling launch.
ONE_GRAD = None

# GSPLAT_HIP_SSIM_FUSED=0: the two-pass loss (partials to HBM) for training too
SSIM_FUSED = os.environ.get("GSPLAT_HIP_SSIM_FUSED", "1") != "0"


def _masked_args(img, gt, gt_index, masks, alphas, backgrounds, _channels):
    """l1_ssim_loss's checks of masks / alphas / backgrounds (ValueError naming
    the argument); returns masks as uint8 (a view of a bool tensor)."""
    if _channels is not None:
        raise ValueError("l1_ssim_loss: _channels does not go with masks / backgrounds")
    if img.dim() != 4:
        raise ValueError(f"l1_ssim_loss: masks / backgrounds need img [B,H,W,C], got "
                         f"{tuple(img.shape)}")
    B, H, W, C = img.shape
    if masks is not None:
        if masks.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"l1_ssim_loss: masks must be bool or uint8, got {masks.dtype}")
        want = (gt.shape[0] if gt_index is not None else B, H, W)
        if tuple(masks.shape) != want:
            raise ValueError(f"l1_ssim_loss: masks must be {list(want)}, got "
                             f"{list(masks.shape)}")
        if masks.device != img.device:
            raise ValueError(f"l1_ssim_loss: masks on {masks.device}, img on {img.device}")
        masks = masks.contiguous()
        if masks.dtype == torch.bool:
            masks = masks.view(torch.uint8)
    if backgrounds is not None:
        if alphas is None:
            raise ValueError("l1_ssim_loss: backgrounds needs alphas")
        if tuple(backgrounds.shape) != (B, C) or backgrounds.dtype != torch.float32 \
                or backgrounds.device != img.device:
            raise ValueError(f"l1_ssim_loss: backgrounds must be float32 [{B}, {C}] on "
                             f"{img.device}, got {backgrounds.dtype} {list(backgrounds.shape)} "
                             f"on {backgrounds.device}")
    if alphas is not None:
        if tuple(alphas.shape) != (B, H, W, 1) or alphas.dtype != torch.float32 \
                or not alphas.is_contiguous() or alphas.device != img.device:
            raise ValueError(f"l1_ssim_loss: alphas must be contiguous float32 [{B}, {H}, {W}, 1] "
                             f"on {img.device}, got {alphas.dtype} {list(alphas.shape)} on "
                             f"{alphas.device}")
    return masks


def compose_masked(img, masks=None, alphas=None, backgrounds=None):
    """(masks ? img : 0) + backgrounds * (1 - alphas) in torch ops: img
    [B,H,W,C], masks [B,H,W] bool / uint8 (non-zero = valid), alphas
    [B,H,W,1], backgrounds [B,C] -- simple_trainer.py:505-506, 629-631.  What
    the fused loss composes in its kernel; the paths without it call this."""
    x = img
    if masks is not None:
        x = torch.where(masks.bool()[..., None], x, torch.zeros((), dtype=x.dtype, device=x.device))
    if backgrounds is not None:
        x = x + backgrounds[:, None, None, :] * (1.0 - alphas)
    return x


def l1_ssim_loss(img, gt, ssim_lambda=0.2, fused=None, gt_index=None, _out_ring=None,
                 _channels=None, masks=None, alphas=None, backgrounds=None):
    """(1 - ssim_lambda) * mean L1 + ssim_lambda * (1 - mean SSIM_valid).
    With a gradient to compute (and C in {1, 3}) the one-pass fused kernel
    runs, unless `fused=False` (or GSPLAT_HIP_SSIM_FUSED=0).  `gt_index`
    (device int64 [1], fused kernel only): `gt` is a stack of targets and
    gt[gt_index] the one of this [1, H, W, C] image -- chosen on the device,
    no copy (the captured training step).  `_out_ring` (internal, with
    gt_index): (ring, seq) device tensors; the loss value is also written to
    ring[(seq - 1) % len(ring)] by the reduction launch (graph_step.py).
    `_channels` (internal): the loss is over img[..., :_channels] (an RGB+D
    render read in place by the fused kernel; its gradient is img-shaped).
    `masks` (bool / uint8 [B,H,W], True = valid; with gt_index a stack [n,H,W]
    indexed like gt), `alphas` ([B,H,W,1] float32 contiguous, as
    rasterization() returns them) and `backgrounds` ([B,C] float32 on the
    device, needs alphas): the loss is taken on
    (masks ? img : 0) + backgrounds * (1 - alphas), the reference trainer's
    masks and random_bkgd.  With a gradient to compute and C in {1, 3} that is
    one kernel with gradients for img (exactly zero under the mask, whatever
    img holds there) and alphas; otherwise torch ops (compose_masked) in
    front of the paths above.  backgrounds and masks get no gradient."""
    if masks is not None or backgrounds is not None:
        masks = _masked_args(img, gt, gt_index, masks, alphas, backgrounds, _channels)
        needs = torch.is_grad_enabled() and (
            img.requires_grad or (backgrounds is not None and alphas.requires_grad))
        if fused is None:
            fused = SSIM_FUSED and needs
        if fused and img.shape[-1] in (1, 3):
            return _L1SSIMLossMasked.apply(img, gt, float(ssim_lambda), gt_index, _out_ring,
                                           masks, alphas, backgrounds)
        if gt_index is not None:
            raise ValueError("l1_ssim_loss: gt_index needs the fused kernel (grad, C in {1, 3})")
        return l1_ssim_loss(compose_masked(img, masks, alphas, backgrounds), gt, ssim_lambda,
                            fused=fused)
    if _channels is not None and _channels != img.shape[-1]:
        if fused is None:
            fused = SSIM_FUSED and torch.is_grad_enabled() and img.requires_grad
        if not (fused and img.dim() == 4 and _channels in (1, 3)):
            img = img[..., :_channels]  # the generic path on the slice
        else:
            return _L1SSIMLossFused.apply(img, gt, float(ssim_lambda), gt_index, _out_ring,
                                          int(_channels))
    if fused is None:
        fused = SSIM_FUSED and torch.is_grad_enabled() and img.requires_grad
    if gt_index is not None:
        if not (fused and img.dim() == 4 and img.shape[-1] in (1, 3)):
            raise ValueError("l1_ssim_loss: gt_index needs the fused kernel (grad, C in {1, 3})")
        return _L1SSIMLossFused.apply(img, gt, float(ssim_lambda), gt_index, _out_ring)
    if fused and img.dim() == 4 and img.shape[-1] in (1, 3):
        return _L1SSIMLossFused.apply(img, gt, float(ssim_lambda))
    return _L1SSIMLoss.apply(img, gt, float(ssim_lambda))


class _GeometryLoss2DGS(torch.autograd.Function):
    """normal_lambda * mean(1 - <R n, alpha n_d>) + dist_lambda * mean(distort)
    in one reduction launch (plus a one-workgroup finish) forward and one
    launch backward (csrc/geom_loss.hip): the normals of the depth are formed
    in registers both ways, no torch pass and no [H,W,3] intermediate."""

    @staticmethod
    def forward(ctx, normals, depths, alphas, camtoworlds, Ks, distort, nl, dl, world, z_depth,
                depth_image):
        # depth_image: `depths` is a contiguous [C,H,W,D] render whose last
        # channel is the depth; its gradient is image-shaped (zeros elsewhere)
        do_n, do_d = nl != 0.0, dl != 0.0
        if not do_n:
            normals = depths = alphas = None
        if not do_d:
            distort = None
        _dev_check(normals, depths, alphas, camtoworlds, Ks, distort)
        lead = normals if do_n else distort
        assert lead.dim() == 4, lead.shape
        C, H, W = lead.shape[:3]
        dev = lead.device
        ps, d_ptr = 1, 0
        if do_n:
            assert normals.shape == (C, H, W, 3), normals.shape
            assert alphas.shape == (C, H, W, 1), alphas.shape
            assert camtoworlds.shape == (C, 4, 4) and Ks.shape == (C, 3, 3), \
                (camtoworlds.shape, Ks.shape)
            normals, alphas = _f32c(normals), _f32c(alphas)
            camtoworlds, Ks = _f32c(camtoworlds), _f32c(Ks)
            if depth_image:
                assert depths.shape[:3] == (C, H, W) and depths.dtype == torch.float32 \
                    and depths.is_contiguous(), depths.shape
                ps = depths.shape[3]
                d_ptr = depths.data_ptr() + 4 * (ps - 1)
            else:
                assert depths.shape == (C, H, W, 1), depths.shape
                # the last channel of an RGB+D render is read in place (pixel stride)
                ps = depths.stride(2)
                if not (depths.dtype == torch.float32 and ps >= 1 and depths.stride(1) == W * ps
                        and depths.stride(0) == H * W * ps):
                    depths, ps = _f32c(depths), 1
                d_ptr = depths.data_ptr()
        if do_d:
            assert distort.shape == (C, H, W, 1), distort.shape
            distort = _f32c(distort)
        ws = torch.empty(max(int(_lib.query("gsplat_hip_geom_loss_2dgs_workspace_bytes",
                                            C, H, W)), 4), dtype=torch.uint8, device=dev)
        out = torch.empty(3, device=dev)
        _lib.call("gsplat_hip_geom_loss_2dgs_fwd", C, H, W, _ptr(normals), d_ptr, int(ps),
                  _ptr(alphas), _ptr(distort), _ptr(camtoworlds), _ptr(Ks), int(bool(z_depth)),
                  int(bool(world)), ctypes.c_float(nl), ctypes.c_float(dl), _ptr(out), _ptr(ws),
                  _stream())
        ctx.save_for_backward(normals, depths, alphas, camtoworlds, Ks)
        ctx.cfg = (C, H, W, int(ps), float(nl), float(dl), bool(world), bool(z_depth),
                   bool(depth_image))
        ctx.dev = dev
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        normals, depths, alphas, camtoworlds, Ks = ctx.saved_tensors
        C, H, W, ps, nl, dl, world, z_depth, depth_image = ctx.cfg
        dev = ctx.dev
        # the upstream scalar is read on the device (the trainer's ONE_GRAD
        # seed as is: no scaling launch either way)
        if g_loss.dtype != torch.float32 or not g_loss.is_contiguous():
            g_loss = g_loss.float().contiguous()
        v_normals = v_depths = v_distort = None
        d_ptr = vd_ptr = 0
        vps = 1
        if nl != 0.0:
            v_normals = torch.empty((C, H, W, 3), device=dev)
            if depth_image:
                v_depths = torch.empty_like(depths)
                vps = ps
                d_ptr = depths.data_ptr() + 4 * (ps - 1)
                vd_ptr = v_depths.data_ptr() + 4 * (ps - 1)
            else:
                v_depths = torch.empty((C, H, W, 1), device=dev)
                d_ptr, vd_ptr = depths.data_ptr(), v_depths.data_ptr()
        if dl != 0.0:
            v_distort = torch.empty((C, H, W, 1), device=dev)
        _lib.call("gsplat_hip_geom_loss_2dgs_bwd", C, H, W, _ptr(normals), d_ptr, ps,
                  _ptr(alphas), _ptr(camtoworlds), _ptr(Ks), int(z_depth), int(world),
                  ctypes.c_float(nl), ctypes.c_float(dl), _ptr(g_loss), _ptr(v_normals), vd_ptr,
                  vps, int(depth_image), _ptr(v_distort), _stream())
        need = ctx.needs_input_grad
        return (v_normals if need[0] else None, v_depths if need[1] else None, None, None, None,
                v_distort if need[5] else None, None, None, None, None, None)


def geometry_loss_2dgs(render_normals, depths, alphas, camtoworlds, Ks, render_distort=None,
                       normal_lambda=5e-2, dist_lambda=1e-2, normals_space="camera",
                       z_depth=True, _depth_image=False):
    """The 2DGS trainer's geometry terms (simple_trainer_2dgs.py:611-632),
    fused in HIP (csrc/geom_loss.hip):

        normal_lambda * mean(1 - <R n, alphas * n_d>) + dist_lambda * mean(render_distort)

    with R = camtoworlds[:, :3, :3], n = render_normals [C,H,W,3] in camera
    space (normals_space="camera", the rasterizer's image) or already rotated
    (normals_space="world", rasterization_2dgs's public output: R is skipped),
    and n_d = depth_to_normal(depths, camtoworlds, Ks, z_depth) formed in the
    kernel.  depths / alphas / render_distort are [C,H,W,1]; depths may be the
    last-channel view of an RGB+D render (read in place).  Both means run
    over all pixels.  Returns a 0-d tensor; gradients go to render_normals,
    depths and render_distort, alphas is a constant (None), and camtoworlds
    / Ks requiring a gradient raise NotImplementedError.  A term whose lambda
    is 0 is skipped and its images may be None.  GPU tensors only.
    `_depth_image` (internal, the training step): depths is the whole
    contiguous [C,H,W,D] render, its depth the last channel, and its gradient
    comes back image-shaped with the other channels zero."""
    if normals_space not in ("camera", "world"):
        raise ValueError(f"normals_space: 'camera' or 'world', got {normals_space!r}")
    nl, dl = float(normal_lambda), float(dist_lambda)
    if nl != 0.0 and (render_normals is None or depths is None or alphas is None):
        raise ValueError("geometry_loss_2dgs: the normal term needs render_normals, depths, alphas")
    if dl != 0.0 and render_distort is None:
        raise ValueError("geometry_loss_2dgs: the distortion term needs render_distort")
    if nl == 0.0 and dl == 0.0:
        raise ValueError("geometry_loss_2dgs: both lambdas are 0")
    for name, t in (("camtoworlds", camtoworlds), ("Ks", Ks)):
        if t is not None and t.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError(
                f"geometry_loss_2dgs: no gradient of {name} (pose / intrinsics optimisation)")
    return _GeometryLoss2DGS.apply(render_normals, depths, alphas, camtoworlds, Ks,
                                   render_distort, nl, dl, normals_space == "world",
                                   bool(z_depth), bool(_depth_image))


def adam_factors(lrs, betas, step):
    """The per-group factors gsplat_hip_adam_step computes on the host, with
    its arithmetic (float lr and beta promoted to double, double pow / sqrt,
    rounded to float): [lr_i / (1 - beta1^t), 1 / sqrt(1 - beta2^t)] per
    group -- what the captured step's device-side variants read."""
    import numpy as np
    b1, b2 = float(np.float32(betas[0])), float(np.float32(betas[1]))
    bc1, bc2 = 1.0 - b1 ** int(step), 1.0 - b2 ** int(step)
    ib = float(np.float32(1.0 / math.sqrt(bc2)))
    return [(float(np.float32(float(np.float32(lr)) / bc1)), ib) for lr in lrs]


def adam_groups(params, grads, exp_avgs, exp_avg_sqs, lrs, betas, eps, step, aux=None,
                modes=None, hyper=None, skip=None):
    """One fused Adam launch (csrc/adam.hip) over flat float32 tensors: group
    i updates params[i] in place from grads[i] (None = zero) with its lr.
    aux/modes form the gradient in-register (gsplat_hip_adam_step_ex); hyper (device
    f32[2 n], adam_factors' values) / skip (device i32 flag): the captured
    step's form (gsplat_hip_adam_step_dev; lrs and step unused)."""
    n = len(params)
    P = ctypes.c_void_p * n
    for t in list(params) + list(exp_avgs) + list(exp_avg_sqs):
        assert t.is_contiguous() and t.dtype == torch.float32
    head = [n, P(*[p.data_ptr() for p in params]),
            P(*[0 if g is None else g.data_ptr() for g in grads])]
    if hyper is not None:
        assert hyper.dtype == torch.float32 and hyper.numel() >= 2 * n
        ax = [None] * n if aux is None else aux
        for a in ax:
            assert a is None or (a.is_contiguous() and a.dtype == torch.float32)
        _lib.call("gsplat_hip_adam_step_dev", *head,
                  P(*[0 if a is None else a.data_ptr() for a in ax]),
                  (ctypes.c_int32 * n)(*[int(m) for m in (modes or [0] * n)]),
                  P(*[m.data_ptr() for m in exp_avgs]), P(*[v.data_ptr() for v in exp_avg_sqs]),
                  (ctypes.c_int64 * n)(*[p.numel() for p in params]), hyper.data_ptr(),
                  float(betas[0]), float(betas[1]), float(eps),
                  0 if skip is None else skip.data_ptr(), _stream())
        return
    tail = [P(*[m.data_ptr() for m in exp_avgs]), P(*[v.data_ptr() for v in exp_avg_sqs]),
            (ctypes.c_int64 * n)(*[p.numel() for p in params]),
            (ctypes.c_float * n)(*[float(x) for x in lrs]), float(betas[0]), float(betas[1]),
            float(eps), int(step)]
    if modes is not None and any(modes):
        for a in aux:
            assert a is None or (a.is_contiguous() and a.dtype == torch.float32)
        _lib.call("gsplat_hip_adam_step_ex", *head,
                  P(*[0 if a is None else a.data_ptr() for a in aux]),
                  (ctypes.c_int32 * n)(*[int(m) for m in modes]), *tail, _stream())
        return
    _lib.call("gsplat_hip_adam_step", *(head + tail), _stream())


class FusedAdam:
    """torch.optim.Adam semantics (per-group lr, shared betas/eps) in one launch.

    (A variant that deferred the SH groups' update to a side stream, to
    overlap the next step's projection and isect, measured slower at M2 --
    620-650 against 660 images/s, profiles/r2_s4_defer: the two split the HBM
    bandwidth instead of filling each other's gaps -- and was removed.)"""

    def __init__(self, params, lrs, betas=(0.9, 0.999), eps=1e-8):
        self.params = list(params)
        self.lrs = [float(x) for x in lrs]
        self.betas, self.eps = betas, eps
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.step_count = 0
        for p in self.params:
            assert p.is_contiguous() and p.dtype == torch.float32

    def _launch(self, idx, grads, xform=None, hyper=None, void=None):
        aux = modes = None
        if xform:
            aux = [xform[i][1] if i in xform else None for i in idx]
            modes = [xform[i][2] if i in xform else 0 for i in idx]
            grads = [xform[i][0] if i in xform else g for i, g in enumerate(grads)]
        adam_groups([self.params[i].data for i in idx], [grads[i] for i in idx],
                    [self.exp_avg[i] for i in idx], [self.exp_avg_sq[i] for i in idx],
                    [self.lrs[i] for i in idx], self.betas, self.eps, self.step_count,
                    aux, modes, hyper, void)

    @torch.no_grad()
    def step(self, skip=(), xform=None, hyper=None, void=None):
        """skip: indices already updated for this step (by the SH backward
        with the update fused in, train_step.Trainer).  xform: {index:
        (grad, aux, mode)} -- the gradient of that group formed in-register
        (adam_step_ex modes: 1 sum, 2 exp VJP, 3 sigmoid VJP).  hyper / void:
        the captured step's device-side factors of the launched groups (in
        launch order, adam_factors) and void-step flag (step_count is then
        the caller's business)."""
        if hyper is None:
            self.step_count += 1
        grads = [p.grad for p in self.params]
        for gr in grads:
            assert gr is None or gr.is_contiguous()
        idx = [i for i in range(len(self.params)) if i not in skip]
        if idx:
            self._launch(idx, grads, xform=xform, hyper=hyper, void=void)

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None


class SideOptimizer:
    """An Adam beside the Gaussians' that owns its state (bilagrid.
    BilateralGridOptimizer, pose.PoseOptimizer, appearance.AppearanceOptimizer),
    launched after it in Trainer.side_opts' order.  A class sets `name`, its slot
    in graph_step.BLOCK, and implements
      factors(it)          that slot's floats for the step after step_count
      launch(s, hyper)     the launch of step `s` (StepInputs); hyper None: the
                           host's factors, counting the step itself (as
                           FusedAdam.step does), else the slot's, the count being
                           the caller's business
      moments()            key -> [exp_avg, exp_avg_sq], the tensors themselves
      checkpoint_tables()  (entries under the reference's keys, entries of the
                           "gsplat_hip" block), the tables themselves
      _workspace(n)        its workspace for n Gaussians, if it has one."""

    name = None
    optimised = True  # listed in Trainer.side_opts: launched, counted, its moments kept
    step_count = 0
    ws, ws_n = None, 0  # the workspace, sized for ws_n Gaussians

    def _workspace(self, n):
        return None

    def prepare(self, n):
        """The workspace for `n` Gaussians (a new size: not inside a capture)."""
        if self.ws_n != n:
            self.ws, self.ws_n = self._workspace(n), n
        return self.ws

    @torch.no_grad()
    def load_moments(self, moments):
        """Copies in those of `moments` (moments()'s keys) that are there."""
        for k, mine in self.moments().items():
            for dst, src in zip(mine, moments.get(k, ())):
                dst.copy_(src)

    @torch.no_grad()
    def load_checkpoint_tables(self, ck, gs, reset=False):
        """Copies in the tables that the file `ck` and its block `gs` carry;
        `reset`: then zero moments and step count as well."""
        hits = [(mine, src[key]) for src, tables in zip((ck, gs), self.checkpoint_tables())
                for key, mine in tables.items() if key in src]
        for mine, theirs in hits:  # a tensor, or a dict of tensors
            for k, t in (mine.items() if isinstance(mine, dict) else [(None, mine)]):
                t.copy_(theirs if k is None else theirs[k])
        if hits and reset:
            for t in sum(self.moments().values(), []):
                t.zero_()
            self.step_count = 0
