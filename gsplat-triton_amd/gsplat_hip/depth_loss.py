"""Sparse depth supervision (examples/simple_trainer.py:647-665, `depth_loss`),
fused in HIP (csrc/depth_loss.hip).

The reference renders RGB+ED (a whole-image division by alpha), slices and
permutes the depth channel, runs F.grid_sample(align_corners=True) at the M
projected SfM points, and takes F.l1_loss of where(d > 0, 1/d, 0) against
1/d_gt.  Here one forward launch reads the 4 M corner pixels of the RGB+D
render in place (dividing at the corners) and reduces the mean; the backward
scatters to those corners.  The points of every image are CSR tables on the
device (`DepthPoints`) and the image is chosen by a device index, so a
captured training step holds one kernel node for all images.

`sparse_depth_loss` is the autograd function for a trainer of the user's own;
`l1_ssim_depth_loss` is the training step's form: the photometric loss and
the depth term as one node whose backward scatters the depth gradient into
the (zero) depth channel of the photometric gradient image.
"""

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib
from ._wrapper import _dev_check, _f32c, _ptr, _stream


class DepthPoints:
    """CSR tables of the images' points on one device: `points` [sum M, 3]
    rows (x, y, d_gt), `offsets` int32 [n + 1]; `max_points` sizes the
    launches.  Built once (Trainer(depth_points=...))."""

    def __init__(self, per_image: Sequence, device):
        rows, offs = [], [0]
        for k, entry in enumerate(per_image):
            pts, dep = entry
            pts = torch.as_tensor(pts, dtype=torch.float32).reshape(-1, 2)
            dep = torch.as_tensor(dep, dtype=torch.float32).reshape(-1)
            if pts.shape[0] != dep.shape[0]:
                raise ValueError(f"depth_points[{k}]: {pts.shape[0]} points, "
                                 f"{dep.shape[0]} depths")
            rows.append(torch.cat([pts.cpu(), dep.cpu()[:, None]], 1))
            offs.append(offs[-1] + pts.shape[0])
        if offs[-1] >= 2 ** 31:
            raise ValueError("depth_points: more than 2^31 points")
        self.n_images = len(rows)
        self.counts = [b - a for a, b in zip(offs[:-1], offs[1:])]
        self.max_points = max(self.counts, default=0)
        table = torch.cat(rows) if rows else torch.zeros(0, 3)
        # (a row of padding: an empty table still has a pointer to hand over)
        self.points = torch.cat([table, torch.zeros(1, 3)]).contiguous().to(device)
        self.offsets = torch.tensor(offs, dtype=torch.int32, device=device)
        self.device = device
        self._ws = None
        if self.points.is_cuda:  # allocated and zeroed here, outside any graph capture
            self.workspace()

    @classmethod
    def from_dense(cls, points, depths_gt):
        """C images of M points each, from device tensors [C,M,2] / [C,M]: no
        host round trip."""
        self = cls.__new__(cls)
        C, M = depths_gt.shape
        dev = points.device
        table = torch.cat([_f32c(points.detach()), _f32c(depths_gt.detach())[..., None]], -1)
        self.points = torch.cat([table.reshape(C * M, 3), table.new_zeros(1, 3)])
        self.offsets = torch.arange(C + 1, dtype=torch.int32, device=dev) * M
        self.n_images, self.counts, self.max_points = C, [M] * C, M
        self.device = dev
        self._ws = _WORKSPACES.get((dev, M))
        if self._ws is None:
            _WORKSPACES[(dev, M)] = self.workspace()
        return self

    def workspace(self):
        """The forward's ticket and partials: zeroed once, here; every launch
        leaves the ticket zero."""
        if self._ws is None:
            n = int(_lib.query("gsplat_hip_depth_loss_workspace_bytes", self.max_points))
            self._ws = torch.zeros(n, dtype=torch.uint8, device=self.points.device)
        return self._ws


# sparse_depth_loss's workspaces by (device, M): zeroed once, reused by every call
_WORKSPACES = {}


def _plane(t, channel):
    """(pointer to `channel` of a contiguous float32 [1,H,W,XS] image, XS)."""
    XS = t.shape[-1]
    return t.data_ptr() + 4 * channel, XS


def _fwd(img, channel, alphas, tab: DepthPoints, cam_index, out, unit):
    _, H, W, _ = img.shape
    d_ptr, ds = _plane(img, channel)
    _lib.call("gsplat_hip_depth_loss_fwd", H, W, d_ptr, ds, _ptr(alphas), 1, _ptr(tab.points),
              _ptr(tab.offsets), tab.n_images, tab.max_points, _ptr(cam_index), _ptr(out),
              _ptr(unit), _ptr(tab.workspace()), _stream())


def _bwd(img, channel, alphas, tab: DepthPoints, cam_index, unit, g_loss, v_img, zero_image,
         v_alphas):
    _, H, W, XS = img.shape
    d_ptr, ds = _plane(img, channel)
    _lib.call("gsplat_hip_depth_loss_bwd", H, W, d_ptr, ds, _ptr(alphas), 1, _ptr(tab.points),
              _ptr(tab.offsets), tab.n_images, tab.max_points, _ptr(cam_index), _ptr(unit),
              _ptr(g_loss), _ptr(v_img), XS, int(channel), int(bool(zero_image)),
              _ptr(v_alphas), _stream())


def _check_table(img, alphas, tab, cam_index):
    assert img.dim() == 4 and img.shape[0] == 1 and img.dtype == torch.float32 \
        and img.is_contiguous(), (img.shape, img.dtype)
    assert alphas is None or (alphas.shape == img.shape[:3] + (1,)
                              and alphas.dtype == torch.float32
                              and alphas.is_contiguous()), alphas.shape
    assert cam_index.dtype == torch.int64 and cam_index.numel() == 1 and cam_index.is_cuda
    assert tab.points.device == img.device, (tab.points.device, img.device)


class _TableDepthLoss(torch.autograd.Function):
    """mean |disp - 1/d_gt| of image cam_index[0] of a DepthPoints table, on
    channel `channel` of a contiguous [1,H,W,XS] image; its gradient is
    image-shaped (zero-filled by the backward's own kernel, then scattered)."""

    @staticmethod
    def forward(ctx, img, alphas, tab, cam_index, channel):
        _check_table(img, alphas, tab, cam_index)
        out = torch.empty(1, device=img.device)
        unit = torch.empty(max(tab.max_points, 1), device=img.device)
        _fwd(img, channel, alphas, tab, cam_index, out, unit)
        ctx.save_for_backward(img, alphas, cam_index, unit)
        ctx.tab, ctx.channel = tab, channel
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        img, alphas, cam_index, unit = ctx.saved_tensors
        if g_loss.dtype != torch.float32 or not g_loss.is_contiguous():
            g_loss = g_loss.float().contiguous()
        v_img = torch.empty_like(img)
        v_alphas = None if alphas is None else torch.empty_like(alphas)
        _bwd(img, ctx.channel, alphas, ctx.tab, cam_index, unit, g_loss, v_img, True, v_alphas)
        return v_img, v_alphas, None, None, None


class _L1SSIMDepthLoss(torch.autograd.Function):
    """(photometric loss, depth term) of an RGB+D render [1,H,W,4] as one
    node: losses._L1SSIMLossFused on the colour channels -- its launch leaves
    the render-shaped unit gradient, zero in the depth channel -- and the depth
    forward.  The backward scales the photometric gradient (not at all for the
    trainer's constant seed) and scatters the depth term's into its channel 3,
    so autograd never sums two 4-channel images."""

    @staticmethod
    def forward(ctx, img, alphas, gt, lam, gt_index, tab, cam_index):
        _check_table(img, alphas, tab, cam_index)
        assert alphas is not None and img.shape[-1] == 4, img.shape
        _, H, W, XS = img.shape
        if gt_index is None:
            assert gt.shape == (1, H, W, 3), (img.shape, gt.shape)
        else:
            assert gt.shape[1:] == (H, W, 3), (img.shape, gt.shape)
            assert gt_index.dtype == torch.int64 and gt_index.is_cuda
        gt = _f32c(gt)
        ws = torch.empty(max(int(_lib.query("gsplat_hip_l1_ssim_loss_fused_workspace_bytes",
                                            1, H, W, 3)), 4), dtype=torch.uint8,
                         device=img.device)
        out = torch.empty(4, device=img.device)
        grad = torch.empty_like(img)
        _lib.call("gsplat_hip_l1_ssim_loss_fused_fwd", 1, H, W, 3, XS, _ptr(img), _ptr(gt),
                  _ptr(gt_index), ctypes.c_float(lam), _ptr(out), _ptr(grad), _ptr(ws), _stream())
        unit = torch.empty(max(tab.max_points, 1), device=img.device)
        _fwd(img, 3, alphas, tab, cam_index, out[3:], unit)
        ctx.save_for_backward(img, alphas, cam_index, unit, grad)
        ctx.tab = tab
        ctx.spent = False
        return out[0], out[3]

    @staticmethod
    def backward(ctx, g_photo, g_depth):
        from . import losses as _losses
        img, alphas, cam_index, unit, grad = ctx.saved_tensors
        if ctx.spent:  # the depth gradient was scattered into the stored image
            raise RuntimeError("l1_ssim_depth_loss: a second backward through the same node")
        ctx.spent = True
        if g_photo is not None and g_photo is not _losses.ONE_GRAD:
            g_photo = g_photo.float().contiguous()
            scaled = torch.empty_like(grad)
            _lib.call("gsplat_hip_l1_ssim_loss_fused_bwd", grad.numel(), _ptr(grad),
                      _ptr(g_photo), _ptr(scaled), _stream())
            grad = scaled
        v_alphas = torch.empty_like(alphas)
        if g_depth is None:
            g_depth = torch.zeros((), device=img.device)
        elif g_depth.dtype != torch.float32 or not g_depth.is_contiguous():
            g_depth = g_depth.float().contiguous()
        # g_photo None: no photometric term upstream -- the image is zero-filled
        _bwd(img, 3, alphas, ctx.tab, cam_index, unit, g_depth, grad, g_photo is None, v_alphas)
        return grad, v_alphas, None, None, None, None, None


class _ColourChannels(torch.autograd.Function):
    """rgbd[..., :3] as a contiguous image (the bilateral grid's input); the
    backward writes the image-shaped gradient itself -- two strided kernels --
    where autograd's slice backward would zero-fill a new image with a memset,
    which a captured step must not hold."""

    @staticmethod
    def forward(ctx, rgbd):
        ctx.shape = rgbd.shape
        return rgbd[..., :3].contiguous()

    @staticmethod
    def backward(ctx, g):
        out = torch.empty(ctx.shape, dtype=g.dtype, device=g.device)
        out[..., :3].copy_(g)
        out[..., 3:].fill_(0.0)
        return out


def colour_channels(rgbd):
    """The colour channels of an RGB+D render, contiguous (_ColourChannels)."""
    return _ColourChannels.apply(rgbd)


def l1_ssim_depth_loss(rgbd, alphas, gt, ssim_lambda, tab: DepthPoints, cam_index,
                       gt_index=None):
    """The training step's pair (l1_ssim_loss(rgbd, gt, _channels=3), mean
    |disp - 1/d_gt| of image cam_index[0]) of an RGB+D render [1,H,W,4] and
    its alphas [1,H,W,1], as one autograd node (_L1SSIMDepthLoss)."""
    _dev_check(rgbd, alphas, gt, cam_index)
    return _L1SSIMDepthLoss.apply(rgbd, alphas, gt, float(ssim_lambda), gt_index, tab, cam_index)


def table_depth_loss(img, alphas, tab: DepthPoints, cam_index, channel=-1):
    """mean |disp - 1/d_gt| of image cam_index[0] (device int64 [1]) of the
    table on `channel` of a contiguous float32 [1,H,W,XS] image."""
    _dev_check(img, alphas, cam_index)
    XS = img.shape[-1]
    return _TableDepthLoss.apply(img, alphas, tab, cam_index, channel % XS)


def sparse_depth_loss(depths, points, depths_gt, alphas: Optional[torch.Tensor] = None, *,
                      channel: int = -1):
    """The reference trainer's depth term (simple_trainer.py:647-664) without
    its scale: mean |disp - 1/depths_gt| over all C * M points, disp the
    reciprocal (0 where not positive) of the expected depth sampled
    bilinearly (grid_sample, align_corners=True, zero padding) at `points`.

    depths [C,H,W,XS]: channel `channel` is used (a 4-channel render is read
    in place); points [C,M,2] in pixels (x, y); depths_gt [C,M].
    With `alphas` [C,H,W,1], depths is the accumulated depth of an "RGB+D"
    render and the kernel divides by max(alpha, 1e-10) at the corners
    (gradients to both); without, depths is already the expected depth
    ("RGB+ED") and the gradient goes to it alone.  M = 0 gives 0 (torch's
    mean of nothing: NaN); the gradient where disp == 1/depths_gt is 0.
    Multiply by scene_scale * depth_lambda as the reference line does.
    GPU tensors only."""
    if depths.dim() != 4:
        raise ValueError(f"sparse_depth_loss: depths [C,H,W,XS], got {tuple(depths.shape)}")
    C, H, W, XS = depths.shape
    if not -XS <= int(channel) < XS:
        raise ValueError(f"sparse_depth_loss: channel {channel} of {XS}")
    if points.dim() != 3 or points.shape[0] != C or points.shape[2] != 2:
        raise ValueError(f"sparse_depth_loss: points [C,M,2] with C = {C}, got "
                         f"{tuple(points.shape)}")
    M = points.shape[1]
    if tuple(depths_gt.shape) != (C, M):
        raise ValueError(f"sparse_depth_loss: depths_gt [{C},{M}], got {tuple(depths_gt.shape)}")
    if alphas is not None and tuple(alphas.shape) != (C, H, W, 1):
        raise ValueError(f"sparse_depth_loss: alphas [{C},{H},{W},1], got "
                         f"{tuple(alphas.shape)}")
    if C < 1 or H < 1 or W < 1:
        raise ValueError("sparse_depth_loss: empty image")
    if C * M >= 2 ** 31:
        raise ValueError("sparse_depth_loss: more than 2^31 points")
    _dev_check(depths, points, depths_gt, alphas)
    dev = depths.device
    tab = DepthPoints.from_dense(points, depths_gt)
    index = torch.arange(C, dtype=torch.int64, device=dev)
    depths = _f32c(depths)
    alphas = _f32c(alphas)
    total = None
    for c in range(C):
        term = _TableDepthLoss.apply(depths[c:c + 1], None if alphas is None else alphas[c:c + 1],
                                     tab, index[c:c + 1], int(channel) % XS)
        total = term if total is None else total + term
    return total / C
