"""Bilateral-grid colour correction (examples/lib_bilagrid.py: BilateralGrid,
slice, total_variation_loss; simple_trainer.py `use_bilateral_grid`), fused in
HIP (csrc/bilagrid.hip).

The parameter is the reference's: `grids` float32 [N, 12, L, Hg, Wg], one 3-D
grid of 3x4 affine colour transforms per training image, channel c = 4 i + j
element (i, j) -- checkpoints interchange.  `bilateral_grid_shape=(X, Y, W)`
means Wg = X, Hg = Y, L = W.

    bilagrid_slice(grids, rgb, grid_index)   rgb [B,H,W,3] -> corrected rgb
    bilagrid_tv_loss(grids)                  total variation (a 0-d tensor)
    bilagrid_identity(num, shape, device)    the initial parameter
    bilagrid_lr(it, max_steps, base)         the reference's learning rate
    BilateralGridOptimizer                   the trainer's grids and their Adam

The pixel coordinates are implicit ((x + 0.5) / W, (y + 0.5) / H: the
trainer's meshgrid), the guidance is the BT.601 gray of the pixel."""

import ctypes
import math

import torch

from . import _lib
from ._wrapper import _dev_check, _f32c, _ptr, _stream
from .losses import FusedAdam, SideOptimizer, adam_factors


def _check_grids(grids):
    if grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError(f"bilagrid: grids must be [N, 12, L, Hg, Wg], got {tuple(grids.shape)}")
    N, _, L, Hg, Wg = grids.shape
    if N < 1 or min(L, Hg, Wg) < 2:
        raise ValueError("bilagrid: at least one grid and every grid dimension >= 2, got "
                         f"{tuple(grids.shape)}")
    return N, L, Hg, Wg


def _scalar_grad(g):
    """The upstream scalar as a device float the kernel reads (no scaling launch)."""
    if g.dtype != torch.float32 or not g.is_contiguous():
        g = g.float().contiguous()
    return g


def _slice_fwd(grids, rgb, index):
    N, L, Hg, Wg = grids.shape[0], grids.shape[2], grids.shape[3], grids.shape[4]
    B, H, W = rgb.shape[:3]
    out = torch.empty_like(rgb)
    _lib.call("gsplat_hip_bilagrid_slice_fwd", B, H, W, N, L, Hg, Wg, _ptr(grids), _ptr(index),
              _ptr(rgb), _ptr(out), _stream())
    return out


def _slice_bwd(grids, rgb, index, v_out, v_grids):
    """v_rgb; the grid gradient is added to v_grids (initialised by the caller)."""
    N, L, Hg, Wg = grids.shape[0], grids.shape[2], grids.shape[3], grids.shape[4]
    B, H, W = rgb.shape[:3]
    v_out = _f32c(v_out)
    v_rgb = torch.empty_like(rgb)
    ws = torch.empty(max(int(_lib.query("gsplat_hip_bilagrid_slice_workspace_bytes", B, H, W, L,
                                        Hg, Wg)), 16), dtype=torch.uint8, device=rgb.device)
    _lib.call("gsplat_hip_bilagrid_slice_bwd", B, H, W, N, L, Hg, Wg, _ptr(grids), _ptr(index),
              _ptr(rgb), _ptr(v_out), _ptr(v_rgb), _ptr(v_grids), _ptr(ws), _stream())
    return v_rgb


def _tv_fwd(grids, scale):
    N, L, Hg, Wg = grids.shape[0], grids.shape[2], grids.shape[3], grids.shape[4]
    ws = torch.empty(max(int(_lib.query("gsplat_hip_bilagrid_tv_workspace_bytes", N, L, Hg, Wg)),
                         4), dtype=torch.uint8, device=grids.device)
    out = torch.empty(2, device=grids.device)
    _lib.call("gsplat_hip_bilagrid_tv_fwd", N, L, Hg, Wg, _ptr(grids), ctypes.c_float(scale),
              _ptr(out), _ptr(ws), _stream())
    return out


def _tv_bwd(grids, scale, g):
    """g * scale * dtv/dgrids, every element written (no zero fill)."""
    N, L, Hg, Wg = grids.shape[0], grids.shape[2], grids.shape[3], grids.shape[4]
    v = torch.empty_like(grids)
    _lib.call("gsplat_hip_bilagrid_tv_bwd", N, L, Hg, Wg, _ptr(grids), ctypes.c_float(scale),
              _ptr(_scalar_grad(g)), _ptr(v), _stream())
    return v


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, rgb, index):
        ctx.save_for_backward(grids, rgb, index)
        return _slice_fwd(grids, rgb, index)

    @staticmethod
    def backward(ctx, v_out):
        grids, rgb, index = ctx.saved_tensors
        v_grids = torch.zeros_like(grids)
        v_rgb = _slice_bwd(grids, rgb, index, v_out, v_grids)
        need = ctx.needs_input_grad
        return v_grids if need[0] else None, v_rgb if need[1] else None, None


class _TV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        ctx.save_for_backward(grids)
        return _tv_fwd(grids, 1.0)[0]

    @staticmethod
    def backward(ctx, g):
        (grids,) = ctx.saved_tensors
        return _tv_bwd(grids, 1.0, g)


class _SliceTV(torch.autograd.Function):
    """The training step's pair: (slice(rgb), scale * tv).  Its backward
    writes the dense grid gradient once -- the total-variation backward stores
    every element, the slice's finish adds the indexed images' node sums -- so
    there is neither a zero fill nor an add of two dense gradients."""

    @staticmethod
    def forward(ctx, grids, rgb, index, scale):
        ctx.save_for_backward(grids, rgb, index)
        ctx.scale = float(scale)
        return _slice_fwd(grids, rgb, index), _tv_fwd(grids, ctx.scale)[0]

    @staticmethod
    def backward(ctx, v_out, g_tv):
        grids, rgb, index = ctx.saved_tensors
        v_grids = torch.zeros_like(grids) if g_tv is None else _tv_bwd(grids, ctx.scale, g_tv)
        v_rgb = None if v_out is None else _slice_bwd(grids, rgb, index, v_out, v_grids)
        return v_grids, v_rgb if ctx.needs_input_grad[1] else None, None, None


def _prepare(grids, rgb, grid_index):
    N, L, Hg, Wg = _check_grids(grids)
    if rgb.dim() != 4 or rgb.shape[-1] != 3:
        raise ValueError(f"bilagrid_slice: rgb must be [B, H, W, 3], got {tuple(rgb.shape)}")
    _dev_check(grids, rgb)
    B = rgb.shape[0]
    if torch.is_tensor(grid_index):
        _dev_check(grid_index)
        index = grid_index.reshape(-1)
        if index.dtype != torch.int64:
            index = index.long()
        index = index.contiguous()
    else:
        vals = [int(grid_index)] * B if isinstance(grid_index, int) else [int(v) for v in grid_index]
        if any(v < 0 or v >= N for v in vals):
            raise IndexError(f"bilagrid_slice: grid_index {vals} out of range for {N} grids")
        index = torch.tensor(vals, dtype=torch.int64, device=rgb.device)
    if index.numel() != B:
        raise ValueError(f"bilagrid_slice: {index.numel()} indices for a batch of {B}")
    return _f32c(grids), _f32c(rgb), index


def bilagrid_slice(grids, rgb, grid_index):
    """Slice the bilateral grids by pixel position and gray guidance and apply
    the 3x4 affine transforms: for pixel (x, y) of rgb[b] ([B,H,W,3]) with the
    grid grids[grid_index[b]],

        A = trilinear(grid; (x+0.5)/W (Wg-1), (y+0.5)/H (Hg-1), clamp(gray,0,1) (L-1))
        out = A[:, :3] @ rgb + A[:, 3],    gray = 0.299 r + 0.587 g + 0.114 b

    (lib_bilagrid.slice on the trainer's pixel meshgrid: grid_sample with
    align_corners=True and border padding).  `grid_index`: a device int64 [B]
    tensor, read on the device (no synchronisation; values are clamped to the
    valid range), or a Python int / sequence (checked).  Gradients go to
    `grids` (dense; rows of images not indexed are zero) and `rgb`; the
    gradient through the guidance is zero where gray <= 0 or gray >= 1, as
    torch's clamp.  GPU tensors only; ValueError for a grid dimension < 2."""
    grids, rgb, index = _prepare(grids, rgb, grid_index)
    return _Slice.apply(grids, rgb, index)


def bilagrid_tv_loss(grids):
    """lib_bilagrid.total_variation_loss of the grids: the mean squared
    forward difference along L, Hg and Wg, summed over the three axes and
    averaged over the N grids.  Reduced in a fixed order (bit-identical
    between calls)."""
    _check_grids(grids)
    _dev_check(grids)
    return _TV.apply(_f32c(grids))


def _slice_tv(grids, rgb, grid_index, scale):
    """(bilagrid_slice, scale * bilagrid_tv_loss) with one dense gradient
    write (the training step; see _SliceTV)."""
    grids, rgb, index = _prepare(grids, rgb, grid_index)
    return _SliceTV.apply(grids, rgb, index, float(scale))


def bilagrid_identity(num, shape=(16, 16, 8), device=None):
    """The initial parameter: `num` identity grids [num, 12, L, Hg, Wg] for
    shape = (X, Y, W) = (Wg, Hg, L); channels 0, 5 and 10 (the diagonal of the
    3x4 matrix) are 1, the rest 0."""
    X, Y, Wd = (int(v) for v in shape)
    if int(num) < 1 or min(X, Y, Wd) < 2:
        raise ValueError(f"bilagrid_identity: num >= 1 and every grid dimension >= 2, got "
                         f"num={num}, shape={tuple(shape)}")
    grids = torch.zeros((int(num), 12, Wd, Y, X), dtype=torch.float32, device=device)
    grids[:, [0, 5, 10]] = 1.0
    return grids


def bilagrid_lr(it, max_steps, base=2e-3):
    """The learning rate of step `it` (0-based): the reference chains
    LinearLR(start_factor=0.01, total_iters=1000) with
    ExponentialLR(gamma=0.01 ** (1 / max_steps)); `base` alone when max_steps
    is None (no schedule, as the means')."""
    if not max_steps:
        return float(base)
    warm = 0.01 + 0.99 * min(int(it), 1000) / 1000.0
    return float(base) * warm * math.pow(0.01, int(it) / float(max_steps))


class BilateralGridOptimizer(SideOptimizer):
    """Trainer(bilateral_grid=True)'s `grids` [n_images, 12, L, Hg, Wg] and their
    optimizer `opt` (simple_trainer.py:300-318): Adam(lr 2e-3 sqrt(BS), eps 1e-15)
    stepped densely every step, its lr on the chained schedule (bilagrid_lr)."""

    name = "bil"
    TV_WEIGHT = 10.0  # simple_trainer.py:664: loss += 10 * tv

    def __init__(self, n_images, shape, device, batch_size=1, max_steps=None):
        self.shape = tuple(int(v) for v in shape)
        if len(self.shape) != 3 or min(self.shape) < 2:
            raise ValueError(f"bilateral_grid_shape: (X, Y, W), each >= 2, got {shape!r}")
        self.grids = torch.nn.Parameter(bilagrid_identity(n_images, self.shape, device=device))
        self.lr, self.max_steps = 2e-3 * math.sqrt(batch_size), max_steps
        self.opt = FusedAdam([self.grids], [self.lr], betas=(0.9, 0.999), eps=1e-15)

    step_count = property(lambda self: self.opt.step_count,  # (FusedAdam.step's own count)
                          lambda self, n: setattr(self.opt, "step_count", n))

    def slice_tv(self, colors, cam_index):
        """(`colors` through the grid of the device index `cam_index`, TV_WEIGHT x
        the grids' total variation): simple_trainer.py:620-630, 663-665."""
        return _slice_tv(self.grids, colors, cam_index, self.TV_WEIGHT)

    def factors(self, it):
        """The grids' Adam: its own betas, the chained schedule's lr (set here)."""
        self.opt.lrs[0] = bilagrid_lr(it, self.max_steps, self.lr)
        return adam_factors(self.opt.lrs, self.opt.betas, self.opt.step_count + 1)[0]

    def launch(self, s, hyper):
        if hyper is None:
            self.factors(s.it)  # (sets this step's learning rate)
            self.opt.step()
        else:
            self.opt.step(hyper=hyper, void=s.void)
        self.opt.zero_grad()

    def moments(self):
        return {"bil_grids": [self.opt.exp_avg[0], self.opt.exp_avg_sq[0]]}

    def checkpoint_tables(self):
        return {}, {"bil_grids": self.grids}
