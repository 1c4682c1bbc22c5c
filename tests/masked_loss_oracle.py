"""Float64 oracle of the masked / composited photometric loss, torch on the
CPU, written apart from gsplat_hip/losses.py:

    x = (m ? c : 0) + b * (1 - a)
    L = (1 - lam) * mean|x - y| + lam * (1 - mean SSIM_valid(x, y))

with the SSIM of train_step.ssim (11x11 Gaussian window, sigma 1.5, "valid"
region, C1 = 0.01^2, C2 = 0.03^2).  loss_and_grads returns L, dL/dc and dL/da
by autograd; closed_forms returns the same two gradients from u = dL/dx as
m ? u : 0 and -sum_ch b_ch u_ch."""

import torch
import torch.nn.functional as F


def _window():
    x = torch.arange(11, dtype=torch.float64) - 5
    w = torch.exp(-(x ** 2) / (2 * 1.5 ** 2))
    return w / w.sum()


def ssim_valid(x, y):
    """Mean SSIM over the valid region of [B,H,W,C] float64 images."""
    x, y = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    C = x.shape[1]
    w = _window()
    wx = w.view(1, 1, 1, -1).repeat(C, 1, 1, 1)
    wy = w.view(1, 1, -1, 1).repeat(C, 1, 1, 1)

    def blur(t):
        return F.conv2d(F.conv2d(t, wx, groups=C), wy, groups=C)

    mu1, mu2 = blur(x), blur(y)
    s11 = blur(x * x) - mu1 * mu1
    s22 = blur(y * y) - mu2 * mu2
    s12 = blur(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return m.mean()


def compose(c, m=None, a=None, b=None):
    """c [B,H,W,C], m [B,H,W] bool or None, a [B,H,W,1], b [B,C] or None."""
    x = c
    if m is not None:
        x = torch.where(m[..., None], x, torch.zeros((), dtype=x.dtype))
    if b is not None:
        x = x + b[:, None, None, :] * (1.0 - a)
    return x


def loss_of(x, y, lam):
    return (1.0 - lam) * (x - y).abs().mean() + lam * (1.0 - ssim_valid(x, y))


def _f64(t):
    return None if t is None else t.detach().double().cpu()


def loss_and_grads(c, y, lam, m=None, a=None, b=None, scale=1.0):
    """(L, d(scale L)/dc, d(scale L)/da or None), float64, by autograd."""
    c, y, a, b = _f64(c), _f64(y), _f64(a), _f64(b)
    m = None if m is None else m.detach().cpu().bool()
    # (a masked pixel's render never reaches the loss: keep non-finite values
    # there out of autograd's 0 * inf)
    if m is not None:
        c = torch.where(m[..., None], c, torch.zeros((), dtype=c.dtype))
    c.requires_grad_(True)
    if b is not None:
        a.requires_grad_(True)
    L = loss_of(compose(c, m, a, b), y, lam)
    (scale * L).backward()
    return L.detach(), c.grad, (a.grad if b is not None else None)


def closed_forms(c, y, lam, m=None, a=None, b=None):
    """(m ? u : 0, -sum_ch b_ch u_ch or None) with u = dL/dx by autograd on x."""
    c, y, a, b = _f64(c), _f64(y), _f64(a), _f64(b)
    m = None if m is None else m.detach().cpu().bool()
    x = compose(c, m, a, b).detach().requires_grad_(True)
    loss_of(x, y, lam).backward()
    u = x.grad
    gc = u if m is None else torch.where(m[..., None], u, torch.zeros((), dtype=u.dtype))
    ga = None if b is None else -(u * b[:, None, None, :]).sum(-1, keepdim=True)
    return gc, ga


def disc_mask(B, H, W, frac=0.45):
    """[B,H,W] bool: a centred disc of radius frac * min(H, W)."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64),
                            torch.arange(W, dtype=torch.float64), indexing="ij")
    r = frac * min(H, W)
    m = (yy - (H - 1) / 2) ** 2 + (xx - (W - 1) / 2) ** 2 <= r * r
    return m[None].repeat(B, 1, 1)


def pixel_mask(B, H, W):
    """[B,H,W] bool: all True but (0,0), (31,31), (32,32), (H-1,W-1) where they exist."""
    m = torch.ones(B, H, W, dtype=torch.bool)
    for i, j in ((0, 0), (31, 31), (32, 32), (H - 1, W - 1)):
        if i < H and j < W:
            m[:, i, j] = False
    return m
