"""Colour-corrected evaluation on the device, backed by libgsplat_hip.so
(csrc/color_correct.hip): the reference's `color_correct`
(examples/lib_bilagrid.py:56-126), which warps a render onto its ground truth
by a quadratic colour map before `cc_psnr` is taken
(examples/simple_trainer.py:906-909).

All leading dimensions are flattened into P rows and fitted jointly.  Per
iteration and output channel the reference solves a masked [P, 10] system with
`torch.linalg.lstsq`; here the 65 masked sums of its normal equations are
accumulated in float64, the 10 x 10 system is solved by a Cholesky
factorisation of the diagonally scaled matrix, and the map is applied in
float64; the iterate is rounded to float32 once per iteration.  A channel whose
system cannot be solved (fewer than 10 unclipped rows, or a pivot below 1e-10)
keeps its values for that iteration and is counted in `fallbacks`, where the
reference asserts or returns what a rank-deficient `lstsq` gives.

Images are data: there is no autograd.  Every launch goes on torch's current
stream, the host reads nothing between the iterations, and two calls on the
same input give the same bits.  There is no CPU or torch fallback.
"""

import torch
from torch import Tensor

from . import _lib
from ._wrapper import _aligned16, _dev_check, _f32c, _ptr, _stream


def color_correct(img: Tensor, ref: Tensor, num_iters: int = 5, eps: float = 0.5 / 255,
                  return_info: bool = False):
    """Warps `img` [..., 3] onto `ref` (same shape), both in [0, 1]: float32
    with `img`'s shape.  `return_info=True` returns (result, {"fallbacks":
    int32 [num_iters, 3]}), 1 where a channel kept its values in an iteration."""
    if img.shape[-1] != ref.shape[-1]:
        raise ValueError(f"img's {img.shape[-1]} and ref's {ref.shape[-1]} channels must match")
    if img.shape[-1] != 3:
        raise ValueError(f"color_correct: the last dimension must be 3, got {img.shape[-1]}")
    if img.shape != ref.shape:
        raise ValueError(f"color_correct: img {list(img.shape)} and ref {list(ref.shape)} differ")
    num_iters = int(num_iters)
    if num_iters < 0:
        raise ValueError(f"color_correct: num_iters {num_iters} < 0")
    if not 0.0 < float(eps) < 0.5:
        raise ValueError(f"color_correct: eps {eps} outside (0, 0.5)")
    _dev_check(img, ref)
    if ref.device != img.device:
        raise _lib.GsplatHipError(f"color_correct: img is on {img.device}, ref on {ref.device}")
    x = _aligned16(_f32c(img.detach()))
    r = _aligned16(_f32c(ref.detach()))
    P = x.numel() // 3
    fallbacks = torch.zeros(num_iters, 3, dtype=torch.int32, device=x.device)
    if num_iters == 0 or P == 0:
        out = x.clone()
    else:
        out = torch.empty_like(x)
        nbytes = _lib.query("gsplat_hip_color_correct_workspace_bytes", P)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        with torch.cuda.device(x.device):
            _lib.call("gsplat_hip_color_correct", P, _ptr(x), _ptr(r), num_iters, float(eps),
                      _ptr(out), _ptr(ws), _ptr(fallbacks), _stream())
    out = out.reshape(img.shape)
    return (out, {"fallbacks": fallbacks}) if return_info else out
