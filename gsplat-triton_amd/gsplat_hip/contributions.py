"""Per-Gaussian contribution scores (csrc/rasterize_score.hip): how much each
Gaussian adds to the rays of a set of views, the quantity that
contribution-based pruning ranks by (LightGaussian's global significance,
RadSplat's max-weight threshold, PUP 3D-GS, Speedy-Splat).

    rasterize_to_contributions  the kernel over given projections and isects
    contribution_scores         cameras in batches: projection, isect, kernel
    prune_splats                row-select a splat dict

With w = alpha * T of a (pixel, Gaussian) pair that the forward rasterizer
blends, a Gaussian's scores are the sum of w (optionally times a per-pixel
weight), the maximum of w and the number of pairs.  One pass over the tiles'
records, no (pixel, Gaussian) pair is ever written to memory.
"""

import math
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._wrapper import (_dev_check, _f32c, _ptr, _stream, fully_fused_projection,
                       isect_offset_encode, isect_tiles)


@torch.no_grad()
def rasterize_to_contributions(
    means2d: Tensor,  # [C, N, 2] or [nnz, 2]
    conics: Tensor,  # [C, N, 3] or [nnz, 3]
    opacities: Tensor,  # [C, N] or [nnz]
    image_width: int,
    image_height: int,
    tile_size: int,
    isect_offsets: Tensor,  # [C, tile_height, tile_width]
    flatten_ids: Tensor,  # [n_isects]
    masks: Optional[Tensor] = None,  # [C, tile_height, tile_width]
    packed: bool = False,
    pixel_weights: Optional[Tensor] = None,  # [C, H, W]
    fold: bool = False,
    out: Optional[Tuple[Tensor, Tensor, Tensor]] = None,
) -> Tuple[Tensor, Tensor, Tensor]:
    """(sum f32, max f32, count i32) per Gaussian row, shaped like `opacities`
    ([C, N] or [nnz]; [N] with fold=True), from the same inputs as
    `rasterize_to_pixels` without colours and backgrounds.

    For every (pixel, Gaussian) pair that `rasterize_to_pixels` blends, with
    w = alpha * T: sum += w * pixel_weights[pixel] (w alone without weights),
    max = max(max, w) (never weighted), count += 1.  `masks` means what it
    means to `rasterize_to_pixels`: masks[tile] == True skips the tile.
    fold=True (dense input only) adds all cameras' rows of a Gaussian into one
    row, so many views need no [C, N] temporaries.  `out` = (sum, max, count)
    of an earlier call accumulates into those buffers (sum +=, max = max,
    count +=) and returns them.

    `max` and `count` have the same bits on every run.  `sum` is added with
    float atomics, one per (Gaussian, tile): the order of the tiles varies, and
    with it the last bits.  Computed under no_grad; there is no backward.
    tile_size must be 16."""
    what = "rasterize_to_contributions"
    if tile_size != 16:
        raise ValueError(f"{what}: tile_size must be 16, got {tile_size}")
    if fold and packed:
        raise ValueError(f"{what}: fold needs dense [C, N] input (a packed row has no camera "
                         "to fold)")
    C, tile_height, tile_width = isect_offsets.shape
    if packed:
        nnz = means2d.size(0)
        assert means2d.shape == (nnz, 2), means2d.shape
        assert conics.shape == (nnz, 3), conics.shape
        assert opacities.shape == (nnz,), opacities.shape
        N, shape = 0, (nnz,)
    else:
        N = means2d.size(1)
        assert means2d.shape == (C, N, 2), means2d.shape
        assert conics.shape == (C, N, 3), conics.shape
        assert opacities.shape == (C, N), opacities.shape
        shape = (N,) if fold else (C, N)
    assert tile_height * tile_size >= image_height, \
        f"Assert Failed: {tile_height} * {tile_size} >= {image_height}"
    assert tile_width * tile_size >= image_width, \
        f"Assert Failed: {tile_width} * {tile_size} >= {image_width}"
    if masks is not None:
        assert masks.shape == isect_offsets.shape, masks.shape
    if pixel_weights is not None:
        assert pixel_weights.shape == (C, image_height, image_width), pixel_weights.shape
    _dev_check(means2d, conics, opacities, isect_offsets, flatten_ids, masks, pixel_weights)
    dev = means2d.device
    if out is None:
        accumulate = 0
        s = torch.empty(shape, dtype=torch.float32, device=dev)
        m = torch.empty(shape, dtype=torch.float32, device=dev)
        n = torch.empty(shape, dtype=torch.int32, device=dev)
    else:
        accumulate = 1
        s, m, n = out
        for t, dt in ((s, torch.float32), (m, torch.float32), (n, torch.int32)):
            if t.shape != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{what}: out must be contiguous (f32, f32, i32) tensors of "
                                 f"shape {list(shape)} on {dev}")
    means2d, conics, opacities = _f32c(means2d), _f32c(conics), _f32c(opacities)
    pw = _f32c(pixel_weights)
    mk = None if masks is None else masks.to(torch.bool).contiguous()
    offsets = isect_offsets.to(torch.int32).contiguous()
    fids = flatten_ids.to(torch.int32).contiguous()
    _lib.call("gsplat_hip_rasterize_score", C, N, s.numel(), image_width, image_height,
              tile_size, tile_width, tile_height, _ptr(means2d), _ptr(conics), _ptr(opacities),
              _ptr(mk), _ptr(pw), _ptr(offsets), fids.numel(), _ptr(fids), int(fold), accumulate,
              _ptr(s), _ptr(m), _ptr(n), _stream())
    return s, m, n


@torch.no_grad()
def contribution_scores(
    means: Tensor,  # [N, 3]
    quats: Optional[Tensor],  # [N, 4]
    scales: Optional[Tensor],  # [N, 3]
    opacities: Tensor,  # [N], activated
    viewmats: Tensor,  # [C, 4, 4]
    Ks: Tensor,  # [C, 3, 3]
    width: int,
    height: int,
    *,
    covars: Optional[Tensor] = None,  # [N, 6] instead of quats and scales
    camera_batch: int = 8,
    pixel_weights: Optional[Tensor] = None,  # [C, H, W]
    near_plane: float = 0.01,
    far_plane: float = 1e10,
    radius_clip: float = 0.0,
    eps2d: float = 0.3,
    rasterize_mode: str = "classic",
) -> Dict[str, Tensor]:
    """{"sum", "max", "count"}, each [N], of a scene over C pinhole cameras:
    the cameras go `camera_batch` at a time through `fully_fused_projection`,
    `isect_tiles`, `isect_offset_encode` and the folded
    `rasterize_to_contributions`, as `rasterization()` renders them (16-pixel
    tiles; "antialiased" multiplies the opacities by the compensations).

    E.g. RadSplat's pruning: `prune_splats(splats, scores["max"] >= 0.01)`."""
    what = "contribution_scores"
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError(f"{what}: rasterize_mode 'classic' or 'antialiased', got "
                         f"{rasterize_mode!r}")
    camera_batch = int(camera_batch)
    if camera_batch < 1:
        raise ValueError(f"{what}: camera_batch must be >= 1, got {camera_batch}")
    C, N = viewmats.size(0), means.size(0)
    assert opacities.shape == (N,), opacities.shape
    if pixel_weights is not None:
        assert pixel_weights.shape == (C, height, width), pixel_weights.shape
    _dev_check(means, opacities, viewmats, Ks, pixel_weights)
    dev = means.device
    out = (torch.zeros(N, dtype=torch.float32, device=dev),
           torch.zeros(N, dtype=torch.float32, device=dev),
           torch.zeros(N, dtype=torch.int32, device=dev))
    tw, th = math.ceil(width / 16), math.ceil(height / 16)
    for a in range(0, C, camera_batch):
        vms, Kb = viewmats[a:a + camera_batch], Ks[a:a + camera_batch]
        B = vms.size(0)
        radii, means2d, depths, conics, comp = fully_fused_projection(
            means, covars, quats, scales, vms, Kb, width, height, eps2d=eps2d,
            near_plane=near_plane, far_plane=far_plane, radius_clip=radius_clip, packed=False,
            calc_compensations=(rasterize_mode == "antialiased"))
        op = opacities[None].expand(B, N)
        if comp is not None:
            op = op * comp
        _, isect_ids, flatten_ids = isect_tiles(means2d, radii, depths, 16, tw, th)
        offsets = isect_offset_encode(isect_ids, B, tw, th)
        rasterize_to_contributions(
            means2d, conics, op, width, height, 16, offsets, flatten_ids,
            pixel_weights=None if pixel_weights is None else pixel_weights[a:a + camera_batch],
            fold=True, out=out)
    return {"sum": out[0], "max": out[1], "count": out[2]}


def prune_splats(splats: Dict[str, Tensor], keep: Tensor) -> Dict[str, Tensor]:
    """A new splat dict (the keys of `load_ply` / `PngCompression.decompress` /
    `merge_splats`) with the rows that `keep` selects: a bool mask [N] or a
    tensor of row indices.  Every tensor of the dict must have N rows."""
    what = "prune_splats"
    if not splats:
        raise ValueError(f"{what}: an empty dict")
    rows = {k: v.shape[0] for k, v in splats.items()}
    N = next(iter(rows.values()))
    if len(set(rows.values())) > 1:
        raise ValueError(f"{what}: the tensors have different numbers of rows: {rows}")
    keep = torch.as_tensor(keep)
    if keep.dtype == torch.bool:
        if keep.shape != (N,):
            raise ValueError(f"{what}: a bool `keep` must have shape [{N}], got "
                             f"{list(keep.shape)}")
    elif keep.dtype in (torch.int32, torch.int64) and keep.dim() == 1:
        if keep.numel() and not (int(keep.min()) >= -N and int(keep.max()) < N):
            raise ValueError(f"{what}: `keep` indexes outside the {N} rows")
        keep = keep.long()
    else:
        raise ValueError(f"{what}: `keep` is a bool mask or a 1-D integer index tensor, got "
                         f"{keep.dtype} {list(keep.shape)}")
    return {k: v[keep.to(v.device)] for k, v in splats.items()}
