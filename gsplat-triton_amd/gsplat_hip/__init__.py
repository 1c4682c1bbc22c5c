"""gsplat_hip -- MI355X (gfx950) backend for the gsplat rasterization hot path.

Exports the backend surface that gsplat/rendering.py imports from
`gsplat.triton_impl._wrapper` (rendering.py:20-27), implemented with
hand-written HIP kernels behind the C ABI in include/gsplat_hip.h, plus a
`rasterization()` front-end mirroring gsplat/rendering.py:44-598.
"""

from ._wrapper import (
    fully_fused_projection,
    isect_offset_encode,
    isect_tiles,
    rasterize_to_pixels,
    spherical_harmonics,
)
from ._wrapper_aux import SelectiveAdam, adam, compute_relocation, quat_scale_to_covar_preci
from ._wrapper_covar import proj, world_to_cam
from ._wrapper_2dgs import fully_fused_projection_2dgs, rasterize_to_pixels_2dgs
from ._wrapper_indices import (
    accumulate,
    accumulate_2dgs,
    rasterize_to_indices_in_range,
    rasterize_to_indices_in_range_2dgs,
)
from .appearance import appearance_colors
from .bilagrid import bilagrid_identity, bilagrid_lr, bilagrid_slice, bilagrid_tv_loss
from .color_correct import color_correct
from .compression import PngCompression
from .depth_loss import sparse_depth_loss
from .io import load_ply, save_ply
from .losses import geometry_loss_2dgs
from .mesh import TSDFVolume, save_mesh_ply
from .pose import pose_adjust
from .rendering import depth_to_normal, rasterization, rasterization_2dgs
from .transform import merge_splats, rotate_sh, sh_rotation_matrices, transform_splats
from .undistort import remap_bilinear, undistort_images

__all__ = [
    "fully_fused_projection",
    "isect_tiles",
    "isect_offset_encode",
    "spherical_harmonics",
    "rasterize_to_pixels",
    "rasterization",
    "fully_fused_projection_2dgs",
    "rasterize_to_pixels_2dgs",
    "rasterization_2dgs",
    "depth_to_normal",
    "geometry_loss_2dgs",
    "sparse_depth_loss",
    "bilagrid_slice",
    "bilagrid_tv_loss",
    "bilagrid_identity",
    "bilagrid_lr",
    "pose_adjust",
    "appearance_colors",
    "PngCompression",
    "color_correct",
    "quat_scale_to_covar_preci",
    "world_to_cam",
    "proj",
    "compute_relocation",
    "adam",
    "SelectiveAdam",
    "rasterize_to_indices_in_range",
    "rasterize_to_indices_in_range_2dgs",
    "accumulate",
    "accumulate_2dgs",
    "undistort_images",
    "remap_bilinear",
    "save_ply",
    "load_ply",
    "TSDFVolume",
    "save_mesh_ply",
    "transform_splats",
    "rotate_sh",
    "sh_rotation_matrices",
    "merge_splats",
]
__version__ = "0.1.0"
