"""One 3DGS training step over the HIP hot path (the unit bench.py measures).

Mirrors the per-iteration work of examples/simple_trainer.py with its default
config (sh_degree 3, packed=False, classic rasterize mode, batch 1):
  render (simple_trainer.py:453-507, 603-615) -> loss 0.8*L1 + 0.2*(1-SSIM,
  "valid" padding) (:642-646) -> backward (:683) -> DefaultStrategy running
  statistics (gsplat/strategy/default.py:213-262) -> Adam on every parameter
  group with the trainer's learning rates and batch scaling (:235-277).

Trainer._run_step is that step, and the only place that issues one: the
eager step (_eager_step) and the graph-replayed step (graph_step.GraphStep)
call it with a StepInputs record saying where the step's inputs live -- host
values and views of the step's camera, or views of the captured step's input
block, its void flag and its rings.  The Adam optimizers beside the
Gaussians' (the bilateral grids', the pose table's, the appearance module's)
own their state (losses.SideOptimizer: Trainer.bil, .pose, .app) and are one
ordered list, Trainer.side_opts.

model="2dgs" runs examples/simple_trainer_2dgs.py's default step instead:
rasterization_2dgs(render_mode="RGB+D") (simple_trainer_2dgs.py:549-563), the
same loss on the RGB channels (:590-594), and the strategy statistics from
meta["gradient_2dgs"] (key_for_gradient, :307-311).  `normal_loss` /
`dist_loss` (off by default, :149-160) add the normal-consistency and depth
distortion terms (:611-632) from their start iterations on: the step then
renders the normal and distortion images with the general surfel rasterizer
and adds losses.geometry_loss_2dgs (one fused HIP launch pair); before, it
is the colours-only step unchanged (the reference multiplies the terms by 0).

`bilateral_grid=True` (3DGS, simple_trainer.py `use_bilateral_grid`): the
render goes through the camera's bilateral grid before the loss
(bilagrid.bilagrid_slice) and 10 x the grids' total variation is added; the
grids `bil.grids` [cameras, 12, L, Hg, Wg] have their own FusedAdam, stepped
densely every step.  evaluate() renders without the grid.

`pose_opt=True` (3DGS, simple_trainer.py `pose_opt`): the camera is adjusted
by its row of `pose.embeds` [cameras, 9] before the render (pose.pose_apply,
`pose_noise` a fixed perturbation applied first), the projection backward
that runs the geometry Adam also leaves the pose partials, and
pose.pose_bwd_adam turns them into the row's gradient and steps the table's
dense Adam with L2 weight decay -- no view matrix requires grad, the step
stays fused and graph-replayed.  evaluate() renders the cameras unadjusted.

`depth_loss=True` (3DGS, simple_trainer.py `depth_loss` / `depth_lambda`):
the step renders RGB+D and adds depth_lambda * scene_scale * the mean
disparity L1 at the image's projected SfM points (`depth_points`, one
(points, depths) pair per training image as colmap.Dataset(load_depths=True)
gives them; kept as CSR tables on the device).  The photometric loss and the
depth term are one autograd node (depth_loss.l1_ssim_depth_loss): one extra
launch forward, a zero fill and a scatter backward, the image chosen by a
device index, so the step stays fused and graph-replayed.

`app_opt=True` (3DGS, simple_trainer.py `app_opt` / `app_embed_dim` /
`app_opt_lr` / `app_opt_reg`): the colours come from the appearance MLP
(appearance.py) over the groups `features` [N,32] and `colors` [N,3] (logits),
which replace sh0 / shN, the step's row of `app.embeds` [cameras, 16] and the
view direction's SH bases at the step's degree; evaluated after the projection
under its radii mask, the means gradient handed to the geometry Adam as the SH
backward's is.  One more launch sums the backward's partial sums and steps the
module's two Adam optimizers (head `app.head`; the table at 10 x the rate with
weight decay, densely).  evaluate() renders with the zero embedding.

With `strategy=DefaultStrategyConfig()` the step also runs the reference's
DefaultStrategy schedule after the optimizer step (simple_trainer.py:808-826
-> gsplat/strategy/default.py:164-211): refine (grow + prune, one HIP
compaction of every parameter and both Adam moments, gsplat_hip.densify)
every `refine_every` steps in (refine_start_iter, refine_stop_iter), opacity
reset every `reset_every` steps.  `sh_degree_interval` enables the SH degree
schedule (simple_trainer.py:600), `max_steps` the means ExponentialLR
(:523-528), `init="sfm"` the SfM initialisation with knn scales, uniform
quaternions and init_opacity (:212-233).

With `strategy=MCMCStrategyConfig()` (gsplat_hip.mcmc) it runs MCMCStrategy
instead (simple_trainer.py:821-829 -> gsplat/strategy/mcmc.py:103-187): no
statistics; after the optimizer step, on refine steps the dead Gaussians are
relocated and 5 % are sampled in (up to cap_max), and every step the
positions get covariance-shaped noise (one fused HIP launch, its normal
draw made in the kernel from the trainer's key and the step) scaled by the
means learning rate of the next step.  With graph=True the steps between
refines are replays with the noise inside; the refines run eagerly.

Multi-GPU, two schemes, one process per GPU, every rank rendering its own
camera each step:
* `gaussian_shard=True` (the reference's multi-GPU training,
  simple_trainer.py:227-229,501 with gsplat/rendering.py:298-494): rank r
  holds the Gaussians [r::world] with their own Adam state and strategy
  statistics; the render is rasterization(distributed=True) -- the local
  Gaussians projected into every rank's camera, the projected pairs
  exchanged peer to peer over RCCL/xGMI, each rank rasterizing its camera
  with all Gaussians -- and the backward exchanges their gradients back, so
  each Gaussian's owner receives its gradient summed over all cameras.  No
  gradient all-reduce: per step a rank moves its shard's projected pairs
  (44 B each way per (Gaussian, camera)), not the whole scene's gradients.
  Densification runs per rank on its own shard, as the reference does.
* replicated (`sharded_optimizer`): every rank holds all Gaussians; the
  gradients are summed over RCCL/xGMI by reduce-scatter, each rank runs Adam
  on its share of the rows, and the updated rows are all-gathered
  (distributed.ShardedAdam; the plain per-group all-reduce + full Adam is
  `sharded_optimizer=False`).  Before a refine the densification statistics
  are summed over the ranks and the split noise comes from a generator seeded
  identically on every rank, so the replicas stay identical.
"""

import dataclasses
import math
import os
from typing import Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import densify
from .densify import DefaultStrategyConfig
from . import mcmc as _mcmc
from .mcmc import MCMCStrategyConfig
from .color_correct import color_correct as _color_correct
from .losses import FusedAdam, l1_ssim_loss, ssim_and_l1
from . import _lib, _wrapper
from .appearance import AppearanceOptimizer
from .bilagrid import BilateralGridOptimizer
from .pose import PoseOptimizer
from .rendering import rasterization, rasterization_2dgs
from .strategy import activate, update_state_

C0 = 0.28209479177387814


def rgb_to_sh(rgb):
    return (rgb - 0.5) / C0


def load_garden_scene(path: str, scene_grid: int = 3):
    """load_test_data(scene_grid) semantics (gsplat/_helper.py:9-55) on the
    cropped garden fixture: tile the [-2,2]^3 crop into a scene_grid^2 grid."""
    d = np.load(path)
    means = torch.from_numpy(d["means3d"]).float()
    colors = torch.from_numpy(d["colors"].astype(np.float32) / 255.0)
    edges = torch.tensor([4.0, 4.0, 4.0])
    r = scene_grid // 2
    gx, gy = torch.meshgrid(torch.arange(-r, r + 1), torch.arange(-r, r + 1), indexing="ij")
    grid = torch.stack([gx, gy, torch.zeros_like(gx)], -1).reshape(-1, 3).float()
    means = (means[None] + grid[:, None] * edges).reshape(-1, 3)
    colors = colors.repeat(scene_grid ** 2, 1)
    return (means, colors, torch.from_numpy(d["viewmats"]), torch.from_numpy(d["Ks"]),
            int(d["width"]), int(d["height"]))


def camera_pool(viewmats, Ks, src_w, src_h, width, height, n, seed=0):
    """`n` cameras: the scene's own cameras first, then small jitters of them;
    intrinsics rescaled to width x height as profiling/main.py:85-87."""
    g = torch.Generator().manual_seed(seed)
    K = Ks.clone()
    K[:, 0, :] *= width / src_w
    K[:, 1, :] *= height / src_h
    vms, ks = [], []
    for i in range(n):
        v = viewmats[i % len(viewmats)].clone()
        if i >= len(viewmats):
            v[:3, 3] += torch.randn(3, generator=g) * 0.05
        vms.append(v)
        ks.append(K[i % len(K)])
    return torch.stack(vms), torch.stack(ks)


def knn_log_scales(points: torch.Tensor, init_scale: float = 1.0) -> torch.Tensor:
    """log of the RMS distance to the 3 nearest neighbours, repeated over the
    3 axes (simple_trainer.py:221-224 with examples/utils.py:141-151 knn):
    the SfM initialisation's scales.  One-off host work (a k-d tree)."""
    from scipy.spatial import cKDTree
    pts = points.detach().cpu().double().numpy()
    d, _ = cKDTree(pts).query(pts, k=4, workers=-1)
    dist2_avg = torch.from_numpy((d[:, 1:] ** 2).mean(-1)).float()
    return torch.log(torch.sqrt(dist2_avg) * init_scale).unsqueeze(-1).repeat(1, 3)


def _gauss_window(size=11, sigma=1.5, device="cpu"):
    x = torch.arange(size, dtype=torch.float32, device=device) - size // 2
    w = torch.exp(-(x ** 2) / (2 * sigma ** 2))
    return w / w.sum()


def ssim(img1, img2, window=None):
    """Mean SSIM with an 11x11 Gaussian window (sigma 1.5), "valid" padding --
    the quantity fused_ssim(..., padding="valid") returns. img: [B,C,H,W]."""
    Cc = img1.shape[1]
    w = _gauss_window(device=img1.device) if window is None else window
    wx = w.view(1, 1, 1, -1).repeat(Cc, 1, 1, 1)
    wy = w.view(1, 1, -1, 1).repeat(Cc, 1, 1, 1)

    def blur(x):
        return F.conv2d(F.conv2d(x, wx, groups=Cc), wy, groups=Cc)

    mu1, mu2 = blur(img1), blur(img2)
    s11 = blur(img1 * img1) - mu1 * mu1
    s22 = blur(img2 * img2) - mu2 * mu2
    s12 = blur(img1 * img2) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return m.mean()


def _mean(x: torch.Tensor) -> torch.Tensor:
    """x.mean() as reductions that each give one output per workgroup: rows
    of 1024, then the row sums (and the tail).  torch's one-output reduction
    of a large tensor splits it over workgroups with a zero-filled semaphore
    buffer -- a memset node, which a captured step must not hold
    (graph_step.check_kernel_nodes_only) -- e.g. the regularisers of
    simple_trainer's mcmc preset at a million Gaussians."""
    x = x.reshape(-1)
    n = x.numel()
    q = n // 1024
    if q == 0:
        return x.sum() / n
    s = x[:q * 1024].view(q, 1024).sum(1).sum()
    if n > q * 1024:
        s = s + x[q * 1024:].sum()
    return s / n


@dataclasses.dataclass
class StepInputs:
    """Where one training step's inputs live (Trainer._run_step).  The eager
    step fills it from host values and views of its camera `ci`, everything
    device-side None; the captured step (graph_step.GraphStep) from the views
    of its input block, its void flag and its rings."""
    deg: int  # SH degree
    terms: tuple  # 2DGS (normal_lambda, dist_lambda), geometry_terms_at
    stats: bool  # accumulate the DefaultStrategy statistics
    viewmats: torch.Tensor  # [W,4,4], W = 1 or the Gaussian-sharded world (rank order)
    Ks: torch.Tensor  # [W,3,3]
    cam: torch.Tensor  # device int64 [1]: the step's image
    targets: torch.Tensor  # the image's target [1,H,W,3], or all of them with gt_index
    gt_index: Optional[torch.Tensor] = None
    c2w: Optional[torch.Tensor] = None  # 2DGS: the camera-to-world [1,4,4]
    it: Optional[int] = None  # host factors: the step index their schedules read
    fetch: Optional[tuple] = None  # activate's: the first launch fetches the input block
    isect: dict = dataclasses.field(default_factory=dict)  # the sync-free isect's keywords
    void: Optional[torch.Tensor] = None  # device i32 flag: every state update reads it
    hyper: Optional[torch.Tensor] = None  # the Gaussians' Adam factors (Trainer._layout order)
    side_hyper: dict = dataclasses.field(default_factory=dict)  # SideOptimizer.name -> factors
    loss_ring: Optional[tuple] = None  # l1_ssim_loss's _out_ring
    bkgd: Optional[torch.Tensor] = None  # random_bkgd: the step's colour, device float32 [1,3]
    vote: bool = False  # several ranks: agree on the void flag beside the loss kernels
    capturing: bool = False  # sharded optimizer: collectives in order, no deferred gather
    geom_applied: bool = False  # _run_step sets it: Trainer.geom_applied, for the side launches


# Trainer options of the one-GPU dense trainer, and the companions (Trainer.
# __init__'s `asked`) each is refused with
_MANY = ("gaussian_shard", "sharded_optimizer", "world_size")
_SPARSE = ("packed", "sparse_grad", "visible_adam")
# option -> (the trainer it runs in, the companions it is refused with)
_REFUSALS = {
    "app_opt": ("the one-GPU dense fused 3DGS trainer only",
                ("pose_opt", "pose_noise", "model='2dgs'") + _SPARSE + _MANY + ("fused=False",)),
    "depth_loss": ("the one-GPU dense fused 3DGS trainer only",
                   ("model='2dgs'",) + _SPARSE + _MANY + ("fused=False",)),
    "pose": ("the one-GPU dense fused 3DGS trainer with the geometry Adam in the projection "
             "backward only",
             ("model='2dgs'",) + _SPARSE + ("antialiased", "opacity_reg", "scale_reg") + _MANY
             + ("fused=False", "GSPLAT_HIP_GEOM_FUSE=0", "GSPLAT_HIP_GEOM_IN_PROJ=0")),
    "bilateral_grid": ("the one-GPU dense 3DGS trainer only", ("model='2dgs'",) + _SPARSE + _MANY),
    # (the mask belongs before the grid's slice, and the depth step has a loss
    # node of its own: both are follow-ups)
    "masks": ("the one-GPU dense 3DGS trainer only",
              ("model='2dgs'",) + _SPARSE + _MANY + ("bilateral_grid", "depth_loss")),
    "random_bkgd": ("the one-GPU dense 3DGS trainer only",
                    ("model='2dgs'",) + _SPARSE + _MANY + ("bilateral_grid", "depth_loss")),
    "normal_loss / dist_loss": ("the one-GPU dense 2DGS trainer only",
                                ("packed", "sparse_grad") + _MANY),
    "compression": ("one-GPU trainers only", _MANY),
    "checkpoint": ("one-GPU trainers only", _MANY),
    "mesh": ("one-GPU trainers only", _MANY),
}


def _refuse(option, asked, name=None):
    """NotImplementedError naming `option` (as `name`) and every companion of
    its _REFUSALS row that the constructor's arguments ask for (`asked`)."""
    scope, companions = _REFUSALS[option]
    off = [c for c in companions if asked[c]]
    if off:
        raise NotImplementedError(f"{name or option}: {scope}; not with {', '.join(off)}")


def _one_grad(device):
    """The constant 1.0 seed of the fused loss's backward (no fill launch; the
    backward recognises it and skips its scaling launch), made outside a
    capture."""
    from . import losses as _losses
    if _losses.ONE_GRAD is None or _losses.ONE_GRAD.device != device:
        _losses.ONE_GRAD = torch.ones((), device=device)
    return _losses.ONE_GRAD


class Trainer:
    """Holds the Gaussian parameters, Adam state and strategy statistics."""

    # every option flag and lazily set attribute has its default here, so a
    # Trainer that did not go through __init__ (a test's skeleton) reads them too
    model = "3dgs"
    bilateral_grid = pose_opt = depth_loss = app_opt = False
    pose_noise = 0.0
    masks = None
    random_bkgd = False
    normal_loss = dist_loss = False
    gshard = packed = sparse_grad = visible_adam = mcmc = False
    sh_adam_in_bwd = geom_fuse = geom_in_proj = geom_applied = False
    rasterize_mode = "classic"
    opacity_reg = scale_reg = 0.0
    dp_emulate_world = _sh_pg = None
    # the owners of the grids', the pose table's and the appearance module's state
    # (None: off); `sides`: those that exist; `side_opts`: those optimised, launch order
    bil = pose = app = None
    sides = side_opts = ()
    _graph = graph_fallback = None
    _param_gen = 0
    split_div = split_threshold = None
    _split_tuned = False

    LRS = {"means": 1.6e-4, "scales": 5e-3, "quats": 1e-3, "opacities": 5e-2,
           "sh0": 2.5e-3, "shN": 2.5e-3 / 20, "features": 2.5e-3, "colors": 2.5e-3}

    def __init__(self, points, rgbs, viewmats, Ks, width, height, sh_degree=3, device="cuda",
                 seed=42, world_size=1, rank=0, ssim_lambda=0.2, scene_scale=1.0,
                 fused=True, model="3dgs", sharded_optimizer=None,
                 strategy: Optional[Union[DefaultStrategyConfig, MCMCStrategyConfig]] = None,
                 sh_degree_interval: Optional[int] = None, max_steps: Optional[int] = None,
                 init: str = "random", init_opacity: float = 0.1, init_scale: float = 1.0,
                 targets: Optional[torch.Tensor] = None, opacity_reg: float = 0.0,
                 scale_reg: float = 0.0, dp_emulate_world: Optional[int] = None,
                 graph: bool = False, isect_capacity: Optional[int] = None,
                 gaussian_shard: bool = False, visible_adam: bool = False,
                 packed: bool = False, sparse_grad: bool = False, antialiased: bool = False,
                 normal_loss: bool = False, normal_lambda: float = 5e-2,
                 normal_start_iter: int = 7000, dist_loss: bool = False,
                 dist_lambda: float = 1e-2, dist_start_iter: int = 3000,
                 bilateral_grid: bool = False, bilateral_grid_shape=(16, 16, 8),
                 pose_opt: bool = False, pose_opt_lr: float = 1e-5, pose_opt_reg: float = 1e-6,
                 pose_noise: float = 0.0, depth_loss: bool = False, depth_lambda: float = 1e-2,
                 depth_points=None, app_opt: bool = False, app_embed_dim: int = 16,
                 app_opt_lr: float = 1e-3, app_opt_reg: float = 1e-6,
                 masks: Optional[torch.Tensor] = None, random_bkgd: bool = False):
        assert model in ("3dgs", "2dgs"), model
        assert init in ("random", "sfm"), init
        # the options of the one-GPU dense trainer, each refused with what it
        # does not run with (_REFUSALS) before any device work
        env = os.environ.get
        asked = {
            "pose_opt": pose_opt, "pose_noise": float(pose_noise) != 0.0,
            "model='2dgs'": model != "3dgs", "packed": packed, "sparse_grad": sparse_grad,
            "visible_adam": visible_adam, "antialiased": antialiased,
            "opacity_reg": float(opacity_reg) != 0.0, "scale_reg": float(scale_reg) != 0.0,
            "gaussian_shard": gaussian_shard, "sharded_optimizer": sharded_optimizer,
            "world_size": world_size != 1, "fused=False": not fused,
            "GSPLAT_HIP_GEOM_FUSE=0": env("GSPLAT_HIP_GEOM_FUSE", "1") == "0",
            "GSPLAT_HIP_GEOM_IN_PROJ=0": env("GSPLAT_HIP_GEOM_IN_PROJ", "1") == "0",
            "bilateral_grid": bool(bilateral_grid), "depth_loss": bool(depth_loss)}
        # simple_trainer.py:505-506 (masks: the render zeroed outside each
        # image's mask before the loss -- an undistorted fisheye image's
        # validity mask, colmap.scene_tensors(parser)["masks"], or the user's
        # own) and random_bkgd (:629-631: a fresh random colour under the
        # render every step); both composed inside the loss kernel
        # (losses.l1_ssim_loss masks / alphas / backgrounds)
        self.random_bkgd = bool(random_bkgd)
        if masks is not None:
            _refuse("masks", asked)
            if masks.dtype != torch.bool or tuple(masks.shape) != (len(viewmats), height, width):
                raise ValueError(f"masks: bool [{len(viewmats)}, {height}, {width}] (True = "
                                 f"valid), got {masks.dtype} {list(masks.shape)}")
            # one uint8 table on the device beside the targets: the loss picks
            # the step's image by the device index it picks the target by
            self.masks = masks.to(device).contiguous().view(torch.uint8)
        if self.random_bkgd:
            _refuse("random_bkgd", asked)
        # simple_trainer.py app_opt / app_embed_dim / app_opt_lr / app_opt_reg
        # (:243-254, 389-410): the colours from appearance.AppearanceOptimizer
        self.app_opt = bool(app_opt)
        self.app_opt_reg = float(app_opt_reg)
        if self.app_opt:
            _refuse("app_opt", asked)
            self.app = AppearanceOptimizer(
                len(viewmats), rgbs, device, seed, float(app_opt_lr) * math.sqrt(world_size),
                self.app_opt_reg, app_embed_dim, sh_degree)
        # simple_trainer.py depth_loss / depth_lambda (:163-165, 647-665): the
        # disparity L1 at each image's projected SfM points (depth_loss.py),
        # added to the loss times depth_lambda * scene_scale; the step then
        # renders RGB+D
        self.depth_loss, self.depth_lambda = bool(depth_loss), float(depth_lambda)
        if self.depth_loss:
            _refuse("depth_loss", asked)
            if depth_points is None:
                raise ValueError("depth_loss: depth_points, one (points [M, 2], depths [M]) per "
                                 "training image, is required")
            if len(depth_points) != len(viewmats):
                raise ValueError(f"depth_loss: {len(depth_points)} depth_points entries for "
                                 f"{len(viewmats)} training images")
        # simple_trainer.py pose_opt / pose_opt_lr / pose_opt_reg / pose_noise
        # (pose.PoseOptimizer); the step stays fused: only where the geometry Adam
        # runs in the projection backward (that backward forms the pose partials)
        self.pose_opt, self.pose_noise = bool(pose_opt), float(pose_noise)
        self.pose_opt_reg = float(pose_opt_reg)
        if self.pose_noise < 0.0:
            raise ValueError(f"pose_noise: a standard deviation >= 0, got {pose_noise!r}")
        if self.pose_active:
            _refuse("pose", asked, "pose_opt" if self.pose_opt else "pose_noise")
            self.pose = PoseOptimizer(
                len(viewmats), device, seed, self.pose_opt, self.pose_noise,
                float(pose_opt_lr) * math.sqrt(world_size), self.pose_opt_reg, max_steps)
        # simple_trainer.py use_bilateral_grid / bilateral_grid_shape: the grids
        # sliced between the render and the loss (bilagrid.BilateralGridOptimizer)
        self.bilateral_grid = bool(bilateral_grid)
        self.bilateral_grid_shape = tuple(int(v) for v in bilateral_grid_shape)
        if self.bilateral_grid:
            _refuse("bilateral_grid", asked)
            self.bil = BilateralGridOptimizer(len(viewmats), bilateral_grid_shape, device,
                                              world_size, max_steps)
        self.sides = [so for so in (self.bil, self.pose, self.app) if so is not None]
        self.side_opts = [so for so in self.sides if so.optimised]
        # simple_trainer_2dgs.py:149-160, 611-632: the normal-consistency and
        # depth-distortion terms, each from its start iteration on (step >
        # start_iter)
        self.normal_loss, self.dist_loss = bool(normal_loss), bool(dist_loss)
        self.normal_lambda, self.dist_lambda = float(normal_lambda), float(dist_lambda)
        self.normal_start_iter, self.dist_start_iter = int(normal_start_iter), int(dist_start_iter)
        if self.normal_loss or self.dist_loss:
            _refuse("normal_loss / dist_loss", asked)
            if model != "2dgs":
                raise ValueError("normal_loss / dist_loss are 2DGS terms: model='2dgs'")
        self.model = model
        g = torch.Generator().manual_seed(seed)  # identical on every rank (replicas)
        N = points.shape[0]
        self.device = device
        self.width, self.height = width, height
        self.sh_degree = sh_degree
        self.ssim_lambda = ssim_lambda
        self.world_size, self.rank = world_size, rank
        self.scene_scale = scene_scale
        # the caller's config object is not modified (a private copy)
        self.strategy = None if strategy is None else dataclasses.replace(strategy)
        # MCMCStrategy (mcmc.py): relocation / sample-add refines and the
        # per-step position noise instead of DefaultStrategy's statistics
        self.mcmc = isinstance(self.strategy, MCMCStrategyConfig)
        if self.mcmc:
            self._binoms = None  # initialize_state's table, on the device at first use
        elif self.strategy is not None and model == "2dgs":
            self.strategy.key_for_gradient = "gradient_2dgs"  # simple_trainer_2dgs.py:307-311
        # simple_trainer.py:135-137, 671-681: |sigmoid(opacities)| / |exp(scales)|
        # mean terms on the raw parameters (0 = off, the default config)
        self.opacity_reg, self.scale_reg = float(opacity_reg), float(scale_reg)
        self.sh_degree_interval = sh_degree_interval
        self.max_steps = max_steps
        K = (sh_degree + 1) ** 2
        sh = torch.zeros(N, K, 3)
        sh[:, 0, :] = rgb_to_sh(rgbs)
        if init == "random":
            # load_test_data(): scales U(0,0.02), unit quats, opacities U(0,1);
            # colours from the SfM points as SH DC terms
            scales = torch.log(torch.rand(N, 3, generator=g) * 0.02 + 1e-4)
            quats = F.normalize(torch.randn(N, 4, generator=g), dim=-1)
            opac = torch.logit(torch.rand(N, generator=g).clamp(1e-3, 1 - 1e-3))
            if not self.app_opt:  # (the last draw: the geometry is a plain trainer's)
                sh[:, 1:, :] = torch.randn(N, K - 1, 3, generator=g) * 0.01
        else:  # simple_trainer.create_splats_with_optimizers, init_type="sfm"
            scales = knn_log_scales(points, init_scale)
            quats = torch.rand(N, 4, generator=g)
            opac = torch.logit(torch.full((N,), float(init_opacity)))
        self.params = {
            "means": points.clone(), "scales": scales, "quats": quats, "opacities": opac,
            "sh0": sh[:, :1].contiguous(), "shN": sh[:, 1:].contiguous(),
        }
        if self.app_opt:
            # simple_trainer.py:243-254: `features` U(0,1) [N,32] and the logits
            # `colors` replace sh0 / shN, ordinary groups of the trainer's Adam
            # (refine, relocate, sample-add carry them like any parameter),
            # drawn with the module (AppearanceOptimizer.groups)
            del self.params["sh0"], self.params["shN"]
            self.params.update(self.app.__dict__.pop("groups"))
        # Gaussian-sharded: this rank's Gaussians [rank::world] of the scene
        # initialised as a whole (simple_trainer.py:221-229: knn scales over
        # all points, then the slice), so the shards together are the
        # one-GPU scene exactly
        self.gshard = bool(gaussian_shard)
        if self.gshard:
            assert model == "3dgs", "gaussian_shard: the 3DGS trainer"
            self.params = {k: v[rank::world_size].contiguous() for k, v in self.params.items()}
            self._n_world = [len(range(r, N, world_size)) for r in range(world_size)]
            N = self.params["means"].shape[0]
        self.params = {k: torch.nn.Parameter(v.float().contiguous().to(device))
                       for k, v in self.params.items()}
        BS = world_size  # batch 1 per rank (simple_trainer.py:261-277)
        self.lrs = [self.LRS[k] * (scene_scale if k == "means" else 1.0) * math.sqrt(BS)
                    for k in self.params]
        self.adam_kw = dict(eps=1e-15 / math.sqrt(BS),
                            betas=(1 - BS * (1 - 0.9), 1 - BS * (1 - 0.999)))
        self.fused = fused
        # simple_trainer.py:263-266,782-797 (cfg.visible_adam): SelectiveAdam --
        # the reference's Adam kernel (no bias correction) on the rows of the
        # Gaussians some camera of the step sees, (radii > 0).any(0); one
        # launch per group (gsplat_hip_selective_adam), no update fused into
        # a backward, steps issued eagerly
        self.visible_adam = bool(visible_adam)
        # simple_trainer.py:123,501 (cfg.packed): the render's [nnz] pairs
        # instead of [C, N] (rasterization(packed=True)); the strategy
        # statistics by index_add over meta["gaussian_ids"] (default.py:240-243);
        # steps issued eagerly
        self.packed = bool(packed)
        assert not (self.packed and (model != "3dgs" or gaussian_shard)), \
            "packed: the one-camera-per-rank 3DGS trainer"
        # simple_trainer.py:125,263-264,767-780 (cfg.sparse_grad): the packed
        # projection's COO gradients (rasterization(sparse_grad=True)), every
        # other gradient made COO over gaussian_ids, torch.optim.SparseAdam
        self.sparse_grad = bool(sparse_grad)
        # simple_trainer.py:129,482 (cfg.antialiased): rasterize_mode
        # "antialiased", the opacities scaled by the projection's compensation
        self.rasterize_mode = "antialiased" if antialiased else "classic"
        if self.sparse_grad:
            assert self.packed, "sparse_grad: packed mode only (simple_trainer.py:769)"
            assert world_size == 1, "sparse_grad: one rank"
        if self.visible_adam or self.sparse_grad:
            assert not (self.visible_adam and self.sparse_grad), "visible_adam or sparse_grad"
            assert not gaussian_shard and not sharded_optimizer, \
                "visible_adam: one rank or replicated ranks with all-reduced gradients"
            sharded_optimizer = False
        # N > 1: gradients reduce-scattered, Adam on this rank's rows, rows
        # all-gathered (distributed.ShardedAdam) instead of all-reduce + full Adam
        # (None: when world_size > 1; True also at world_size 1, for tests)
        if sharded_optimizer is None:
            sharded_optimizer = world_size > 1 and not self.gshard
        assert not (self.gshard and sharded_optimizer), "gaussian_shard: a local optimizer"
        self.sharded = fused and sharded_optimizer
        # measurement only (bench.py --dp-emulate W): one rank shards its
        # optimizer rows as W ranks would (ShardedAdam emulate_world)
        self.dp_emulate_world = dp_emulate_world if self.sharded else None
        # one rank, fused path: the SH coefficients' Adam step runs inside the
        # SH-colour backward (gsplat_hip_sh_colors_bwd_adam), so their
        # gradients never go through HBM; GSPLAT_HIP_SH_ADAM_IN_BWD=0 turns it off
        # (Gaussian-sharded too: the SH backward sums its shard's gradient over
        # every rank's camera in the kernel before the update)
        self.sh_adam_in_bwd = (fused and not self.sharded and not self.visible_adam
                               and not self.sparse_grad and not self.app_opt
                               and (world_size == 1 or self.gshard)
                               and os.environ.get("GSPLAT_HIP_SH_ADAM_IN_BWD", "1") != "0")
        # the exp / sigmoid VJPs and the means-gradient sum formed inside the
        # geometry groups' Adam (gsplat_hip_adam_step_ex): at one rank, and
        # under the sharded optimizer on the reduced shard (ShardedAdam.step)
        self.geom_fuse = (fused and not self.visible_adam and not self.sparse_grad
                          and (world_size == 1 or self.sharded or self.gshard)
                          and os.environ.get("GSPLAT_HIP_GEOM_FUSE", "1") != "0")
        # one rank: the geometry groups' whole Adam step inside the
        # projection backward (gsplat_hip_projection_bwd_adam, 2DGS:
        # gsplat_hip_projection_2dgs_bwd_adam), so their gradients never go
        # through HBM; GSPLAT_HIP_GEOM_IN_PROJ=0 turns it off.  Not with the
        # regularisers (extra terms on the raw parameters)
        self.geom_in_proj = (self.geom_fuse and world_size == 1 and not self.gshard
                             and not self.sharded and model in ("3dgs", "2dgs")
                             and self.opacity_reg == 0.0 and self.scale_reg == 0.0
                             and os.environ.get("GSPLAT_HIP_GEOM_IN_PROJ", "1") != "0")
        # sharded optimizer: the SH group's collectives on a communicator of
        # their own (issued from a gradient hook during the backward), the
        # geometry's on the default group
        self._sh_pg = None
        if self.sharded:
            import torch.distributed as dist
            self._sh_pg = dist.new_group(list(range(dist.get_world_size())))
        self._sh_ready = 0
        self.opt = self._make_optimizer(list(self.params.values()))
        self._register_hooks()
        assert self.pose is None or self.geom_in_proj, \
            "pose_opt: the geometry Adam in the projection backward"
        if self.depth_loss:
            # the images' points as CSR tables on the device, built once; the
            # step names its image by a device index
            from .depth_loss import DepthPoints
            self.depth_table = DepthPoints(depth_points, device)
        # an eager step names its image by a one-element view of this table (the
        # captured step: by the camera index of its input block)
        self._cam_index = torch.arange(len(viewmats), dtype=torch.int64, device=device)
        self.viewmats = viewmats.to(device)
        self.Ks = Ks.to(device)
        if targets is None:
            gt = torch.Generator().manual_seed(1234)
            targets = torch.rand(len(viewmats), height, width, 3, generator=gt)
        self.targets = targets.to(device)
        self.grad2d = torch.zeros(N, device=device)
        self.count = torch.zeros(N, device=device)
        # state["radii"] (default.py:235-262): the largest screen radius of each
        # Gaussian normalised by max(W, H), tracked only while it is used
        self.radii2d = (torch.zeros(N, device=device) if self.strategy is not None
                        and getattr(self.strategy, "refine_scale2d_stop_iter", 0) > 0 else None)
        # split noise: the same stream on every rank (replicas stay identical);
        # Gaussian-sharded: a stream per shard
        self.rng = torch.Generator(device=device).manual_seed(
            seed + (7919 * rank if self.gshard else 0))
        # MCMC position noise: drawn in the noise kernel from this key and the
        # step (mcmc.inject_noise), so a replayed or re-run step draws the same
        self._noise_seed = ((seed + (7919 * rank if self.gshard else 0) + 1)
                            * 0x9E3779B97F4A7C15) % (1 << 64)
        self.window = _gauss_window(device=device)
        self.last_meta = None
        self.refine_log = []  # (step, n_dupli, n_split, n_prune, N after)
        # graph=True: the step as HIP graph replays where the configuration
        # allows (graph_step.graphable: fused one-rank 3DGS; with a
        # DefaultStrategy schedule the refines run eagerly between replays);
        # isect_capacity: its isect arrays' initial size (default: 1.25 x the
        # first camera's count)
        self._graph = None
        self.graph_fallback = None  # why the captured step fell back to eager, if it did
        if graph:
            from .graph_step import GraphStep, graphable
            if graphable(self):
                self._graph = GraphStep(self, capacity=isect_capacity)

    # ------------------------------------------------------------ optimizer
    def _make_optimizer(self, params):
        if self.sharded:
            from .distributed import ShardedAdam
            # geometry first: the next projection waits for it; the SH rows
            # only before the next step's colours (after its isect)
            names = list(self.params)
            groups = [[names.index(k) for k in ("means", "scales", "quats", "opacities")],
                      [names.index(k) for k in ("sh0", "shN")]]
            return ShardedAdam(params, self.lrs, groups=groups,
                               group_pgs=[None, self._sh_pg],
                               emulate_world=self.dp_emulate_world, **self.adam_kw)
        groups = [{"params": [p], "lr": lr, "name": k}
                  for (k, p), lr in zip(self.params.items(), self.lrs)]
        if self.visible_adam:
            from ._wrapper_aux import SelectiveAdam
            return SelectiveAdam(groups, **self.adam_kw)
        if self.sparse_grad:
            return torch.optim.SparseAdam(groups, **self.adam_kw)
        if self.fused:  # HIP loss + one-launch Adam (csrc/ssim.hip, csrc/adam.hip)
            return FusedAdam(params, self.lrs, **self.adam_kw)
        return torch.optim.Adam(groups, foreach=True, **self.adam_kw)

    def _register_hooks(self):
        """Sharded optimizer: reduce-scatter the SH group as soon as the
        SH-colour backward has produced both of its gradients (the rest of
        the backward -- projection, activations -- is still to run), from a
        post-accumulate hook on sh0 and shN."""
        if not self.sharded:
            return
        for k in ("sh0", "shN"):
            self.params[k].register_post_accumulate_grad_hook(self._sh_grad_ready)

    def _sh_grad_ready(self, param):
        self._sh_ready += 1
        if self._sh_ready == 2:
            self.opt.reduce_early(1)

    def _set_means_lr(self, lr):
        if isinstance(self.opt, torch.optim.Optimizer):
            self.opt.param_groups[0]["lr"] = lr
        else:
            self.opt.lrs[0] = lr

    def moments(self):
        """name -> [exp_avg, exp_avg_sq] as full tensors shaped like the
        parameter (gathered over the ranks for the sharded optimizer), then the
        side optimizers' ("bil_grids", "pose_embeds", "app_embeds", "app_head")."""
        out = self._gaussian_moments()
        if self.side_opts:
            self.sync()
        for so in self.side_opts:
            out.update(so.moments())
        return out

    # --------------------------------------------- pose_opt, app_opt: access
    def app_state_dict(self):
        """The appearance module's state under the reference module's keys
        (AppearanceOptimizer.state_dict), synced."""
        self.sync()
        return self.app.state_dict()

    @property
    def pose_active(self) -> bool:
        """The step renders through pose.pose_apply (pose_opt or pose_noise)."""
        return self.pose_opt or self.pose_noise > 0.0

    def pose_lr_at(self, it: int) -> float:
        """The pose optimizer's learning rate at step `it` (PoseOptimizer.lr_at)."""
        return self.pose.lr_at(it)

    @torch.no_grad()
    def adjusted_viewmats(self, ids=None):
        """The refined view matrices [len(ids), 4, 4] of the training cameras
        `ids` (default: all): T(embeds)^-1 T(noise)^-1 viewmat."""
        self.sync()
        ids = list(range(len(self.viewmats))) if ids is None else [int(i) for i in ids]
        vms = self.viewmats.float().contiguous()
        if self.pose is None:
            return vms[ids].clone()
        out = torch.empty(len(ids), 4, 4, device=vms.device)
        for k, ci in enumerate(ids):
            self.pose.apply(vms[ci:ci + 1], self._cam_index[ci:ci + 1], out=out[k:k + 1])
        return out

    def _gaussian_moments(self):
        names = list(self.params)
        if self.sharded:
            return {k: list(mv) for k, mv in zip(names, self.opt.full_state())}
        if isinstance(self.opt, FusedAdam):
            self.sync()
            return {k: [self.opt.exp_avg[i], self.opt.exp_avg_sq[i]]
                    for i, k in enumerate(names)}
        out = {}
        for k in names:
            st = self.opt.state.get(self.params[k], {})
            if "exp_avg" not in st:  # no step taken yet
                z = torch.zeros_like(self.params[k])
                st = {"exp_avg": z, "exp_avg_sq": z.clone()}
            out[k] = [st["exp_avg"], st["exp_avg_sq"]]
        return out

    def _load_moments(self, moments):
        params = list(self.params.values())
        names = list(self.params)
        for so in self.side_opts:  # (those that `moments` names: a checkpoint's)
            so.load_moments(moments)
        if self.sharded:
            step = self.opt.step_count
            self.opt = self._make_optimizer(params)
            self.opt.load_full_state([moments[k] for k in names], step)
        elif isinstance(self.opt, FusedAdam):
            self.opt.params = params
            self.opt.exp_avg = [moments[k][0] for k in names]
            self.opt.exp_avg_sq = [moments[k][1] for k in names]
        else:
            old = self.opt
            step = next(iter(old.state.values()), {}).get("step")
            lrs = [g["lr"] for g in old.param_groups]
            self.opt = self._make_optimizer(params)
            for g, lr in zip(self.opt.param_groups, lrs):
                g["lr"] = lr
            if step is not None:
                for k, p in self.params.items():
                    self.opt.state[p] = {"step": step.clone() if torch.is_tensor(step) else step,
                                         "exp_avg": moments[k][0],
                                         "exp_avg_sq": moments[k][1]}

    def sync(self):
        """Order the current stream after any optimizer communication still in
        flight (the sharded optimizer's deferred all-gathers): call before
        reading the parameters outside the training step (checkpoint, eval)."""
        if self._graph is not None:
            self._graph.sync()
            if self._graph.failed is not None:  # a recovery's re-capture failed
                self.graph_fallback = self._graph.failed
                self._graph = None
        if self.sharded:
            self.opt.wait()

    def release_graph(self):
        """Stop replaying: settle the captured step's replays, destroy its
        graph (before destroy_process_group, see GraphStep.release) and issue
        later steps eagerly."""
        if self._graph is not None:
            self._graph.release()
            self._graph = None

    def synced_params(self):
        self.sync()
        return self.params

    # ---------------------------------------------------------------- step
    def camera_index(self, it: int) -> int:
        return (it * self.world_size + self.rank) % len(self.viewmats)

    def sh_degree_at(self, it: int) -> int:
        if self.sh_degree_interval is None:
            return self.sh_degree
        return min(it // self.sh_degree_interval, self.sh_degree)

    def world_cameras(self, ci: int, world_ci=None):
        """Gaussian-sharded: the (viewmats, Ks) of every rank's camera, rank
        order -- the training schedule's (rank r renders (it*world + r) % n)
        or an explicit list `world_ci`."""
        n = len(self.viewmats)
        if world_ci is None:
            world_ci = [(ci - self.rank + r) % n for r in range(self.world_size)]
        key = tuple(int(c) for c in world_ci)
        cache = self.__dict__.setdefault("_wcam_cache", {})
        if key not in cache:
            if len(cache) > 4 * n:
                cache.clear()
            idx = torch.tensor(key, device=self.viewmats.device)
            cache[key] = (self.viewmats.index_select(0, idx), self.Ks.index_select(0, idx))
        return cache[key]

    def geometry_terms_at(self, it: int):
        """(normal_lambda, dist_lambda) of step `it`, 0.0 for a term that is
        off or not yet started (simple_trainer_2dgs.py:612,627: step > start)."""
        nl = self.normal_lambda if self.normal_loss and it > self.normal_start_iter else 0.0
        dl = self.dist_lambda if self.dist_loss and it > self.dist_start_iter else 0.0
        return nl, dl

    def camtoworld(self, ci: int) -> torch.Tensor:
        """[1,4,4] inverse of camera `ci`'s viewmat, inverted on the host in
        float64 (the captured step's input block holds the same values)."""
        cache = self.__dict__.setdefault("_c2w_cache", {})
        if ci not in cache:
            vm = self.viewmats[ci].detach().float().cpu().numpy().astype(np.float64)
            cache[ci] = torch.from_numpy(np.linalg.inv(vm).astype(np.float32))[None].to(
                self.viewmats.device)
        return cache[ci]

    def geometry_loss(self, meta, Ks, terms):
        """The active geometry terms of a render made with `geometry=terms`."""
        from .losses import geometry_loss_2dgs
        nl, dl = terms
        normals, alphas, distort = meta["_geometry"]
        return geometry_loss_2dgs(normals if nl else None, meta["_rgbd"], alphas,
                                  meta["camtoworlds"], Ks, distort if dl else None,
                                  normal_lambda=nl, dist_lambda=dl, _depth_image=True)

    def render(self, ci: Optional[int], sh_degree: Optional[int] = None,
               fusion: Optional[_wrapper.StepFusion] = None, world_ci=None, geometry=None,
               viewmats=None, Ks=None, camtoworlds=None, cam_index=None, fetch=None,
               isect=None):
        """Render camera `ci`; `fusion` (a training step's StepFusion) goes to
        the nodes whose backward hands their gradients to the optimizer.
        `geometry` (2DGS): the step's (normal_lambda, dist_lambda); with one
        non-zero the normal and distortion images are rendered too
        (meta["_geometry"], geometry_loss).
        Gaussian-sharded: a collective -- every rank renders its own camera
        with all ranks' Gaussians (`world_ci`: see world_cameras).
        A training step (StepInputs) also gives
        `viewmats` / `Ks`: [W,4,4] / [W,3,3] instead of camera `ci`'s own: W =
        1, or the Gaussian-sharded world's cameras in rank order;
        `camtoworlds` (2DGS): the camera's inverse view matrix [1,4,4];
        `cam_index`: the device index [1] of the step's image -- its pose rows
        adjust the camera (pose_opt / pose_noise) and its embedding row colours
        the render (app_opt); None: the camera as given, the zero embedding;
        `fetch`: strategy.activate's (the captured step's input block);
        `isect`: the sync-free intersection's rasterization keywords."""
        p = self.params
        deg = self.sh_degree if sh_degree is None else sh_degree
        isect = isect or {}
        hook = None
        if self.sharded and not self.opt.capturing:
            # the previous step's all-gathers: geometry before the projection,
            # the SH rows only before the colours (evaluated after isect); a
            # captured step leaves none in flight (ShardedAdam.capturing)
            names = list(self.params)
            self.opt.wait([names.index(k) for k in ("means", "scales", "quats", "opacities")])
            sh_idx = [names.index(k) for k in ("sh0", "shN")]
            hook = lambda: self.opt.wait(sh_idx)  # noqa: E731
        if self.fused and not self.sparse_grad:
            # one HIP launch each way for both activations (sparse_grad: torch's,
            # whose backward takes the projection's COO gradients)
            scales, opac = activate(p["scales"], p["opacities"], fusion, fetch=fetch)
        else:
            scales, opac = torch.exp(p["scales"]), torch.sigmoid(p["opacities"])
        if viewmats is None:
            vms, K = self.viewmats[ci:ci + 1], self.Ks[ci:ci + 1]
        else:  # this rank's camera of the step's
            r = self.rank if self.gshard else 0
            vms, K = viewmats[r:r + 1], Ks[r:r + 1]
        if cam_index is not None and self.pose is not None:  # launch (a): the step's view matrix
            vms = self.pose.apply(_wrapper._f32c(vms), cam_index)
        absgrad = getattr(self.strategy, "absgrad", False)
        if self.model == "2dgs":
            if hook is not None:
                hook()
            geo = geometry is not None and any(geometry)
            if geo:
                kw = dict(_geometry=True, distloss=bool(geometry[1]),
                          _camtoworlds=self.camtoworld(ci) if camtoworlds is None else camtoworlds)
            else:
                kw = dict(_colors_only=True)
            rc, ra, rn, _, rd, _, meta = rasterization_2dgs(
                p["means"], p["quats"], scales, opac, (p["sh0"], p["shN"]), vms, K, self.width,
                self.height, sh_degree=deg, packed=False, near_plane=0.01, far_plane=1e10,
                render_mode="RGB+D", absgrad=absgrad, _fusion=fusion, **kw, **isect)
            meta["_rgbd"] = rc  # the loss reads its colour channels in place
            if geo:
                meta["_geometry"] = (rn, ra, rd)
            return rc[..., :3], ra, meta
        dkw = {}
        if self.gshard:
            dkw = dict(distributed=True, _world_counts=self._n_world,
                       _world_cameras=(self.world_cameras(ci, world_ci) if viewmats is None
                                       else (viewmats, Ks)))
        if self.app_opt:
            # the colours of the appearance MLP at `deg`, rendered as plain
            # colours (sh_degree None), evaluated after the projection
            coeffs, deg_r = p["colors"], None
            dkw["_app"] = self.app.colors(p, vms, deg, cam_index, fusion)
        else:
            coeffs, deg_r = ((p["sh0"], p["shN"]) if self.fused
                             else torch.cat([p["sh0"], p["shN"]], 1)), deg
        with _wrapper.fwd_split(self.split_div, self.split_threshold):
            rc, ra, meta = rasterization(
                p["means"], p["quats"], scales, opac, coeffs, vms, K, self.width, self.height,
                sh_degree=deg_r, packed=self.packed, near_plane=0.01, far_plane=1e10,
                radius_clip=0.0, rasterize_mode=self.rasterize_mode, absgrad=absgrad,
                render_mode="RGB+D" if self.depth_loss else "RGB", sparse_grad=self.sparse_grad,
                _colors_ready=hook, _fusion=fusion, **dkw, **isect)
        if self.depth_loss:  # the losses read the RGB+D render in place (depth_losses)
            meta["_rgbd"] = rc
            return rc[..., :3], ra, meta
        return rc, ra, meta

    def depth_losses(self, rgbd, alphas, gt, cam_index, gt_index=None):
        """(photometric loss, depth_lambda * scene_scale * the depth term, the
        bilateral grids' tv or None) of an RGB+D render [1,H,W,4] for the image
        of the device index `cam_index`.  Without the bilateral grid the two
        losses are one autograd node (depth_loss.l1_ssim_depth_loss); with it
        the grid is applied to the colour channels alone."""
        from . import depth_loss as _dl
        weight = self.depth_lambda * self.scene_scale
        if self.bilateral_grid:
            colors, tv = self.bil.slice_tv(_dl.colour_channels(rgbd), cam_index)
            photo = l1_ssim_loss(colors, gt, self.ssim_lambda, gt_index=gt_index)
            term = _dl.table_depth_loss(rgbd, alphas, self.depth_table, cam_index, 3)
            return photo, weight * term, tv
        photo, term = _dl.l1_ssim_depth_loss(rgbd, alphas, gt, self.ssim_lambda,
                                             self.depth_table, cam_index, gt_index=gt_index)
        return photo, weight * term, None

    def _tune_split(self, it: int):
        """Once, before the first step (and so before a graph capture freezes
        the forward's variant):
        * the split-forward threshold's divisor from the scene's termination.
          Pixels that rarely stop early (n_eff / n_isects > 0.75, M3: 0.89)
          make the heaviest tiles the forward's tail: split more of them
          (divisor 1100); scenes that terminate early (M2: 0.56) keep 550,
          whose split-capable variant would only cost occupancy.
          One-GPU 3DGS on the HIP path; GSPLAT_HIP_FWD_SPLIT_DIV set by the
          user wins;
        * which forward variant every render of this trainer launches: the
          split-capable one with this first render's threshold fixed if the
          render has a tile above it, else the plain one.  Decided once, so
          eager and captured steps run the same kernel with the same
          threshold (a captured step's isect count is its capacity) (the library's default heuristic reads an
          earlier render's largest tile from host-mapped memory with no sync:
          eager renders would pick a variant by timing).
        Both are this trainer's: its renders (and its graph capture) set them
        around their launches and restore the previous values
        (_wrapper.fwd_split), nothing else in the process sees them.  Costs
        one eager render (no backward) before the first step; a
        Gaussian-sharded render is a collective, and every rank's first step
        runs it."""
        self._split_tuned = True
        if self.model != "3dgs" or not self.fused:
            return
        colors, _, meta = self.render(self.camera_index(it), self.sh_degree_at(it))
        self.term_ratio = _wrapper.forward_termination_ratio(colors, meta, self.width, self.height)
        if self.world_size == 1 and not os.environ.get("GSPLAT_HIP_FWD_SPLIT_DIV"):
            self.split_div = 1100 if self.term_ratio > 0.75 else 550
        n = int(meta["isect_counts"][0]) if "isect_counts" in meta else meta["flatten_ids"].numel()
        with _wrapper.fwd_split(self.split_div):
            thr = _wrapper.fwd_split_threshold(n)
        self.max_tile_first = _wrapper.max_tile_isects(meta)
        self.split_launch = 1 if 0 <= thr < self.max_tile_first else 0
        # > 0: the split-capable forward at this fixed threshold; 0: never
        self.split_threshold = max(int(thr), 1) if self.split_launch else 0
        del colors, meta

    def step(self, it: int):
        if not self._split_tuned:
            self._tune_split(it)
        if self._graph is not None:
            from .graph_step import GraphCaptureError
            try:
                loss = self._graph.step(it)
            except GraphCaptureError as e:
                # the capture failed (on any rank of a sharded job): eager
                # steps from here on, in this process (no re-exec); steps a
                # failed recovery voided have been re-run eagerly already
                import warnings
                self.graph_fallback = str(e)
                warnings.warn(f"gsplat_hip: {e}; issuing the training steps eagerly")
                self._graph = None
            else:
                if self.strategy is not None:
                    # eager refine / reset: drains the replays first
                    self.post_step(it, replayed=True)
                if self._graph is not None and self._graph.failed is not None:
                    self.graph_fallback = self._graph.failed  # (failed in that drain)
                    self._graph = None
                return loss
        loss = self._eager_step(it)
        if self.strategy is not None:
            self.post_step(it)
        return loss

    def _eager_step(self, it: int):
        """Training step `it` issued from the host (no refine / reset: post_step)."""
        ci = self.camera_index(it)
        if self.max_steps:  # means ExponentialLR: this step's lr, before the
            # backward that may run the geometry update (geom_in_proj)
            self._set_means_lr(self.lrs[0] * (0.01 ** (1.0 / self.max_steps)) ** it)
        vms, Ks = self.world_cameras(ci) if self.gshard else \
            (self.viewmats[ci:ci + 1], self.Ks[ci:ci + 1])
        loss, meta = self._run_step(StepInputs(
            deg=self.sh_degree_at(it), terms=self.geometry_terms_at(it),
            stats=self.strategy is None or (not self.mcmc
                                            and it < self.strategy.refine_stop_iter),
            viewmats=vms, Ks=Ks, cam=self._cam_index[ci:ci + 1], targets=self.targets[ci:ci + 1],
            c2w=self.camtoworld(ci) if self.model == "2dgs" else None, it=it,
            bkgd=(torch.tensor([self.bkgd_at(it)], dtype=torch.float32, device=self.device)
                  if self.random_bkgd else None)))
        self.last_meta = meta
        return loss

    def bkgd_at(self, it: int):
        """random_bkgd's colour of step `it`: three float32 in [0, 1), a pure
        function of (the trainer's seed, it) -- a counter-based host generator
        (splitmix64 of the counter) keyed by the seed's noise key, which a
        checkpoint already carries; no stream state, nothing drawn from
        self.rng.  Eager, replayed and resumed steps therefore see the same
        colours.  (The reference draws torch.rand(1, 3) from the global
        generator: the same distribution, another sequence.)"""
        m64 = (1 << 64) - 1
        out = []
        for ch in range(3):
            z = (int(self._noise_seed) ^ ((3 * int(it) + ch + 1) * 0xD1B54A32D192ED03)) & m64
            for _ in range(2):  # splitmix64's finaliser, twice
                z = (z + 0x9E3779B97F4A7C15) & m64
                z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
                z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
                z ^= z >> 31
            out.append(float(np.float32((z >> 40) * (1.0 / (1 << 24)))))  # 24 bits: exact, < 1
        return tuple(out)

    def _layout(self):
        """(groups of the Gaussians' Adam launches in launch order, offset of
        the SH-Adam factors): a captured step's device-side factors
        (StepInputs.hyper) are laid out in that order."""
        if self.sharded:
            idx = [i for sel in self.opt.launch_plan() for i in sel]
            return idx, 2 * len(idx)
        names = list(self.params)
        sh = {names.index(k) for k in ("sh0", "shN") if k in names}
        idx = [i for i in range(len(names)) if not (self.sh_adam_in_bwd and i in sh)]
        return idx, 2 * len(idx)

    def _run_step(self, s: StepInputs):
        """Issue one whole training step -- the only place that does: the
        fusion, activations, pose adjustment and render; the bilateral grid's
        slice or the depth losses, the photometric loss, the geometry terms, tv
        and the regularisers; the backward with the constant seed, the strategy
        statistics, the Gaussians' Adam and the side optimizers'.  Trainer.
        _eager_step and GraphStep._body are its callers; they differ in where
        the inputs `s` live.  Returns (loss, the render's meta)."""
        self._sh_ready = 0  # the sharded optimizer's SH reduce-scatter hook
        fusion = self._make_fusion(s)
        # (the activations first -- a captured step's fetch its input block --
        # then the pose adjustment: Trainer.render)
        colors, alphas, meta = self.render(
            None, s.deg, fusion, geometry=s.terms, viewmats=s.viewmats, Ks=s.Ks,
            camtoworlds=s.c2w, cam_index=s.cam, fetch=s.fetch, isect=s.isect)
        if self.model == "3dgs":
            # DefaultStrategy.step_pre_backward: the means2d gradient is
            # captured by a hook (retain_grad would clone it into .grad), into a
            # box of its own (a hook holding `meta` would tie the render's
            # tensors and their autograd graph into a reference cycle).  2DGS:
            # the densification input is a leaf, its .grad read after the
            # backward (a hook keeping a reference would make AccumulateGrad
            # clone the gradient -- a memcpy node in a captured step)
            box = {}
            meta["means2d"].register_hook(lambda g: box.__setitem__("means2d_grad", g))
        tv = None
        if self.bilateral_grid and not self.depth_loss:
            # simple_trainer.py:620-630, 663-665: the camera's grid applied to
            # the render, 10 x the grids' total variation added to the loss
            colors, tv = self.bil.slice_tv(colors, s.cam)
        vote = None
        if s.vote:  # the ranks' overflow flags, agreed beside the loss kernels
            import torch.distributed as dist
            from . import distributed as gdist
            vote = dist.all_reduce(s.void, op=dist.ReduceOp.MAX, async_op=True,
                                   group=gdist.current_capture_group())
        if self.depth_loss:  # simple_trainer.py:647-665: the photometric loss and the depth term
            photo, term, tv = self.depth_losses(meta["_rgbd"], alphas, s.targets, s.cam,
                                                gt_index=s.gt_index)
            loss = photo + term
        elif self.fused and (self.masks is not None or self.random_bkgd):
            # the render masked and put over the step's colour inside the loss kernel
            m = self.masks
            if m is not None and s.gt_index is None:
                m = m.index_select(0, s.cam)  # (eager: the image's own [1,H,W])
            loss = l1_ssim_loss(colors, s.targets, self.ssim_lambda, gt_index=s.gt_index,
                                _out_ring=s.loss_ring, masks=m, alphas=alphas,
                                backgrounds=s.bkgd)
        elif self.fused:  # (2DGS: the RGB+D render's colour channels in place)
            two = self.model == "2dgs"
            loss = l1_ssim_loss(meta["_rgbd"] if two else colors, s.targets, self.ssim_lambda,
                                gt_index=s.gt_index, _out_ring=s.loss_ring,
                                _channels=3 if two else None)
        else:
            if self.masks is not None or self.random_bkgd:  # the same, in torch ops
                from .losses import compose_masked
                colors = compose_masked(
                    colors, None if self.masks is None else self.masks.index_select(0, s.cam),
                    alphas, s.bkgd)
            l1 = F.l1_loss(colors, s.targets)
            ssim_loss = 1.0 - ssim(colors.permute(0, 3, 1, 2), s.targets.permute(0, 3, 1, 2),
                                   self.window)
            loss = l1 * (1.0 - self.ssim_lambda) + ssim_loss * self.ssim_lambda
        if any(s.terms):
            loss = loss + self.geometry_loss(meta, s.Ks, s.terms)
        if tv is not None:
            loss = loss + tv
        loss = self._regularise(loss)
        if vote is not None:
            vote.wait()
            ring, slot = s.isect["_isect_report"]
            _lib.call("gsplat_hip_status_to_ring", s.void.data_ptr(), ring, slot.data_ptr(),
                      _wrapper._stream())
        if self.fused and loss.dim() == 0:
            torch.autograd.backward(loss, _one_grad(loss.device))
        else:
            loss.backward()
        if self.model == "3dgs":
            meta.update(box)
        if self.world_size > 1 and not self.sharded and not self.gshard:
            self.allreduce_grads()
        if s.stats:
            self.update_state(meta, skip=s.void)
        # whether this step's geometry update ran inside the projection backward
        s.geom_applied = self.geom_applied = bool(
            fusion is not None and fusion.geom_adam is not None and fusion.geom_adam.applied)
        xform = self._geom_xform(fusion)
        hyper = s.hyper
        if self.sharded:  # reduce-scatter, Adam on this rank's rows, all-gather
            if hyper is not None:
                assert not self._sh_skip(fusion)
                hyper = hyper[:self._layout()[1]]
            self.opt.step(defer_gather=not s.capturing, xform=xform, hyper=hyper, void=s.void)
        elif self.visible_adam:  # simple_trainer.py:782-797
            if meta.get("gaussian_ids") is not None:  # packed: the Gaussians of the pairs
                vis = torch.zeros(self.params["opacities"].shape[0], dtype=torch.bool,
                                  device=self.params["opacities"].device)
                vis[meta["gaussian_ids"]] = True
            else:  # (radii > 0).any(0)
                vis = meta["radii"] > 0
                if vis.dim() > 2:  # per-axis radii [C, N, 2]
                    vis = vis.all(-1)
                vis = vis.any(0)
            self.opt.step(vis)
        elif self.sparse_grad:  # simple_trainer.py:767-780, then SparseAdam
            ids = meta["gaussian_ids"]
            for k, p in self.params.items():
                g = p.grad
                if g is None or g.is_sparse:
                    continue
                p.grad = torch.sparse_coo_tensor(indices=ids[None], values=g[ids], size=p.size(),
                                                 is_coalesced=meta["n_cameras"] == 1)
            self.opt.step()
        elif isinstance(self.opt, torch.optim.Optimizer):  # fused=False: torch's Adam
            self.opt.step()
        else:
            skip = self._sh_skip(fusion)
            kw = {}
            if hyper is not None:
                # the launched groups are the launch plan's tail (the geometry
                # groups, its head, may have been updated by the projection
                # backward): their factors start at that offset
                idx, sh_off = self._layout()
                launched = tuple(i for i in range(len(self.params)) if i not in skip)
                assert launched == tuple(idx[len(idx) - len(launched):]), (skip, idx)
                kw = dict(hyper=hyper[2 * (len(idx) - len(launched)):sh_off], void=s.void)
            self.opt.step(skip=skip, xform=xform, **kw)
        self.opt.zero_grad(set_to_none=True)
        for so in self.side_opts:  # the grids', the pose table's, the appearance module's
            so.launch(s, s.side_hyper.get(so.name))
        return loss, meta

    def _regularise(self, loss):
        """simple_trainer.py:671-681: the opacity / scale regularisers on the raw
        parameters (their gradients reach .grad of the raw tensors through
        torch autograd; the fused optimizer adds them as extra terms)."""
        p = self.params
        if self.opacity_reg > 0.0:
            loss = loss + self.opacity_reg * _mean(torch.abs(torch.sigmoid(p["opacities"])))
        if self.scale_reg > 0.0:
            loss = loss + self.scale_reg * _mean(torch.abs(torch.exp(p["scales"])))
        return loss

    def _make_fusion(self, s: StepInputs) -> Optional[_wrapper.StepFusion]:
        """This step's StepFusion (None when nothing is fused): the SH groups'
        Adam inside the SH backward (sh_adam_in_bwd), the geometry groups'
        gradient transforms inside their Adam (geom_fuse) or their whole Adam
        inside the projection backward (geom_in_proj).  With s.hyper the
        updates read their factors there (Trainer._layout) and the void flag."""
        fused = isinstance(self.opt, FusedAdam)
        step = self.opt.step_count + 1 if fused and s.hyper is None else 1  # (unused with s.hyper)
        names = list(self.params)
        idx, sh_off = self._layout() if s.hyper is not None else (None, None)
        fa = None
        if self.sh_adam_in_bwd and fused:
            i0, i1 = names.index("sh0"), names.index("shN")
            o = self.opt
            fa = _wrapper.ShAdamInBackward(
                self.params["sh0"].data, self.params["shN"].data, o.exp_avg[i0],
                o.exp_avg_sq[i0], o.exp_avg[i1], o.exp_avg_sq[i1], o.lrs[i0], o.lrs[i1],
                o.betas, o.eps, step,
                hyper=None if s.hyper is None else s.hyper[sh_off:sh_off + 3], skip=s.void)
        geom = self.geom_fuse and (fused or self.sharded)
        ga = None
        if self.geom_in_proj and fused:
            hyper = None
            if s.hyper is not None:
                # the geometry groups' factors are the first launch groups':
                # (ss, ib) of means, scales, quats, opacities at [0, 8); the SH
                # groups follow when their update is not fused into the SH backward
                assert [names[i] for i in idx][:len(self.GEOM)] == list(self.GEOM), (idx, names)
                hyper = s.hyper[:2 * len(idx)]
            ga = self.geom_adam_in_backward(step, hyper=hyper, skip=s.void)
            if self.pose_opt:
                ga.pose_ws = self.pose.prepare(self.params["means"].shape[0])
        if fa is None and not geom:
            return None
        return _wrapper.StepFusion(sh_adam=fa, geom=geom, geom_adam=ga)

    GEOM = ("means", "scales", "quats", "opacities")

    def geom_adam_in_backward(self, step, hyper=None, skip=None):
        """The geometry groups' Adam step for the projection backward
        (_wrapper.GeomAdamInBackward), in the trainer's group order."""
        names = list(self.params)
        o = self.opt
        ix = [names.index(k) for k in self.GEOM]
        return _wrapper.GeomAdamInBackward(
            [self.params[k].data for k in self.GEOM], [o.exp_avg[i] for i in ix],
            [o.exp_avg_sq[i] for i in ix], [o.lrs[i] for i in ix], o.betas, o.eps, step,
            hyper=hyper, skip=skip)

    def _sh_skip(self, fusion):
        """Indices of the groups whose update a backward already applied: the
        SH groups (SH-colour backward) and the geometry groups (projection
        backward).  Their .grad must then be empty: a loss term reaching them
        by another path would have been left out of that update."""
        if fusion is None:
            return ()
        names = list(self.params)
        done = []
        if fusion.sh_adam is not None and fusion.sh_adam.applied:
            done += [("sh0", "shN"), "GSPLAT_HIP_SH_ADAM_IN_BWD=0", "SH-colour"]
        if fusion.geom_adam is not None and fusion.geom_adam.applied:
            done += [self.GEOM, "GSPLAT_HIP_GEOM_IN_PROJ=0", "projection"]
        out = []
        for j in range(0, len(done), 3):
            keys, env, who = done[j:j + 3]
            for k in keys:
                if self.params[k].grad is not None:
                    raise RuntimeError(
                        f"{k} received a gradient outside the {who} backward while its Adam "
                        f"step was fused into that backward; set {env} for losses with extra "
                        "terms on those parameters")
            out += [names.index(k) for k in keys]
        return tuple(sorted(out))

    def _geom_xform(self, fusion):
        """FusedAdam xform of the gradients the fusion took: means = its .grad +
        the SH backward's part (autograd's sum), log-scales / logits = the exp
        / sigmoid VJPs of the activation backward formed in-register.  A
        gradient that also reached .grad of the raw log-scales / logits (a
        regulariser, simple_trainer.py:671-681) is added as an extra term:
        the VJP is then formed in torch with activate_bwd's operation order
        and summed with it, which is autograd's accumulation exactly."""
        if fusion is None or not fusion.geom:
            return None
        if fusion.geom_adam is not None and fusion.geom_adam.applied:
            return None  # the projection backward ran the geometry update
        names = list(self.params)
        xf = {}
        if fusion.v_dirs is not None:
            gm = self.params["means"].grad
            xf[names.index("means")] = (fusion.v_dirs, None, 0) if gm is None else \
                (gm, fusion.v_dirs, 1)
        if fusion.act_taken:
            for key, v, act, mode in (("scales", fusion.v_scales, fusion.scales, 2),
                                      ("opacities", fusion.v_opac, fusion.opac, 3)):
                if v is None:
                    continue  # that activation did not reach the loss
                extra = self.params[key].grad
                if extra is None:
                    xf[names.index(key)] = (v, act, mode)
                else:
                    vjp = v * act if mode == 2 else v * (1.0 - act) * act
                    xf[names.index(key)] = ((vjp + extra).contiguous(), None, 0)
        return xf or None

    # ---------------------------------------------------------------- eval
    @torch.no_grad()
    def evaluate(self, cameras=None, viewmats=None, Ks=None, images=None, masks=None,
                 color_correct=False):
        """simple_trainer.py:854-932's eval metrics: render each camera,
        clamp to [0, 1], PSNR (data range 1) and SSIM (11x11 Gaussian, the
        fused "valid" SSIM of the loss) against the target, averaged.  Either
        indices into the trainer's camera pool / targets, or explicit
        viewmats [M,4,4], Ks [M,3,3] and images [M,H,W,3].  LPIPS is not
        computed (its network weights are a download).  A trainer with masks
        zeroes each pool camera's render outside its mask before the metrics
        (simple_trainer.py:871-884 passes the masks to the render); `masks`
        [M,H,W] bool does so for the explicit form.  No background is added.

        color_correct=True adds `cc_psnr` and `cc_ssim` (simple_trainer.py:
        906-909, reported there for bilateral-grid runs): each clamped render,
        after the mask, is first warped onto its target by
        gsplat_hip.color_correct, which takes out the per-image exposure and
        white balance that a bilateral grid or app_opt run leaves to the image;
        the same metrics, averaged the same way.  Masked pixels are 0, below
        the fit's clipping threshold, so they take no part in the fit."""
        self.sync()
        if viewmats is None:
            idx = list(range(len(self.viewmats))) if cameras is None else list(cameras)
            viewmats, Ks, images = self.viewmats[idx], self.Ks[idx], self.targets[idx]
            if masks is None and self.masks is not None:
                masks = self.masks[idx]
        if masks is not None:
            if tuple(masks.shape) != (len(viewmats), self.height, self.width):
                raise ValueError(f"evaluate: masks [{len(viewmats)}, {self.height}, "
                                 f"{self.width}], got {list(masks.shape)}")
            masks = masks.to(self.device).bool()
        psnrs, ssims, cc_psnrs, cc_ssims = [], [], [], []
        saved = self.viewmats, self.Ks
        try:
            self.viewmats, self.Ks = viewmats.to(self.device), Ks.to(self.device)
            self.__dict__.pop("_wcam_cache", None)
            for i in range(len(viewmats)):
                # Gaussian-sharded: every rank renders camera i (a collective)
                colors, _, _ = self.render(i, world_ci=[i] * self.world_size)
                if masks is not None:
                    colors = torch.where(masks[i:i + 1, ..., None], colors,
                                         torch.zeros((), device=colors.device))
                colors = torch.clamp(colors, 0.0, 1.0)
                gt = images[i:i + 1].to(self.device)
                mse = torch.mean((colors - gt) ** 2)
                psnrs.append(float(-10.0 * torch.log10(mse)))
                ssims.append(float(ssim_and_l1(colors, gt)[0]))
                if color_correct:
                    cc = _color_correct(colors, gt)
                    cc_psnrs.append(float(-10.0 * torch.log10(torch.mean((cc - gt) ** 2))))
                    cc_ssims.append(float(ssim_and_l1(cc, gt)[0]))
        finally:
            self.viewmats, self.Ks = saved
            self.__dict__.pop("_wcam_cache", None)
        out = {"psnr": sum(psnrs) / len(psnrs), "ssim": sum(ssims) / len(ssims),
               "num_images": len(psnrs)}
        if color_correct:
            out["cc_psnr"] = sum(cc_psnrs) / len(cc_psnrs)
            out["cc_ssim"] = sum(cc_ssims) / len(cc_ssims)
        return out

    @torch.no_grad()
    def evaluate_compressed(self, compress_dir, cameras=None, viewmats=None, Ks=None,
                            images=None, compression=None, color_correct=False):
        """simple_trainer.py's run_compression (compression="png"): compress the
        current parameters into `compress_dir` (compression.PngCompression, or
        the instance given), decompress them and evaluate what came back --
        evaluate()'s cameras, render path and metrics (app_opt: the zero
        embedding), plus `compressed_bytes` (the sum of the file sizes in
        `compress_dir`) and `num_GS` (the n^2 Gaussians of the grid);
        `color_correct` is evaluate()'s.  The
        trainer's parameters, optimizer state and captured step are not
        touched: the decompressed splats stand in only for these renders."""
        _refuse("compression", {"gaussian_shard": self.gshard,
                                "sharded_optimizer": bool(self.sharded),
                                "world_size": self.world_size != 1},
                name="evaluate_compressed (compression)")
        from .compression import PngCompression
        comp = PngCompression(verbose=False) if compression is None else compression
        os.makedirs(compress_dir, exist_ok=True)
        comp.compress(compress_dir, {k: p.data for k, p in self.synced_params().items()})
        splats = comp.decompress(compress_dir)
        # a side optimizer's workspace is sized for the Gaussians (a captured step
        # holds its address): the renders of the n^2 get one of their own
        keep = [(so, so.ws, so.ws_n) for so in self.side_opts]
        saved = self.params
        try:
            self.params = {k: splats[k].to(self.device, saved[k].dtype).contiguous()
                           for k in saved}
            out = self.evaluate(cameras, viewmats, Ks, images, color_correct=color_correct)
            out["num_GS"] = int(self.params["means"].shape[0])
        finally:
            self.params = saved
            for so, ws, n in keep:
                so.ws, so.ws_n = ws, n
        out["compressed_bytes"] = sum(
            os.path.getsize(os.path.join(compress_dir, f)) for f in os.listdir(compress_dir)
            if os.path.isfile(os.path.join(compress_dir, f)))
        return out

    # ---------------------------------------------------------------- mesh
    @torch.no_grad()
    def extract_mesh(self, voxel_size=None, resolution=256, bounds=None, sdf_trunc=None,
                     depth_trunc=None, depth_mode="median", alpha_min=0.5, cameras=None,
                     camera_batch=8, colors=True, min_weight=0.0, path=None,
                     max_voxels=1 << 30):
        """The surface of the current Gaussians as a triangle mesh: the
        training cameras (or the pool indices `cameras`) rendered
        `camera_batch` at a time through the public rasterization_2dgs /
        rasterization ("RGB+ED"), their z-depth fused into a TSDF volume and
        marching cubes at 0 (mesh.TSDFVolume).  Returns (vertices [V,3],
        faces [F,3] int32, colors [V,3] or None) on the device and writes
        them to `path` (mesh.save_mesh_ply) when given.

        depth_mode: "median" (2DGS only: render_median) or "expected"
        bounds:     (lo, hi), three numbers each; None: the box of the means
                    between the per-axis 1 % and 99 % quantiles, grown by
                    sdf_trunc
        voxel_size: None: the longest side of the bounds is `resolution` cells
        sdf_trunc:  None: 5 voxel_size;  depth_trunc: None: no limit
        A trainer with masks zeroes alpha outside each image's mask, so those
        pixels are not fused.  app_opt: geometry only (colors=False).  The
        parameters, the optimizer state and a captured step are not touched."""
        name = "extract_mesh"
        _refuse("mesh", {"gaussian_shard": self.gshard, "sharded_optimizer": bool(self.sharded),
                         "world_size": self.world_size != 1}, name=name + " (mesh)")
        if self.app_opt and colors:
            raise NotImplementedError(f"{name}: app_opt colours depend on the image's embedding; "
                                      "pass colors=False for the geometry alone")
        if depth_mode not in ("median", "expected"):
            raise ValueError(f"{name}: depth_mode 'median' or 'expected', got {depth_mode!r}")
        if depth_mode == "median" and self.model != "2dgs":
            raise ValueError(f"{name}: the 3DGS model renders the expected depth only; pass "
                             "depth_mode='expected'")
        camera_batch, max_voxels = int(camera_batch), int(max_voxels)
        if camera_batch < 1:
            raise ValueError(f"{name}: camera_batch must be >= 1, got {camera_batch}")
        if voxel_size is not None and not float(voxel_size) > 0.0:
            raise ValueError(f"{name}: voxel_size must be positive, got {voxel_size!r}")
        if sdf_trunc is not None and not float(sdf_trunc) > 0.0:
            raise ValueError(f"{name}: sdf_trunc must be positive, got {sdf_trunc!r}")
        if voxel_size is None and int(resolution) <= (
                10 if bounds is None and sdf_trunc is None else 0):
            raise ValueError(f"{name}: resolution {resolution!r} leaves no cells")
        if bounds is not None:
            lo, hi = ([float(v) for v in b] for b in bounds)
            if len(lo) != 3 or len(hi) != 3 or not all(a <= b for a, b in zip(lo, hi)):
                raise ValueError(f"{name}: bounds must be (lo, hi) of three numbers, lo <= hi")
        idx = list(range(len(self.viewmats))) if cameras is None else [int(c) for c in cameras]
        if any(not 0 <= c < len(self.viewmats) for c in idx):
            raise ValueError(f"{name}: cameras must index the {len(self.viewmats)} training "
                             "cameras")
        from .mesh import TSDFVolume, save_mesh_ply
        self.sync()
        p = {k: v.detach() for k, v in self.params.items()}
        if bounds is None:
            n = p["means"].shape[0]
            ks = (max(1, math.ceil(0.01 * n)), max(1, math.ceil(0.99 * n)))
            q = [[float(p["means"][:, a].kthvalue(k).values) for a in range(3)] for k in ks]
            lo, hi = q
            grow = sdf_trunc
        else:
            grow = 0.0
        side = max(b - a for a, b in zip(lo, hi))
        if voxel_size is None:
            # side + 2 grow = resolution cells, with grow = sdf_trunc = 5 cells by default
            h = (side / (int(resolution) - 10) if grow is None
                 else (side + 2.0 * float(grow)) / int(resolution))
            if not h > 0.0:
                raise ValueError(f"{name}: the bounds are empty: pass voxel_size")
        else:
            h = float(voxel_size)
        trunc = 5.0 * h if sdf_trunc is None else float(sdf_trunc)
        grow = trunc if grow is None else float(grow)
        lo, hi = [a - grow for a in lo], [b + grow for b in hi]
        dims = [int(math.ceil((b - a) / h - 1e-6)) + 1 for a, b in zip(lo, hi)]
        if dims[0] * dims[1] * dims[2] > max_voxels:
            raise ValueError(f"{name}: a volume of {dims} grid points is more than max_voxels="
                             f"{max_voxels}; pass a larger voxel_size or tighter bounds")
        vol = TSDFVolume(lo, h, dims, sdf_trunc=trunc, device=self.device, colors=bool(colors))
        scales, opac = torch.exp(p["scales"]), torch.sigmoid(p["opacities"])
        for a in range(0, len(idx), camera_batch):
            ids = torch.tensor(idx[a:a + camera_batch], device=self.device)
            vms, Ks = self.viewmats.index_select(0, ids), self.Ks.index_select(0, ids)
            if self.model == "2dgs":
                out = rasterization_2dgs(p["means"], p["quats"], scales, opac,
                                         (p["sh0"], p["shN"]), vms, Ks, self.width, self.height,
                                         sh_degree=self.sh_degree, packed=False, near_plane=0.01,
                                         far_plane=1e10, render_mode="RGB+ED",
                                         depth_mode=depth_mode)
                rgbd, alphas, median = out[0], out[1], out[5]
                depth = median if depth_mode == "median" else rgbd[..., 3:4]
            else:
                if self.app_opt:  # geometry only: any colours do
                    coeffs, deg = p["colors"], None
                else:
                    coeffs, deg = (p["sh0"], p["shN"]), self.sh_degree
                rgbd, alphas, _ = rasterization(p["means"], p["quats"], scales, opac, coeffs, vms,
                                                Ks, self.width, self.height, sh_degree=deg,
                                                packed=False, near_plane=0.01, far_plane=1e10,
                                                rasterize_mode=self.rasterize_mode,
                                                render_mode="RGB+ED")
                depth = rgbd[..., 3:4]
            if self.masks is not None:
                alphas = alphas * self.masks.index_select(0, ids)[..., None].to(alphas.dtype)
            vol.integrate(depth.contiguous(), _wrapper._f32c(vms), _wrapper._f32c(Ks),
                          colors=rgbd[..., :3].contiguous() if colors else None, alphas=alphas,
                          depth_trunc=math.inf if depth_trunc is None else float(depth_trunc),
                          alpha_min=alpha_min)
        mesh = vol.extract_mesh(min_weight=min_weight)
        if path is not None:
            save_mesh_ply(path, *mesh)
        return mesh

    # ---------------------------------------------------------- persistence
    def save_checkpoint(self, path, step: int):
        """simple_trainer.py save_steps (:734-747): one torch.save file with the
        reference's keys ("step", "splats", "pose_adjust", "app_module"), which
        its `ckpt=` reads, plus a "gsplat_hip" block with everything else the
        next step reads (checkpoint.py), so load_checkpoint resumes the run
        exactly.  `step`: the index of the last completed step.  Calls sync()
        first; the trainer and a captured step are left untouched."""
        from . import checkpoint
        checkpoint.save(self, path, step)

    def load_checkpoint(self, paths, resume: bool = True) -> int:
        """Returns the checkpoint's step.  resume=True (one file written by
        save_checkpoint): the configuration fingerprint must match (ValueError
        naming every field that differs); parameters, moments, step counts, side
        optimizers, statistics and generator state are restored, and the
        caller continues with step(step + 1).  A list of files, resume=False,
        or a file of the reference trainer: its evaluation path
        (simple_trainer.py:1055-1064) -- the files' Gaussians concatenated,
        pose_adjust / app_module from the first, zero moments and step counts,
        fresh statistics."""
        from . import checkpoint
        return checkpoint.load(self, paths, resume)

    def load_splats(self, splats):
        """load_checkpoint's evaluation path for a dict name -> tensor, e.g.
        from gsplat_hip.load_ply or PngCompression.decompress."""
        from . import checkpoint
        checkpoint.load_splats(self, splats)

    def save_ply(self, path, sh_degree: Optional[int] = None, transform=None):
        """simple_trainer.py save_ply / ply_steps (:748-765): gsplat_hip.save_ply
        of the synced parameters; app_opt: the colours baked at the zero
        embedding and zero view direction at `sh_degree` (the reference passes
        the step's sh_degree_to_use; None: the trainer's sh_degree).

        `transform` ([4,4] similarity, numpy or tensor): the parameters go
        through `gsplat_hip.transform_splats` first, so the file is written in
        another frame; `transform=np.linalg.inv(parser.transform)` gives
        COLMAP's frame for a scene trained on `colmap.Parser(normalize=True)`.
        With app_opt the baked colours do not depend on the view, so only the
        geometry moves.  None: the bytes written are those of the parameters
        as they are."""
        from . import checkpoint
        return checkpoint.save_ply(self, path, sh_degree, transform)

    # ------------------------------------------------------------ strategy
    def post_step(self, it: int, replayed: bool = False):
        """DefaultStrategy.step_post_backward after the statistics
        (default.py:175-211): refine, then the opacity reset.  MCMC: its
        step_post_backward (mcmc_step); `replayed`: step `it` ran as a graph
        replay, which applied the position noise itself unless `it` refines."""
        cfg = self.strategy
        if self.mcmc:
            self.mcmc_step(it, noise=not (replayed and not cfg.is_refine_step(it)))
            return
        if it >= cfg.refine_stop_iter:
            return
        if cfg.is_refine_step(it):
            self.refine(it)
        if cfg.is_reset_step(it):
            self.reset_opacity()

    @torch.no_grad()
    def refine(self, it: int):
        self.sync()
        self.last_meta = None  # its tensors are sized for the old Gaussians
        if self.world_size > 1 and not self.gshard:
            # every rank accumulated its own cameras: the batch statistics are
            # the sums (the screen radii: their maximum)
            import torch.distributed as dist
            works = [dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=True)
                     for t in (self.grad2d, self.count)]
            if self.radii2d is not None:
                works.append(dist.all_reduce(self.radii2d, op=dist.ReduceOp.MAX, async_op=True))
            for w in works:
                w.wait()
        params = {k: p.data for k, p in self.params.items()}
        radii2d = self.radii2d if it < self.strategy.refine_scale2d_stop_iter else None
        new_p, new_m, counts = densify.refine(params, self._gaussian_moments(), self.grad2d, self.count,
                                              it, self.strategy, self.scene_scale,
                                              generator=self.rng, radii2d=radii2d)
        self.params = {k: torch.nn.Parameter(v) for k, v in new_p.items()}
        self._load_moments(new_m)
        self._register_hooks()
        n = self.params["means"].shape[0]
        self.grad2d = torch.zeros(n, device=self.device)
        self.count = torch.zeros(n, device=self.device)
        if self.radii2d is not None:
            self.radii2d = torch.zeros(n, device=self.device)
        self.refine_log.append((it,) + tuple(counts) + (n,))
        self._param_gen += 1  # a captured step re-captures
        if self.gshard and self.world_size > 1:  # each shard refined alone
            from .distributed import all_gather_int32
            self._n_world = all_gather_int32(self.world_size, n, device=self.device)

    @torch.no_grad()
    def mcmc_step(self, it: int, noise: bool = True):
        """MCMCStrategy.step_post_backward (mcmc.py:103-145) after step `it`'s
        optimizer update: on its refine steps relocate the dead Gaussians and
        sample in new ones (mcmc_refine), then the position noise (unless a
        graph replay of the step applied it)."""
        if self.strategy.is_refine_step(it):
            self.mcmc_refine(it)
        if noise:
            self.mcmc_noise(it)

    def mcmc_scaler(self, it: int) -> float:
        """The noise scale of step `it`: the means learning rate the reference
        passes (its scheduler already stepped, simple_trainer.py:808-829)
        times noise_lr (mcmc.py:143-145)."""
        lr = self.lrs[0]
        if self.max_steps:
            lr = lr * (0.01 ** (1.0 / self.max_steps)) ** (it + 1)
        return lr * self.strategy.noise_lr

    @torch.no_grad()
    def mcmc_noise(self, it: int):
        """inject_noise_to_position for step `it`, drawn in the kernel from
        (trainer key, it): the draw a graph replay of the step makes."""
        self.sync()
        _mcmc.inject_noise({k: p.data for k, p in self.params.items()}, self.mcmc_scaler(it),
                           seed=self._noise_seed, step=it)

    @torch.no_grad()
    def mcmc_refine(self, it: int):
        """_relocate_gs + _add_new_gs (mcmc.py:147-187) over the parameters and
        the Adam moments.  Gaussian-sharded: each shard alone, cap_max split
        evenly over the ranks."""
        cfg = self.strategy
        self.sync()
        self.last_meta = None
        if self._binoms is None:
            self._binoms = _mcmc.binoms(self.device)
        params = {k: p.data for k, p in self.params.items()}
        moms = self._gaussian_moments()
        dead = torch.sigmoid(params["opacities"].flatten()) <= cfg.min_opacity
        n_reloc = _mcmc.relocate(params, moms, dead, self._binoms, cfg.min_opacity,
                                 generator=self.rng)
        gshard = self.gshard and self.world_size > 1
        cap = -(-cfg.cap_max // self.world_size) if gshard else cfg.cap_max
        n_add = _mcmc.n_to_add(params["means"].shape[0], cap)
        if n_add > 0:
            params, moms = _mcmc.sample_add(params, moms, n_add, self._binoms, cfg.min_opacity,
                                            generator=self.rng)
        self.params = {k: torch.nn.Parameter(v) for k, v in params.items()}
        self._load_moments(moms)
        self._register_hooks()
        n = self.params["means"].shape[0]
        self.grad2d = torch.zeros(n, device=self.device)
        self.count = torch.zeros(n, device=self.device)
        self.refine_log.append((it, n_reloc, n_add, n))
        if cfg.verbose:
            print(f"Step {it}: Relocated {n_reloc} GSs. Added {n_add} GSs. Now having {n} GSs.")
        self._param_gen += 1
        if gshard:
            from .distributed import all_gather_int32
            self._n_world = all_gather_int32(self.world_size, n, device=self.device)

    @torch.no_grad()
    def reset_opacity(self):
        self.sync()
        value = self.strategy.prune_opa * 2.0
        if self.sharded:
            lim = float(torch.logit(torch.tensor(value, dtype=torch.float32)))
            self.params["opacities"].data.clamp_(max=lim)
            self.opt.zero_moments(list(self.params).index("opacities"))
        else:
            moms = self._gaussian_moments()
            densify.reset_opacity({"opacities": self.params["opacities"].data},
                                  {"opacities": moms["opacities"]}, value)

    def densify_desc(self):
        if self.strategy is None:
            return "off (DefaultStrategy statistics only; fixed Gaussian count)"
        c = self.strategy
        if self.mcmc:
            return (f"MCMCStrategy relocate + add every {c.refine_every} steps in "
                    f"({c.refine_start_iter}, {c.refine_stop_iter}), cap {c.cap_max}, position "
                    f"noise every step (noise_lr {c.noise_lr:g}); refines so far "
                    f"(step, relocated, added, N): {self.refine_log}")
        return (f"DefaultStrategy refine every {c.refine_every} steps in "
                f"({c.refine_start_iter}, {c.refine_stop_iter}), opacity reset every "
                f"{c.reset_every}; refines so far: {self.refine_log}")

    def allreduce_grads(self):
        """SUM the Gaussian gradients over ranks (RCCL over xGMI); issued
        largest-first so the long shN transfer starts earliest."""
        import torch.distributed as dist
        works = []
        for k in ("shN", "means", "quats", "scales", "sh0", "opacities"):
            gr = self.params[k].grad
            if gr is not None:
                works.append(dist.all_reduce(gr, op=dist.ReduceOp.SUM, async_op=True))
        for w in works:
            w.wait()

    @torch.no_grad()
    def update_state(self, meta, skip=None):
        """DefaultStrategy._update_state for packed=False without the host
        sync of torch.where (default.py:213-262): same sums, masked; the
        screen-radius maximum of state["radii"] while refine_scale2d_stop_iter
        > 0 (default.py:255-262).  `skip` (the fused dense path, a captured
        step): the device flag of a void step, which leaves the statistics."""
        if self.strategy is not None:
            key = self.strategy.key_for_gradient
        else:
            key = "gradient_2dgs" if self.model == "2dgs" else "means2d"
        if self.radii2d is not None:
            # radii / max(W, H) in float32 (int tensor / python float); the
            # reference's "should be scatter max" over the visible pairs --
            # invisible entries have radius 0 and leave the maximum unchanged
            r = meta["radii"].float() / float(max(meta["width"], meta["height"]))
            self.radii2d = torch.maximum(self.radii2d, r.amax(0))
        absgrad = getattr(self.strategy, "absgrad", False)
        if absgrad:
            g = meta[key].absgrad
        else:
            g = meta.get("means2d_grad") if key == "means2d" else None
            g = meta[key].grad if g is None else g
        if g is None:
            return
        if meta.get("gaussian_ids") is not None:  # packed: [nnz] pairs (default.py:240-254)
            ids = meta["gaussian_ids"]
            g = g.clone()
            g[..., 0] *= meta["width"] / 2.0 * meta["n_cameras"]
            g[..., 1] *= meta["height"] / 2.0 * meta["n_cameras"]
            self.grad2d.index_add_(0, ids, g.norm(dim=-1))
            self.count.index_add_(0, ids, torch.ones_like(ids, dtype=torch.float32))
            if self.radii2d is not None:
                self.radii2d[ids] = torch.maximum(
                    self.radii2d[ids],
                    meta["radii"].float() / float(max(meta["width"], meta["height"])))
            return
        if self.fused:
            update_state_(self.grad2d, self.count, g, meta["radii"], meta["width"],
                          meta["height"], meta["n_cameras"], skip=skip)
            return
        sx = meta["width"] / 2.0 * meta["n_cameras"]
        sy = meta["height"] / 2.0 * meta["n_cameras"]
        sel = meta["radii"] > 0  # [C, N]
        # elementwise hypot instead of a reduction over a size-2 dim
        nrm = torch.where(sel, torch.hypot(g[..., 0] * sx, g[..., 1] * sy), 0.0)
        if nrm.shape[0] == 1:
            self.grad2d.add_(nrm[0])
            self.count.add_(sel[0])
        else:
            self.grad2d.add_(nrm.sum(0))
            self.count.add_(sel.sum(0))
