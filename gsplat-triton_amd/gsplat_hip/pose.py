"""Camera pose optimisation (examples/utils.py CameraOptModule,
simple_trainer.py `pose_opt` / `pose_noise`), in HIP (csrc/pose.hip).

The parameter is the reference's: a float32 table [n_images, 9], row e =
(dx[3], d6[6]), zero-initialised (`pose_adjust.embeds.weight`: checkpoints
interchange).  R = rotation_6d_to_matrix(d6 + identity), T = [[R, dx], [0, 1]];
the adjusted camera-to-world is c2w T.

    pose_adjust(camtoworlds, deltas)    c2w T(deltas), differentiable in deltas
    pose_lr(it, max_steps, base)        the reference's learning rate

The trainer's pieces (Trainer(pose_opt=True)): pose_apply writes the step's
view matrix T^-1 viewmat, the projection backward leaves per-block pose
partials in a workspace (pose_workspace) and pose_bwd_adam reduces them in a
fixed order, chains them to the row and steps Adam over the whole table."""

import ctypes

import torch

from . import _lib
from ._wrapper import _dev_check, _f32c, _ptr, _stream
from .losses import SideOptimizer, adam_factors

BETAS = (0.9, 0.999)
EPS = 1e-8


def pose_lr(it, max_steps, base):
    """ExponentialLR(gamma = 0.01 ** (1 / max_steps)) on the pose optimizer
    (simple_trainer.py): the lr in force at step `it`; no schedule without
    max_steps (as the means')."""
    if not max_steps:
        return float(base)
    return float(base) * 0.01 ** (it / float(max_steps))


class _PoseAdjust(torch.autograd.Function):
    @staticmethod
    def forward(ctx, camtoworlds, deltas):
        c, d = _f32c(camtoworlds), _f32c(deltas)
        _dev_check(c, d)
        ctx.save_for_backward(c, d)
        ctx.delta_shape = deltas.shape
        out = torch.empty_like(c)
        _lib.call("gsplat_hip_pose_adjust_fwd", c.numel() // 16, _ptr(c), _ptr(d), _ptr(out),
                  _stream())
        return out

    @staticmethod
    def backward(ctx, v_out):
        c, d = ctx.saved_tensors
        v = torch.empty_like(d)
        _lib.call("gsplat_hip_pose_adjust_bwd", c.numel() // 16, _ptr(c), _ptr(d),
                  _ptr(_f32c(v_out)), _ptr(v), _stream())
        return None, v.view(ctx.delta_shape)


def pose_adjust(camtoworlds, deltas):
    """camtoworlds [..., 4, 4] times T(deltas [..., 9]) (CameraOptModule.forward
    after its embedding lookup).  The gradient goes to `deltas`; the cameras
    get none."""
    if camtoworlds.shape[-2:] != (4, 4) or deltas.shape[-1:] != (9,) or \
            camtoworlds.shape[:-2] != deltas.shape[:-1]:
        raise ValueError("pose_adjust: camtoworlds [..., 4, 4] and deltas [..., 9] with the same "
                         f"batch shape, got {tuple(camtoworlds.shape)} and {tuple(deltas.shape)}")
    return _PoseAdjust.apply(camtoworlds, deltas)


def _check_table(t, n, what):
    assert t.shape == (n, 9) and t.dtype == torch.float32 and t.is_contiguous(), (what, t.shape)


def _check_camera(base_viewmat, cam_index):
    assert base_viewmat.numel() == 16 and base_viewmat.dtype == torch.float32 \
        and base_viewmat.is_contiguous(), (base_viewmat.shape, base_viewmat.stride())
    assert cam_index.dtype == torch.int64 and cam_index.numel() == 1


def pose_workspace(N, device):
    """The projection backward's per-block pose partials (uninitialised)."""
    nbytes = int(_lib.query("gsplat_hip_pose_workspace_bytes", int(N)))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def pose_apply(base_viewmat, cam_index, embeds=None, noise=None, out=None, camtoworld_out=None):
    """out [1,4,4] = T(embeds[cam])^-1 T(noise[cam])^-1 base_viewmat: one
    launch; `cam_index` a device int64 [1], read on the device."""
    table = embeds if embeds is not None else noise
    n = table.shape[0]
    for t, what in ((embeds, "embeds"), (noise, "noise")):
        if t is not None:
            _check_table(t, n, what)
    _check_camera(base_viewmat, cam_index)
    _dev_check(base_viewmat, cam_index, table)
    if out is None:
        out = torch.empty(1, 4, 4, device=base_viewmat.device)
    _lib.call("gsplat_hip_pose_apply", n, _ptr(base_viewmat), _ptr(cam_index), _ptr(embeds),
              _ptr(noise), _ptr(out), _ptr(camtoworld_out), _stream())
    return out


def pose_bwd_adam(workspace, N, base_viewmat, cam_index, embeds, exp_avg, exp_avg_sq, lr,
                  weight_decay, step, noise=None, betas=BETAS, eps=EPS, hyper=None, skip=None):
    """The pose gradient of the step from `workspace` (the projection
    backward's partials of N Gaussians) and the dense Adam-with-L2 step over
    the whole table, one launch.  `hyper`: device f32[2] factors of a captured
    step (then lr / step are unused); `skip`: the device void-step flag."""
    n = embeds.shape[0]
    for t, what in ((embeds, "embeds"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _check_table(t, n, what)
    if noise is not None:
        _check_table(noise, n, "noise")
    _check_camera(base_viewmat, cam_index)
    _dev_check(workspace, base_viewmat, cam_index, embeds, exp_avg, exp_avg_sq)
    need = int(_lib.query("gsplat_hip_pose_workspace_bytes", int(N))) // 4
    assert workspace.dtype == torch.float32 and workspace.numel() >= need, (workspace.shape, need)
    _lib.call("gsplat_hip_pose_bwd_adam", n, int(N), _ptr(workspace), _ptr(base_viewmat),
              _ptr(cam_index), _ptr(embeds), _ptr(noise), _ptr(exp_avg), _ptr(exp_avg_sq),
              ctypes.c_float(lr), ctypes.c_float(betas[0]), ctypes.c_float(betas[1]),
              ctypes.c_float(eps), ctypes.c_float(weight_decay), int(step), _ptr(hyper),
              _ptr(skip), _stream())


class PoseOptimizer(SideOptimizer):
    """Trainer(pose_opt / pose_noise)'s state: `embeds` [n_images, 9] (utils.py
    CameraOptModule: embeds.weight, zero_init) with the moments of its Adam(lr
    pose_opt_lr sqrt(BS), weight_decay pose_opt_reg), the fixed perturbation
    `noise` (pose_perturb.random_init: N(0, pose_noise) from a generator of its
    own, or None), the step's view matrix and the projection backward's
    workspace.  `optimised` False (pose_noise alone): nothing is stepped."""

    name = "pose"

    def __init__(self, n_images, device, seed, optimised, noise_std, lr, weight_decay, max_steps):
        self.optimised, self.max_steps = bool(optimised), max_steps
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        self.embeds = torch.zeros(n_images, 9, device=device)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.embeds), torch.zeros_like(self.embeds)
        self.noise = None
        if noise_std > 0.0:
            g = torch.Generator().manual_seed(seed + 1013)
            self.noise = (torch.randn(n_images, 9, generator=g) * noise_std).to(device)
        self.viewmat = torch.empty(1, 4, 4, device=device)  # the step's view matrix

    def lr_at(self, it):
        """The learning rate at step `it` (pose_lr on pose_opt_lr sqrt(BS))."""
        return pose_lr(it, self.max_steps, self.lr)

    def _workspace(self, n):
        return pose_workspace(n, self.embeds.device)

    def apply(self, base, cam_index, out=None):
        """Launch (a): `base` [1,4,4] adjusted by the noise and embedding rows of
        the device index `cam_index` into `out` (default: the step's buffer)."""
        return pose_apply(base, cam_index, self.embeds if self.optimised else None, self.noise,
                          out=self.viewmat if out is None else out)

    def factors(self, it):
        return adam_factors([self.lr_at(it)], BETAS, self.step_count + 1)[0]

    def launch(self, s, hyper):
        """Launch (c): the pose gradient from the projection backward's partials
        and the pose Adam over the whole table."""
        if not s.geom_applied:
            raise RuntimeError("pose_opt: the projection backward did not run the geometry "
                               "Adam, so it formed no pose gradient (a loss term outside the "
                               "render reached the geometry parameters?)")
        lr, step = 0.0, 1  # unused with the device factors
        if hyper is None:
            self.step_count += 1
            lr, step = self.lr_at(s.it), self.step_count
        pose_bwd_adam(self.ws, self.ws_n, _f32c(s.viewmats), s.cam, self.embeds, self.exp_avg,
                      self.exp_avg_sq, lr, self.weight_decay, step, noise=self.noise, hyper=hyper,
                      skip=s.void)

    def moments(self):
        return {"pose_embeds": [self.exp_avg, self.exp_avg_sq]}

    def checkpoint_tables(self):
        return ({"pose_adjust": {"embeds.weight": self.embeds}} if self.optimised else {},
                {} if self.noise is None else {"pose_noise_table": self.noise})
