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
