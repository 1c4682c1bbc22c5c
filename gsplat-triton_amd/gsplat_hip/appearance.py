"""Appearance optimisation (examples/utils.py AppearanceOptModule,
simple_trainer.py `app_opt`), in HIP (csrc/appearance.hip).

The per-Gaussian colour comes from a small MLP instead of SH coefficients:

    x      = cat(embeds[image] (16), features[n] (32), sh_bases(normalize(means[n] - campos)) (16))
    colors = sigmoid(Linear(64,3)(ReLU(Linear(64,64)(ReLU(Linear(64,64)(x))))) + base_colors[n])

The dimensions are the reference trainer's and fixed: feature_dim 32, embed_dim
16, module SH degree 3, width 64, depth 2.

    appearance_colors(features, base_colors, embeds, means, campos, head, sh_degree, masks)
        differentiable in features, base_colors, embeds, the head and means

The trainer's pieces: app_colors_fwd / app_colors_bwd (the two kernels; the
backward leaves per-workgroup partial sums of the head's and the embedding's
gradients in a workspace) and app_reduce_adam (their ordered sum, and the
reference's two Adam optimizers in place)."""

import ctypes
import math

import torch

from . import _lib
from ._wrapper import _aligned16, _dev_check, _f32c, _ptr, _stream
from .losses import SideOptimizer, adam_factors

FEATURE_DIM = 32
EMBED_DIM = 16
SH_DEGREE = 3
WIDTH = 64
HEAD_SHAPES = ((64, 64), (64,), (64, 64), (64,), (3, 64), (3,))
HEAD_KEYS = ("color_head.0.weight", "color_head.0.bias", "color_head.2.weight",
             "color_head.2.bias", "color_head.4.weight", "color_head.4.bias")
HEAD_NUMEL = 8515
BETAS = (0.9, 0.999)
EPS = 1e-8
EMBED_LR_MULT = 10.0  # simple_trainer.py: the embedding's lr is 10 x the head's


def head_tensors(head):
    """The six tensors W1, b1, W2, b2, W3, b3 from a sequence of six, a state
    dict with the reference module's keys (`color_head.{0,2,4}.{weight,bias}`,
    with or without the `color_head.` prefix) or a module with a `color_head`."""
    if hasattr(head, "color_head"):
        head = head.color_head.state_dict()
    if isinstance(head, dict):
        keys = HEAD_KEYS if HEAD_KEYS[0] in head else tuple(k[len("color_head."):]
                                                            for k in HEAD_KEYS)
        missing = [k for k in keys if k not in head]
        if missing:
            raise ValueError(f"appearance head: missing {missing}")
        head = [head[k] for k in keys]
    head = list(head)
    if len(head) != 6:
        raise ValueError(f"appearance head: six tensors (W1, b1, W2, b2, W3, b3), got {len(head)}")
    for t, shape in zip(head, HEAD_SHAPES):
        if tuple(t.shape) != shape:
            raise ValueError("appearance head: the fixed layout is Linear(64,64), Linear(64,64), "
                             f"Linear(64,3); got a tensor of shape {tuple(t.shape)} for {shape}")
    return head


def _check_shapes(features, base_colors, embeds, means, campos, sh_degree, masks):
    if features.dim() != 2 or features.shape[1] != FEATURE_DIM:
        raise ValueError(f"appearance: features [N, {FEATURE_DIM}], got {tuple(features.shape)}")
    N = features.shape[0]
    if tuple(base_colors.shape) != (N, 3) or tuple(means.shape) != (N, 3):
        raise ValueError("appearance: base_colors and means [N, 3], got "
                         f"{tuple(base_colors.shape)} and {tuple(means.shape)}")
    if campos.dim() != 2 or campos.shape[1] != 3:
        raise ValueError(f"appearance: campos [C, 3], got {tuple(campos.shape)}")
    C = campos.shape[0]
    if embeds is not None and tuple(embeds.shape) != (C, EMBED_DIM):
        raise ValueError(f"appearance: embeds [C, {EMBED_DIM}] or None, got {tuple(embeds.shape)}")
    if not 0 <= int(sh_degree) <= SH_DEGREE:
        raise ValueError(f"appearance: sh_degree in 0..{SH_DEGREE}, got {sh_degree}")
    if masks is not None and tuple(masks.shape) != (C, N):
        raise ValueError(f"appearance: masks [C, N], got {tuple(masks.shape)}")
    return C, N


def _check_rows(**tensors):
    """The kernels read `features` and read and write `v_features` as float4
    rows and everything else as plain float32 arrays: each given tensor must be
    float32 and contiguous, the feature rows 16-byte aligned as well."""
    for name, t in tensors.items():
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"appearance: {name} must be float32 and contiguous, got "
                             f"{t.dtype}, strides {tuple(t.stride())}")
        if name in ("features", "v_features") and t.data_ptr() % 16:
            raise ValueError(f"appearance: {name} must be 16-byte aligned (its rows are read "
                             "as float4); pass a fresh tensor instead of an offset view")


def _check_masks(masks, radii):
    if masks is not None and (masks.dtype not in (torch.uint8, torch.bool)
                              or not masks.is_contiguous()):
        raise ValueError("appearance: masks must be contiguous bool / uint8")
    if radii is not None and (radii.dtype != torch.int32 or not radii.is_contiguous()):
        raise ValueError("appearance: radii must be contiguous int32")


def _head_ptrs(head):
    return (ctypes.c_void_p * 6)(*[t.data_ptr() for t in head])


def app_workspace(N, C, device):
    """The backward's per-workgroup partial sums (uninitialised)."""
    nbytes = int(_lib.query("gsplat_hip_app_workspace_bytes", int(N), int(C)))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def app_colors_fwd(features, base_colors, means, campos, head, sh_degree, embeds=None,
                   embed_ids=None, masks=None, radii=None, out=None):
    """colors [C, N, 3], one launch.  `embeds` [n_images, 16] with the device
    int64 `embed_ids` [C] choosing the rows, or neither: the zero embedding.
    `masks` (bool/u8 [C, N]) and `radii` (int32 [C, N], visible where > 0)
    hide rows.  All tensors float32, contiguous, on the GPU."""
    C, N = campos.shape[0], features.shape[0]
    _dev_check(features, base_colors, means, campos, embeds, embed_ids, masks, radii, *head)
    _check_rows(features=features, base_colors=base_colors, means=means, campos=campos,
                embeds=embeds, out=out, **{f"head[{i}]": t for i, t in enumerate(head)})
    _check_masks(masks, radii)
    if out is None:
        out = torch.empty(C, N, 3, dtype=torch.float32, device=features.device)
    _lib.call("gsplat_hip_app_colors_fwd", C, N, int(sh_degree), _ptr(means), _ptr(campos),
              _ptr(features), _ptr(base_colors), _ptr(embeds), _ptr(embed_ids),
              0 if embeds is None else embeds.shape[0], _head_ptrs(head), _ptr(masks),
              _ptr(radii), _ptr(out), _stream())
    return out


def app_colors_bwd(v_colors, features, base_colors, means, campos, head, sh_degree, workspace,
                   embeds=None, embed_ids=None, masks=None, radii=None, v_base_colors=None,
                   v_features=None, v_means=None):
    """The per-row gradients (v_base_colors [N,3], v_features [N,32], v_means
    [N,3], summed over cameras, fully written) and the workspace rows that
    app_reduce_adam sums.  One launch."""
    C, N = campos.shape[0], features.shape[0]
    _dev_check(v_colors, features, base_colors, means, campos, embeds, embed_ids, masks, radii,
               workspace, *head)
    _check_rows(v_colors=v_colors, features=features, base_colors=base_colors, means=means,
                campos=campos, embeds=embeds, v_base_colors=v_base_colors,
                v_features=v_features, v_means=v_means,
                **{f"head[{i}]": t for i, t in enumerate(head)})
    _check_masks(masks, radii)
    need = int(_lib.query("gsplat_hip_app_workspace_bytes", N, C)) // 4
    assert workspace.dtype == torch.float32 and workspace.numel() >= need, (workspace.shape, need)
    dev = features.device
    if v_base_colors is None:
        v_base_colors = torch.empty(N, 3, dtype=torch.float32, device=dev)
    if v_features is None:
        v_features = torch.empty(N, FEATURE_DIM, dtype=torch.float32, device=dev)
    if v_means is None:
        v_means = torch.empty(N, 3, dtype=torch.float32, device=dev)
    _lib.call("gsplat_hip_app_colors_bwd", C, N, int(sh_degree), _ptr(means), _ptr(campos),
              _ptr(features), _ptr(base_colors), _ptr(embeds), _ptr(embed_ids),
              0 if embeds is None else embeds.shape[0], _head_ptrs(head), _ptr(masks),
              _ptr(radii), _ptr(v_colors), _ptr(v_base_colors), _ptr(v_features), _ptr(v_means),
              _ptr(workspace), _stream())
    return v_base_colors, v_features, v_means


def app_reduce(workspace, N, C, grads=None):
    """grads [8515 + 16 C]: the head's gradients in the flat order W1, b1, W2,
    b2, W3, b3, then 16 per camera for its embedding row.  No step."""
    _dev_check(workspace)
    if grads is None:
        grads = torch.empty(HEAD_NUMEL + EMBED_DIM * C, dtype=torch.float32,
                            device=workspace.device)
    _lib.call("gsplat_hip_app_reduce_adam", int(C), int(N), _ptr(workspace), _ptr(grads), 0,
              None, None, None, None, None, 0, None, None, ctypes.c_float(0), ctypes.c_float(0),
              ctypes.c_float(0), ctypes.c_float(0), ctypes.c_float(0), ctypes.c_float(0), 0,
              None, None, _stream())
    return grads


def app_reduce_adam(workspace, N, C, grads, head, head_exp_avg, head_exp_avg_sq, lr, step,
                    embeds=None, embed_ids=None, embed_exp_avg=None, embed_exp_avg_sq=None,
                    embed_weight_decay=0.0, embed_lr_mult=EMBED_LR_MULT, betas=BETAS, eps=EPS,
                    hyper=None, skip=None):
    """The ordered sum of the workspace rows into `grads`, then the
    reference's two optimizers in place: Adam(lr) on the head (moments flat
    [8515]) and Adam(lr * embed_lr_mult, weight_decay) on the whole table.
    `hyper`: device f32[4] factors of a captured step (then lr / step are
    unused); `skip`: the device void-step flag."""
    _dev_check(workspace, grads, head_exp_avg, head_exp_avg_sq, embeds, embed_ids, embed_exp_avg,
               embed_exp_avg_sq, *head)
    assert head_exp_avg.numel() == HEAD_NUMEL and head_exp_avg_sq.numel() == HEAD_NUMEL
    assert grads.numel() >= HEAD_NUMEL + EMBED_DIM * C
    _lib.call("gsplat_hip_app_reduce_adam", int(C), int(N), _ptr(workspace), _ptr(grads), 1,
              _head_ptrs(head), _ptr(head_exp_avg), _ptr(head_exp_avg_sq), _ptr(embeds),
              _ptr(embed_ids), 0 if embeds is None else embeds.shape[0], _ptr(embed_exp_avg),
              _ptr(embed_exp_avg_sq), ctypes.c_float(lr), ctypes.c_float(betas[0]),
              ctypes.c_float(betas[1]), ctypes.c_float(eps), ctypes.c_float(embed_lr_mult),
              ctypes.c_float(embed_weight_decay), int(step), _ptr(hyper), _ptr(skip), _stream())
    return grads


class _AppearanceColors(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, base_colors, embeds, means, campos, masks, sh_degree, *head):
        f = _aligned16(_f32c(features))
        b, m, cp = _f32c(base_colors), _f32c(means), _f32c(campos)
        e = _f32c(embeds)
        hd = [_f32c(t) for t in head]
        mk = None if masks is None else masks.to(torch.uint8).contiguous()
        _dev_check(f, b, m, cp, e, mk, *hd)
        C = cp.shape[0]
        ids = None if e is None else torch.arange(C, dtype=torch.int64, device=f.device)
        ctx.save_for_backward(f, b, m, cp, e, ids, mk, *hd)
        ctx.sh_degree = int(sh_degree)
        return app_colors_fwd(f, b, m, cp, hd, sh_degree, embeds=e, embed_ids=ids, masks=mk)

    @staticmethod
    def backward(ctx, v_colors):
        f, b, m, cp, e, ids, mk, *hd = ctx.saved_tensors
        C, N = cp.shape[0], f.shape[0]
        ws = app_workspace(N, C, f.device)
        v_b, v_f, v_m = app_colors_bwd(_f32c(v_colors), f, b, m, cp, hd, ctx.sh_degree, ws,
                                       embeds=e, embed_ids=ids, masks=mk)
        g = app_reduce(ws, N, C)
        v_head, o = [], 0
        for shape in HEAD_SHAPES:
            n = shape[0] * (shape[1] if len(shape) > 1 else 1)
            v_head.append(g[o:o + n].view(shape))
            o += n
        v_e = None if e is None else g[HEAD_NUMEL:HEAD_NUMEL + EMBED_DIM * C].view(C, EMBED_DIM)
        return (v_f, v_b, v_e, v_m, None, None, None, *v_head)


class _TrainerColors(torch.autograd.Function):
    """The training step's colours [1, N, 3] (Trainer(app_opt=True)): the
    forward kernel over the projection's radii, the backward kernel leaving the
    head's and the embedding row's partial sums in the module's workspace
    (AppearanceOptimizer.launch sums them and steps the module's optimizers) and
    handing dL/dmeans to the step's StepFusion, as the SH colours' backward
    does, so the projection backward's geometry Adam sees the whole gradient."""

    @staticmethod
    def forward(ctx, features, base_colors, means, radii, campos, sh_degree, embeds, embed_ids,
                workspace, fusion, *head):
        if fusion is not None and fusion.geom and ctx.needs_input_grad[2]:
            fusion.expect_v_dirs = True
        f, b, m = _aligned16(_f32c(features)), _f32c(base_colors), _f32c(means)
        r = radii.to(torch.int32).contiguous()
        cp = _f32c(campos)
        ctx.save_for_backward(f, b, m, r, cp, embeds, embed_ids, workspace, *head)
        ctx.sh_degree, ctx.fusion = int(sh_degree), fusion
        return app_colors_fwd(f, b, m, cp, head, sh_degree, embeds=embeds, embed_ids=embed_ids,
                              radii=r)

    @staticmethod
    def backward(ctx, v_colors):
        f, b, m, r, cp, e, ids, ws, *hd = ctx.saved_tensors
        v_b, v_f, v_m = app_colors_bwd(_f32c(v_colors), f, b, m, cp, hd, ctx.sh_degree, ws,
                                       embeds=e, embed_ids=ids, radii=r)
        if not ctx.needs_input_grad[2]:
            v_m = None
        elif ctx.fusion is not None:
            v_m = ctx.fusion.take_means_grad(v_m)
        return (v_f, v_b, v_m) + (None,) * (7 + len(hd))


def trainer_colors(features, base_colors, means, radii, campos, head, sh_degree, embeds,
                   embed_ids, workspace, fusion=None):
    """Trainer(app_opt=True)'s colour node (see _TrainerColors); `radii` is
    the projection's [1, N] or per-axis [1, N, 2] (visible where all > 0)."""
    if radii.dim() == 3:
        radii = radii.amin(-1)
    return _TrainerColors.apply(features, base_colors, means, radii, campos, int(sh_degree),
                                embeds, embed_ids, workspace, fusion, *head)


def appearance_colors(features, base_colors, embeds, means, campos, head, sh_degree, masks=None):
    """colors [C, N, 3] of the reference's AppearanceOptModule followed by the
    trainer's `sigmoid(. + colors)` (simple_trainer.py:389-410).

    features [N, 32], base_colors [N, 3] (logits), embeds [C, 16] (the rows of
    the step's images) or None (the zero embedding of the reference's
    evaluation), means [N, 3], campos [C, 3] (camera centres), head the six
    tensors W1, b1, W2, b2, W3, b3 or anything with the reference module's
    `color_head` state layout, sh_degree 0..3 (bases beyond it are zero),
    masks bool [C, N] (rows it hides get colour 0 and no gradient).

    Gradients go to features, base_colors, embeds, the head and means; the
    camera centres get none (NotImplementedError if they ask for one)."""
    hd = head_tensors(head)
    _check_shapes(features, base_colors, embeds, means, campos, sh_degree, masks)
    if campos.requires_grad:
        raise NotImplementedError("appearance_colors: no gradient for campos (a pose gradient "
                                  "through the view directions is not implemented)")
    _dev_check(features, base_colors, embeds, means, campos, masks, *hd)
    return _AppearanceColors.apply(features, base_colors, embeds, means, campos, masks,
                                   int(sh_degree), *hd)


class AppearanceOptimizer(SideOptimizer):
    """Trainer(app_opt=True)'s module (utils.py AppearanceOptModule) and its two
    Adam optimizers: `embeds` [n_images, 16], N(0,1); the head, one buffer `flat`
    in the order W1, b1, W2, b2, W3, b3 with `head` its six views (torch's
    default Linear initialisation, U(+-1/sqrt(fan_in)), the last layer zero);
    both pairs of moments, the gradient buffer, the colour backward's workspace.
    Every draw comes from a generator of its own.  `groups`: the initial
    `features` U(0,1) [N,32] and logits `colors`, which the trainer takes as
    groups of its own Adam (the rgbs clamped to [1/512, 1 - 1/512] first: the
    reference's plain logit gives +-inf for pure black or white SfM points)."""

    name = "app"

    def __init__(self, n_images, rgbs, device, seed, lr, weight_decay, embed_dim, sh_degree):
        if int(embed_dim) != 16:
            raise ValueError("app_opt: app_embed_dim is fixed at 16 (the kernels' layout), "
                             f"got {embed_dim!r}")
        if int(sh_degree) != 3:
            raise ValueError("app_opt: sh_degree is fixed at 3 (the module's 16 bases), "
                             f"got {sh_degree!r}")
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        g = torch.Generator().manual_seed(seed + 2027)
        self.groups = {"features": torch.rand(rgbs.shape[0], FEATURE_DIM, generator=g),
                       "colors": torch.logit(rgbs.float().clamp(1.0 / 512, 1.0 - 1.0 / 512))}
        self.embeds = torch.randn(n_images, EMBED_DIM, generator=g).to(device)
        flat = (torch.rand(HEAD_NUMEL, generator=g) * 2.0 - 1.0) * (1.0 / math.sqrt(WIDTH))
        flat[2 * (WIDTH * WIDTH + WIDTH):] = 0.0
        self.flat = flat.to(device)
        self.head = [t.view(shape) for t, shape in zip(
            self.flat.split([math.prod(shape) for shape in HEAD_SHAPES]), HEAD_SHAPES)]
        self.head_moments = [torch.zeros_like(self.flat), torch.zeros_like(self.flat)]
        self.embed_moments = [torch.zeros_like(self.embeds), torch.zeros_like(self.embeds)]
        self.grads = torch.zeros(HEAD_NUMEL + EMBED_DIM, device=device)

    def _workspace(self, n):
        return app_workspace(n, 1, self.embeds.device)

    def colors(self, params, viewmats, sh_degree, cam_index, fusion):
        """rasterization(_app=...)'s callable: the colours [1,N,3] of the camera
        `viewmats` [1,4,4] from the projection's radii (invisible Gaussians are
        skipped), the embedding row of the device index `cam_index` (None: the
        zero embedding of the reference's evaluation)."""
        ws = self.prepare(params["means"].shape[0])
        vm = viewmats.detach()
        # the camera centre -R^T t, elementwise on the device
        campos = -(vm[:, :3, :3] * vm[:, :3, 3:4]).sum(1)
        return lambda radii: trainer_colors(
            params["features"], params["colors"], params["means"], radii, campos, self.head,
            sh_degree, None if cam_index is None else self.embeds, cam_index, ws, fusion)

    def factors(self, it):
        """torch's Adam for the head (lr) and the embedding table (10 x lr)."""
        lrs = [self.lr, self.lr * EMBED_LR_MULT]
        (sh, ib), (se, _) = adam_factors(lrs, BETAS, self.step_count + 1)
        return sh, ib, se, 0.0

    def launch(self, s, hyper):
        """After the backward: the ordered sum of the colour backward's partial
        sums and the module's two Adam optimizers in place (head: lr; the
        embedding table: 10 x lr with app_opt_reg as weight decay, dense)."""
        if hyper is None:
            self.step_count += 1
        app_reduce_adam(self.ws, self.ws_n, 1, self.grads, self.head, *self.head_moments,
                        self.lr, self.step_count, embeds=self.embeds, embed_ids=s.cam,
                        embed_exp_avg=self.embed_moments[0],
                        embed_exp_avg_sq=self.embed_moments[1],
                        embed_weight_decay=self.weight_decay, hyper=hyper, skip=s.void)

    def moments(self):
        return {"app_embeds": list(self.embed_moments), "app_head": list(self.head_moments)}

    def checkpoint_tables(self):
        return {"app_module": {"embeds.weight": self.embeds, **dict(zip(HEAD_KEYS, self.head))}}, {}

    def state_dict(self):
        """A copy under the reference module's keys: checkpoints interchange."""
        return {k: t.detach().clone() for k, t in self.checkpoint_tables()[0]["app_module"].items()}
