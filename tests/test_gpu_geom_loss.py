"""GPU: the fused 2DGS geometry loss (gsplat_hip.geometry_loss_2dgs,
csrc/geom_loss.hip) -- normal consistency between the rendered normals and
the normals of the rendered depth, plus depth distortion.

The truth in every test is the torch composition of code that predates the
kernel, evaluated in float64: rendering._rotate, rendering._depth_to_normal_torch
and plain torch ops,

    nl * mean(1 - <R n, alpha * n_d>) + dl * mean(distort).

The bar for the loss and for each gradient is
max(1e-4 * max|f64|, 4 * e32), e32 the error of the same composition run in
float32 on the GPU (measured here); 1e-4 is the bar of
test_depth_to_normal_matches_torch_formula."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NL, DL = 0.05, 0.01


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def _inputs(C, H, W, seed=0, block=True):
    """float64 CPU inputs: depth 2 + U(0,1), alpha U(0,1), unit normals scaled
    by alpha, distort U(0,1), a 6x9 background block (depth 0, alpha 0) where
    it fits, per-camera random rotations / translations and intrinsics."""
    g = torch.Generator().manual_seed(seed)
    depth = 2.0 + torch.rand(C, H, W, 1, generator=g, dtype=torch.float64)
    alpha = torch.rand(C, H, W, 1, generator=g, dtype=torch.float64)
    if block and H >= 12 and W >= 16:
        depth[:, 5:11, 4:13] = 0.0
        alpha[:, 5:11, 4:13] = 0.0
    n = torch.nn.functional.normalize(
        torch.randn(C, H, W, 3, generator=g, dtype=torch.float64), dim=-1) * alpha
    distort = torch.rand(C, H, W, 1, generator=g, dtype=torch.float64)
    c2w = torch.eye(4, dtype=torch.float64).repeat(C, 1, 1)
    Ks = torch.zeros(C, 3, 3, dtype=torch.float64)
    for c in range(C):
        q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
        q = q * torch.sign(torch.diagonal(r))
        if torch.det(q) < 0:
            q[:, 0] = -q[:, 0]
        c2w[c, :3, :3] = q
        c2w[c, :3, 3] = torch.randn(3, generator=g, dtype=torch.float64)
        f = float(W) * (1.0 + 0.2 * c)
        Ks[c] = torch.tensor([[f, 0, W / 2 + 0.3 * c], [0, 1.1 * f, H / 2 - 0.2 * c],
                              [0, 0, 1]], dtype=torch.float64)
    return n, depth, alpha, c2w, Ks, distort


def _compose(n, depth, alpha, c2w, Ks, distort, nl=NL, dl=DL, world=False, z_depth=True):
    """The loss as the parent commit's user would compose it."""
    from gsplat_hip.rendering import _depth_to_normal_torch, _rotate
    loss = 0.0
    if nl:
        nw = n if world else _rotate(c2w[..., :3, :3], n)
        nd = _depth_to_normal_torch(depth, c2w, Ks, z_depth=z_depth)
        loss = loss + nl * (1.0 - (nw * (alpha.detach() * nd)).sum(-1)).mean()
    if dl:
        loss = loss + dl * distort.mean()
    return loss


def _loss_and_grads(fn, n, depth, alpha, c2w, Ks, distort, **kw):
    leaves = [t.detach().clone().requires_grad_(True) for t in (n, depth, distort)]
    loss = fn(leaves[0], leaves[1], alpha, c2w, Ks, leaves[2], **kw)
    loss.backward()
    return [loss.detach()] + [t.grad for t in leaves]


CASES = {
    "ragged": dict(shape=(1, 37, 53), kw={}),
    "ragged_ray_depth": dict(shape=(1, 37, 53), kw=dict(z_depth=False)),
    "ragged_world": dict(shape=(1, 37, 53), kw=dict(world=True)),
    "two_cameras_rgbd": dict(shape=(2, 19, 70), kw={}, rgbd=True),
    "one_interior": dict(shape=(1, 3, 3), kw={}),
}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(float64 inputs, float64 truth, float32-composition error per quantity)."""
    case = CASES[name]
    ins = _inputs(*case["shape"], seed=len(name))
    truth = _loss_and_grads(_compose, *ins, **case["kw"])
    f32 = _loss_and_grads(_compose, *[t.float().to(DEV) for t in ins], **case["kw"])
    e32 = [float((a.double().cpu() - b).abs().max()) for a, b in zip(f32, truth)]
    return ins, truth, e32


def _hip(ins, rgbd=False, world=False, z_depth=True, nl=NL, dl=DL):
    """loss and gradients (normals, depth, distort) of the kernel on float32
    copies; rgbd: the depth is channel 3 of a [C,H,W,4] leaf."""
    from gsplat_hip import geometry_loss_2dgs
    n, depth, alpha, c2w, Ks, distort = [t.float().to(DEV) for t in ins]
    n.requires_grad_(True)
    distort.requires_grad_(True)
    if rgbd:
        img = torch.cat([torch.rand(*depth.shape[:3], 3, device=DEV), depth], -1)
        img.requires_grad_(True)
        d_in = img[..., 3:4]
        assert not d_in.is_contiguous()
    else:
        img = depth.requires_grad_(True)
        d_in = img
    loss = geometry_loss_2dgs(n, d_in, alpha, c2w, Ks, distort, normal_lambda=nl,
                              dist_lambda=dl, normals_space="world" if world else "camera",
                              z_depth=z_depth)
    assert loss.dim() == 0
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), n.grad, img.grad, distort.grad


@pytest.mark.parametrize("name", list(CASES))
def test_matches_float64_composition(name):
    case = CASES[name]
    ins, truth, e32 = _reference(name)
    loss, vn, vd, vdist = _hip(ins, rgbd=case.get("rgbd", False), **case["kw"])
    if case.get("rgbd"):
        assert torch.count_nonzero(vd[..., :3]) == 0
        vd = vd[..., 3:4]
    for what, got, want, e in zip(("loss", "v_normals", "v_depth", "v_distort"),
                                  (loss, vn, vd, vdist), truth, e32):
        assert got.shape == want.shape, (what, got.shape, want.shape)
        assert torch.isfinite(got).all(), what
        err = float((got.double().cpu() - want).abs().max())
        bar = max(1e-4 * float(want.abs().max()), 4.0 * e)
        print(f"{name} {what}: err {err:.3e} bar {bar:.3e} (f32 composition {e:.3e}, "
              f"max|f64| {float(want.abs().max()):.3e})")
        assert err <= bar, (name, what, err, bar)


@pytest.mark.parametrize("shape", [(1, 2, 5), (1, 1, 1)])
def test_all_border_images(shape):
    """No interior pixel: n_d = 0 everywhere, the normal term is 1."""
    ins = _inputs(*shape, seed=3, block=False)
    loss, vn, vd, vdist = _hip(ins)
    want = NL * 1.0 + DL * float(ins[5].float().double().mean())
    assert abs(float(loss) - want) <= 1e-6, (float(loss), want)
    assert torch.count_nonzero(vn) == 0 and torch.count_nonzero(vd) == 0
    P = shape[0] * shape[1] * shape[2]
    torch.testing.assert_close(vdist, torch.full_like(vdist, DL / P), rtol=1e-6, atol=0)


def test_deterministic():
    ins, _, _ = _reference("ragged")
    a, b = _hip(ins), _hip(ins)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_term_gating():
    from gsplat_hip import geometry_loss_2dgs
    from gsplat_hip._lib import GsplatHipError
    ins, _, _ = _reference("ragged")
    n, depth, alpha, c2w, Ks, distort = [t.float().to(DEV) for t in ins]
    # each term alone, the other's images absent
    only_d = geometry_loss_2dgs(None, None, None, c2w, Ks, distort, normal_lambda=0.0,
                                dist_lambda=DL)
    only_n = geometry_loss_2dgs(n, depth, alpha, c2w, Ks, None, normal_lambda=NL,
                                dist_lambda=0.0)
    both = geometry_loss_2dgs(n, depth, alpha, c2w, Ks, distort, normal_lambda=NL,
                              dist_lambda=DL)
    torch.testing.assert_close(only_d, DL * distort.mean(), rtol=1e-5, atol=1e-8)
    want_n = _compose(*ins, dl=0.0)
    assert abs(float(only_n) - float(want_n)) <= 1e-4 * abs(float(want_n))
    torch.testing.assert_close(only_n + only_d, both, rtol=1e-6, atol=1e-8)
    # the gradients of a single term
    n1 = n.clone().requires_grad_(True)
    d1 = depth.clone().requires_grad_(True)
    geometry_loss_2dgs(n1, d1, alpha, c2w, Ks, None, normal_lambda=NL, dist_lambda=0.0).backward()
    n2 = n.clone().requires_grad_(True)
    d2 = depth.clone().requires_grad_(True)
    t2 = distort.clone().requires_grad_(True)
    geometry_loss_2dgs(n2, d2, alpha, c2w, Ks, t2, normal_lambda=NL, dist_lambda=DL).backward()
    assert torch.equal(n1.grad, n2.grad) and torch.equal(d1.grad, d2.grad)
    t3 = distort.clone().requires_grad_(True)
    geometry_loss_2dgs(None, None, None, c2w, Ks, t3, normal_lambda=0.0,
                       dist_lambda=DL).backward()
    assert torch.equal(t3.grad, t2.grad)
    # alphas is a constant
    a4 = alpha.clone().requires_grad_(True)
    n4 = n.clone().requires_grad_(True)
    geometry_loss_2dgs(n4, depth, a4, c2w, Ks, distort).backward()
    assert a4.grad is None and n4.grad is not None
    # no CPU fallback, no silent pose gradient
    with pytest.raises(GsplatHipError):
        geometry_loss_2dgs(*[t.float() for t in ins])
    with pytest.raises(NotImplementedError):
        geometry_loss_2dgs(n, depth, alpha, c2w.clone().requires_grad_(True), Ks, distort)
    with pytest.raises(NotImplementedError):
        geometry_loss_2dgs(n, depth, alpha, c2w, Ks.clone().requires_grad_(True), distort)


def test_strided_depth_gradient_in_place():
    """Depth as channel 3 of an RGB+D leaf: its gradient is zero in the colour
    channels and the contiguous-depth result in channel 3."""
    ins, _, _ = _reference("two_cameras_rgbd")
    _, vn_c, vd_c, _ = _hip(ins, rgbd=False)
    _, vn_s, vd_s, _ = _hip(ins, rgbd=True)
    assert vd_s.shape[-1] == 4
    assert torch.count_nonzero(vd_s[..., :3]) == 0
    assert torch.equal(vd_s[..., 3:4], vd_c)
    assert torch.equal(vn_s, vn_c)
