"""GPU: l1_ssim_loss(masks=, alphas=, backgrounds=) -- the loss of
(masks ? img : 0) + backgrounds * (1 - alphas), composed inside the fused loss
kernel (csrc/ssim.hip fused_masked_kernel), against the float64 oracle of
tests/masked_loss_oracle.py.

The bar of every comparison with the oracle: ten times the float32 torch
composition's own error against the oracle on the same inputs
(losses.compose_masked, train_step.ssim and autograd, on the GPU), floored by
the tolerances of test_gpu_trainer.py's test_l1_ssim_loss_matches_torch: loss
rtol 1e-4 / atol 1e-5, gradients (grad_alpha too) rtol 1e-3 / atol 1e-9.

Measured on an MI355X (profiles/masked_loss/parity.txt): see MEASURED below."""

import pytest
import torch

import masked_loss_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

MEASURED = """30 oracle cases: loss errors up to 2.0e-07 (the 11 x 11 image, the float32
composition's own 3.7e-08 there), elsewhere up to 6.3e-08; gradients up to
7.3e-08 at max |g| 7.0e-02 and grad_alpha up to 1.7e-08 at 1.7e-02 (11 x 11),
elsewhere below 1e-09 at max |g| 1e-04 .. 3e-03; with the incoming gradient
2.5: grad 9.0e-11, grad_alpha 8.0e-11; grad_alpha under the mask 3.1e-11 at
1.4e-04.  All-true mask: loss and gradient equal the plain call's bits."""

SHAPES = [(1, 64, 80, 3), (2, 37, 131, 3), (1, 12, 100, 3), (1, 11, 11, 1), (3, 45, 33, 1)]
LAM = 0.2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def _mask(kind, B, H, W):
    return {"disc": O.disc_mask, "pixels": O.pixel_mask, "none": lambda *a: None}[kind](B, H, W)


_CASES = {}


def _case(shape, kind, bkgd, scale=1.0):
    """Inputs (CPU), the oracle's (loss, dL/dimg, dL/dalpha) and the float32
    torch composition's own errors against it: computed once per case."""
    key = (shape, kind, bkgd, scale)
    if key in _CASES:
        return _CASES[key]
    from gsplat_hip.losses import compose_masked
    from gsplat_hip.train_step import ssim
    B, H, W, C = shape
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C)
    img = torch.rand(B, H, W, C, generator=g)
    gt = torch.rand(B, H, W, C, generator=g)
    alphas = torch.rand(B, H, W, 1, generator=g)
    back = (torch.rand(B, C, generator=g) * 0.8 + 0.1) if bkgd else None
    m = _mask(kind, B, H, W)
    L, gc, ga = O.loss_and_grads(img, gt, LAM, m, alphas, back, scale=scale)
    # the float32 composition on the GPU
    i32 = img.to(DEV).requires_grad_(True)
    a32 = alphas.to(DEV).requires_grad_(bkgd)
    x = compose_masked(i32, None if m is None else m.to(DEV), a32,
                       None if back is None else back.to(DEV))
    y = gt.to(DEV)
    l32 = (x - y).abs().mean() * (1 - LAM) + (1 - ssim(x.permute(0, 3, 1, 2),
                                                       y.permute(0, 3, 1, 2))) * LAM
    (scale * l32).backward()
    own = dict(loss=abs(float(l32) - float(L)),
               grad=float((i32.grad.double().cpu() - gc).abs().max()),
               galpha=float((a32.grad.double().cpu() - ga).abs().max()) if bkgd else 0.0)
    _CASES[key] = dict(img=img, gt=gt, alphas=alphas, back=back, m=m, L=L, gc=gc, ga=ga, own=own)
    return _CASES[key]


def _ours(c, scale=1.0, img=None, **kw):
    from gsplat_hip.losses import l1_ssim_loss
    img = (c["img"] if img is None else img).to(DEV).requires_grad_(True)
    alphas = c["alphas"].to(DEV).requires_grad_(True)
    loss = l1_ssim_loss(img, c["gt"].to(DEV), LAM,
                        masks=None if c["m"] is None else c["m"].to(DEV), alphas=alphas,
                        backgrounds=None if c["back"] is None else c["back"].to(DEV), **kw)
    (scale * loss if scale != 1.0 else loss).backward()
    return loss.detach(), img.grad, alphas.grad


def _within(name, got, want, own, rtol, atol):
    got = got.double().cpu()
    err = (got - want).abs()
    allowed = torch.maximum(torch.full_like(want, 10.0 * own), atol + rtol * want.abs())
    print(f"  {name}: max err {float(err.max()):.3e}, max|want| {float(want.abs().max()):.3e}, "
          f"fp32 composition's own error {own:.3e}")
    assert bool((err <= allowed).all()), (name, float(err.max()), float(allowed.min()))


@pytest.mark.parametrize("bkgd", [False, True], ids=["nobkgd", "bkgd"])
@pytest.mark.parametrize("kind", ["disc", "pixels", "none"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradients_match_the_oracle(shape, kind, bkgd):
    c = _case(shape, kind, bkgd)
    print(f"{shape} {kind} bkgd={bkgd}")
    loss, g, ga = _ours(c)
    _within("loss", loss.reshape(()), c["L"].reshape(()), c["own"]["loss"], 1e-4, 1e-5)
    _within("grad", g, c["gc"], c["own"]["grad"], 1e-3, 1e-9)
    if bkgd:
        assert ga is not None and ga.shape == c["alphas"].shape
        _within("grad_alpha", ga, c["ga"], c["own"]["galpha"], 1e-3, 1e-9)
    else:
        assert ga is None


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]], ids=lambda s: "x".join(map(str, s)))
def test_option_off_is_todays_result(shape):
    from gsplat_hip.losses import l1_ssim_loss
    B, H, W, C = shape
    c = _case(shape, "none", False)
    a = c["img"].to(DEV).requires_grad_(True)
    la = l1_ssim_loss(a, c["gt"].to(DEV), LAM)
    la.backward()
    b = c["img"].to(DEV).requires_grad_(True)
    lb = l1_ssim_loss(b, c["gt"].to(DEV), LAM,
                      masks=torch.ones(B, H, W, dtype=torch.bool, device=DEV),
                      alphas=c["alphas"].to(DEV), backgrounds=None)
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("bkgd", [False, True], ids=["nobkgd", "bkgd"])
def test_masked_pixels_are_dead(bkgd):
    shape = SHAPES[1]
    c = _case(shape, "disc", bkgd)
    dead = ~c["m"]
    loss, g, ga = _ours(c)
    dirty = c["img"].clone()
    dirty[dead] = float("nan")
    dirty[:, 0, 0] = float("inf")
    dirty[:, -1, -1] = -float("inf")
    assert not bool(c["m"][:, 0, 0].any()) and not bool(c["m"][:, -1, -1].any())
    loss_d, g_d, ga_d = _ours(c, img=dirty)
    assert bool(torch.isfinite(loss_d)) and torch.equal(loss_d, loss)
    assert torch.equal(g_d, g) and bool(torch.isfinite(g_d).all())
    assert float(g_d[dead.to(DEV)].abs().max()) == 0.0
    assert float(g_d.abs().max()) > 0.0
    if bkgd:
        assert torch.equal(ga_d, ga)
        want = c["ga"][dead]
        assert float(want.abs().max()) > 1e-9  # not vacuous: the oracle's own value there
        _within("grad_alpha under the mask", ga_d[dead.to(DEV)], want, c["own"]["galpha"],
                1e-3, 1e-9)
        assert float(ga_d[dead.to(DEV)].abs().max()) > 0.0


def test_all_false_mask():
    from gsplat_hip.losses import l1_ssim_loss
    B, H, W, C = SHAPES[0]
    c = _case(SHAPES[0], "none", False)
    img = c["img"].to(DEV).requires_grad_(True)
    loss = l1_ssim_loss(img, c["gt"].to(DEV), LAM,
                        masks=torch.zeros(B, H, W, dtype=torch.bool, device=DEV))
    loss.backward()
    assert float(img.grad.abs().max()) == 0.0
    want = O.loss_of(torch.zeros(B, H, W, C, dtype=torch.float64), c["gt"].double(), LAM)
    torch.testing.assert_close(loss.double().cpu(), want, rtol=1e-4, atol=1e-5)


def test_stack_index_and_ring():
    from gsplat_hip.losses import l1_ssim_loss
    H, W = 37, 131
    g = torch.Generator().manual_seed(5)
    gt = torch.rand(4, H, W, 3, generator=g).to(DEV)
    masks = torch.stack([O.disc_mask(1, H, W, f)[0] for f in (0.45, 0.3, 0.2, 0.4)]).to(DEV)
    img0 = torch.rand(1, H, W, 3, generator=g).to(DEV)
    alphas = torch.rand(1, H, W, 1, generator=g).to(DEV)
    back = torch.tensor([[0.2, 0.5, 0.9]], device=DEV)
    for k in (0, 3):
        outs = []
        for form in ("direct", "index", "ring"):
            img = img0.clone().requires_grad_(True)
            al = alphas.clone().requires_grad_(True)
            kw = dict(masks=masks[k:k + 1], alphas=al, backgrounds=back)
            if form == "direct":
                loss = l1_ssim_loss(img, gt[k:k + 1].contiguous(), LAM, **kw)
            else:
                kw["masks"] = masks
                idx = torch.tensor([k], device=DEV)
                ring = torch.zeros(8, device=DEV)
                seq = torch.tensor([6], dtype=torch.int64, device=DEV)
                if form == "ring":
                    kw["_out_ring"] = (ring, seq)
                loss = l1_ssim_loss(img, gt, LAM, gt_index=idx, **kw)
                if form == "ring":
                    assert torch.equal(ring[(6 - 1) % 8], loss.detach())
                    assert int((ring != 0).sum()) == 1
            loss.backward()
            outs.append((loss.detach(), img.grad, al.grad))
        for o in outs[1:]:
            assert all(torch.equal(x, y) for x, y in zip(outs[0], o))


def test_two_calls_are_bit_identical():
    c = _case(SHAPES[1], "disc", True)
    a, b = _ours(c), _ours(c)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_incoming_gradient_scales_both_gradients():
    c = _case(SHAPES[1], "disc", True, scale=2.5)
    loss, g, ga = _ours(c, scale=2.5)
    _within("loss", loss.reshape(()), c["L"].reshape(()), c["own"]["loss"], 1e-4, 1e-5)
    _within("grad x 2.5", g, c["gc"], c["own"]["grad"], 1e-3, 1e-9)
    _within("grad_alpha x 2.5", ga, c["ga"], c["own"]["galpha"], 1e-3, 1e-9)
    one = _case(SHAPES[1], "disc", True)
    assert float(c["gc"].abs().max()) > 2.0 * float(one["gc"].abs().max())


def test_no_grad_and_unfused_paths_compose_in_torch():
    from gsplat_hip.losses import l1_ssim_loss
    c = _case(SHAPES[0], "disc", True)
    kw = dict(masks=c["m"].to(DEV), alphas=c["alphas"].to(DEV), backgrounds=c["back"].to(DEV))
    with torch.no_grad():
        l0 = l1_ssim_loss(c["img"].to(DEV), c["gt"].to(DEV), LAM, **kw)
    torch.testing.assert_close(l0.double().cpu(), c["L"], rtol=1e-4, atol=1e-5)
    img = c["img"].to(DEV).requires_grad_(True)
    l1 = l1_ssim_loss(img, c["gt"].to(DEV), LAM, fused=False, **kw)
    l1.backward()
    torch.testing.assert_close(l1.double().cpu(), c["L"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(img.grad.double().cpu(), c["gc"], rtol=1e-3, atol=1e-9)


def test_argument_errors():
    from gsplat_hip.losses import l1_ssim_loss
    img = torch.rand(1, 20, 24, 3, device=DEV, requires_grad=True)
    gt = torch.rand(1, 20, 24, 3, device=DEV)
    back = torch.rand(1, 3, device=DEV)
    ok = torch.ones(1, 20, 24, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match="alphas"):
        l1_ssim_loss(img, gt, LAM, backgrounds=back)
    with pytest.raises(ValueError, match="masks"):
        l1_ssim_loss(img, gt, LAM, masks=ok[:, :10])
    with pytest.raises(ValueError, match="masks"):
        l1_ssim_loss(img, gt, LAM, masks=ok.float())
    with pytest.raises(ValueError, match="_channels"):
        l1_ssim_loss(img, gt, LAM, masks=ok, _channels=3)
    with pytest.raises(ValueError, match="backgrounds"):
        l1_ssim_loss(img, gt, LAM, alphas=torch.rand(1, 20, 24, 1, device=DEV),
                     backgrounds=torch.rand(1, 4, device=DEV))
    with pytest.raises(ValueError, match="alphas"):
        l1_ssim_loss(img, gt, LAM, alphas=torch.rand(1, 20, 24, device=DEV), backgrounds=back)
