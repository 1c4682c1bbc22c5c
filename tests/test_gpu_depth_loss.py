"""GPU: the sparse depth-loss kernel pair (csrc/depth_loss.hip) against the
reference's composition (examples/simple_trainer.py:647-664 on an RGB+ED
render) written with torch ops in float64 on the CPU: the value and the
gradients with respect to the accumulated depth D and alpha.

Tolerance: the error of the same composition in float32 on the GPU against
the float64 oracle, on the same inputs, times ten (the atomics' summation
order), with a floor of 1e-6 of the largest magnitude of the quantity
compared.  Inputs keep |disp - 1/d_gt| away from zero (checked on the
oracle), so no sign depends on rounding.

Measured on an MI355X (profiles/depth_loss/parity.txt, every case prints its
own figures); the comparisons closest to their bars:
  loss       max 2.40, fp32 composition 1.6e-07, kernel 7.7e-08, bar 2.4e-06
  dL/dD      max 1.33, fp32 composition 1.0e-07, kernel 1.3e-07, bar 1.3e-06
  dL/dalpha  max 2.03, fp32 composition 2.3e-07, kernel 2.6e-07, bar 2.3e-06
(the 13-point image, where the floor decides).  In 37 of the 40 comparisons
the kernel is closer to the oracle than the float32 composition (2 to 2,400
times; it samples at (x, y) itself, the composition at the rounded
normalise / un-normalise round trip), e.g. the loss of the 257-point image
6.1e-08 against 1.5e-06, and dL/dD with the zero-alpha corner (magnitude
2.6e+11) 7.6e+03 against 3.4e+06."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def reference_term(depths, pts, dgt):
    """simple_trainer.py:649-664 without the scale: depths [1, H, W, 1] (the
    RGB+ED render's depth channel), pts [M, 2], dgt [M] -> (the mean disparity
    L1, disp - 1/d_gt [1, M]); differentiable."""
    _, H, W, _ = depths.shape
    points = pts[None]
    points = torch.stack([points[:, :, 0] / (W - 1) * 2 - 1,
                          points[:, :, 1] / (H - 1) * 2 - 1], dim=-1)  # normalize to [-1, 1]
    grid = points.unsqueeze(2)  # [1, M, 1, 2]
    s = F.grid_sample(depths.permute(0, 3, 1, 2), grid, align_corners=True)  # [1, 1, M, 1]
    s = s.squeeze(3).squeeze(1)  # [1, M]
    # the reference's where(s > 0, 1 / s, 0) with the reciprocal taken of a safe
    # argument: the same values, and a zero gradient where s <= 0 (autograd
    # of the reference's line gives 0 * inf = NaN at s == 0, a sample whose
    # corners are all empty; the kernel's gradient there is 0)
    pos = s > 0.0
    disp = torch.where(pos, 1.0 / torch.where(pos, s, torch.ones_like(s)), torch.zeros_like(s))
    disp_gt = 1.0 / dgt[None]
    return F.l1_loss(disp, disp_gt), disp - disp_gt


def composition(D, A, pts, dgt):
    """The reference's lines on one image: D, A [H, W] (A None: D is already
    the expected depth), pts [M, 2], dgt [M] -> (loss, dL/dD, dL/dA,
    min |disp - 1/d_gt|).  An image without points gives 0 and zero gradients
    (the documented difference: torch's mean of nothing is NaN)."""
    D = D.detach().clone().requires_grad_(True)
    A = None if A is None else A.detach().clone().requires_grad_(True)
    if pts.shape[0] == 0:
        return (torch.zeros((), dtype=D.dtype, device=D.device), torch.zeros_like(D),
                None if A is None else torch.zeros_like(D), float("inf"))
    ed = D if A is None else D / A.clamp(min=1e-10)  # the RGB+ED render's division
    loss, diff = reference_term(ed[None, :, :, None], pts, dgt)
    grads = torch.autograd.grad(loss, [D] if A is None else [D, A])
    margin = float(diff.detach().abs().min())
    return loss.detach(), grads[0], (None if A is None else grads[1]), margin


def _image(H, W, seed):
    """alpha in (0.3, 1), D = alpha * U(1, 3); one pixel with alpha = 0 (its D
    kept), one 2 x 2 cell with alpha = 0 and D = 0."""
    g = torch.Generator().manual_seed(seed)
    A = torch.rand(H, W, generator=g, dtype=torch.float64) * 0.7 + 0.3
    D = A * (torch.rand(H, W, generator=g, dtype=torch.float64) * 2.0 + 1.0)
    A[2, 5] = 0.0
    A[5:7, 1:3] = 0.0
    D[5:7, 1:3] = 0.0
    return D, A


def _special_points(H, W):
    return [
        (3.0, 2.0),                # exactly on the pixel lattice: weights 1, 0, 0, 0
        (0.0, 0.0),                # the origin
        (W - 0.5, 1.3),            # x in (W - 1, W): the right corners are padding
        (2.7, H - 0.25),           # y in (H - 1, H)
        (W - 0.125, H - 0.625),    # both
        (6.1, 3.2), (6.5, 3.5), (6.9, 3.9), (6.5, 3.5), (6.3, 3.7),  # one cell: collisions
        (4.6, 1.4),                # one corner (5, 2) with alpha = 0
        (1.5, 5.5), (1.2, 5.9),    # all four corners alpha = 0, D = 0: ed = 0
    ]


def _points(H, W, M, seed):
    """The special points first, then uniform ones; d_gt on either side of
    the rendered depth (1/d_gt in (0.125, 0.25) or (2.5, 5))."""
    g = torch.Generator().manual_seed(seed)
    sp = torch.tensor(_special_points(H, W), dtype=torch.float64)
    rnd = torch.rand(max(M, 1), 2, generator=g, dtype=torch.float64) \
        * torch.tensor([W - 1e-3, H - 1e-3], dtype=torch.float64)
    pts = torch.cat([sp, rnd])[:M]
    far = torch.rand(M, generator=g, dtype=torch.float64) * 4.0 + 4.0
    near = torch.rand(M, generator=g, dtype=torch.float64) * 0.2 + 0.2
    dgt = torch.where(torch.arange(M) % 2 == 0, far, near)
    # float32-representable inputs: the kernel and both compositions see the same numbers
    return pts.float().double(), dgt.float().double()


TABLES = {"0-1-63": (0, 1, 63), "65-257-13": (65, 257, 13)}
SHAPES = {"8x8": (8, 8), "16x12": (12, 16)}  # (H, W)


@functools.lru_cache(maxsize=None)
def _case(shape, table):
    """Inputs and the float64 oracle of a (shape, table) pair, computed once."""
    H, W = SHAPES[shape]
    D, A = _image(H, W, seed=H * 100 + W)
    D, A = D.float().double(), A.float().double()
    images = [_points(H, W, M, seed=17 * k + M) for k, M in enumerate(TABLES[table])]
    oracle = [composition(D, A, p, d) for p, d in images]
    return D, A, images, oracle


def _bar(ref32, ref64):
    own = float((ref32.double().cpu() - ref64).abs().max())
    top = float(ref64.abs().max())
    return 10.0 * own, 1e-6 * top, own, top


def _compare(tag, got, ref32, ref64):
    ten, floor, own, top = _bar(ref32, ref64)
    err = float((got.double().cpu() - ref64).abs().max())
    bar = max(ten, floor)
    print(f"  {tag}: max|ref| {top:.6e}, fp32 composition vs fp64 {own:.3e}, kernel vs fp64 "
          f"{err:.3e}, bar {bar:.3e}")
    assert err <= bar, (tag, err, bar)


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_table_kernel_against_fp64_oracle(shape, table):
    """Three images in one table, the image chosen by a device index; the
    render is a 4-channel image read in place."""
    from gsplat_hip.depth_loss import DepthPoints, table_depth_loss
    D, A, images, oracle = _case(shape, table)
    H, W = D.shape
    tab = DepthPoints(images, DEV)
    assert tab.counts == list(TABLES[table])
    g = torch.Generator().manual_seed(3)
    for i, (pts, dgt) in enumerate(images):
        rgbd = torch.rand(1, H, W, 4, generator=g)
        rgbd[0, :, :, 3] = D.float()
        rgbd = rgbd.to(DEV).requires_grad_(True)
        alphas = A.float().reshape(1, H, W, 1).to(DEV).requires_grad_(True)
        index = torch.tensor([i], dtype=torch.int64, device=DEV)
        loss = table_depth_loss(rgbd, alphas, tab, index, 3)
        v_img, v_alpha = torch.autograd.grad(loss, [rgbd, alphas])
        M = pts.shape[0]
        print(f"{shape} table {table} image {i} (M = {M}):")
        if M == 0:
            assert float(loss.detach()) == 0.0 and not v_img.any() and not v_alpha.any()
            continue
        l64, d64, a64, margin = oracle[i]
        assert margin > 1e-3, margin  # the input condition, on the oracle
        l32, d32, a32, _ = composition(D.float().to(DEV), A.float().to(DEV), pts.float().to(DEV),
                                       dgt.float().to(DEV))
        assert not v_img[..., :3].any()  # the colour channels get no gradient
        _compare("loss", loss.detach().reshape(1), l32.reshape(1), l64.reshape(1))
        _compare("dL/dD", v_img[0, :, :, 3], d32, d64)
        _compare("dL/dalpha", v_alpha[0, :, :, 0], a32, a64)
        # zero alpha at a corner: no alpha gradient there; at all corners: none at all
        assert float(v_alpha[0, 2, 5, 0]) == 0.0 and not v_alpha[0, 5:7, 1:3, 0].any()


def test_forward_is_bit_identical_between_calls():
    from gsplat_hip.depth_loss import DepthPoints, table_depth_loss
    D, A, images, _ = _case("16x12", "65-257-13")
    H, W = D.shape
    tab = DepthPoints(images, DEV)
    rgbd = D.float().reshape(1, H, W, 1).to(DEV)
    alphas = A.float().reshape(1, H, W, 1).to(DEV)
    index = torch.tensor([1], dtype=torch.int64, device=DEV)
    vals = [float(table_depth_loss(rgbd, alphas, tab, index)) for _ in range(4)]
    assert len(set(vals)) == 1, vals
    # an index outside the table is clamped, not followed
    hi = torch.tensor([99], dtype=torch.int64, device=DEV)
    lo = torch.tensor([-3], dtype=torch.int64, device=DEV)
    assert float(table_depth_loss(rgbd, alphas, tab, hi)) == \
        float(table_depth_loss(rgbd, alphas, tab, index + 1))
    assert float(table_depth_loss(rgbd, alphas, tab, lo)) == \
        float(table_depth_loss(rgbd, alphas, tab, index - 1))


def _public_inputs(M=65):
    """C = 3 images of M points each for gsplat_hip.sparse_depth_loss."""
    H, W = SHAPES["16x12"]
    Ds, As, Ps, Gs = [], [], [], []
    for c in range(3):
        D, A = _image(H, W, seed=50 + c)
        p, d = _points(H, W, M, seed=70 + c)
        Ds.append(D.float().double()), As.append(A.float().double())
        Ps.append(p), Gs.append(d)
    return torch.stack(Ds), torch.stack(As), torch.stack(Ps), torch.stack(Gs)


def _public_reference(D, A, P, G, dtype, device):
    """The mean over the C images of the composition (equal M: the reference's
    mean over [C, M])."""
    C = D.shape[0]
    outs = [composition(D[c].to(device, dtype), None if A is None else A[c].to(device, dtype),
                        P[c].to(device, dtype), G[c].to(device, dtype)) for c in range(C)]
    assert min(o[3] for o in outs) > 1e-3
    loss = torch.stack([o[0] for o in outs]).mean()
    vD = torch.stack([o[1] for o in outs]) / C
    vA = None if A is None else torch.stack([o[2] for o in outs]) / C
    return loss, vD, vA


@pytest.mark.parametrize("form", ["alphas", "no-alphas"])
def test_public_function_in_place_and_contiguous(form):
    """gsplat_hip.sparse_depth_loss on C = 3 images: the 4-channel render read
    in place against a contiguous [C,H,W,1] copy of the same data, both
    against the oracle; with alphas (RGB+D) and without (RGB+ED: the depth
    image is the expected depth and the only gradient)."""
    import gsplat_hip
    D, A, P, G = _public_inputs()
    if form == "no-alphas":
        D = (D / A.clamp(min=1e-10)).clamp(max=1e6).float().double()  # the expected depth
        A = None
    C, H, W = D.shape
    l64, d64, a64 = _public_reference(D, A, P, G, torch.float64, "cpu")
    l32, d32, a32 = _public_reference(D, A, P, G, torch.float32, DEV)
    g = torch.Generator().manual_seed(5)
    rgbd = torch.rand(C, H, W, 4, generator=g)
    rgbd[..., 3] = D.float()
    rgbd = rgbd.to(DEV).requires_grad_(True)
    alone = D.float().reshape(C, H, W, 1).to(DEV).requires_grad_(True)
    pts, dgt = P.float().to(DEV), G.float().to(DEV)
    res = []
    for tag, img in (("in place", rgbd), ("contiguous", alone)):
        alphas = None if A is None else A.float().reshape(C, H, W, 1).to(DEV).requires_grad_(True)
        loss = gsplat_hip.sparse_depth_loss(img, pts, dgt, alphas)
        grads = torch.autograd.grad(loss, [img] if A is None else [img, alphas])
        print(f"sparse_depth_loss ({form}, {tag}):")
        _compare("loss", loss.detach().reshape(1), l32.reshape(1), l64.reshape(1))
        _compare("dL/dD", grads[0][..., -1], d32, d64)
        if A is not None:
            _compare("dL/dalpha", grads[1][..., 0], a32, a64)
        res.append((loss.detach(), grads[0][..., -1]))
    assert not torch.autograd.grad(
        gsplat_hip.sparse_depth_loss(rgbd, pts, dgt, None), rgbd)[0][..., :3].any()
    assert float(res[0][0]) == float(res[1][0])  # the same reads, the same fixed-order sum
    # channel by number: the same plane
    a = None if A is None else A.float().reshape(C, H, W, 1).to(DEV)
    assert float(gsplat_hip.sparse_depth_loss(rgbd.detach(), pts, dgt, a, channel=3)) == \
        float(res[0][0])


def test_public_function_without_points():
    """M = 0: exactly 0 and zero gradients (torch: NaN)."""
    import gsplat_hip
    rgbd = torch.rand(2, 8, 8, 4, device=DEV, requires_grad=True)
    alphas = torch.rand(2, 8, 8, 1, device=DEV, requires_grad=True)
    loss = gsplat_hip.sparse_depth_loss(rgbd, torch.zeros(2, 0, 2, device=DEV),
                                        torch.zeros(2, 0, device=DEV), alphas)
    assert float(loss) == 0.0
    v_img, v_alpha = torch.autograd.grad(loss, [rgbd, alphas])
    assert not v_img.any() and not v_alpha.any()
