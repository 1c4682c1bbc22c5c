"""GPU: the fused bilateral-grid slice and total variation
(gsplat_hip.bilagrid_slice / bilagrid_tv_loss, csrc/bilagrid.hip).

The truth in every test is the torch composition written here, evaluated in
float64 on the CPU: F.grid_sample(mode="bilinear", align_corners=True,
padding_mode="border") of the indexed grids at the pixel centres and the gray
guidance, the 3x4 matmul, and the index_select total variation.

The bar for each output tensor is max(1e-4 * max|f64|, 4 * e32), e32 the error
of the same composition run in float32 on the GPU (measured here), as
tests/test_gpu_geom_loss.py.

The gray of the composition is summed as 0.299 r + (0.587 g + 0.114 b): in
float64 that is exactly 1.0 for a pixel of ones (the left-to-right sum is
1 - 1e-16, inside the clamp), so the block of ones sits on torch's border
where no gradient passes to the guidance."""

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


def _gray(rgb):
    return 0.299 * rgb[..., 0] + (0.587 * rgb[..., 1] + 0.114 * rgb[..., 2])


def _affine(grids, rgb, idx):
    """[B,H,W,12] matrices sliced from grids[idx] (lib_bilagrid's forward)."""
    B, H, W, _ = rgb.shape
    x = (torch.arange(W, dtype=rgb.dtype, device=rgb.device) + 0.5) / W
    y = (torch.arange(H, dtype=rgb.dtype, device=rgb.device) + 0.5) / H
    gx = ((x - 0.5) * 2)[None, None, :].expand(B, H, W)
    gy = ((y - 0.5) * 2)[None, :, None].expand(B, H, W)
    gz = _gray(rgb) * 2.0 - 1.0
    xyz = torch.stack([gx, gy, gz], -1)[:, None]  # [B,1,H,W,3]
    A = F.grid_sample(grids[idx], xyz, mode="bilinear", align_corners=True,
                      padding_mode="border")  # [B,12,1,H,W]
    return A[:, :, 0].permute(0, 2, 3, 1)


def _slice(grids, rgb, idx):
    A = _affine(grids, rgb, idx).reshape(*rgb.shape[:3], 3, 4)
    return torch.matmul(A[..., :3], rgb.unsqueeze(-1)).squeeze(-1) + A[..., 3]


def _tv(x):
    tv = 0.0
    for i in range(2, x.dim()):
        n = x.shape[i]
        x1 = x.index_select(i, torch.arange(1, n, device=x.device))
        x2 = x.index_select(i, torch.arange(0, n - 1, device=x.device))
        tv = tv + ((x1 - x2) ** 2).sum() / x1[0].numel()
    return tv / x.shape[0]


def _blocks(H, W):
    """(rows of the zeros block, rows of the ones block, their columns)."""
    h = max(1, H // 5)
    return slice(0, h), slice(2 * h, 3 * h), slice(W // 3, max(2 * W // 3, W // 3 + 1))


# shape = (X, Y, W) of the grid; image H x W
CASES = {
    "small_grid": dict(shape=(5, 3, 4), N=3, B=1, H=37, W=53, idx=[1]),
    "default_grid": dict(shape=(16, 16, 8), N=2, B=1, H=67, W=131, idx=[0]),
    "image_smaller_than_grid": dict(shape=(16, 16, 8), N=2, B=1, H=7, W=9, idx=[1]),
    "tile_crosses_nodes": dict(shape=(16, 16, 8), N=2, B=1, H=270, W=480, idx=[1]),
    "batch_two_indices": dict(shape=(16, 16, 8), N=3, B=2, H=40, W=56, idx=[2, 0]),
    "batch_same_index": dict(shape=(6, 5, 3), N=2, B=2, H=33, W=47, idx=[1, 1]),
}


def _inputs(name):
    c = CASES[name]
    g = torch.Generator().manual_seed(len(name))
    X, Y, Wd = c["shape"]
    grids = torch.zeros(c["N"], 12, Wd, Y, X, dtype=torch.float64)
    grids[:, [0, 5, 10]] = 1.0
    grids = grids + 0.1 * torch.randn(grids.shape, generator=g, dtype=torch.float64)
    rgb = torch.rand(c["B"], c["H"], c["W"], 3, generator=g, dtype=torch.float64) * 1.6 - 0.3
    rz, ro, cols = _blocks(c["H"], c["W"])
    rgb[:, rz, cols] = 0.0
    rgb[:, ro, cols] = 1.0
    v_out = torch.randn(rgb.shape, generator=g, dtype=torch.float64)
    return grids, rgb, torch.tensor(c["idx"], dtype=torch.int64), v_out


def _run(slice_fn, tv_fn, grids, rgb, idx, v_out):
    """[out, v_rgb, v_grids (slice), tv, v_grids (tv)]"""
    gl, rl = grids.detach().clone().requires_grad_(True), rgb.detach().clone().requires_grad_(True)
    out = slice_fn(gl, rl, idx)
    out.backward(v_out)
    g2 = grids.detach().clone().requires_grad_(True)
    tv = tv_fn(g2)
    tv.backward()
    return [out.detach(), rl.grad, gl.grad, tv.detach(), g2.grad]


@functools.lru_cache(maxsize=None)
def _reference(name):
    ins = _inputs(name)
    truth = _run(_slice, _tv, *ins)
    f32 = _run(_slice, _tv, *[t.float().to(DEV) if t.is_floating_point() else t.to(DEV)
                              for t in ins])
    e32 = [float((a.double().cpu() - b).abs().max()) for a, b in zip(f32, truth)]
    return ins, truth, e32


def _hip(ins):
    import gsplat_hip
    grids, rgb, idx, v_out = [t.float().to(DEV) if t.is_floating_point() else t.to(DEV)
                              for t in ins]
    return _run(gsplat_hip.bilagrid_slice, gsplat_hip.bilagrid_tv_loss, grids, rgb, idx, v_out)


NAMES = ("out", "v_rgb", "v_grids", "tv", "v_grids_tv")


@pytest.mark.parametrize("name", list(CASES))
def test_values_and_gradients_match_float64(name):
    ins, truth, e32 = _reference(name)
    ours = _hip(ins)
    bad = []
    for what, a, b, e in zip(NAMES, ours, truth, e32):
        bar = max(1e-4 * float(b.abs().max()), 4.0 * e)
        err = float((a.double().cpu() - b).abs().max())
        print(f"{name} {what}: err {err:.3e} bar {bar:.3e} (e32 {e:.3e}, "
              f"max|f64| {float(b.abs().max()):.3e})")
        if not err <= bar:
            bad.append((what, err, bar))
    assert not bad, bad


@pytest.mark.parametrize("name", ["small_grid", "batch_two_indices"])
def test_rows_of_unindexed_images_are_exactly_zero(name):
    ins, _, _ = _reference(name)
    v_grids = _hip(ins)[2]
    rest = [n for n in range(CASES[name]["N"]) if n not in CASES[name]["idx"]]
    assert rest
    assert int(torch.count_nonzero(v_grids[rest])) == 0
    assert all(float(v_grids[n].abs().max()) > 0 for n in CASES[name]["idx"])


@pytest.mark.parametrize("name", ["small_grid", "tile_crosses_nodes"])
def test_no_guidance_gradient_on_the_clamp_borders(name):
    """The blocks of exact zeros and exact ones: gray = 0 and gray = 1.  The
    float64 autograd gradient there is the matrix path alone (torch's clamp
    convention), and with a grid whose 3x3 part is zero -- only the offsets
    vary -- v_rgb is the guidance path alone: exactly zero in both blocks,
    non-zero strictly inside the clamp."""
    import gsplat_hip
    ins, truth, _ = _reference(name)
    grids, rgb, idx, v_out = ins
    c = CASES[name]
    rz, ro, cols = _blocks(c["H"], c["W"])
    A = _affine(grids, rgb, idx).reshape(*rgb.shape[:3], 3, 4)
    matrix_path = torch.einsum("bhwkj,bhwk->bhwj", A[..., :3], v_out)
    for rows in (rz, ro):
        assert float((truth[1][:, rows, cols] - matrix_path[:, rows, cols]).abs().max()) < 1e-12
    g = torch.Generator().manual_seed(7)
    off = torch.zeros(grids.shape)
    off[:, [3, 7, 11]] = torch.randn(off[:, [3, 7, 11]].shape, generator=g)
    rl = rgb.float().to(DEV).requires_grad_(True)
    gsplat_hip.bilagrid_slice(off.to(DEV), rl, idx.to(DEV)).backward(v_out.float().to(DEV))
    v = rl.grad
    assert int(torch.count_nonzero(v[:, rz, cols])) == 0
    assert int(torch.count_nonzero(v[:, ro, cols])) == 0
    gray = _gray(rgb)
    inside = ((gray > 0.05) & (gray < 0.95)).to(DEV)
    outside = ((gray < -1e-4) | (gray > 1 + 1e-4)).to(DEV)
    assert int(inside.sum()) > 0 and int(outside.sum()) > 0
    assert float(v[inside].abs().max()) > 0
    assert int(torch.count_nonzero(v[outside])) == 0


def test_identity_grid_returns_its_input():
    import gsplat_hip
    g = torch.Generator().manual_seed(3)
    rgb = (torch.rand(2, 45, 61, 3, generator=g) * 1.6 - 0.3).to(DEV)
    grids = gsplat_hip.bilagrid_identity(3, device=DEV)
    out = gsplat_hip.bilagrid_slice(grids, rgb, [2, 0])
    assert float((out - rgb).abs().max()) <= 1e-6
    assert float(gsplat_hip.bilagrid_tv_loss(grids)) == 0.0


@pytest.mark.parametrize("name", ["default_grid", "tile_crosses_nodes"])
def test_two_backward_runs_are_bit_identical(name):
    """registers, lane-ordered workgroup sums and an ordered
    finish -- no atomics -- so every output repeats bit for bit."""
    ins, _, _ = _reference(name)
    a, b = _hip(ins), _hip(ins)
    for what, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), what


def test_python_index_and_argument_errors():
    import gsplat_hip
    ins, _, _ = _reference("small_grid")
    grids, rgb = ins[0].float().to(DEV), ins[1].float().to(DEV)
    a = gsplat_hip.bilagrid_slice(grids, rgb, 1)
    b = gsplat_hip.bilagrid_slice(grids, rgb, torch.tensor([1], device=DEV))
    assert torch.equal(a, b)
    with pytest.raises(IndexError):
        gsplat_hip.bilagrid_slice(grids, rgb, 3)
    for shape in ((1, 12, 1, 4, 4), (1, 12, 4, 1, 4), (1, 12, 4, 4, 1)):
        bad = torch.zeros(shape, device=DEV)
        with pytest.raises(ValueError):
            gsplat_hip.bilagrid_slice(bad, rgb, 0)
        with pytest.raises(ValueError):
            gsplat_hip.bilagrid_tv_loss(bad)
    with pytest.raises(ValueError):
        gsplat_hip.bilagrid_identity(2, (16, 1, 8), device=DEV)
