"""GPU: the wide-channel rasterizer (csrc/rasterize_wide.hip, `wide=True`)
against the float64 oracle, under tile masks, and through rasterization().

Scenes, oracle runs and bars are tests/raster_cases.py's, unchanged.  On the
CPU the float32 oracle stays within these bars against the float64 oracle on
each of the five cases (forward from its own render, the same last ids;
backward from its own alphas and last ids): nothing outside for any output,
but one v_conics row on the edge scene at D = 96 (close_most allows two)."""

import numpy as np
import pytest
import torch

import raster_cases as RC
from raster_cases import (build_case, check_forward, check_grads, close_most, oracle_backward,
                          oracle_forward, tile_mask)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = np.float64
GRADS = ("v_means2d", "v_conics", "v_colors", "v_opacities", "v_backgrounds")
# (scene, channels) at 16x16 tiles: padding inside one 32-block; exactly two
# blocks; two forward slabs, the last partial; long tiles with early
# termination; the value edges
CASES = [("sparse", 40), ("sparse", 64), ("sparse", 160), ("dense", 64), ("edge", 96)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401  (fails loudly if the .so is missing)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _render(case, masks=None, **kw):
    """rasterize_to_pixels(wide=True) forward and backward of a case (with
    backgrounds requiring grad, absgrad and a cotangent on the alphas): dict
    of numpy outputs named as the oracle's.  A HIP error ends the session."""
    import gsplat_hip
    ins = [T(x).requires_grad_(True)
           for x in (case.means2d, case.conics, case.colors, case.opacities)]
    ins.append(T(case.backgrounds).requires_grad_(True))
    try:
        rc, ra = gsplat_hip.rasterize_to_pixels(
            *ins[:4], case.W, case.H, case.ts, T(case.offsets), T(case.flatten_ids),
            backgrounds=ins[4], masks=None if masks is None else T(masks), absgrad=True,
            wide=True, **kw)
        assert type(rc.grad_fn).__name__ == "_RasterizeToPixelsWideBackward"
        last_ids = rc.grad_fn.saved_tensors[9]  # saved by the forward, as _RasterizeToPixels
        loss = (rc * T(case.v_colors)).sum() + (ra * T(case.v_alphas)).sum()
        grads = torch.autograd.grad(loss, ins)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"GPU fault, stopping: {e}", returncode=3)
        raise
    out = {"colors": rc, "alphas": ra, "last_ids": last_ids,
           "v_means2d_abs": ins[0].absgrad, **dict(zip(GRADS, grads))}
    out = {k: v.detach().cpu().numpy() for k, v in out.items()}
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    return out


@pytest.mark.parametrize("kind,D", CASES)
def test_wide_vs_float64_oracle(kind, D):
    """Forward at FWD_BARS, gradients at GRAD_BARS against the float64 oracle
    run from the kernel's own alphas and last ids; on the edge scene, where no
    threshold hangs on rounding, the oracle's last ids exactly."""
    case = build_case(kind, 16, D, backend="hip")
    got = _render(case)
    ref = oracle_forward(case, F64)
    check_forward(got, ref, f"{kind} D={D}")
    if kind == "edge":
        assert np.array_equal(got["last_ids"], ref["last_ids"])
    check_grads(got, oracle_backward(case, F64, got["alphas"], got["last_ids"]), f"{kind} D={D}")


def test_wide_tile_masks():
    """masks[tile] == True skips the tile in both directions, as in the
    existing kernels: background and alpha exactly 0 there, the oracle over
    the unmasked tiles elsewhere, exactly zero rows for Gaussians that touch
    masked tiles only."""
    case = build_case("sparse", 16, 64, backend="hip")
    mask = tile_mask(case)
    only = RC.only_masked_gaussians(case, mask)
    assert only.any()
    tiles = np.flatnonzero(~mask.reshape(-1))
    got = _render(case, masks=mask)
    px = np.repeat(np.repeat(mask, 16, 1), 16, 2)[:, :case.H, :case.W]
    assert not got["alphas"][px].any() and not got["last_ids"][px].any()
    for c in range(case.C):
        assert np.array_equal(got["colors"][c][px[c]],
                              np.broadcast_to(case.backgrounds[c], (int(px[c].sum()), case.D)))
    ref = oracle_forward(case, F64, tiles=tiles)
    check_forward(got, ref, "masked")
    check_grads(got, oracle_backward(case, F64, ref["alphas"], ref["last_ids"], tiles=tiles),
                "masked")
    for k in ("v_means2d", "v_conics", "v_colors", "v_opacities", "v_means2d_abs"):
        assert not got[k].reshape(case.C * case.N, -1)[only].any(), k


@pytest.mark.parametrize("packed", [False, True])
def test_rasterization_wide_channels(packed):
    """rasterization(wide_channels=True) with 47 feature channels and RGB+ED
    (48 rasterized channels) against the chunked path of wide_channels=False:
    outputs at FWD_BARS, gradients at GRAD_BARS' tolerances (the loosest of
    the rasterizer gradients a parameter's gradient flows through).

    meta["means2d"].absgrad is held to the float64 oracle's backward on the
    front end's own projected tensors instead: the chunked path cannot serve
    as its reference.  Every 32-channel render overwrites .absgrad with its
    own sum over pixels of |gradient of that slice|, so the attribute ends as
    one slice's, and no sum of slices' absolute values is the absolute value
    of the pixel's whole gradient.  Measured: 769 of 800 rows (packed: of 782)
    differ from the wide path's beyond 5e-3, by up to 134."""
    import gsplat_hip
    N, C, W, H = 400, 2, 48, 40
    means, quats, scales, opac, vm, K = RC._garden_scene(N, C, W, H, seed=3, scale=0.1)
    g = torch.Generator().manual_seed(5)
    feats, bg = torch.rand(N, 47, generator=g), torch.rand(C, 47, generator=g)
    vc, va = torch.randn(C, H, W, 48, generator=g), torch.randn(C, H, W, 1, generator=g)

    def run(wide):
        ins = [x.to(DEV).requires_grad_(True) for x in (means, quats, scales, opac, feats)]
        rc, ra, meta = gsplat_hip.rasterization(
            *ins, vm.to(DEV), K.to(DEV), W, H, sh_degree=None, render_mode="RGB+ED",
            packed=packed, absgrad=True, backgrounds=bg.to(DEV), wide_channels=wide)
        grads = torch.autograd.grad((rc * vc.to(DEV)).sum() + (ra * va.to(DEV)).sum(), ins)
        out = {"colors": rc, "alphas": ra, "absgrad": meta["means2d"].absgrad,
               **dict(zip(("means", "quats", "scales", "opacities", "features"), grads))}
        return {k: v.detach().cpu().numpy() for k, v in out.items()}, meta

    (got, meta), (ref, _) = run(True), run(False)
    check_forward(got, ref, f"packed={packed}")
    tols = {"means": 5e-3, "quats": 5e-3, "scales": 5e-3, "opacities": 2e-3, "features": 1e-3}
    for k, tol in tols.items():
        close_most(got[k], ref[k], tol, tol, f"packed={packed} {k}", rows=True)

    # the rasterizer's inputs and cotangents behind the front end: colours =
    # (features, depth), the last output divided by the alphas (ED)
    from oracle import gsplat_oracle as O
    m = {k: meta[k].detach().cpu().numpy() for k in ("means2d", "conics", "opacities", "depths",
                                                     "isect_offsets", "flatten_ids")}
    f = feats.numpy()[meta["gaussian_ids"].cpu().numpy()] if packed else np.broadcast_to(
        feats.numpy(), (C, N, 47))
    cols = np.concatenate([f, m["depths"][..., None]], -1)
    bgs = np.concatenate([bg.numpy(), np.zeros((C, 1), np.float32)], -1)
    a, v = got["alphas"].astype(F64), vc.numpy().astype(F64)
    v_cols = np.concatenate([v[..., :-1], v[..., -1:] / a.clip(1e-10)], -1)
    v_alph = va.numpy() - np.where(a > 1e-10, v[..., -1:] * got["colors"][..., -1:] / a.clip(1e-10),
                                   0.0)
    with O.precision(F64):
        geo = (m["means2d"], m["conics"], cols, m["opacities"], bgs, W, H, 16, m["isect_offsets"],
               m["flatten_ids"])
        last = O.raster_fwd(*geo)[2]
        v_abs = O.raster_bwd(*geo, a, last, v_cols, v_alph, absgrad=True)[5]
    close_most(got["absgrad"], v_abs.reshape(got["absgrad"].shape), 5e-3, 5e-3,
               f"packed={packed} absgrad", rows=True)


def test_wide_refuses_other_tile_sizes():
    case = build_case("sparse", 8, 40, backend="hip")
    with pytest.raises(NotImplementedError, match="tile_size=8"):
        _render(case)
