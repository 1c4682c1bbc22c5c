"""CPU: the scenes of the rasterizer's GPU matrix (tests/raster_cases.py) do
what they are for, and the float32 oracle agrees with the float64 oracle on
every one of them with ZERO elements / rows outside the GPU tolerances.

The second point is what makes the GPU matrix sharp: close_most allows a
kernel max(2, 1e-4 n) threshold flips against the float64 truth.  If the
reference algorithm in float32 already used that allowance up, a wrong kernel
could hide behind it; here it uses none of it."""

import numpy as np
import pytest

import raster_cases as RC
from raster_cases import FWD_BARS, GRAD_BARS, build_case, n_outside, oracle_backward, oracle_forward

F32, F64 = np.float32, np.float64


def _outliers_forward(case, tiles=None):
    f32 = oracle_forward(case, F32, tiles=tiles)
    f64 = oracle_forward(case, F64, tiles=tiles)
    out = {k: n_outside(f32[k], f64[k], *FWD_BARS[k]) for k in FWD_BARS}
    return out, f32, f64


def _outliers_backward(case, fwd32, variant, tiles=None):
    """Both precisions from the same forward alphas / last ids (the float32
    ones, which stand in for a kernel's), as the GPU tests feed the oracle."""
    g = {p: oracle_backward(case, p, fwd32["alphas"], fwd32["last_ids"], tiles=tiles,
                            **RC.VARIANTS[variant]) for p in (F32, F64)}
    out = {}
    for k, (tol, rows) in GRAD_BARS.items():
        if g[F64][k] is not None:
            assert np.isfinite(g[F32][k]).all() and np.isfinite(g[F64][k]).all(), k
            out[k] = n_outside(g[F32][k], g[F64][k], tol, tol, rows=rows)
    return out


def _assert_none(out, what):
    assert not any(out.values()), (what, out)


# --------------------------------------------- a, b: the instantiation matrix
@pytest.mark.parametrize("ts,D", RC.MATRIX)
def test_sparse_fp32_oracle_has_no_outliers(ts, D):
    case = build_case("sparse", ts, D)
    # every tile size leaves partial tiles: in x always, in y except 52 = 13 * 4
    assert case.W % ts and (case.H % ts or ts == 4)
    assert 3000 < case.flatten_ids.size < 40000
    out, f32, _ = _outliers_forward(case)
    _assert_none(out, "forward")
    assert f32["alphas"].max() < 1 - 1e-4 * 1.5, "a pixel is near termination"
    for variant in RC.VARIANTS:
        _assert_none(_outliers_backward(case, f32, variant), variant)


def test_sparse_tiles_stay_short():
    """The sparse scene keeps every tile in one backward chunk (256) at the
    16x16 tile size, so the matrix runs the plain paths."""
    for D in RC.SUPPORTED_D:
        assert build_case("sparse", 16, D).n_per_tile.max() < 512


# --------------------------------------------------------- c: long tiles
@pytest.mark.parametrize("D", RC.LONG_D)
def test_dense_scene_is_long_and_terminates(D):
    case = build_case("dense", 16, D)
    assert case.n_per_tile.max() > 2048, case.n_per_tile.max()
    out, f32, f64 = _outliers_forward(case)
    _assert_none(out, "forward")
    # terminated: the forward stopped before the tile's last isect would have
    # pushed T to <= 1e-4
    assert (f64["alphas"] >= 1 - 2e-4).mean() > 0.2, (f64["alphas"] >= 1 - 2e-4).mean()
    assert np.array_equal(f32["last_ids"], f64["last_ids"])
    # the GPU bars of this scene are relative to the float32 oracle's own
    # outliers and error: pin the former at zero
    _assert_none(_outliers_backward(case, f32, "bg_abs"), "backward")


# --------------------------------------------------------------- d: masks
@pytest.mark.parametrize("kind,ts,D,seed", RC.MASK_CASES)
def test_masked_fp32_oracle_has_no_outliers(kind, ts, D, seed):
    case = build_case(kind, ts, D, seed=seed)
    if kind == "dense":
        assert case.n_per_tile.max() > 2048, case.n_per_tile.max()
    mask = RC.tile_mask(case)
    frac = mask.mean()
    assert 0.1 < frac <= 0.67 and mask.reshape(-1)[np.argmax(case.n_per_tile)]
    assert mask.reshape(-1)[0]
    only = RC.only_masked_gaussians(case, mask)
    assert only.sum() >= 1, "no Gaussian lies in masked tiles only"
    tiles = np.flatnonzero(~mask.reshape(-1))
    out, f32, f64 = _outliers_forward(case, tiles)
    _assert_none(out, "forward")
    # masked tiles: alpha 0, colour = background
    ts_ = case.ts
    for t in np.flatnonzero(mask.reshape(-1)):
        c, rem = divmod(int(t), case.th * case.tw)
        ty, tx = divmod(rem, case.tw)
        blk = (c, slice(ty * ts_, (ty + 1) * ts_), slice(tx * ts_, (tx + 1) * ts_))
        assert not f64["alphas"][blk].any()
        assert np.array_equal(f64["colors"][blk],
                              np.broadcast_to(case.backgrounds[c].astype(F64),
                                              f64["colors"][blk].shape))
    # the Gaussian of isect 0: in masked tiles only wherever the mask could take
    # all its tiles, and -- in the cases listed -- it would get a gradient from
    # tile 0 if the backward did not skip the tile (elsewhere it stays under
    # 1/255 there)
    g0 = int(case.flatten_ids[0])
    if kind == "sparse" or seed is not None:
        assert only[g0]
    if (kind, ts, D, seed) in RC.MASK_FIRST_CONTRIBUTES:
        full = oracle_forward(case, F64)
        g = oracle_backward(case, F64, full["alphas"], full["last_ids"], tiles=[0])
        assert g["v_colors"].reshape(case.C * case.N, -1)[g0].any()
    g = oracle_backward(case, F64, f64["alphas"], f64["last_ids"], tiles=tiles)
    for k in ("v_means2d", "v_conics", "v_colors", "v_means2d_abs"):
        assert not g[k].reshape(case.C * case.N, -1)[only].any(), k
    # (the dense cases' GPU bar is relative to the float32 oracle: zero here)
    _assert_none(_outliers_backward(case, f32, "bg_abs", tiles), "backward")


def test_mask_cases_cover_the_backward_mask_in_every_kernel():
    """A Gaussian that shows a backward ignoring the mask exists for the
    record (16, 3) and gather (16, 16) 16x16 backward, the chunked backward
    under the split forward (dense) and the generic kernel (12, 8 and 8, 3)."""
    assert set(RC.MASK_FIRST_CONTRIBUTES) <= set(RC.MASK_CASES)
    assert {(k, t, d) for k, t, d, _ in RC.MASK_FIRST_CONTRIBUTES} == \
        {(k, t, d) for k, t, d, _ in RC.MASK_CASES}


# ---------------------------------------------------------- e: edge scene
def test_edge_scene_geometry():
    g = RC.edge_geometry()
    ex = g.exact[0]
    assert ex.sum() == RC.EDGE_N_EXACT and (~ex).sum() == RC.EDGE_N_NEEDLES
    m = g.means2d[0][ex]
    assert np.array_equal(m - np.floor(m), np.full_like(m, 0.5))
    a, b, c = (g.conics[0][:, i].astype(F64) for i in range(3))
    det = a * c - b * b
    assert (det[ex] < 0).sum() == 3 * RC.EDGE_N_EXACT // 5       # the indefinite conics
    assert (det[~ex] > 0).all()
    # needles: minor sigma 0.35-0.8 px, major 6-25 px
    tr = a[~ex] + c[~ex]
    l_hi = 0.5 * (tr + np.sqrt(tr * tr - 4 * det[~ex]))
    l_lo = det[~ex] / l_hi
    assert (1 / np.sqrt(l_hi) < 0.81).all() and (1 / np.sqrt(l_lo) > 5.9).all()
    ops = set(np.unique(g.opacities[0][ex]).tolist())
    assert ops == {float(np.float32(x)) for x in RC.EDGE_OPACITIES}
    assert np.float32(0.004) > np.float32(1 / 255) > np.float32(0.0039)
    d = g.depths[0]
    assert np.unique(d).size <= d.size - d.size // 5 + 1          # ties
    outside = (g.means2d[0][~ex] < 0).any(-1) | (g.means2d[0][~ex, 0] > 40) \
        | (g.means2d[0][~ex, 1] > 36)
    assert outside.sum() >= 10


@pytest.mark.parametrize("ts,D", RC.EDGE_CASES)
def test_edge_fp32_oracle_has_no_outliers(ts, D):
    case = build_case("edge", ts, D)
    out, f32, f64 = _outliers_forward(case)
    _assert_none(out, "forward")
    # no threshold decision of this scene hangs on rounding
    assert np.array_equal(f32["last_ids"], f64["last_ids"])
    assert (f64["alphas"] >= 0.99).sum() >= 10, (f64["alphas"] >= 0.99).sum()
    g = {p: oracle_backward(case, p, f32["alphas"], f32["last_ids"]) for p in (F32, F64)}
    for p in g:
        for k, v in g[p].items():
            assert np.isfinite(v).all(), (p, k)  # (NaN in v_opacities before the oracle's fix)
    _assert_none({k: n_outside(g[F32][k], g[F64][k], tol, tol, rows=rows)
                  for k, (tol, rows) in GRAD_BARS.items()}, "backward")
    # zero-opacity Gaussians, and those below 1/255: all-zero gradient rows
    dead = case.opacities.reshape(-1) < 1 / 255
    assert dead.sum() >= RC.EDGE_N_EXACT // 3
    has_isect = np.bincount(case.flatten_ids, minlength=case.N) > 0
    assert (dead & has_isect).sum() >= 5
    for k in ("v_means2d", "v_conics", "v_colors", "v_opacities", "v_means2d_abs"):
        assert not g[F64][k].reshape(case.N, -1)[dead].any(), k
