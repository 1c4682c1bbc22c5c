"""Scenes, oracle runs and comparisons for the rasterizer's test matrix
(tests/test_raster_cases_host.py on the CPU, tests/test_gpu_raster_matrix.py
on the GPU).  A helper, not a conftest: no tests, and nothing of the HIP
package is imported at module level.

Three scenes, each built to drive particular kernel paths:

  sparse  a projected random cloud on a 70x52 image (partial tiles at every
          tile size, 16 / 12 / 8 / 4): a few hundred isects per tile at
          most, no pixel terminates.  The instantiation matrix.
  dense   6000 large Gaussians on 40x36: thousands of isects in one tile
          (several backward chunks and more than two split-forward chunks),
          a large share of the pixels terminating at T <= 1e-4.
  edge    hand-built in 2-D: alpha clamped at 0.999, indefinite conics,
          opacities just above / below 1/255 and exactly 0, needle-shaped
          Gaussians centred outside the tiles they touch, tied depths.

`backend="oracle"` projects and intersects with the numpy oracle (CPU);
`backend="hip"` with gsplat_hip, as the existing GPU tests do.
"""

import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

SUPPORTED_D = (1, 2, 3, 4, 8, 16, 32)
TILE_SIZES = (16, 12, 8, 4)

# The project's bars for the rasterizer against a truth (test_gpu_parity.py,
# after the reference's test_ras2pix.py:132-161): name -> (tol, by rows).
FWD_BARS = {"colors": (1e-5, 2e-5), "alphas": (1e-5, 2e-5)}  # (rtol, atol)
GRAD_BARS = {"v_means2d": (5e-3, True), "v_conics": (1e-3, True), "v_colors": (1e-3, True),
             "v_opacities": (2e-3, False), "v_means2d_abs": (5e-3, True),
             "v_backgrounds": (5e-3, False)}


# ------------------------------------------------------------- comparisons
def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def close_most(a, b, rtol, atol, what="", max_frac=1e-4, min_count=2, rows=False,
               out_bound=None):
    """allclose up to a handful of threshold flips: a Gaussian whose alpha is
    within float rounding of 1/255 (or a pixel whose T is within rounding of
    1e-4) can land on the other side of the cut in two correct fp32
    implementations (different FMA contraction / exp).  At most
    max(min_count, max_frac * n) elements -- or, with rows=True, rows of the
    last axis (all gradient components of one Gaussian) -- may exceed the
    tolerance, and each of those by at most `out_bound` in absolute value.

    Default bound: a flip adds or drops one Gaussian of alpha ~1/255 at one
    pixel, which moves that pixel's colour / alpha by <= 1/255 * |c| and every
    later contribution by a factor (1 - 1/255): <= 2/255 of the largest value,
    taken as 0.01 * max|b| (+ atol).  Gradient call sites pass their own."""
    a, b = _np(a), _np(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad_el = ~np.isclose(a, b, rtol=rtol, atol=atol)
    bad = bad_el
    if rows and bad.ndim > 1:
        bad = bad.reshape(-1, bad.shape[-1]).any(-1)
    allowed = max(min_count, int(max_frac * bad.size))
    diff = np.abs(a.astype(np.float64) - b)
    assert bad.sum() <= allowed, (
        f"{what}: {bad.sum()} of {bad.size} {'rows' if rows else 'elements'} outside "
        f"rtol={rtol} atol={atol} (allowed {allowed}); max abs diff {diff.max()}")
    if out_bound is None:
        out_bound = 0.01 * float(np.abs(b).max(initial=0.0)) + atol
    if bad_el.any():
        worst = float(diff[bad_el].max())
        assert worst <= out_bound, (
            f"{what}: an outlier is off by {worst}, beyond the one-flip bound {out_bound}")


def n_outside(a, b, rtol, atol, rows=False):
    """Elements (rows of the last axis with rows=True) that close_most counts
    as outside the tolerance; NaN on either side counts."""
    a, b = _np(a), _np(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    bad = ~np.isclose(a, b, rtol=rtol, atol=atol)
    if rows and bad.ndim > 1:
        bad = bad.reshape(-1, bad.shape[-1]).any(-1)
    return int(bad.sum())


def max_err(a, b):
    a, b = _np(a).astype(np.float64), _np(b).astype(np.float64)
    return float(np.abs(a - b).max(initial=0.0))


def check_forward(got, ref, what="", errors=None):
    """Colours and alphas at the project's bars (rtol 1e-5, atol 2e-5)."""
    for k, (rtol, atol) in FWD_BARS.items():
        if errors is not None:
            errors[k] = max(errors.get(k, 0.0), max_err(got[k], ref[k]))
        close_most(got[k], ref[k], rtol, atol, f"{what} {k}")


def check_grads(got, ref, what="", errors=None):
    """Every gradient present in `got` at the project's bars."""
    for k, (tol, rows) in GRAD_BARS.items():
        if got.get(k) is None:
            continue
        assert ref.get(k) is not None, (what, k)
        if errors is not None:
            errors[k] = max(errors.get(k, 0.0), max_err(got[k], ref[k]))
        close_most(got[k], ref[k], tol, tol, f"{what} {k}", rows=rows)


def check_grads_relative(got, exact, ref32, what="", errors=None, ref64=None):
    """test_raster_chunked_backward's bar for long tiles, where a few rows are
    ill-conditioned in float32 (ra = 1 / (1 - alpha) reaches 1000 and
    T gD - rD cancels): no worse than the float32 oracle is against float64.
    At most max(2, 3x) its out-of-tolerance rows, max error within 2x its max
    error + tol.  The yardstick is the float32 oracle's error against the
    float64 oracle run from the same forward (`ref64`; `exact` if None); the
    kernel's error is taken against `exact`."""
    for k, (tol, _) in GRAD_BARS.items():
        if got.get(k) is None:
            continue
        truth = np.asarray(exact[k], np.float64)
        base = truth if ref64 is None else np.asarray(ref64[k], np.float64)
        e_ours = np.abs(_np(got[k]).astype(np.float64) - truth)
        e_ref = np.abs(np.asarray(ref32[k], np.float64) - base)

        def bad_rows(e, t):
            bad = ~(e <= tol + tol * np.abs(t))  # NaN counts as bad
            return bad.reshape(-1, bad.shape[-1]).any(-1) if bad.ndim > 1 else bad

        n_ours, n_ref = int(bad_rows(e_ours, truth).sum()), int(bad_rows(e_ref, base).sum())
        if errors is not None:
            errors[k] = max(errors.get(k, 0.0), float(e_ours.max(initial=0.0)))
            errors[k + "_fp32_oracle"] = max(errors.get(k + "_fp32_oracle", 0.0),
                                             float(e_ref.max(initial=0.0)))
        assert n_ours <= max(2, 3 * n_ref), (what, k, n_ours, n_ref)
        assert e_ours.max(initial=0.0) <= 2 * e_ref.max(initial=0.0) + tol, (
            what, k, e_ours.max(), e_ref.max())


# ------------------------------------------------------------------ scenes
def _garden_scene(n, C, W, H, seed=0, scale=0.02):
    """test_garden.npz is not part of the repository: a synthetic scene of the
    same statistics (means in [-2,2]^3 in front of C cameras)."""
    g = torch.Generator().manual_seed(seed)
    means = (torch.rand(n, 3, generator=g) * 4 - 2)
    quats = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1)
    scales = torch.rand(n, 3, generator=g) * scale
    opac = torch.rand(n, generator=g)
    vm = torch.eye(4)[None].repeat(C, 1, 1)
    for c in range(C):
        a = 0.4 * c
        vm[c, :3, :3] = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0],
                                      [-math.sin(a), 0, math.cos(a)]])
        vm[c, 2, 3] = 5.0
    K = torch.tensor([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]])[None].repeat(C, 1, 1)
    return means, quats, scales, opac, vm, K


EDGE_CONICS = ((0.25, 0.0, 0.25), (0.25, 0.5, 0.25), (0.125, -0.5, 0.125),
               (0.5, 0.25, 0.03125), (0.0625, 0.0, 1.0))  # the 2nd, 3rd and 4th are indefinite
EDGE_OPACITIES = (1.0, 0.9, 0.5, 0.004, 0.0039, 0.0)  # 1/255 = 0.0039216 lies between
EDGE_N_EXACT = 60
EDGE_N_NEEDLES = 60


def edge_geometry(W=40, H=36, seed=10):
    """The edge scene in 2-D: means2d, conics, opacities [1,120(,k)] float32,
    radii int32, depths.

    Exact group (60): means on pixel centres (integer + 0.5, from -3 to W + 3),
    dyadic conics and integer pixel offsets, so sigma is exact in float32 and
    no threshold decision hangs on rounding: opacity 1.0 on a pixel centre
    clamps alpha at 0.999 (zero alpha gradient), 0.004 * exp(-sigma) stays
    above 1/255 only where sigma <= 0.0198, 0.0039 and 0.0 never contribute,
    and the three indefinite conics give sigma < 0 (down to about -300, where
    float32 exp(-sigma) overflows) on part of every tile.
    Needles (60): major sigma 6-25 px, minor 0.35-0.8 px, any angle, centred
    up to 20 px outside the image: the Gaussians that a culling test against
    the tile rectangle can wrongly drop.
    Every fifth depth is tied with the one before it.

    The needles' sigma cancels in float32 (terms of a few thousand): the seed
    is one at which the float32 oracle still has no element outside the GPU
    tolerances of the float64 one (tests/test_raster_cases_host.py pins it)."""
    rng = np.random.default_rng(seed)
    n0, n1 = EDGE_N_EXACT, EDGE_N_NEEDLES
    m2 = np.zeros((n0 + n1, 2), np.float64)
    cn = np.zeros((n0 + n1, 3), np.float64)
    op = np.zeros(n0 + n1, np.float64)
    radii = np.zeros(n0 + n1, np.int32)
    m2[:n0, 0] = rng.integers(-3, W + 3, n0) + 0.5
    m2[:n0, 1] = rng.integers(-3, H + 3, n0) + 0.5
    # the first few on pixels inside the image: alpha = 1.0 clamps there
    m2[:n0, 0] = np.where(np.arange(n0) % 6 == 0, np.clip(m2[:n0, 0], 0.5, W - 0.5), m2[:n0, 0])
    m2[:n0, 1] = np.where(np.arange(n0) % 6 == 0, np.clip(m2[:n0, 1], 0.5, H - 0.5), m2[:n0, 1])
    for i in range(n0):
        cn[i] = EDGE_CONICS[i % len(EDGE_CONICS)]
        op[i] = EDGE_OPACITIES[i % len(EDGE_OPACITIES)]
    radii[:n0] = rng.integers(3, 14, n0)
    s_major = rng.uniform(6.0, 25.0, n1)
    s_minor = rng.uniform(0.35, 0.8, n1)
    th = rng.uniform(0.0, np.pi, n1)
    c, s = np.cos(th), np.sin(th)
    ia, ib = 1.0 / s_major ** 2, 1.0 / s_minor ** 2  # inverse covariance R diag(ia, ib) R^T
    cn[n0:, 0] = c * c * ia + s * s * ib
    cn[n0:, 1] = c * s * (ia - ib)
    cn[n0:, 2] = s * s * ia + c * c * ib
    m2[n0:, 0] = rng.uniform(-20.0, W + 20.0, n1)
    m2[n0:, 1] = rng.uniform(-20.0, H + 20.0, n1)
    op[n0:] = rng.uniform(0.05, 1.0, n1)
    radii[n0:] = np.ceil(3.0 * s_major).astype(np.int32)
    depths = rng.uniform(1.0, 10.0, n0 + n1)
    depths[5::5] = depths[4:-1:5]
    order = rng.permutation(n0 + n1)  # interleave the groups in index order too
    f = lambda x: np.ascontiguousarray(x[order][None]).astype(np.float32)
    return SimpleNamespace(means2d=f(m2), conics=f(cn), opacities=f(op),
                           radii=np.ascontiguousarray(radii[order][None]), depths=f(depths),
                           exact=np.ascontiguousarray((order < n0)[None]))


@functools.lru_cache(maxsize=None)
def _geometry(kind, seed, backend):
    """(W, H, C, means2d, conics, opacities, radii, depths) of a scene, numpy."""
    if kind == "edge":
        g = edge_geometry()
        return 40, 36, 1, g.means2d, g.conics, g.opacities, g.radii, g.depths
    if kind == "sparse":
        N, C, W, H, scale = 1500, 2, 70, 52, 0.05
    elif kind == "dense":
        N, C, W, H, scale = 6000, 1, 40, 36, 0.15
    else:
        raise ValueError(kind)
    means, quats, scales, opac, vm, K = _garden_scene(N, C, W, H, seed=seed, scale=scale)
    if backend == "hip":
        import gsplat_hip
        dev = "cuda"
        radii, m2, d, cn, _ = gsplat_hip.fully_fused_projection(
            means.to(dev), None, quats.to(dev), scales.to(dev), vm.to(dev), K.to(dev), W, H)
        radii, m2, d, cn = (x.cpu().numpy() for x in (radii, m2, d, cn))
    else:
        from oracle import gsplat_oracle as O
        radii, m2, d, cn, _ = O.proj_fwd(means.numpy(), quats.numpy(), scales.numpy(),
                                         vm.numpy(), K.numpy(), W, H)
    ops = np.ascontiguousarray(opac.numpy()[None].repeat(C, 0))
    return W, H, C, m2, cn, ops, radii, d


@functools.lru_cache(maxsize=None)
def build_case(kind, ts, D, backend="oracle", seed=None):
    """One case of the matrix: scene `kind` intersected with tiles of `ts`
    pixels, D colour channels.  Everything numpy float32 / int32; treat as
    read-only (cached).  `seed`: of the scene's geometry (default: D for the
    sparse scene, 0 for the dense one; the edge scene has its own)."""
    if seed is None:
        seed = D if kind == "sparse" else 0
    W, H, C, m2, cn, ops, radii, depths = _geometry(kind, seed, backend)
    tw, th = math.ceil(W / ts), math.ceil(H / ts)
    if backend == "hip":
        import gsplat_hip
        dev = "cuda"
        T = lambda x: torch.from_numpy(x).to(dev)
        _, ids, fids = gsplat_hip.isect_tiles(T(m2), T(radii), T(depths), ts, tw, th)
        off = gsplat_hip.isect_offset_encode(ids, C, tw, th).cpu().numpy()
        fids = fids.cpu().numpy()
    else:
        from oracle import gsplat_oracle as O
        _, ids, fids = O.isect_tiles(m2, radii, depths, ts, tw, th)
        off = O.isect_offset_encode(ids, C, tw, th)
    N = ops.shape[1]
    g = torch.Generator().manual_seed(1000 + 10 * D + ts)
    cols = torch.rand(C, N, D, generator=g).numpy()
    bg = torch.rand(C, D, generator=g).numpy()
    vrc = torch.randn(C, H, W, D, generator=g).numpy()
    vra = torch.randn(C, H, W, 1, generator=g).numpy()
    n_per_tile = np.diff(np.append(off.reshape(-1).astype(np.int64), len(fids)))
    return SimpleNamespace(kind=kind, ts=ts, D=D, backend=backend, seed=seed, W=W, H=H, C=C, N=N, tw=tw, th=th,
                           means2d=m2, conics=cn, opacities=ops, colors=cols, backgrounds=bg,
                           radii=radii, depths=depths, offsets=off.astype(np.int32),
                           flatten_ids=fids.astype(np.int32), v_colors=vrc, v_alphas=vra,
                           n_per_tile=n_per_tile)


def tile_mask(case, frac=0.3, seed=0):
    """bool[C, th, tw]: about `frac` of the tiles at random, the heaviest
    tile, and tile 0 with (where that leaves the mask under 60 %) every other
    tile of the Gaussian of isect 0.

    Tile 0 matters for the backward: a masked tile's last ids are all 0, which
    already ends the backward's range at isect 1 -- before the start of every
    tile but the first.  Only in tile 0 does skipping the tile depend on the
    backward reading the mask; with the first Gaussian's other tiles masked
    too, its rows must then be exactly zero."""
    rng = np.random.default_rng(seed + 7 * case.ts + case.D)
    n = case.C * case.th * case.tw
    m = rng.random(n) < frac
    m[int(np.argmax(case.n_per_tile))] = True
    m[0] = True
    if m.all():
        m[int(np.argmin(case.n_per_tile[1:])) + 1] = False
    assert case.n_per_tile[0] > 0, "tile 0 is empty"
    tile_of = np.repeat(np.arange(n), case.n_per_tile)
    m0 = m.copy()
    m0[tile_of[case.flatten_ids == case.flatten_ids[0]]] = True
    if m0.mean() <= 0.6:
        m = m0
    return m.reshape(case.C, case.th, case.tw)


def only_masked_gaussians(case, mask):
    """bool[C * N]: Gaussians with isects, all of them in masked tiles."""
    tile_of = np.repeat(np.arange(case.n_per_tile.size), case.n_per_tile)
    masked = mask.reshape(-1)[tile_of]
    G = case.C * case.N
    n_all = np.bincount(case.flatten_ids, minlength=G)
    n_masked = np.bincount(case.flatten_ids[masked], minlength=G)
    return (n_all > 0) & (n_all == n_masked)


# ------------------------------------------------------------------ oracle
_fwd_cache = {}


def oracle_forward(case, prec, use_bg=True, tiles=None):
    """O.raster_fwd of a case in `prec` (np.float32 / np.float64): dict of
    colors, alphas, last_ids.  `tiles`: flat indices of the tiles to render,
    the others stay 0 (background with use_bg).  The compositing runs once per
    (case with its backend, precision, tiles); the background term, (1 - alpha) * bg as the
    oracle adds it, is applied to the cached sums."""
    from oracle import gsplat_oracle as O
    key = (case.kind, case.ts, case.D, case.seed, case.backend, np.dtype(prec).name,
           None if tiles is None else tuple(int(t) for t in tiles))
    if key not in _fwd_cache:
        with O.precision(prec):
            _fwd_cache[key] = O.raster_fwd(
                case.means2d, case.conics, case.colors, case.opacities, None, case.W, case.H,
                case.ts, case.offsets, case.flatten_ids, tiles=tiles)
    acc, alphas, last = _fwd_cache[key]
    colors = acc
    if use_bg:
        one = np.dtype(prec).type(1.0)
        colors = acc + (one - alphas) * case.backgrounds.astype(prec)[:, None, None, :]
    return {"colors": colors, "alphas": alphas, "last_ids": last}


def oracle_backward(case, prec, alphas, last_ids, use_bg=True, use_v_alphas=True, absgrad=True,
                    tiles=None):
    """O.raster_bwd of a case in `prec`, from the given forward alphas and
    last ids (the kernel's own, as the existing tests do, or the oracle's).
    Without `use_v_alphas` the alpha cotangent is zero (null in the ABI)."""
    from oracle import gsplat_oracle as O
    vra = case.v_alphas if use_v_alphas else np.zeros_like(case.v_alphas)
    with O.precision(prec):
        out = O.raster_bwd(case.means2d, case.conics, case.colors, case.opacities,
                           case.backgrounds if use_bg else None, case.W, case.H, case.ts,
                           case.offsets, case.flatten_ids, _np(alphas).astype(prec),
                           _np(last_ids), case.v_colors, vra, absgrad=absgrad, tiles=tiles)
    return dict(zip(("v_means2d", "v_conics", "v_colors", "v_opacities", "v_backgrounds",
                     "v_means2d_abs"), out))


# --------------------------------------------------------- the GPU matrix
VARIANTS = {  # a: (backgrounds given and requiring grad, absgrad, loss on alphas too)
    "bg_abs": dict(use_bg=True, absgrad=True, use_v_alphas=True),
    "nobg": dict(use_bg=False, absgrad=False, use_v_alphas=False),
}
MATRIX = [(ts, D) for ts in TILE_SIZES for D in SUPPORTED_D]   # a, sparse
GATHER_D = (1, 3, 8)                                          # b, sparse, ts 16
LONG_D = (1, 8, 16, 32)                                       # c, dense, ts 16
LONG_MODES = {"chunk256": (256, 0), "chunk64": (64, 0), "split512": (256, 512)}  # chunk, split
# d: (kind, ts, D, scene seed).  The first five are the issue's; in the last
# three -- other seeds of the same scenes -- the Gaussian of isect 0 reaches
# 1/255 in tile 0, as it does at (16, 3) and (12, 8): the only Gaussian through
# which a backward that ignored the mask would show (see tile_mask), here for
# the gather-path backward, the 8-pixel tiles and the chunked backward too.
MASK_CASES = [("sparse", 16, 3, None), ("sparse", 16, 16, None), ("sparse", 8, 3, None),
              ("sparse", 12, 8, None), ("dense", 16, 8, None),
              ("sparse", 16, 16, 100), ("sparse", 8, 3, 100), ("dense", 16, 8, 100)]
MASK_FIRST_CONTRIBUTES = [("sparse", 16, 3, None), ("sparse", 12, 8, None), ("sparse", 16, 16, 100),
                          ("sparse", 8, 3, 100), ("dense", 16, 8, 100)]
LONG_KERNEL_ALPHA_D = (1, 8)  # c: where the truth from the kernel's own alphas is held too
EDGE_CASES = [(16, 3), (16, 16), (8, 2), (12, 4)]             # e
