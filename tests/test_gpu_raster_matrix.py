"""GPU: every instantiation of the rasterizer against the float64 oracle.

The rasterizer is compiled in two families -- wave-per-tile kernels for 16x16
tiles (csrc/rasterize16.hip, planned by rasterize16_plan.hip) and
workgroup-per-tile kernels for the other tile sizes (csrc/rasterize.hip) -- each for D in {1, 2, 3, 4, 8, 16, 32}, the
backward with and without absgrad; the 16x16 family also has a record and an
array-gather path, a split forward and a chunked backward.  Scenes, oracle
runs and bars: tests/raster_cases.py; tests/test_raster_cases_host.py shows
on the CPU that the float32 oracle has nothing outside these bars on any
case, so close_most's allowance for threshold flips is the kernel's alone.

  a  instantiation matrix: sparse scene, D x tile size, two variants
     (backgrounds + absgrad + alpha loss / none of them: null pointers)
  b  array-gather path of the 16x16 kernels for D <= 10 (records off)
  c  long tiles: chunked backward (256, 64) and split forward, D = 1 .. 32
  d  tile masks, forward and backward, also under the split forward
  e  value edges: clamped alpha, indefinite conics, opacities around 1/255
     and 0, needles centred outside their tiles, tied depths

The largest error of every output per group is printed as one JSON line when
the module finishes (pytest -s shows it).
"""

import json

import numpy as np
import pytest
import torch

import raster_cases as RC
from raster_cases import (build_case, check_forward, check_grads, check_grads_relative,
                          oracle_backward, oracle_forward)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = np.float32, np.float64
ERRORS = {}  # group -> output -> largest |kernel - float64 oracle| seen


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401  (fails loudly if the .so is missing)
    yield
    print("\nraster_matrix_errors " + json.dumps(ERRORS, sort_keys=True))


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _case(kind, ts, D):
    return build_case(kind, ts, D, backend="hip")


def _render(case, **kw):
    """_render_case; a HIP error (a fault on the card) ends the session: no
    further kernel is launched on a card that has faulted."""
    try:
        return _render_case(case, **kw)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"GPU fault, stopping: {e}", returncode=3)
        raise


def _render_case(case, use_bg=True, absgrad=True, use_v_alphas=True, masks=None, backward=True):
    """rasterize_to_pixels forward and backward of a case: dict of numpy
    outputs named as the oracle's."""
    import gsplat_hip
    ins = [T(x).requires_grad_(True)
           for x in (case.means2d, case.conics, case.colors, case.opacities)]
    bg = T(case.backgrounds).requires_grad_(True) if use_bg else None
    rc, ra = gsplat_hip.rasterize_to_pixels(
        *ins, case.W, case.H, case.ts, T(case.offsets), T(case.flatten_ids), backgrounds=bg,
        masks=None if masks is None else T(masks), absgrad=absgrad)
    out = {"colors": rc.detach().cpu().numpy(), "alphas": ra.detach().cpu().numpy(),
           # saved by the forward (autograd node of its output), see test_gpu_parity._last_ids
           "last_ids": rc.grad_fn.saved_tensors[9].cpu().numpy()}
    if not backward:
        return out
    loss = (rc * T(case.v_colors)).sum()
    if use_v_alphas:
        loss = loss + (ra * T(case.v_alphas)).sum()
    grads = torch.autograd.grad(loss, ins + ([bg] if use_bg else []))
    torch.cuda.synchronize()
    for k, g in zip(("v_means2d", "v_conics", "v_colors", "v_opacities", "v_backgrounds"), grads):
        out[k] = g.cpu().numpy()
    if absgrad:
        out["v_means2d_abs"] = ins[0].absgrad.cpu().numpy()
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    return out


def _check_vs_float64(case, got, variant, group, what, tiles=None, own_forward=True):
    """Forward and gradients against the float64 oracle at the project's
    bars.  The oracle's backward starts from the kernel's own alphas and last
    ids (own_forward), as the existing tests do, or from the oracle's."""
    v = RC.VARIANTS[variant]
    err = ERRORS.setdefault(group, {})
    ref = oracle_forward(case, F64, use_bg=v["use_bg"], tiles=tiles)
    check_forward(got, ref, what, err)
    src = got if own_forward else ref
    check_grads(got, oracle_backward(case, F64, src["alphas"], src["last_ids"], tiles=tiles, **v),
                what, err)
    return ref


# ------------------------------------------------ a: instantiation matrix
@pytest.mark.parametrize("variant", list(RC.VARIANTS))
@pytest.mark.parametrize("ts,D", RC.MATRIX)
def test_matrix_vs_float64_oracle(ts, D, variant):
    """Every (tile size, D) instantiation of the forward and of the backward
    (ABS on with "bg_abs", off with "nobg", where backgrounds and
    v_render_alphas reach the ABI as null) on the sparse scene: partial tiles
    on the right and bottom edges, and at 12 / 4 pixel tiles idle lanes in the
    workgroup (144 pixels in 192 threads, 16 in 64)."""
    case = _case("sparse", ts, D)
    got = _render(case, **RC.VARIANTS[variant])
    _check_vs_float64(case, got, variant, "a", f"ts={ts} D={D} {variant}")


# ------------------------------------------------------- b: gather path
@pytest.mark.parametrize("D", RC.GATHER_D)
def test_gather_path_vs_float64_oracle(D, monkeypatch):
    """The 16x16 kernels gathering the four attribute arrays for D <= 10 (what
    a record table over 2 GiB falls back to): the float64 oracle's bars, and
    the forward of the record path bit for bit (the same floats reach the
    same arithmetic)."""
    from gsplat_hip import _wrapper
    case = _case("sparse", 16, D)
    assert _wrapper.RECORDS, "the record path is the default"
    rec = _render(case, backward=False)
    monkeypatch.setattr(_wrapper, "RECORDS", False)
    got = _render(case)
    _check_vs_float64(case, got, "bg_abs", "b", f"gather D={D}")
    for k in ("colors", "alphas", "last_ids"):
        assert np.array_equal(got[k], rec[k]), k


# --------------------------------------------------------- c: long tiles
def _with_chunk(chunk, split, fn):
    """fn() with the backward's chunk length and the split forward's threshold
    (0: off) set, both restored."""
    from gsplat_hip import _lib, _wrapper
    _lib.query("gsplat_hip_debug_set_chunk", chunk)
    try:
        with _wrapper.fwd_split(None, threshold=split):
            return fn()
    finally:
        _lib.query("gsplat_hip_debug_set_chunk", 256)  # the library default


_long_unsplit = {}


@pytest.mark.parametrize("mode", list(RC.LONG_MODES))
@pytest.mark.parametrize("D", RC.LONG_D)
def test_long_tiles_vs_float64_oracle(D, mode):
    """Dense scene (one tile with about 2,900 isects, 40 % of the pixels
    terminating): the chunked backward at 256 and 64 isects per chunk with the
    unsplit forward, and the split forward (tiles over 512 isects, chunks of
    1024) -- state slots of (1 + D) * 256 floats, and for D = 16 / 32 the
    array-gather path.  Forward at the project's bars; gradients at
    test_raster_chunked_backward's bar, relative to the float32 oracle's own
    error against float64 (raster_cases.check_grads_relative).  Alphas: the
    same bits at either chunk length; the split forward's equal to the unsplit
    forward's up to the chunk products' rounding.

    The truth here is the float64 oracle run end to end (its backward from
    its own alphas), not from the kernel's float32 alphas as elsewhere.  On
    terminated pixels T_final = 1 - alpha is about 1e-4 and known from a
    float32 alpha to 6e-4 only, and a float64 backward that starts from it is
    that far from the true gradient: measured on this scene, at D = 32, max
    |v_conics| 10.6, the float64 oracle from the kernel's alphas is 2.4e-3
    off the end-to-end one (D = 3: 4.2e-4, D = 8: 8.2e-4).  The unchunked
    backward rebuilds T from 1 - alpha and lands on the former (3e-6 away,
    2.4e-3 from the true gradient); the chunked backward takes T at the chunk
    boundaries from the forward's state and lands on the true gradient
    (1.2e-4 away, 2.4e-3 from the former -- which the bar against the former,
    2 x 2.3e-5 + 1e-3, would call a failure at D = 16 and 32).  The yardstick
    is unchanged: the float32 oracle's error against the float64 oracle from
    the same (the kernel's) alphas.  Measured max errors against the truth,
    chunk 256, D = 32: v_means2d 1.8e-4, v_conics 1.2e-4, v_colors 2.8e-4,
    v_opacities 4.3e-4; the float32 oracle's: 6.6e-6, 2.3e-5, 1.1e-5, 1.9e-5."""
    chunk, split = RC.LONG_MODES[mode]
    case = _case("dense", 16, D)
    assert case.n_per_tile.max() > max(2048, 4 * chunk), case.n_per_tile.max()
    got = _with_chunk(chunk, split, lambda: _render(case))
    err = ERRORS.setdefault("c", {})
    exact = oracle_forward(case, F64)
    check_forward(got, exact, f"dense D={D} {mode}", err)
    g64 = oracle_backward(case, F64, exact["alphas"], exact["last_ids"])
    g64k = oracle_backward(case, F64, got["alphas"], got["last_ids"])
    g32k = oracle_backward(case, F32, got["alphas"], got["last_ids"])
    check_grads_relative(got, g64, g32k, f"dense D={D} {mode}", err, ref64=g64k)
    if D in RC.LONG_KERNEL_ALPHA_D:
        # the same bar against the float64 oracle from the kernel's own alphas
        # and last ids, where the 1 - alpha rounding above stays inside it
        check_grads_relative(got, g64k, g32k, f"dense D={D} {mode}, kernel alphas",
                             ERRORS.setdefault("c_kernel_alphas", {}))
    if mode == "chunk256":
        _long_unsplit[D] = got
        return
    if D not in _long_unsplit:
        _long_unsplit[D] = _with_chunk(256, 0, lambda: _render(case, backward=False))
    base = _long_unsplit[D]["alphas"]
    if split:  # up to the chunk products' rounding, as test_split_forward_matches_unsplit
        RC.close_most(got["alphas"], base, 1e-5, 1e-5, "split vs unsplit alphas", max_frac=1e-3)
    else:      # the chunk length changes colour sums only, as test_raster_chunked_backward
        assert np.array_equal(got["alphas"], base)


# --------------------------------------------------------------- d: masks
@pytest.mark.parametrize("kind,ts,D,seed", RC.MASK_CASES)
def test_tile_masks_forward_and_backward(kind, ts, D, seed):
    """masks[tile] == True skips the tile in both directions.  Forward:
    masked tiles are background with alpha exactly 0, every other pixel has
    the unmasked render's bits.  Backward: the oracle over the unmasked tiles,
    exactly zero rows for Gaussians that touch masked tiles only.  The dense
    case runs under the split forward with its heaviest tile -- planned as
    split -- masked.  The last three cases are further seeds of the same
    scenes in which the Gaussian of isect 0 contributes in (masked) tile 0,
    the one place where the backward's own reading of the mask decides
    (raster_cases.tile_mask)."""
    case = build_case(kind, ts, D, backend="hip", seed=seed)
    mask = RC.tile_mask(case)
    only = RC.only_masked_gaussians(case, mask)
    assert mask.reshape(-1)[np.argmax(case.n_per_tile)] and only.any()
    tiles = np.flatnonzero(~mask.reshape(-1))
    run = (lambda f: _with_chunk(256, 512, f)) if kind == "dense" else (lambda f: f())
    got = run(lambda: _render(case, masks=mask))
    plain = run(lambda: _render(case, backward=False))
    px_masked = np.zeros((case.C, case.H, case.W), bool)
    for t in np.flatnonzero(mask.reshape(-1)):
        c, rem = divmod(int(t), case.th * case.tw)
        ty, tx = divmod(rem, case.tw)
        px_masked[c, ty * ts:(ty + 1) * ts, tx * ts:(tx + 1) * ts] = True
    assert not got["alphas"][px_masked].any()
    for c in range(case.C):
        assert np.array_equal(got["colors"][c][px_masked[c]],
                              np.broadcast_to(case.backgrounds[c],
                                              (int(px_masked[c].sum()), D)))
    for k in ("colors", "alphas"):
        assert np.array_equal(got[k][~px_masked], plain[k][~px_masked]), k
    err = ERRORS.setdefault("d", {})
    ref = oracle_forward(case, F64, tiles=tiles)
    check_forward(got, ref, f"masked {kind} ts={ts} D={D}", err)
    g64 = oracle_backward(case, F64, ref["alphas"], ref["last_ids"], tiles=tiles)
    if kind == "dense":
        g32 = oracle_backward(case, F32, ref["alphas"], ref["last_ids"], tiles=tiles)
        check_grads_relative(got, g64, g32, f"masked {kind} ts={ts} D={D}", err)
    else:
        check_grads(got, g64, f"masked {kind} ts={ts} D={D}", err)
    for k in ("v_means2d", "v_conics", "v_colors", "v_opacities", "v_means2d_abs"):
        assert not got[k].reshape(case.C * case.N, -1)[only].any(), k


# ----------------------------------------------------------- e: edge scene
@pytest.mark.parametrize("ts,D", RC.EDGE_CASES)
def test_edge_values_vs_float64_oracle(ts, D):
    """Clamped alpha, indefinite conics (sigma down to about -300), opacities
    0.004 / 0.0039 / 0, needles centred outside the tiles they cross, tied
    depths: the project's bars, last ids equal to the oracle's, everything
    finite (asserted in _render), exactly zero rows for the Gaussians that
    never reach 1/255."""
    import gsplat_hip
    case = _case("edge", ts, D)
    host = build_case("edge", ts, D)  # the isects: bit-exact with the oracle's
    assert np.array_equal(case.offsets, host.offsets)
    assert np.array_equal(case.flatten_ids, host.flatten_ids)
    got = _render(case)
    ref = _check_vs_float64(case, got, "bg_abs", "e", f"edge ts={ts} D={D}")
    assert np.array_equal(got["last_ids"], ref["last_ids"])
    dead = case.opacities.reshape(-1) < 1 / 255
    for k in ("v_means2d", "v_conics", "v_colors", "v_opacities", "v_means2d_abs"):
        assert not got[k].reshape(case.N, -1)[dead].any(), k
