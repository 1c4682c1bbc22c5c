"""GPU: every instantiation and entry point of the 2DGS rasterizer
(csrc/surfel.hip, csrc/surfel_cull.h) against the float64 oracle of
tests/surfel_cases.py.

Cases and oracle: surfel_cases.py.  last_ids and median_ids (read from the
autograd node's saved tensors) are compared exactly; every image and gradient
is bounded by max(FACTOR x bar, FLOOR) relative to the largest |oracle value|,
with no outlier allowance; bar is the larger float32 error of two float32
evaluations of the same case and tile size (tests/golden/surfel_matrix.npz);
tests/test_surfel_cases_host.py shows on the CPU that plain float32
arithmetic meets it and decides every pair as float64 does.

  a  the instantiation matrix on `sparse`: forward and backward at tile 16
     over every compiled D (fwd2s_kernel for D <= 4, fwd2_kernel otherwise and
     at D <= 4 with SREC off; bwd2_kernel general and LEAN, with / without
     absgrad, with backgrounds and an alpha loss / with neither); fwd_kernel
     and bwd_kernel at tile 4, 8 and 12; the forward at tile 32; a padded
     channel count
  b  the entry-point options against the oracle: _colors_only, _depths,
     _visible, _n_isects_device, ORDER on / off, two cameras
  c  `dense`: 1204-isect tiles, 82 % of the pixels ending at T <= 1e-4
  d  tile masks, tile 16 and 8, with / without backgrounds
  e  `thin`, `cull`, `edge`, `gate_alpha`, `gate_thalf`: a contributor lost
     to the strip culling, a value edge or a gate decided wrongly at equality
     fails here

The largest error of every output per group, with its bar and bound, is
printed as one JSON line when the module finishes (pytest -s shows it).
"""

import json
import os

import numpy as np
import pytest
import torch

import surfel_cases as SC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERRORS = {}  # group -> output -> the entry with the largest err / bound
BARS = SC.load_bars(os.path.join(GOLDEN, "surfel_matrix.npz"))
ALL_D = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 32, 33)
SOME_D = (1, 3, 4, 9, 17, 33)
GRADS = ("v_means2d", "v_ray_transforms", "v_colors", "v_opacities", "v_normals", "v_densify")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401  (fails loudly if the .so is missing)
    yield
    line = {g: {k: {f: float(f"{r[f]:.3g}") for f in ("err", "bar", "bound")} for k, r in o.items()}
            for g, o in ERRORS.items()}
    print("\nsurfel_matrix_errors " + json.dumps(line, sort_keys=True, separators=(",", ":")))
    for g, o in sorted(ERRORS.items()):
        k = max(o, key=lambda k: o[k]["ratio"])
        print(f"surfel_matrix group {g}: largest err / bound {o[k]['ratio']:.3f} ({k}, {o[k]['case']})")


def T(x, grad=False):
    return torch.from_numpy(np.array(x)).to(DEV).requires_grad_(grad)  # the cases stay read-only


def npy(t):
    return t.detach().cpu().numpy()


def _gpu(fn):
    """fn() and a synchronize; a HIP error (a fault on the card) ends the
    session: no further kernel is launched on a card that has faulted."""
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"GPU fault, stopping: {e}", returncode=3)
        raise


def check(group, name, ts, what, variant, pairs):
    """pairs: {output: (ours, oracle)}; the bar is that of
    "<name>:<ts>:<variant>:<output>".  Prints and records every figure, then
    asserts each against max(FACTOR x bar, FLOOR)."""
    bad = []
    for k, (ours, ref) in pairs.items():
        bar = BARS[f"{name}:{ts}:{variant}:{k}"]
        assert ours.shape == ref.shape, (name, what, k, ours.shape, ref.shape)
        assert np.isfinite(ours).all(), (name, what, k)
        e, b = SC.rel_err(ours, ref), SC.bound(bar)
        print(f"{name} ts {ts} {what}: {k}: err {e:.3e}  bound {b:.3e}  (bar {bar:.3e})")
        rec = ERRORS.setdefault(group, {})
        if k not in rec or e / b > rec[k]["ratio"]:
            rec[k] = {"err": e, "bar": bar, "bound": b, "ratio": e / b, "case": f"{name} ts {ts} {what}"}
        if not e <= b:
            bad.append((k, e, b))
    assert not bad, (name, ts, what, bad)


def _raster(name, ts, D, bg, masks=None, absgrad=False, lean=False, v_alpha=True, backward=True,
            split_depth=False, extra_rows=0, capacity=0, colors_only=False):
    """rasterize_to_pixels_2dgs forward (and backward) of a case: dict of
    numpy outputs named as the oracle's."""
    from gsplat_hip import rasterize_to_pixels_2dgs
    c, geo, ch = SC.build(name), SC.tiles(name, ts), SC.channels(D)

    def rows(a):  # extra_rows surfels appended to camera 0's: no isect refers to them
        a = np.asarray(a)
        if not extra_rows:
            return a
        assert c.C == 1
        return np.concatenate([a, a[:, :extra_rows]], 1)

    ins = {k: T(rows(getattr(c, k)), True) for k in ("m2", "rt", "opac", "nr")}
    cols = rows(c.colors[..., ch])
    kw = {}
    if split_depth:
        ins["colors"], ins["depths"] = T(cols[..., :-1], True), T(cols[..., -1], True)
        kw["_depths"] = ins["depths"]
    else:
        ins["colors"] = T(cols, True)
    bgt = T(c.bg[:, ch], True) if bg else None
    densify = torch.zeros_like(ins["m2"], requires_grad=True)
    fids = geo.fids
    if capacity:  # a capacity-sized flatten_ids, the count on the device
        fids = np.concatenate([fids, np.zeros(capacity - len(fids), np.int32)])
        kw["_n_isects_device"] = T(np.array([len(geo.fids)], np.int64))
    if extra_rows:
        kw["_visible"] = T(np.concatenate([geo.tpg, np.zeros((1, extra_rows), np.int32)], 1))
    outs = rasterize_to_pixels_2dgs(
        ins["m2"], ins["rt"], ins["colors"], ins["opac"], ins["nr"], densify, c.W, c.H, ts,
        T(geo.off), T(fids), backgrounds=bgt, masks=None if masks is None else T(masks),
        absgrad=absgrad, distloss=True, _colors_only=colors_only, **kw)
    saved = outs[1].grad_fn.saved_tensors  # the forward's: ..., last_ids, median_ids, depths
    out = {k: (None if o is None else npy(o)) for k, o in zip(SC.FWD_OUT, outs)}
    out["last_ids"] = npy(saved[12]).astype(np.int64)
    out["median_ids"] = None if saved[13] is None else npy(saved[13]).astype(np.int64)
    if not backward:
        return out
    loss = (outs[0] * T(c.v_colors[..., ch])).sum()
    if v_alpha:
        loss = loss + (outs[1] * T(c.v_alphas)).sum()
    if not lean:
        loss = loss + (outs[2] * T(c.v_normals)).sum() + (outs[3] * T(c.v_distort)).sum() + \
            (outs[4] * T(c.v_median)).sum()
    wrt = [ins["m2"], ins["rt"], ins["colors"], ins["opac"], ins["nr"], densify] + \
        ([bgt] if bg else []) + ([ins["depths"]] if split_depth else [])
    gr = torch.autograd.grad(loss, wrt, allow_unused=True)
    gr = [np.zeros(tuple(t.shape), np.float32) if g is None else npy(g) for g, t in zip(gr, wrt)]
    out.update(dict(zip(GRADS, gr[:6])))
    if bg:
        out["v_backgrounds"] = gr[6]
    if split_depth:
        out["v_colors"] = np.concatenate([out["v_colors"], gr[-1][..., None]], -1)
    if absgrad:
        out["v_means2d_abs"] = npy(ins["m2"].absgrad)
    if extra_rows:  # the rows no isect refers to are not written
        for k in GRADS + (("v_means2d_abs",) if absgrad else ()):
            out[k] = out[k][:, :-extra_rows]
    return out


def _compare(group, name, ts, D, bg, what, masks=None, absgrad=False, lean=False, v_alpha=True,
             backward=True, images=SC.FWD_OUT, **kw):
    got = _gpu(lambda: _raster(name, ts, D, bg, masks, absgrad, lean, v_alpha, backward, **kw))
    ref = SC.fwd64(name, ts, D, bg, masks)
    assert np.array_equal(got["last_ids"], ref["last_ids"]), \
        (name, ts, what, "last_ids", int((got["last_ids"] != ref["last_ids"]).sum()))
    if got["median_ids"] is not None:
        assert np.array_equal(got["median_ids"], ref["median_ids"]), \
            (name, ts, what, "median_ids", int((got["median_ids"] != ref["median_ids"]).sum()))
    check(group, name, ts, what, "fwd", {k: (got[k], ref[k]) for k in images})
    if backward:
        b = SC.bwd64(name, ts, D, bg, masks, lean, v_alpha)
        if bg and D not in ALL_D:
            b = dict(b, v_backgrounds=SC.padded_background_gradient(b["v_backgrounds"]))
        keys = GRADS + (("v_means2d_abs",) if absgrad else ()) + (("v_backgrounds",) if bg else ())
        check(group, name, ts, what, "lean" if lean else "bwd", {k: (got[k], b[k]) for k in keys})
        if lean:
            assert not got["v_normals"].any()
    return got


VARIANTS = ((True, True), (False, False))  # (backgrounds and an alpha loss) / neither: null pointers


# ----------------------------------------------- a: the instantiation matrix
@pytest.mark.parametrize("D", ALL_D)
def test_a_tile16_every_channel_count(monkeypatch, D):
    """fwd2s_kernel (D <= 4) or fwd2_kernel, bwd2_kernel general and LEAN."""
    from gsplat_hip import _lib, _wrapper_2dgs
    assert _wrapper_2dgs.SREC and _wrapper_2dgs.ORDER
    assert (_lib.query("gsplat_hip_rasterize_2dgs_record_floats", D, 16) > 0) == (D <= 4)
    for i, (bg, va) in enumerate(VARIANTS):
        absgrad = i == 0
        _compare("a", "sparse", 16, D, bg, f"D{D} bg{int(bg)} general", absgrad=absgrad, v_alpha=va)
        _compare("a", "sparse", 16, D, bg, f"D{D} bg{int(bg)} general abs{int(not absgrad)}",
                 absgrad=not absgrad, v_alpha=va)
        if D <= 4:  # the LEAN backward: colours and alphas only
            for ab in (False, True):
                _compare("a", "sparse", 16, D, bg, f"D{D} bg{int(bg)} lean abs{int(ab)}", absgrad=ab,
                         lean=True, v_alpha=va, images=("colors", "alphas"))
    if D <= 4:  # the LDS-queue forward where the records would serve
        monkeypatch.setattr(_wrapper_2dgs, "SREC", False)
        _compare("a", "sparse", 16, D, True, f"D{D} queue forward", absgrad=True)


@pytest.mark.parametrize("D", SOME_D)
@pytest.mark.parametrize("ts", (4, 8, 12))
def test_a_one_pixel_per_lane(ts, D):
    """fwd_kernel / bwd_kernel: a quarter-filled wave (4), one wave (8), three
    waves with a partial one (12)."""
    for i, (bg, va) in enumerate(VARIANTS):
        _compare("a", "sparse", ts, D, bg, f"D{D} bg{int(bg)}", absgrad=i == 0, v_alpha=va)
    _compare("a", "sparse", ts, D, True, f"D{D} abs0", absgrad=False)


@pytest.mark.parametrize("D", (1, 3, 4, 9, 16, 17))
def test_a_tile32_forward(D):
    """The 1024-thread forward on partial tiles (the backward refuses tile
    sizes above 16)."""
    for bg in (True, False):
        _compare("a", "sparse", 32, D, bg, f"D{D} bg{int(bg)}", backward=False)


@pytest.mark.parametrize("D", (32, 33))
def test_a_tile32_refuses_what_the_lds_cannot_hold(D):
    """16 waves x 64 records x 52 floats is 208 KiB of queues, a CU has 160:
    refused with the reason (before: `launch failed: invalid argument`)."""
    from gsplat_hip._lib import GsplatHipError
    with pytest.raises(GsplatHipError, match="needs 212992 B of LDS"):
        _raster("sparse", 32, D, True, backward=False)


def test_a_padded_channel_count():
    """10 channels run as 16 with the depth kept last."""
    for bg, va in VARIANTS:
        got = _compare("a", "sparse", 16, 10, bg, f"D10 bg{int(bg)}", absgrad=True, v_alpha=va)
        assert got["colors"].shape[-1] == 10 and got["v_colors"].shape[-1] == 10


# ------------------------------------------------- b: the entry-point options
@pytest.mark.parametrize("D", (3, 4))
def test_b_colors_only(D):
    for bg, va in VARIANTS:
        got = _compare("b", "sparse", 16, D, bg, f"D{D} bg{int(bg)} colors_only", absgrad=bg,
                       lean=True, v_alpha=va, images=("colors", "alphas"), colors_only=True)
        assert got["normals"] is None and got["distort"] is None and got["median"] is None
        assert got["median_ids"] is None


@pytest.mark.parametrize("srec", (True, False))
def test_b_depths_in_place(monkeypatch, srec):
    from gsplat_hip import _wrapper_2dgs
    monkeypatch.setattr(_wrapper_2dgs, "SREC", srec)
    _compare("b", "sparse", 16, 4, False, f"_depths srec{int(srec)}", absgrad=True, split_depth=True)
    _compare("b", "sparse", 16, 4, False, f"_depths srec{int(srec)} lean", lean=True,
             split_depth=True, images=("colors", "alphas"))
    if not srec:
        _compare("b", "sparse", 8, 9, False, "_depths ts8 D9", absgrad=True, split_depth=True)


@pytest.mark.parametrize("D", (4, 9))
def test_b_visible_rows(D):
    """_visible: 20 surfels no isect refers to get no record and no gradient
    row; the others' results are the oracle's."""
    _compare("b", "sparse", 16, D, True, f"D{D} _visible", absgrad=True, extra_rows=20)
    _compare("b", "sparse", 16, D, False, f"D{D} _visible lean", lean=D <= 4, extra_rows=20,
             images=("colors", "alphas") if D <= 4 else SC.FWD_OUT)


@pytest.mark.parametrize("ts,D", [(16, 4), (16, 9), (8, 3)])
def test_b_isect_count_on_the_device(ts, D):
    n = len(SC.tiles("sparse", ts).fids)
    _compare("b", "sparse", ts, D, True, f"D{D} _n_isects_device", absgrad=True, capacity=n + 1000)


@pytest.mark.parametrize("order", (True, False))
def test_b_tile_order_and_two_cameras(monkeypatch, order):
    from gsplat_hip import _wrapper_2dgs
    monkeypatch.setattr(_wrapper_2dgs, "ORDER", order)
    for D in (4, 9):
        _compare("b", "sparse_c2", 16, D, True, f"D{D} order{int(order)}", absgrad=True)
    _compare("b", "sparse_c2", 16, 3, False, f"D3 order{int(order)} lean", lean=True, v_alpha=False,
             images=("colors", "alphas"))


# ------------------------------------------------------------------ c: dense
@pytest.mark.parametrize("D", (1, 4, 9, 33))
def test_c_dense(D):
    """Multi-batch walks, the early-break ballots, the T <= 1e-4 exit."""
    _compare("c", "dense", 16, D, True, f"D{D} general", absgrad=True)
    _compare("c", "dense", 16, D, False, f"D{D} general bg0", v_alpha=False)
    if D <= 4:
        _compare("c", "dense", 16, D, True, f"D{D} lean", absgrad=True, lean=True,
                 images=("colors", "alphas"))


# ------------------------------------------------------------- d: tile masks
@pytest.mark.parametrize("bg", (True, False))
@pytest.mark.parametrize("ts,D", [(16, 4), (16, 9), (8, 4), (8, 17)])
def test_d_tile_masks(ts, D, bg):
    masks = SC.tile_masks("sparse", ts)
    _compare("d", "sparse", ts, D, bg, f"D{D} bg{int(bg)} masks", masks=masks, absgrad=True)
    if ts == 16 and D <= 4:
        _compare("d", "sparse", ts, D, bg, f"D{D} bg{int(bg)} masks lean", masks=masks, lean=True,
                 images=("colors", "alphas"))


# ------------------------------------- e: thin, cull, edge and the alpha gate
@pytest.mark.parametrize("ts,D", [(16, 4), (16, 9), (8, 4)])
@pytest.mark.parametrize("name", ("thin", "cull", "edge", "gate_alpha", "gate_thalf"))
def test_e_culling_and_edges(monkeypatch, name, ts, D):
    from gsplat_hip import _wrapper_2dgs
    _compare("e", name, ts, D, True, f"D{D} general", absgrad=True)
    if ts == 16 and D <= 4:
        _compare("e", name, ts, D, False, f"D{D} lean", absgrad=True, lean=True, v_alpha=False,
                 images=("colors", "alphas"))
        monkeypatch.setattr(_wrapper_2dgs, "SREC", False)
        _compare("e", name, ts, D, True, f"D{D} queue forward", absgrad=False)


@pytest.mark.parametrize("ts,srec", [(16, True), (16, False), (8, True)])
def test_e_alpha_gate_at_equality(monkeypatch, ts, srec):
    """alpha == opacity at the three centre pixels: float32(1/255) and the
    float32 above contribute, the float32 below does not -- in the forward's
    log-domain gate, in the backward's and in surfel_keep alike."""
    from gsplat_hip import _wrapper_2dgs
    monkeypatch.setattr(_wrapper_2dgs, "SREC", srec)
    c = SC.build("gate_alpha")
    got = _gpu(lambda: _raster("gate_alpha", ts, 4, False, absgrad=True))
    alphas = [float(got["alphas"][0, y, x, 0]) for y, x in c.centres]
    print("alphas at the centres", alphas, "opacities", c.opac[0].tolist())
    # alphas are 1 - T with T = 1 - opacity: the opacity to half an ulp of 1
    assert abs(alphas[0] - float(c.opac[0, 0])) <= 2.0 ** -24 and alphas[1] == 0.0 and \
        abs(alphas[2] - float(c.opac[0, 2])) <= 2.0 ** -24
    assert np.count_nonzero(got["alphas"]) == 2
    vo = got["v_opacities"][0]
    assert vo[0] != 0 and vo[1] == 0 and vo[2] != 0, vo
