"""Contribution scores (csrc/rasterize_score.hip) against a plain float64 loop
over the very arrays handed to the kernel.  Bars: FWD_BARS["alphas"] through
close_most; `sum` with atol times the Gaussian's reference count; `count` equal
except on close_most's allowed number of Gaussians, each off by at most its
near-gate pairs.  Outliers: close_most's one-flip bound, 2/255 of a weight 1."""

import numpy as np
import pytest
import torch

import raster_cases as RC
from proj_cases import GATE_MARGIN, REDRAW_CAP

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL, ATOL = RC.FWD_BARS["alphas"]
FLIP = 2.0 / 255.0 + ATOL


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def truth(m2, cn, op, W, H, off, fids, row_of, n_rows, masks=None, pw=None):
    """sum, max, count and near-gate pairs per output row, in float64."""
    m2, cn, op = (np.asarray(x, np.float64).reshape(-1, k) for x, k in ((m2, 2), (cn, 3), (op, 1)))
    C, th, tw = off.shape
    ends = np.append(off.reshape(-1), len(fids))
    s, m = np.zeros(n_rows), np.zeros(n_rows)
    n, near = np.zeros(n_rows, np.int64), np.zeros(n_rows, np.int64)
    ly, lx = np.divmod(np.arange(256), 16)
    for t in range(C * th * tw):
        if masks is not None and masks.reshape(-1)[t]:
            continue
        c, r = divmod(t, th * tw)
        py, px = (r // tw) * 16 + ly, (r % tw) * 16 + lx
        alive = (px < W) & (py < H)
        wgt = 1.0 if pw is None else pw[c, np.minimum(py, H - 1), np.minimum(px, W - 1)]
        Tr = np.ones(256)
        for g in fids[ends[t]:ends[t + 1]]:
            dx, dy = m2[g, 0] - (px + 0.5), m2[g, 1] - (py + 0.5)
            sig = 0.5 * (cn[g, 0] * dx * dx + cn[g, 2] * dy * dy) + cn[g, 1] * dx * dy
            with np.errstate(all="ignore"):
                al = np.minimum(0.999, op[g, 0] * np.exp(-sig))
            nT = Tr * (1.0 - al)
            hit = alive & (sig >= 0) & (al >= 1.0 / 255.0)
            keep = hit & (nT > 1e-4)
            w = np.where(keep, al * Tr, 0.0)
            k = row_of[g]
            s[k] += (w * wgt).sum()
            m[k] = max(m[k], w.max())
            n[k] += keep.sum()
            near[k] += (alive & (sig >= 0) & (np.abs(al * 255.0 - 1.0) <= GATE_MARGIN)).sum() \
                + (hit & (np.abs(nT / 1e-4 - 1.0) <= 1.0 / 255.0 + GATE_MARGIN)).sum()
            Tr = np.where(keep, nT, Tr)
            alive &= ~(hit & ~keep)
    return s, m, n, near


def check(got, ref, what):
    s, m, n = (x.cpu().numpy().reshape(-1) for x in got)
    rs, rm, rn, near = ref
    print(f"{what}: max|dsum|={np.abs(s - rs).max():.3e} max|dmax|={np.abs(m - rm).max():.3e} "
          f"count mismatches={(n != rn).sum()} near-gate Gaussians={(near > 0).sum()}/{n.size}")
    RC.close_most(m, rm, RTOL, ATOL, what + " max", out_bound=FLIP)
    RC.close_most(s, rs, RTOL, ATOL * np.maximum(rn, 1), what + " sum", out_bound=FLIP)
    bad = n != rn
    assert bad.sum() <= max(2, int(1e-4 * n.size)), (what, int(bad.sum()))
    assert (np.abs(n - rn) <= near)[bad].all(), (what, n[bad], rn[bad], near[bad])


def variant_inputs(kind, variant):
    """(kernel keyword arguments as numpy, truth arguments) of a case."""
    case = RC.build_case(kind, 16, 3, backend="hip")
    G = case.C * case.N
    m2, cn, op, fids = case.means2d, case.conics, case.opacities, case.flatten_ids
    kw, masks, pw, row_of, n_rows = {}, None, None, np.arange(G), G
    if variant == "fold":
        kw["fold"], row_of, n_rows = True, np.arange(G) % case.N, case.N
    elif variant == "packed":  # the rows with a radius, as a packed projection returns them
        valid = (case.radii.reshape(G, -1) > 0).all(-1)
        rank = np.cumsum(valid) - 1
        m2, cn, op = m2.reshape(G, 2)[valid], cn.reshape(G, 3)[valid], op.reshape(G)[valid]
        fids = rank[fids].astype(np.int32)
        kw["packed"], row_of, n_rows = True, np.arange(len(op)), len(op)
    elif variant == "mask":
        kw["masks"] = masks = RC.tile_mask(case)
    elif variant == "weights":
        kw["pixel_weights"] = pw = np.random.default_rng(3).uniform(
            0.0, 1.0, (case.C, case.H, case.W)).astype(np.float32)
    args = (m2, cn, op, case.W, case.H, 16, case.offsets, fids)
    return case, args, kw, (m2, cn, op, case.W, case.H, case.offsets, fids, row_of, n_rows,
                            masks, pw)


def run(args, kw, **extra):
    import gsplat_hip
    m2, cn, op, W, H, ts, off, fids = args
    kw = {k: (T(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    return gsplat_hip.rasterize_to_contributions(T(m2), T(cn), T(op), W, H, ts, T(off), T(fids),
                                                 **kw, **extra)


@pytest.mark.parametrize("kind,variant", [
    ("sparse", "plain"), ("sparse", "fold"), ("dense", "plain"), ("edge", "plain"),
    ("sparse", "packed"), ("sparse", "mask"), ("dense", "weights")])
def test_scores_vs_float64_loop(kind, variant):
    case, args, kw, targs = variant_inputs(kind, variant)
    ref = truth(*targs)
    assert (ref[3] > 0).mean() <= REDRAW_CAP, "too many near-gate Gaussians: another seed"
    assert ref[2].sum() > 0
    if kind == "dense":  # several batches in a tile
        assert case.n_per_tile.max() > 1000
    check(run(args, kw), ref, f"{kind} {variant}")


def test_out_accumulates_over_calls():
    """Camera 0, then camera 1 into the same folded buffers == both at once."""
    case, args, kw, _ = variant_inputs("sparse", "fold")
    m2, cn, op, W, H, ts, off, fids = args
    both = run(args, kw)
    cut = int(off[1, 0, 0])
    out = run((m2[:1], cn[:1], op[:1], W, H, ts, off[:1], fids[:cut]), kw)
    got = run((m2[1:], cn[1:], op[1:], W, H, ts, off[1:] - cut, fids[cut:] - case.N), kw, out=out)
    assert all(a is b for a, b in zip(got, out))
    assert torch.equal(got[1], both[1]) and torch.equal(got[2], both[2])
    torch.testing.assert_close(got[0], both[0], rtol=RTOL, atol=ATOL)


def test_max_and_count_are_deterministic():
    _, args, kw, _ = variant_inputs("dense", "plain")
    a, b = run(args, kw), run(args, kw)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def _scene(n=300, C=3, W=40, H=36):
    """A cloud in front of three cameras; a third of it outside every view."""
    means, quats, scales, opac, vm, K = RC._garden_scene(n, C, W, H, seed=5, scale=0.3)
    means[::3, 0] += 40.0
    return [x.to(DEV) for x in (means, quats, scales, opac, vm, K)] + [W, H]


@pytest.mark.parametrize("mode", ["classic", "covars", "antialiased"])
def test_contribution_scores_over_cameras(mode):
    """camera_batch=2 over 3 cameras (ragged last batch) == per-camera truths, reduced here."""
    import gsplat_hip
    means, quats, scales, opac, vm, K, W, H = _scene()
    N, aa = len(means), mode == "antialiased"
    covars = None
    if mode == "covars":
        covars = gsplat_hip.quat_scale_to_covar_preci(quats, scales, True, False, triu=True)[0]
    got = gsplat_hip.contribution_scores(
        means, quats, scales, opac, vm, K, W, H, covars=covars, camera_batch=2,
        rasterize_mode="antialiased" if aa else "classic")
    ref = [np.zeros(N), np.zeros(N), np.zeros(N, np.int64), np.zeros(N, np.int64)]
    tw, th = -(-W // 16), -(-H // 16)
    for c in range(len(vm)):
        radii, m2, d, cn, comp = gsplat_hip.fully_fused_projection(
            means, covars, quats, scales, vm[c:c + 1], K[c:c + 1], W, H, calc_compensations=aa)
        _, ids, fids = gsplat_hip.isect_tiles(m2, radii, d, 16, tw, th)
        off = gsplat_hip.isect_offset_encode(ids, 1, tw, th)
        op = opac[None] * comp if aa else opac[None]
        s, m, n, near = truth(*(x.cpu().numpy() for x in (m2, cn, op)), W, H, off.cpu().numpy(),
                              fids.cpu().numpy(), np.arange(N), N)
        ref = [ref[0] + s, np.maximum(ref[1], m), ref[2] + n, ref[3] + near]
    assert (ref[2][::3] == 0).all() and (ref[2] > 0).sum() > N // 4
    check((got["sum"], got["max"], got["count"]), ref, f"scores {mode}")


def test_pruning_unscored_gaussians_keeps_the_renders():
    """Gaussians no scored pixel blended are removed; the scored views render as before."""
    import gsplat_hip
    means, quats, scales, opac, vm, K, W, H = _scene()
    colors = torch.rand(len(means), 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    sc = gsplat_hip.contribution_scores(means, quats, scales, opac, vm, K, W, H, camera_batch=2)
    full = dict(means=means, quats=quats, scales=scales, opacities=opac, colors=colors)
    kept = gsplat_hip.prune_splats(full, sc["count"] > 0)
    assert 0 < len(kept["means"]) <= len(means) - len(means[::3])
    out = []
    for sp in (kept, full):
        rc, ra, _ = gsplat_hip.rasterization(sp["means"], sp["quats"], sp["scales"],
                                             sp["opacities"], sp["colors"], vm, K, W, H)
        out.append({"colors": rc, "alphas": ra})
    RC.check_forward(out[0], {k: v.cpu().numpy() for k, v in out[1].items()}, "pruned")
