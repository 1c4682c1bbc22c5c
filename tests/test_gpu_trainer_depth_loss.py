"""GPU: sparse depth supervision in the 3DGS trainer (Trainer(depth_loss=True,
depth_points=...)): the fused step, eager and graph-replayed.

* the first-step loss is the plain trainer's plus depth_lambda * scene_scale *
  the float64 oracle's term on the plain trainer's render;
* one step's means gradient against autograd through the unfused path
  (rasterization(render_mode="RGB+ED"), the torch composition, l1_ssim_loss);
* the graph-replayed trainer tracks the eager one over all cameras (different
  M, one image without points; also with the bilateral grid, with the camera
  pose optimised, and across a refine), kernel nodes only;
* with the option off the captured step is unchanged;
* means pushed along their view rays: the depth error falls, and ends below
  that of the same run without the option.

The scene: the garden crop at 64 x 64, ~2,000 Gaussians made a few pixels
wide, four cameras; the points of an image are positions sampled from the
unperturbed scene's expected depth where alpha > 0.5, their depths moved by
+-10 % so that |disp - 1/d_gt| stays away from zero at the start.

Measured on an MI355X (profiles/depth_loss/parity.txt): points per image 207,
231, 0, 342; first-step loss 0.5014469624 against 0.5014469347 expected (err
2.8e-08, the float32 composition's own error 1.6e-09, bar 5.0e-07); means
gradient max|g| 1.315e-02 of which the depth term 1.149e-02, unfused
run-to-run spread 9.3e-10, fused against unfused 4.5e-08, bar 1.3e-06; graph
against eager after six steps: parameters within 1.3e-05 (the opacities),
first moments within 3.0e-08; captured step 40 kernel nodes without the
option, 49 with it; depth error 0.03465 -> 0.00193 in 200 steps with the
option, 0.01589 without."""

import pytest
import torch

from test_gpu_depth_loss import composition, reference_term
from test_gpu_trainer_pose import _trainer_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
EMPTY = 2  # the image without points


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def _fatten(tr):
    """Splats a few pixels wide, identically for every trainer.  Three different
    axes: an isotropic splat has no quaternion gradient, and Adam would turn
    the rounding noise left in its place into steps of the full learning rate."""
    tr.params["scales"].data.copy_(torch.tensor([-2.7, -3.0, -3.5]).expand(
        tr.params["scales"].shape))
    tr.params["opacities"].data.fill_(0.0)
    return tr


def _render_depth(tr, ci):
    """(accumulated depth D, alpha) [H, W] of camera ci with tr's Gaussians."""
    from gsplat_hip import rasterization
    p = tr.params
    with torch.no_grad():
        rc, ra, _ = rasterization(
            p["means"], p["quats"], torch.exp(p["scales"]), torch.sigmoid(p["opacities"]),
            (p["sh0"], p["shN"]), tr.viewmats[ci:ci + 1], tr.Ks[ci:ci + 1], tr.width, tr.height,
            sh_degree=tr.sh_degree, packed=False, near_plane=0.01, far_plane=1e10,
            radius_clip=0.0, render_mode="RGB+D")
    return rc[0, :, :, 3].clone(), ra[0, :, :, 0].clone()


_CACHE = {}


def _scene():
    """(scene, per-image (points, depths) on the CPU, targets): computed once."""
    if "scene" in _CACHE:
        return _CACHE["scene"]
    from gsplat_hip.train_step import Trainer
    scene = _trainer_scene()
    means, rgbs, vm, K, W, H = scene
    truth = _fatten(Trainer(means, rgbs, vm, K, W, H, device=DEV))
    with torch.no_grad():
        targets = torch.cat([truth.render(ci)[0] for ci in range(len(vm))]).contiguous().cpu()
    points = []
    for ci in range(len(vm)):
        if ci == EMPTY:
            points.append((torch.zeros(0, 2), torch.zeros(0)))
            continue
        D, A = _render_depth(truth, ci)
        D, A = D.double().cpu(), A.double().cpu()
        g = torch.Generator().manual_seed(40 + ci)
        xy = torch.rand(300 + 50 * ci, 2, generator=g, dtype=torch.float64) \
            * torch.tensor([W - 1.001, H - 1.001], dtype=torch.float64)
        x0, y0 = xy[:, 0].floor().long(), xy[:, 1].floor().long()
        a_min = torch.stack([A[y0, x0], A[y0, x0 + 1], A[y0 + 1, x0], A[y0 + 1, x0 + 1]]).min(0)[0]
        ED = D / A.clamp(min=1e-10)
        wx, wy = xy[:, 0] - x0, xy[:, 1] - y0
        d = ((1 - wx) * (1 - wy) * ED[y0, x0] + wx * (1 - wy) * ED[y0, x0 + 1]
             + (1 - wx) * wy * ED[y0 + 1, x0] + wx * wy * ED[y0 + 1, x0 + 1])
        keep = a_min > 0.5
        xy, d = xy[keep], d[keep]
        d = d * torch.where(torch.arange(len(d)) % 2 == 0, 1.1, 0.9)
        points.append((xy.float(), d.float()))
    counts = [len(d) for _, d in points]
    print("points per image:", counts)
    assert all(c >= 100 for i, c in enumerate(counts) if i != EMPTY), counts
    assert len({c for c in counts}) == len(counts), counts  # a different M per image
    _CACHE["scene"] = (scene, points, targets)
    return _CACHE["scene"]


def _make(graph=False, **kw):
    from gsplat_hip.train_step import Trainer
    (means, rgbs, vm, K, W, H), points, targets = _scene()
    kw.setdefault("depth_loss", True)
    if kw["depth_loss"]:
        kw.setdefault("depth_points", points)
    kw.setdefault("max_steps", 100)
    # (targets: the trainer's random images unless given -- the initial render
    # is the scene the points come from, and |render - target| must not be 0)
    return _fatten(Trainer(means, rgbs, vm, K, W, H, device=DEV, graph=graph, **kw))


def test_first_step_loss_is_the_plain_loss_plus_the_oracle_term():
    """Tolerance: ten times the float32 torch composition's own error against
    the float64 oracle on the same render, scaled like the term, with a floor
    of 1e-6 of the loss (the photometric part is the plain trainer's own
    launch on the same colours; the sum is one float32 addition)."""
    _, points, _ = _scene()
    lam, scale = 0.25, 1.5
    plain = _make(depth_loss=False, scene_scale=scale)
    ci = plain.camera_index(0)
    assert ci != EMPTY
    D, A = _render_depth(plain, ci)
    pts, dgt = points[ci]
    t64, _, _, margin = composition(D.double().cpu(), A.double().cpu(), pts.double(), dgt.double())
    t32 = composition(D, A, pts.to(DEV), dgt.to(DEV))[0]
    assert margin > 1e-3, margin
    base = float(plain.step(0).detach())
    tr = _make(depth_lambda=lam, scene_scale=scale)
    loss = float(tr.step(0).detach())
    want = base + lam * scale * float(t64)
    own = abs(float(t32) - float(t64)) * lam * scale
    bar = max(10.0 * own, 1e-6 * abs(want))
    print(f"first-step loss: plain {base!r}, oracle term {float(t64)!r} (margin {margin:.3e}), "
          f"expected {want!r}, got {loss!r}; fp32 composition's own error {own:.3e}, "
          f"err {abs(loss - want):.3e}, bar {bar:.3e}")
    assert float(t64) > 0.0
    assert abs(loss - want) <= bar, (loss, want, bar)


def _unfused_means_gradient(tr, ci, it, pts, dgt, weight):
    """dL/dmeans of the step's loss through the existing unfused path: plain
    autograd on detached parameters, the RGB+ED render, the torch composition."""
    from gsplat_hip import rasterization
    from gsplat_hip.losses import l1_ssim_loss
    p = tr.params
    means = p["means"].detach().clone().requires_grad_(True)
    rc, _, _ = rasterization(
        means, p["quats"].detach(), torch.exp(p["scales"].detach()),
        torch.sigmoid(p["opacities"].detach()), (p["sh0"].detach(), p["shN"].detach()),
        tr.viewmats[ci:ci + 1], tr.Ks[ci:ci + 1], tr.width, tr.height,
        sh_degree=tr.sh_degree_at(it), packed=False, near_plane=0.01, far_plane=1e10,
        radius_clip=0.0, render_mode="RGB+ED")
    loss = l1_ssim_loss(rc[..., :3], tr.targets[ci:ci + 1], tr.ssim_lambda)
    term, _ = reference_term(rc[..., 3:], pts, dgt)
    (g,) = torch.autograd.grad(loss + weight * term, means)
    return g.double().cpu()


@pytest.mark.parametrize("pose", [False, True], ids=["plain", "pose_opt"])
def test_one_step_means_gradient_matches_the_unfused_path(pose):
    """After step 1 from zero state exp_avg / (1 - beta1) of the means is their
    gradient.  Tolerance: 10 x the larger of the unfused path's own
    run-to-run spread over three runs and 1e-5 max|g| (the pose test's rule).
    A build whose depth gradient does not reach the means fails: the depth
    term is weighted to dominate (depth_lambda 1).  With pose_opt the same
    gradient comes out of the projection backward's pose variant, and the
    pose row moves (its partials include the v_depths path)."""
    _, points, _ = _scene()
    it, lam = 0, 1.0
    tr = _make(depth_lambda=lam, **(dict(pose_opt=True) if pose else {}))
    ci = tr.camera_index(it)
    pts, dgt = (t.to(DEV) for t in points[ci])
    refs = [_unfused_means_gradient(tr, ci, it, pts, dgt, lam * tr.scene_scale)
            for _ in range(3)]
    no_depth = _unfused_means_gradient(tr, ci, it, pts, dgt, 0.0)
    spread = max(float((a - refs[0]).abs().max()) for a in refs[1:])
    g_ref = refs[0]
    tr.step(it)
    tr.sync()
    g = tr.moments()["means"][0].double().cpu() / 0.1
    top = float(g_ref.abs().max())
    bar = 10.0 * max(spread, 1e-5 * top)
    err = float((g - g_ref).abs().max())
    part = float((g_ref - no_depth).abs().max())
    print(f"means gradient: max|g| {top:.6e}, the depth term's share max {part:.6e}, unfused "
          f"run-to-run spread {spread:.3e}, fused-vs-unfused err {err:.3e}, bar {bar:.3e}")
    assert part > 100.0 * bar, (part, bar)  # the test can tell a missing depth gradient
    assert err <= bar, (err, bar)
    if pose:
        assert float(tr.pose.embeds[ci].abs().max()) > 0.0


def _run(graph, steps=6, **kw):
    tr = _make(graph, **kw)
    assert (tr._graph is not None) == graph
    losses = [tr.step(it) for it in range(steps)]
    tr.sync()
    assert tr.graph_fallback is None, tr.graph_fallback
    out = dict(params={k: p.detach().clone() for k, p in tr.params.items()},
               exp_avg=[m.clone() for m in tr.opt.exp_avg], means=tr.params["means"].detach(),
               losses=torch.tensor([float(x.detach()) for x in losses]), tr=tr)
    if getattr(tr, "pose_opt", False):
        m, v = tr.moments()["pose_embeds"]
        out["pose"] = dict(embeds=tr.pose.embeds.detach().clone(), m=m.clone(), v=v.clone())
    return out


@pytest.mark.parametrize("variant", ["plain", "bilagrid", "pose_opt"])
def test_graph_trainer_tracks_eager(variant):
    """Six steps over the four cameras (a different M each, one image without
    points), kernel nodes only.  The tolerances are those of the existing
    comparisons of the same quantities: the Gaussian parameters to rtol 1e-3 /
    atol 1e-5, their first moments to rtol 1e-2 / atol 1e-6 and the losses to
    rtol 1e-4 / atol 1e-6 (test_gpu_trainer_bilagrid's
    test_graph_trainer_tracks_eager); with pose_opt the pose table and its
    moments within 10 x the larger of the eager run-to-run spread and 1e-5
    max (test_gpu_trainer_pose's)."""
    kw = {"plain": {}, "bilagrid": dict(bilateral_grid=True),
          "pose_opt": dict(pose_opt=True, pose_opt_lr=1e-3)}[variant]
    a, b = _run(False, **kw), _run(True, **kw)
    g = b["tr"]._graph
    assert g.replays >= 6
    assert set(g.census) <= {"kernel", "empty"}, g.census
    assert sorted({b["tr"].camera_index(it) for it in range(6)}) == [0, 1, 2, 3]
    for k in a["params"]:
        err = float((b["params"][k] - a["params"][k]).abs().max())
        print(f"{variant} {k}: graph-vs-eager max diff {err:.3e}, max {float(a['params'][k].abs().max()):.3e}")
    for x, y in zip(a["exp_avg"], b["exp_avg"]):
        print(f"{variant} exp_avg {tuple(x.shape)}: graph-vs-eager max diff "
              f"{float((y - x).abs().max()):.3e}, max {float(x.abs().max()):.3e}")
    torch.testing.assert_close(b["losses"], a["losses"], rtol=1e-4, atol=1e-6)
    for k in a["params"]:
        torch.testing.assert_close(b["params"][k], a["params"][k], rtol=1e-3, atol=1e-5)
    for x, y in zip(a["exp_avg"], b["exp_avg"]):
        torch.testing.assert_close(y, x, rtol=1e-2, atol=1e-6)
    if variant == "pose_opt":
        a2 = _run(False, **kw)
        for k in ("embeds", "m", "v"):
            spread = float((a2["pose"][k] - a["pose"][k]).abs().max())
            top = float(a["pose"][k].abs().max())
            err = float((b["pose"][k] - a["pose"][k]).abs().max())
            bar = 10.0 * max(spread, 1e-5 * top)
            print(f"pose {k}: graph-vs-eager {err:.3e}, eager run-to-run {spread:.3e}, max "
                  f"{top:.3e}, bar {bar:.3e}")
            assert top > 0.0 and err <= bar, (k, err, bar)
    b["tr"].release_graph()


def test_refine_recaptures_with_the_depth_term():
    from gsplat_hip.densify import DefaultStrategyConfig
    cfg = DefaultStrategyConfig(refine_start_iter=1, refine_every=3, reset_every=7)
    out = _run(True, steps=8, strategy=cfg)
    tr = out["tr"]
    assert len(tr.refine_log) >= 2, tr.refine_log
    assert tr._graph.recaptures >= 2
    assert set(tr._graph.census) <= {"kernel", "empty"}, tr._graph.census
    assert torch.isfinite(out["losses"]).all() and torch.isfinite(out["means"]).all()
    tr.release_graph()


def test_mcmc_schedule_with_the_depth_term():
    from gsplat_hip.mcmc import MCMCStrategyConfig
    cfg = MCMCStrategyConfig(refine_start_iter=1, refine_every=3, cap_max=2200)
    out = _run(True, steps=8, strategy=cfg)
    tr = out["tr"]
    assert len(tr.refine_log) >= 2, tr.refine_log
    assert set(tr._graph.census) <= {"kernel", "empty"}, tr._graph.census
    assert torch.isfinite(out["losses"]).all() and torch.isfinite(out["means"]).all()
    tr.release_graph()


def _make_absent():
    """A graph trainer built without any of the new arguments."""
    from gsplat_hip.train_step import Trainer
    (means, rgbs, vm, K, W, H), _, _ = _scene()
    return _fatten(Trainer(means, rgbs, vm, K, W, H, device=DEV, graph=True, max_steps=100))


def test_option_off_leaves_the_captured_step_unchanged():
    """Absent or off the node census is the same and the render has three
    channels; on, the step holds more kernels and still nothing else."""
    _, points, _ = _scene()
    makers = [_make_absent, lambda: _make(True, depth_loss=False),
              lambda: _make(True, depth_loss=False, depth_points=points), lambda: _make(True)]
    census = []
    for k, make in enumerate(makers):
        tr = make()
        for it in range(2):
            tr.step(it)
        tr.sync()
        assert tr.graph_fallback is None, tr.graph_fallback
        census.append(dict(tr._graph.census))
        with torch.no_grad():
            colors, _, meta = tr.render(0)
        assert colors.shape[-1] == 3
        assert ("_rgbd" in meta) == (k == 3)
        tr.release_graph()
    print("census:", census)
    assert census[0] == census[1] == census[2], census
    for c in census:
        assert set(c) <= {"kernel", "empty"}, c
    assert census[3]["kernel"] > census[0]["kernel"], census


def _depth_error(tr, points):
    """mean |disp - 1/d_gt| over all images' points, with tr's Gaussians."""
    total, n = 0.0, 0
    for ci, (pts, dgt) in enumerate(points):
        if len(dgt) == 0:
            continue
        D, A = _render_depth(tr, ci)
        ed = (D / A.clamp(min=1e-10))[None, :, :, None]
        term, _ = reference_term(ed, pts.to(DEV), dgt.to(DEV))
        total += float(term) * len(dgt)
        n += len(dgt)
    return total / n


def test_depth_term_pulls_perturbed_means_back():
    """The means pushed away from the cameras along the rays from the cameras'
    mean centre (by 0-6 %), the true depths as supervision, 200 replayed
    steps with depth_lambda 1.0: the depth error ends below its start, and
    below the end of the same run without the option.  Two measured runs, no
    number fixed in advance."""
    (means, rgbs, vm, K, W, H), points, targets = _scene()
    true_points = []
    for i, (p, d) in enumerate(points):  # the +-10 % taken back: the true depths
        f = torch.where(torch.arange(len(d)) % 2 == 0, 1.1, 0.9)
        true_points.append((p, d / f))
    centre = torch.linalg.inv(vm.double())[:, :3, 3].mean(0).float()
    g = torch.Generator().manual_seed(9)
    push = 1.0 + 0.06 * torch.rand(len(means), 1, generator=g)
    moved = centre + (means - centre) * push
    res = {}
    for on in (True, False):
        kw = dict(depth_loss=True, depth_lambda=1.0, depth_points=true_points) if on else \
            dict(depth_loss=False)
        tr = _make(True, max_steps=200, targets=targets, **kw)
        tr.params["means"].data.copy_(moved.to(DEV))
        start = _depth_error(tr, true_points)
        for it in range(200):
            tr.step(it)
        tr.sync()
        assert tr.graph_fallback is None, tr.graph_fallback
        res[on] = (start, _depth_error(tr, true_points))
        tr.release_graph()
    print(f"depth error: start {res[True][0]:.6f}; after 200 steps {res[True][1]:.6f} with "
          f"depth_loss, {res[False][1]:.6f} without")
    assert res[True][0] == pytest.approx(res[False][0], rel=1e-6)
    assert res[True][1] < res[True][0], res
    assert res[True][1] < res[False][1], res
