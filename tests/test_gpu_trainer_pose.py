"""GPU: camera pose optimisation in the 3DGS trainer (Trainer(pose_opt=True,
pose_noise=...)): the fused step, eager and graph-replayed.

* the first step renders exactly what a plain trainer renders;
* one step's pose gradient against autograd through the unfused path
  (rasterization(viewmats=inv(c2w T(e))) with e.requires_grad);
* the graph-replayed trainer tracks the eager one (also with the bilateral
  grid, and across a refine), kernel nodes only;
* with the options off the captured step is unchanged;
* frozen Gaussians, perturbed cameras: the poses are recovered."""

import os

import pytest
import torch

from test_gpu_pose import pose_T

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def _trainer_scene(n_cams=4, W=64, H=64, stride=56):
    """The garden crop's every 56th point at 64 x 64: ~2,000 Gaussians."""
    from gsplat_hip.train_step import camera_pool, load_garden_scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(root, "tests", "golden", "garden_scene.npz"), scene_grid=1)
    means, rgbs = means[::stride].contiguous(), rgbs[::stride].contiguous()
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=n_cams)
    return means, rgbs, vm.float(), K.float(), W, H


def test_first_step_renders_what_a_plain_trainer_renders():
    """Zero embeddings reproduce the view matrix bit for bit and the forward
    has no atomics: the first-step losses are equal (up to the plain
    trainer's own run-to-run spread, should it have one; measured: none,
    0.5278211832046509 three times)."""
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    losses = []
    for kw in ({}, {}, dict(pose_opt=True)):
        tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, max_steps=100, **kw)
        losses.append(float(tr.step(0).detach()))
        tr.sync()
    off, off2, on = losses
    print(f"first-step loss: plain {off!r} / {off2!r}, pose_opt {on!r}")
    assert abs(on - off) <= abs(off2 - off), losses


def _unfused_pose_gradient(tr, ci, it):
    """dL/de at e = 0 of the plain trainer's loss through the existing unfused
    path: viewmats that require grad (torch.inverse, the separate SH pass,
    atomics into v_viewmats)."""
    from gsplat_hip import rasterization
    from gsplat_hip.losses import l1_ssim_loss
    p = tr.params
    e = torch.zeros(9, device=DEV, requires_grad=True)
    c2w = torch.linalg.inv(tr.viewmats[ci])
    vm = torch.inverse(c2w @ pose_T(e))[None]
    colors, _, _ = rasterization(
        p["means"].detach(), p["quats"].detach(), torch.exp(p["scales"].detach()),
        torch.sigmoid(p["opacities"].detach()), (p["sh0"].detach(), p["shN"].detach()), vm,
        tr.Ks[ci:ci + 1], tr.width, tr.height, sh_degree=tr.sh_degree_at(it), packed=False,
        near_plane=0.01, far_plane=1e10, radius_clip=0.0)
    loss = l1_ssim_loss(colors, tr.targets[ci:ci + 1], tr.ssim_lambda)
    (g,) = torch.autograd.grad(loss, e)
    return g.double().cpu()


def test_one_step_pose_gradient_matches_the_unfused_path():
    """After step 1 from zero init exp_avg / (1 - beta1) of the camera's row is
    the pose gradient (weight decay of a zero row adds nothing).

    Tolerance: 10 x the larger of the unfused path's own run-to-run spread
    over three runs (its backward uses float atomics) and 1e-5 max|g|.
    Measured on an MI355X (profiles/pose_opt/parity.txt): max|g| 1.378e-01,
    unfused run-to-run spread 1.49e-08, fused against unfused 7.38e-07, bar
    1.378e-05 (the 1e-5 max|g| term decides it)."""
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    it = 0
    plain = Trainer(means, rgbs, vm, K, W, H, device=DEV, max_steps=100)
    ci = plain.camera_index(it)
    refs = [_unfused_pose_gradient(plain, ci, it) for _ in range(3)]
    spread = max(float((a - refs[0]).abs().max()) for a in refs[1:])
    g_ref = refs[0]
    tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, max_steps=100, pose_opt=True)
    tr.step(it)
    tr.sync()
    m, v = (t.double().cpu() for t in tr.moments()["pose_embeds"])
    g = m[ci] / 0.1
    top = float(g_ref.abs().max())
    bar = 10.0 * max(spread, 1e-5 * top)
    err = float((g - g_ref).abs().max())
    print(f"pose gradient: max|g| {top:.6e}, unfused run-to-run spread {spread:.3e}, "
          f"fused-vs-unfused err {err:.3e}, bar {bar:.3e}\n  fused   {g.tolist()}\n"
          f"  unfused {g_ref.tolist()}")
    assert top > 0.0
    assert err <= bar, (err, bar)
    others = [r for r in range(4) if r != ci]
    assert not m[others].any() and not v[others].any()  # g = wd * 0 for the other rows
    assert float(tr.pose.embeds[ci].abs().max()) > 0.0
    assert not tr.pose.embeds[others].any()


def _run(graph, steps=6, **kw):
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, graph=graph, max_steps=100,
                 pose_opt=True, pose_opt_lr=1e-3, pose_noise=0.01, **kw)
    assert (tr._graph is not None) == graph
    losses = [tr.step(it) for it in range(steps)]
    tr.sync()
    assert tr.graph_fallback is None, tr.graph_fallback
    assert tr.pose.step_count == steps
    m, v = tr.moments()["pose_embeds"]
    out = dict(embeds=tr.pose.embeds.detach().clone(), m=m.clone(), v=v.clone(),
               losses=torch.tensor([float(x.detach()) for x in losses]), tr=tr)
    return out


@pytest.mark.parametrize("bilagrid", [False, True], ids=["plain", "bilagrid"])
def test_graph_trainer_tracks_eager(bilagrid):
    """Six steps over the four cameras: embeddings and moments of the replayed
    trainer within the one-step test's tolerance of the eager one's (10 x the
    larger of the eager run-to-run spread and 1e-5 max), kernel nodes only."""
    kw = dict(bilateral_grid=True) if bilagrid else {}
    a, a2, b = _run(False, **kw), _run(False, **kw), _run(True, **kw)
    g = b["tr"]._graph
    assert g.replays >= 6
    assert set(g.census) <= {"kernel", "empty"}, g.census
    assert sorted({b["tr"].camera_index(it) for it in range(6)}) == [0, 1, 2, 3]
    for k in ("embeds", "m", "v"):
        spread = float((a2[k] - a[k]).abs().max())
        top = float(a[k].abs().max())
        err = float((b[k] - a[k]).abs().max())
        bar = 10.0 * max(spread, 1e-5 * top)
        print(f"{k}: graph-vs-eager {err:.3e}, eager run-to-run {spread:.3e}, max {top:.3e}, "
              f"bar {bar:.3e}")
        assert top > 0.0 and err <= bar, (k, err, bar)
    torch.testing.assert_close(b["losses"], a["losses"], rtol=1e-4, atol=1e-6)
    assert all(float(a["embeds"][n].abs().max()) > 0 for n in range(4))
    b["tr"].release_graph()


def test_refine_recaptures_and_keeps_the_pose_state():
    from gsplat_hip.densify import DefaultStrategyConfig
    cfg = DefaultStrategyConfig(refine_start_iter=1, refine_every=3, reset_every=7)
    out = _run(True, steps=8, strategy=cfg)
    tr = out["tr"]
    assert len(tr.refine_log) >= 2, tr.refine_log
    assert tr._graph.recaptures >= 2
    assert set(tr._graph.census) <= {"kernel", "empty"}, tr._graph.census
    n = tr.params["means"].shape[0]
    assert tr.pose.ws.numel() >= 16 * ((n + 255) // 256)
    assert torch.isfinite(out["embeds"]).all() and torch.isfinite(out["losses"]).all()
    assert all(float(out["embeds"][k].abs().max()) > 0 for k in range(4))
    # every row's moments lived through the refines
    assert float(out["v"].max(dim=1).values.min()) > 0.0
    tr.release_graph()


def test_mcmc_schedule_with_pose_opt():
    """MCMCStrategy (no regularisers: the geometry Adam stays in the
    projection backward): relocation / sample-add refines re-capture, the
    position noise and the pose launches share the captured step."""
    from gsplat_hip.mcmc import MCMCStrategyConfig
    cfg = MCMCStrategyConfig(refine_start_iter=1, refine_every=3, cap_max=2200)
    out = _run(True, steps=8, strategy=cfg)
    tr = out["tr"]
    assert len(tr.refine_log) >= 2, tr.refine_log
    assert tr.params["means"].shape[0] > 1997  # Gaussians were sampled in
    assert set(tr._graph.census) <= {"kernel", "empty"}, tr._graph.census
    assert torch.isfinite(out["embeds"]).all() and torch.isfinite(out["losses"]).all()
    assert all(float(out["embeds"][k].abs().max()) > 0 for k in range(4))
    tr.release_graph()


def test_options_off_leave_the_captured_step_unchanged():
    """Absent or off, the node census is the same; pose_noise adds launch (a),
    pose_opt launches (a) and (c) (the projection backward's variant replaces
    a kernel, it adds none)."""
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    census = []
    for kw in ({}, dict(pose_opt=False, pose_noise=0.0), dict(pose_noise=0.01),
               dict(pose_opt=True), dict(pose_opt=True, pose_noise=0.01)):
        tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, graph=True, max_steps=100, **kw)
        for it in range(2):
            tr.step(it)
        tr.sync()
        assert tr.graph_fallback is None, tr.graph_fallback
        census.append(dict(tr._graph.census))
        tr.release_graph()
    print("census:", census)
    assert census[0] == census[1], census
    for c in census:
        assert set(c) <= {"kernel", "empty"}, c
    assert census[2]["kernel"] == census[0]["kernel"] + 1, census
    assert census[3]["kernel"] == census[0]["kernel"] + 2, census
    assert census[4]["kernel"] == census[0]["kernel"] + 2, census


def _recovery(seed, steps=400):
    """Frozen Gaussians, targets from the true cameras, perturbed cameras
    passed in: (translation error before, after, mean loss with pose_opt,
    mean loss without)."""
    from gsplat_hip.train_step import Trainer

    class Frozen(Trainer):
        LRS = {k: 0.0 for k in Trainer.LRS}

    means, rgbs, vm, K, W, H = _trainer_scene()
    n = len(vm)

    def fatten(tr):  # splats a few pixels wide, identically for every trainer
        tr.params["scales"].data.fill_(-3.0)
        tr.params["opacities"].data.fill_(0.0)

    truth = Frozen(means, rgbs, vm, K, W, H, device=DEV)
    fatten(truth)
    with torch.no_grad():
        targets = torch.cat([truth.render(ci)[0] for ci in range(n)]).clone()
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(n, 9, generator=g, dtype=torch.float64) * 1e-2
    vm_pert = torch.linalg.inv(torch.linalg.inv(vm.double()) @ pose_T(noise)).float()

    def terr(v):
        return float((v.cpu()[:, :3, 3] - vm[:, :3, 3]).norm(dim=-1).mean())

    res = {}
    for on in (True, False):
        tr = Frozen(means, rgbs, vm_pert, K, W, H, device=DEV, graph=True, max_steps=steps,
                    targets=targets, pose_opt=on, pose_opt_lr=3e-4)
        fatten(tr)
        losses = [tr.step(it) for it in range(steps)]
        tr.sync()
        assert tr.graph_fallback is None, tr.graph_fallback
        res[on] = (sum(float(x) for x in losses[-n:]) / n, terr(tr.adjusted_viewmats()))
        assert torch.equal(tr.params["means"].detach().cpu(), means)  # frozen
        tr.release_graph()
    before = terr(vm_pert)
    assert res[False][1] == pytest.approx(before, rel=1e-6)
    return before, res[True][1], res[True][0], res[False][0]


def test_pose_recovery():
    """Strict orderings, no tuned ratio: the refined cameras are closer to the
    true ones than the perturbed cameras were, and the loss over the cameras
    is lower than without pose_opt.  Seeds 0, 1, 2 measured on an MI355X
    (profiles/pose_opt/parity.txt): translation error 0.0232 -> 0.0057,
    0.0183 -> 0.0027, 0.0220 -> 0.0025; mean loss 0.0314 -> 0.0039,
    0.0248 -> 0.0017, 0.0339 -> 0.0029.  Seed 0 kept here."""
    before, after, loss_on, loss_off = _recovery(0)
    print(f"translation error {before:.5f} -> {after:.5f}; mean loss {loss_off:.6f} (off) "
          f"-> {loss_on:.6f} (pose_opt)")
    assert after < before, (after, before)
    assert loss_on < loss_off, (loss_on, loss_off)
