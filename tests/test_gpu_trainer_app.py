"""GPU: the 3DGS trainer's appearance optimisation (Trainer(app_opt=True),
simple_trainer.py `app_opt`): eager steps against the same steps composed in
torch (the oracle MLP of tests/app_oracle.py, rasterization(colors=...,
sh_degree=None), torch.optim.Adam x 2 for the module and the trainer's Adam
for the Gaussians), the captured step against the eager one with its node
census, refines under both strategies, the run with bilateral_grid and
depth_loss on top, and evaluate() with the zero embedding.

Tolerances are those of the existing trainer comparisons
(test_gpu_trainer_bilagrid.test_graph_trainer_tracks_eager): parameters to
rtol 1e-3 / atol 1e-5, first moments to rtol 1e-2 / atol 1e-6, losses to
rtol 1e-4 / atol 1e-6."""

import pytest
import torch

import app_oracle as O
from test_gpu_trainer_bilagrid import _trainer_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def _prepare(tr):
    """Splats a few pixels wide on three different axes (an isotropic splat
    has no quaternion gradient: Adam would step on rounding noise) and, with
    the option, a last layer off zero so that the trunk, the features, the
    embedding and the view direction carry gradient; identical for every
    trainer.

    Adam's eps is torch's default 1e-8 here instead of the trainer's 1e-15, in
    the trainer and in the composition alike.  The features' gradient is a
    64-term dot product per element, so an element can cancel to within its
    rounding error (about 1e-7 of gradients of 1e-4: 1e-11), where the sign
    depends on the summation order; g / (|g| + 1e-15) turns that sign into a
    whole step.  Measured with 1e-15: 10 of 111,808 feature elements off by up
    to 3.2e-3 (1.3 steps) after three steps while every first moment agreed to
    1e-11, and 2 elements off by 5e-5 between eager and replayed steps, which
    run the same kernels.  With 1e-8 a gradient error of 1e-11 moves a
    parameter by lr x 1e-3 at the most, inside the comparisons' tolerance, and
    gradients above 1e-8 -- all that carry signal -- step as before."""
    tr.params["scales"].data.copy_(torch.tensor([-2.7, -3.0, -3.5]).expand(
        tr.params["scales"].shape))
    tr.params["opacities"].data.fill_(0.0)
    tr.opt.eps = 1e-8
    tr.adam_kw = dict(tr.adam_kw, eps=1e-8)
    if getattr(tr, "app_opt", False):
        g = torch.Generator().manual_seed(5)
        tr.app.head[4].copy_((torch.randn(3, 64, generator=g) * 0.3).to(DEV))
        tr.app.head[5].copy_((torch.randn(3, generator=g) * 0.1).to(DEV))
    return tr


def _make(graph=False, **kw):
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    kw.setdefault("app_opt", True)
    return _prepare(Trainer(means, rgbs, vm, K, W, H, device=DEV, graph=graph, **kw))


def _module_state(tr):
    tr.sync()
    m = tr.moments()
    return dict(embeds=tr.app.embeds.detach().clone(),
                head=torch.cat([t.detach().reshape(-1) for t in tr.app.head]).clone(),
                embeds_m=m["app_embeds"][0].clone(), head_m=m["app_head"][0].clone())


def test_eager_steps_match_the_torch_composition():
    from gsplat_hip import rasterization
    from gsplat_hip.losses import FusedAdam, l1_ssim_loss
    steps = 3
    tr = _make()
    assert tr._graph is None
    p = {k: v.detach().clone().requires_grad_(True) for k, v in tr.params.items()}
    embeds = tr.app.embeds.detach().clone().requires_grad_(True)
    head = [t.detach().clone().requires_grad_(True) for t in tr.app.head]
    opt = FusedAdam(list(p.values()), tr.lrs, **tr.adam_kw)
    opt_head = torch.optim.Adam(head, lr=1e-3)
    opt_embeds = torch.optim.Adam([embeds], lr=1e-3 * 10.0, weight_decay=1e-6)
    want_losses, got_losses = [], []
    embeds0 = tr.app.embeds.detach().clone()
    for it in range(steps):
        ci = tr.camera_index(it)
        vm = tr.viewmats[ci:ci + 1]
        campos = torch.inverse(vm)[:, :3, 3]
        colors = O.app_colors(p["features"], p["colors"], embeds[ci:ci + 1], p["means"], campos,
                              head, tr.sh_degree_at(it))
        render, _, _ = rasterization(
            p["means"], p["quats"], torch.exp(p["scales"]), torch.sigmoid(p["opacities"]),
            colors, vm, tr.Ks[ci:ci + 1], tr.width, tr.height, sh_degree=None, packed=False,
            near_plane=0.01, far_plane=1e10, radius_clip=0.0)
        loss = l1_ssim_loss(render, tr.targets[ci:ci + 1], tr.ssim_lambda)
        colors.retain_grad()
        loss.backward()
        if it == 0:
            # the part of dL/dmeans that comes through the view direction
            again = O.app_colors(p["features"].detach(), p["colors"].detach(),
                                 embeds[ci:ci + 1].detach(), p["means"], campos,
                                 [t.detach() for t in head], tr.sh_degree_at(it))
            dir_part = torch.autograd.grad(again, p["means"], colors.grad)[0]
        assert float(head[0].grad.abs().max()) > 0 and float(embeds.grad[ci].abs().max()) > 0
        assert float(p["features"].grad.abs().max()) > 0
        opt.step()
        opt.zero_grad()
        for o in (opt_head, opt_embeds):
            o.step()
            o.zero_grad()
        want_losses.append(float(loss.detach()))
        got_losses.append(float(tr.step(it).detach()))
        assert tr.geom_applied  # the projection backward ran the geometry Adam
        if it == 0:
            # ... reached that Adam: had it been left out, the means' first
            # moment (0.1 x the gradient after one step) would be off by
            # 0.1 x the whole part at the row where the part is largest; it
            # must be off by less than half of that
            tr.sync()
            row = int(dir_part.abs().amax(1).argmax())
            part = 0.1 * float(dir_part[row].abs().max())
            err = float((tr.moments()["means"][0][row] - opt.exp_avg[0][row]).abs().max())
            print(f"means first moment, row {row}: the direction's part {part:.3e}, error "
                  f"{err:.3e}")
            assert part > 0.0 and err < 0.5 * part, (part, err)
    tr.sync()
    assert tr.app.step_count == steps and tr.opt.step_count == steps
    print("losses:", got_losses, want_losses)
    torch.testing.assert_close(torch.tensor(got_losses), torch.tensor(want_losses),
                               rtol=1e-4, atol=1e-6)
    moms = tr.moments()
    for i, k in enumerate(tr.params):
        err = float((tr.params[k].detach() - p[k].detach()).abs().max())
        err_m = float((moms[k][0] - opt.exp_avg[i]).abs().max())
        print(f"{k}: max parameter difference {err:.3e}, first moment {err_m:.3e} "
              f"(max {float(opt.exp_avg[i].abs().max()):.3e})")
    for i, k in enumerate(tr.params):
        torch.testing.assert_close(tr.params[k].detach(), p[k].detach(), rtol=1e-3, atol=1e-5)
        torch.testing.assert_close(moms[k][0], opt.exp_avg[i], rtol=1e-2, atol=1e-6)
    got = _module_state(tr)
    want_head = torch.cat([t.detach().reshape(-1) for t in head])
    want_head_m = torch.cat([opt_head.state[t]["exp_avg"].reshape(-1) for t in head])
    torch.testing.assert_close(got["head"], want_head, rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(got["head_m"], want_head_m, rtol=1e-2, atol=1e-6)
    torch.testing.assert_close(got["embeds"], embeds.detach(), rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(got["embeds_m"], opt_embeds.state[embeds]["exp_avg"],
                               rtol=1e-2, atol=1e-6)
    # the table's Adam is dense: the image no step showed moved by its decay
    unseen = [c for c in range(len(tr.viewmats)) if c not in
              {tr.camera_index(it) for it in range(steps)}]
    assert unseen and float((got["embeds"][unseen] - embeds0[unseen]).abs().min()) > 0.0
    assert float(got["embeds_m"][unseen].abs().max()) > 0.0


def _run(graph, steps=8, **kw):
    tr = _make(graph, **kw)
    assert (tr._graph is not None) == graph
    losses = [tr.step(it) for it in range(steps)]
    tr.sync()
    assert tr.graph_fallback is None, tr.graph_fallback
    out = dict(params={k: q.detach().clone() for k, q in tr.params.items()},
               exp_avg=[m.clone() for m in tr.opt.exp_avg],
               losses=torch.tensor([float(x.detach()) for x in losses]), tr=tr)
    if tr.app_opt:
        out["module"] = _module_state(tr)
    return out


def test_graph_trainer_tracks_eager():
    """Eight steps over the four cameras, the SH degree schedule live (a
    re-capture per degree), kernel nodes only."""
    a = _run(False, max_steps=100, sh_degree_interval=2)
    b = _run(True, max_steps=100, sh_degree_interval=2)
    g = b["tr"]._graph
    assert g.replays >= 8 and g.recaptures >= 4
    assert set(g.census) <= {"kernel", "empty"}, g.census
    assert a["tr"].app.step_count == b["tr"].app.step_count == 8
    torch.testing.assert_close(b["losses"], a["losses"], rtol=1e-4, atol=1e-6)
    assert len(set(b["losses"].tolist())) == 8
    for k in a["params"]:
        torch.testing.assert_close(b["params"][k], a["params"][k], rtol=1e-3, atol=1e-5)
    for x, y in zip(a["exp_avg"], b["exp_avg"]):
        torch.testing.assert_close(y, x, rtol=1e-2, atol=1e-6)
    for k in ("embeds", "head"):
        torch.testing.assert_close(b["module"][k], a["module"][k], rtol=1e-3, atol=1e-5)
    for k in ("embeds_m", "head_m"):
        torch.testing.assert_close(b["module"][k], a["module"][k], rtol=1e-2, atol=1e-6)
    b["tr"].release_graph()


def test_option_off_leaves_the_captured_step_unchanged():
    """Absent or off the node census is the same; on, the step holds the
    module's kernels instead of the SH ones and still kernels only."""
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    makers = [lambda: _prepare(Trainer(means, rgbs, vm, K, W, H, device=DEV, graph=True)),
              lambda: _make(True, app_opt=False), lambda: _make(True)]
    census = []
    for make in makers:
        tr = make()
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
    # camera centre (3), colours forward and backward, reduce + Adam; the
    # features / colors groups' Adam launch replaces the SH backward's
    assert census[2]["kernel"] > census[0]["kernel"], census


@pytest.mark.parametrize("strategy", ["default", "mcmc"])
def test_refine_boundary(strategy):
    if strategy == "default":
        from gsplat_hip.densify import DefaultStrategyConfig
        cfg = DefaultStrategyConfig(refine_start_iter=1, refine_every=3, reset_every=7)
    else:
        from gsplat_hip.mcmc import MCMCStrategyConfig
        cfg = MCMCStrategyConfig(refine_start_iter=1, refine_every=3,
                                 cap_max=int(1.2 * _trainer_scene()[0].shape[0]))
    out = _run(True, steps=8, strategy=cfg, max_steps=100)
    tr = out["tr"]
    n = tr.params["means"].shape[0]
    assert len(tr.refine_log) >= 2, tr.refine_log
    if strategy == "mcmc":  # 5 % sampled in at each refine, below the cap
        assert n > _trainer_scene()[0].shape[0]
    assert tr._graph.recaptures >= 2
    assert set(tr._graph.census) <= {"kernel", "empty"}, tr._graph.census
    assert tr.params["features"].shape == (n, 32) and tr.params["colors"].shape == (n, 3)
    moms = tr.moments()
    for k in ("features", "colors"):
        assert moms[k][0].shape == tr.params[k].shape == moms[k][1].shape
        assert torch.isfinite(tr.params[k]).all()
    assert torch.isfinite(out["losses"]).all() and torch.isfinite(out["params"]["means"]).all()
    assert tr.app.step_count == 8
    tr.release_graph()


def test_with_bilateral_grid_and_depth_loss():
    from test_gpu_trainer_depth_loss import _scene
    _, points, _ = _scene()
    kw = dict(bilateral_grid=True, depth_loss=True, depth_points=points, max_steps=100)
    a, b = _run(False, steps=6, **kw), _run(True, steps=6, **kw)
    assert set(b["tr"]._graph.census) <= {"kernel", "empty"}, b["tr"]._graph.census
    assert torch.isfinite(a["losses"]).all()
    torch.testing.assert_close(b["losses"], a["losses"], rtol=1e-4, atol=1e-6)
    for k in a["params"]:
        torch.testing.assert_close(b["params"][k], a["params"][k], rtol=1e-3, atol=1e-5)
    for k in ("embeds", "head"):
        torch.testing.assert_close(b["module"][k], a["module"][k], rtol=1e-3, atol=1e-5)
    assert a["tr"].bil.opt.step_count == b["tr"].bil.opt.step_count == 6
    b["tr"].release_graph()


def test_evaluate_renders_with_the_zero_embedding():
    from gsplat_hip import rasterization
    from gsplat_hip.losses import ssim_and_l1
    tr = _make()
    for it in range(2):
        tr.step(it)
    tr.sync()
    p = {k: v.detach() for k, v in tr.params.items()}
    psnrs, ssims, with_row = [], [], []
    for ci in range(len(tr.viewmats)):
        vm = tr.viewmats[ci:ci + 1]
        campos = torch.inverse(vm)[:, :3, 3]
        renders = []
        for e in (torch.zeros(1, 16, device=DEV), tr.app.embeds[ci:ci + 1]):
            colors = O.app_colors(p["features"], p["colors"], e, p["means"], campos,
                                  [t.detach() for t in tr.app.head], 3)
            renders.append(rasterization(
                p["means"], p["quats"], torch.exp(p["scales"]), torch.sigmoid(p["opacities"]),
                colors, vm, tr.Ks[ci:ci + 1], tr.width, tr.height, sh_degree=None, packed=False,
                near_plane=0.01, far_plane=1e10, radius_clip=0.0)[0].clamp(0.0, 1.0))
        gt = tr.targets[ci:ci + 1]
        psnrs.append(float(-10.0 * torch.log10(torch.mean((renders[0] - gt) ** 2))))
        ssims.append(float(ssim_and_l1(renders[0], gt)[0]))
        with_row.append(float(-10.0 * torch.log10(torch.mean((renders[1] - gt) ** 2))))
        with torch.no_grad():
            got = tr.render(ci)[0]
        torch.testing.assert_close(got.clamp(0.0, 1.0), renders[0], rtol=1e-4, atol=1e-5)
    ev = tr.evaluate()
    assert ev["num_images"] == 4
    assert abs(ev["psnr"] - sum(psnrs) / 4) < 1e-3, (ev, psnrs)
    assert abs(ev["ssim"] - sum(ssims) / 4) < 1e-4, (ev, ssims)
    # the embedding rows do change the render: the comparison can tell them apart
    assert abs(sum(with_row) / 4 - sum(psnrs) / 4) > 1e-2, (with_row, psnrs)
