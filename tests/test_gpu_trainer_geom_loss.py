"""GPU: the 2DGS trainer's normal-consistency and distortion terms
(Trainer(normal_loss=..., dist_loss=...), losses.geometry_loss_2dgs).

* one eager step against torch autograd of the public
  rasterization_2dgs(render_mode="RGB+D", distloss=True) outputs composed as
  examples/simple_trainer_2dgs.py composes them;
* the graph-replayed trainer tracks the eager one across both start
  iterations (three captures: colours only, normal term, both terms);
* the configurations that do not support the terms refuse them."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def _trainer_scene(n_cams=3, W=320, H=240, stride=8):
    """The garden crop's every 8th point at 320 x 240: 13,974 surfels."""
    from gsplat_hip.train_step import camera_pool, load_garden_scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(root, "tests", "golden", "garden_scene.npz"), scene_grid=1)
    means, rgbs = means[::stride].contiguous(), rgbs[::stride].contiguous()
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=n_cams)
    return means, rgbs, vm, K, W, H


NL, DL = 1.0, 10.0


def _truth(tr, params, it, terms):
    """Loss and parameter gradients of step `it` from the public surface and
    torch autograd, with or without the two geometry terms."""
    from gsplat_hip import rasterization_2dgs
    from gsplat_hip.losses import l1_ssim_loss
    p = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    ci = tr.camera_index(it)
    rc, ra, rn, rnd, rdist, _, _ = rasterization_2dgs(
        p["means"], p["quats"], torch.exp(p["scales"]), torch.sigmoid(p["opacities"]),
        torch.cat([p["sh0"], p["shN"]], 1), tr.viewmats[ci:ci + 1], tr.Ks[ci:ci + 1],
        tr.width, tr.height, sh_degree=tr.sh_degree_at(it), near_plane=0.01, far_plane=1e10,
        render_mode="RGB+D", distloss=True)
    loss = l1_ssim_loss(rc[..., :3], tr.targets[ci:ci + 1], tr.ssim_lambda)
    if terms:
        nd = rnd.reshape(rn.shape) * ra.detach()
        loss = loss + NL * (1.0 - (rn * nd).sum(-1)).mean() + DL * rdist.mean()
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {k: v.grad.detach().clone() for k, v in p.items()}


def test_eager_step_matches_autograd_of_the_composition():
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    it = 1
    runs = []
    for _ in range(2):  # two identical runs: the backward's float atomics' spread
        tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, model="2dgs", normal_loss=True,
                     dist_loss=True, normal_start_iter=0, dist_start_iter=0, normal_lambda=NL,
                     dist_lambda=DL, max_steps=100)
        assert tr.geometry_terms_at(it) == (NL, DL)
        init = {k: v.detach().clone() for k, v in tr.params.items()}
        loss = float(tr.step(it).detach())
        tr.sync()
        b1 = tr.opt.betas[0]
        runs.append((loss, {k: m.detach().clone() / (1.0 - b1)
                            for k, m in zip(tr.params, tr.opt.exp_avg)}, init))
    (loss_a, ga, init), (_, gb, _) = runs
    want_loss, want = _truth(tr, init, it, terms=True)
    _, plain = _truth(tr, init, it, terms=False)
    assert abs(loss_a - want_loss) <= 1e-4 * abs(want_loss), (loss_a, want_loss)
    for k in want:
        spread = float((ga[k] - gb[k]).abs().max())
        top = float(want[k].abs().max())
        bar = max(4.0 * spread, 1e-4 * top)
        err = float((ga[k] - want[k]).abs().max())
        moved = float((want[k] - plain[k]).abs().max())
        print(f"{k}: err {err:.3e} bar {bar:.3e} (spread {spread:.3e}, max|truth| {top:.3e}), "
              f"terms move the gradient by {moved:.3e}")
        assert err <= bar, (k, err, bar)
        if k in ("means", "quats", "scales"):
            # the comparison would not pass with the terms dropped
            assert moved > 100.0 * bar, (k, moved, bar)


def test_graph_trainer_tracks_eager_across_start_iterations():
    """test_graph_2dgs_trainer_tracks_eager's twin with both terms on, the
    normal term from step 3 (start 2) and the distortion term from step 4
    (start 3): the replayed run re-captures at each and never falls back."""
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    out = {}
    for run in ("eager", "eager2", "graph"):
        graph = run == "graph"
        tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, model="2dgs", graph=graph,
                     max_steps=100, normal_loss=True, dist_loss=True, normal_start_iter=2,
                     dist_start_iter=3)
        assert (tr._graph is not None) == graph
        losses = [tr.step(it) for it in range(6)]
        tr.sync()
        assert tr.graph_fallback is None, tr.graph_fallback
        out[run] = ({k: p.detach().clone() for k, p in tr.params.items()},
                    [m.clone() for m in tr.opt.exp_avg], tr.opt.step_count,
                    tr.grad2d.clone(), tr.count.clone(), [float(x) for x in losses])
        if graph:
            g = tr._graph
            assert g.replays >= 6
            assert set(g.census) <= {"kernel", "empty"}, g.census
            assert g.recaptures >= 3, g.recaptures
    a, a2, b = out["eager"], out["eager2"], out["graph"]
    assert a[2] == b[2] == 6
    torch.testing.assert_close(torch.tensor(b[5]), torch.tensor(a[5]), rtol=1e-4, atol=1e-6)
    assert len(set(b[5])) == 6, b[5]
    for k in a[0]:
        torch.testing.assert_close(b[0][k], a[0][k], rtol=1e-3, atol=1e-5)
    for x, y in zip(a[1], b[1]):
        torch.testing.assert_close(y, x, rtol=1e-2, atol=1e-6)
    torch.testing.assert_close(b[4], a[4], rtol=0, atol=0)
    spread = float((a2[3] - a[3]).abs().max())
    gmax = float(a[3].abs().max())
    err = (b[3] - a[3]).abs()
    bar = max(4.0 * spread, 1e-5 * gmax)
    print(f"grad2d: graph-vs-eager {float(err.max()):.3e}, eager run-to-run {spread:.3e}, "
          f"{int((err > bar).sum())} of {err.numel()} above {bar:.3e}")
    assert int((err > bar).sum()) <= max(2, err.numel() // 2000), (float(err.max()), spread)
    assert float(err.max()) <= 1e-3 * gmax, (float(err.max()), gmax)


def test_refusals():
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    for kw in (dict(normal_loss=True), dict(dist_loss=True)):
        with pytest.raises(ValueError):
            Trainer(means, rgbs, vm, K, W, H, device=DEV, model="3dgs", **kw)
        with pytest.raises(NotImplementedError):
            Trainer(means, rgbs, vm, K, W, H, device=DEV, packed=True, **kw)
        with pytest.raises(NotImplementedError):
            Trainer(means, rgbs, vm, K, W, H, device=DEV, model="2dgs", sharded_optimizer=True,
                    **kw)
