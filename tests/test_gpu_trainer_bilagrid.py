"""GPU: the 3DGS trainer's bilateral grid (Trainer(bilateral_grid=True),
gsplat_hip.bilagrid_slice / bilagrid_tv_loss).

* one eager step against autograd of the torch composition
  (test_gpu_bilagrid's: grid_sample, matmul, index_select total variation) on
  the same render: the loss, and the grid optimizer's moments, which are
  linear and quadratic in the gradient (the parameter step itself is
  sign-like at step 1 and would hide errors);
* with the grid still identity the Gaussians' first step is the grid-off
  trainer's;
* the graph-replayed trainer tracks the eager one over 8 steps, all cameras;
* with the option off the captured step is the parent's;
* the configurations that do not support the grid refuse it."""

import os

import pytest
import torch

from test_gpu_bilagrid import _slice, _tv

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def _trainer_scene(n_cams=4, W=96, H=64, stride=32):
    """The garden crop's every 32nd point at 96 x 64: ~3,500 Gaussians."""
    from gsplat_hip.train_step import camera_pool, load_garden_scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(root, "tests", "golden", "garden_scene.npz"), scene_grid=1)
    means, rgbs = means[::stride].contiguous(), rgbs[::stride].contiguous()
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=n_cams)
    return means, rgbs, vm, K, W, H


def _perturb(tr, amount=0.05):
    """Move the grids off the identity, identically for every trainer."""
    g = torch.Generator().manual_seed(11)
    tr.bil.grids.data.add_((amount * torch.randn(tr.bil.grids.shape, generator=g)).to(DEV))


def test_eager_step_matches_autograd_of_the_composition():
    from gsplat_hip.losses import l1_ssim_loss
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    it = 1
    tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, bilateral_grid=True, max_steps=100)
    assert tr.bil.grids.shape == (4, 12, 8, 16, 16)
    _perturb(tr)
    grids0 = tr.bil.grids.detach().clone()
    ci = tr.camera_index(it)
    with torch.no_grad():  # the step's render (evaluate()'s: without the grid)
        colors = tr.render(ci, tr.sh_degree_at(it))[0].clone()
    loss = float(tr.step(it).detach())
    tr.sync()
    assert tr.bil.opt.step_count == 1

    def compose(dtype, dev):
        g = grids0.to(dev, dtype).requires_grad_(True)
        out = _slice(g, colors.to(dev, dtype), torch.tensor([ci], device=dev))
        leaf = out.detach().float().to(DEV).requires_grad_(True)
        photo = l1_ssim_loss(leaf, tr.targets[ci:ci + 1], tr.ssim_lambda)
        photo.backward()
        tv = _tv(g)
        (10.0 * tv).backward(retain_graph=True)
        out.backward(leaf.grad.to(dev, dtype))
        return float(photo.detach()) + 10.0 * float(tv.detach()), g.grad.double().cpu()

    want_loss, g64 = compose(torch.float64, "cpu")
    _, g32 = compose(torch.float32, DEV)
    e32 = float((g32 - g64).abs().max())
    top = float(g64.abs().max())
    bar = max(1e-4 * top, 4.0 * e32)
    assert abs(loss - want_loss) <= 1e-4 * abs(want_loss), (loss, want_loss)
    m, v = (t.double().cpu() for t in tr.moments()["bil_grids"])
    err_m = float((m - 0.1 * g64).abs().max())
    err_v = float((v - 0.001 * g64 ** 2).abs().max())
    print(f"grid gradient: max {top:.3e}, e32 {e32:.3e}, bar {bar:.3e}; exp_avg err "
          f"{err_m:.3e} (bar {0.1 * bar:.3e}), exp_avg_sq err {err_v:.3e} "
          f"(bar {0.001 * 2 * top * bar:.3e})")
    assert top > 0 and float(g64[ci].abs().max()) > 100.0 * bar
    assert err_m <= 0.1 * bar, (err_m, bar)
    assert err_v <= 0.001 * 2.0 * top * bar, (err_v, top, bar)
    # the grids moved, the moments survive a reload (checkpoint / refine path)
    assert float((tr.bil.grids.detach() - grids0).abs().max()) > 0
    moms = tr.moments()
    tr._load_moments(moms)
    assert tr.bil.opt.exp_avg[0] is moms["bil_grids"][0]
    assert set(moms) == set(tr.params) | {"bil_grids"}


def test_identity_grid_leaves_the_first_gaussian_step_unchanged():
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    out = []
    for kw in ({}, {}, dict(bilateral_grid=True)):
        tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, max_steps=100, **kw)
        tr.step(0)
        tr.sync()
        out.append(({k: p.detach().clone() for k, p in tr.params.items()},
                    [m.clone() for m in tr.opt.exp_avg]))
    off, off2, on = out
    for k in off[0]:
        torch.testing.assert_close(on[0][k], off[0][k], rtol=1e-3, atol=1e-5)
    for k, a, a2, b in zip(off[0], off[1], off2[1], on[1]):
        spread = float((a2 - a).abs().max())
        err = float((b - a).abs().max())
        bar = max(4.0 * spread, 1e-5 * float(a.abs().max()))
        print(f"{k}: exp_avg on-vs-off {err:.3e}, off run-to-run {spread:.3e}, bar {bar:.3e}")
        assert err <= bar, (k, err, bar)


def test_graph_trainer_tracks_eager():
    """test_graph_trainer_tracks_eager's twin with the grid on: 8 steps over
    the 4 cameras, the warm-up schedule live (max_steps), the grids off the
    identity so every image's slab carries signal."""
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    out = {}
    for run in ("eager", "graph"):
        graph = run == "graph"
        tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, graph=graph, max_steps=100,
                     bilateral_grid=True)
        assert (tr._graph is not None) == graph
        _perturb(tr)
        start = tr.bil.grids.detach().clone()
        losses = [tr.step(it) for it in range(8)]
        tr.sync()
        assert tr.graph_fallback is None, tr.graph_fallback
        assert sorted({tr.camera_index(it) for it in range(8)}) == [0, 1, 2, 3]
        out[run] = ({k: p.detach().clone() for k, p in tr.params.items()},
                    [m.clone() for m in tr.opt.exp_avg], tr.opt.step_count,
                    tr.bil.grids.detach().clone(), tr.bil.opt.exp_avg[0].clone(),
                    [float(x) for x in losses], tr.bil.opt.step_count)
        assert all(float((out[run][3][n] - start[n]).abs().max()) > 0 for n in range(4))
        if graph:
            g = tr._graph
            assert g.replays >= 8
            assert set(g.census) <= {"kernel", "empty"}, g.census
    a, b = out["eager"], out["graph"]
    assert a[2] == b[2] == 8 and a[6] == b[6] == 8
    torch.testing.assert_close(torch.tensor(b[5]), torch.tensor(a[5]), rtol=1e-4, atol=1e-6)
    assert len(set(b[5])) == 8, b[5]
    for k in a[0]:
        torch.testing.assert_close(b[0][k], a[0][k], rtol=1e-3, atol=1e-5)
    for x, y in zip(a[1], b[1]):
        torch.testing.assert_close(y, x, rtol=1e-2, atol=1e-6)
    for n in range(4):
        torch.testing.assert_close(b[3][n], a[3][n], rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(b[4], a[4], rtol=1e-2, atol=1e-6)


def test_option_off_is_the_parent_step():
    """Without the option (absent or False) the captured step has the same
    node census; with it, more kernels and still kernels only."""
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    census = []
    for kw in ({}, dict(bilateral_grid=False), dict(bilateral_grid=True)):
        tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, graph=True, max_steps=100, **kw)
        for it in range(2):
            tr.step(it)
        tr.sync()
        assert tr.graph_fallback is None, tr.graph_fallback
        assert (tr.bil is not None) == bool(kw.get("bilateral_grid"))
        census.append(dict(tr._graph.census))
        tr.release_graph()
    assert census[0] == census[1], census
    assert set(census[2]) <= {"kernel", "empty"}, census[2]
    # slice, tv (2), tv backward, slice backward (2), the loss sum, the grid Adam
    assert census[2]["kernel"] >= census[0]["kernel"] + 8, census


def test_refusals():
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    for kw in (dict(model="2dgs"), dict(packed=True), dict(packed=True, sparse_grad=True),
               dict(visible_adam=True), dict(sharded_optimizer=True), dict(world_size=2),
               dict(gaussian_shard=True, world_size=2)):
        with pytest.raises(NotImplementedError):
            Trainer(means, rgbs, vm, K, W, H, device=DEV, bilateral_grid=True, **kw)
    with pytest.raises(ValueError):
        Trainer(means, rgbs, vm, K, W, H, device=DEV, bilateral_grid=True,
                bilateral_grid_shape=(16, 16, 1))
