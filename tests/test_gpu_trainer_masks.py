"""GPU: Trainer(masks=..., random_bkgd=True) -- the render zeroed outside each
image's mask and put over a per-step random colour inside the fused loss
kernel; eager and graph-replayed, against the float64 oracle
(tests/masked_loss_oracle.py) and the unfused torch composition.

The scene: the garden crop at 64 x 64, ~2,000 Gaussians made a few pixels
wide, four cameras (test_gpu_trainer_depth_loss's); a disc mask of another
radius per image, one image all True.

Bars: the first-step loss within ten times the float32 torch composition's
own error against the oracle, floored by rtol 1e-4 / atol 1e-5 of the loss;
one-step gradients within 10 x the larger of the unfused path's run-to-run
spread and 1e-5 max|g| (test_gpu_trainer_depth_loss's rule); graph against
eager with that test's tolerances for the same scene (parameters rtol 1e-3 /
atol 1e-5, first moments rtol 1e-2 / atol 1e-6, losses rtol 1e-4 / atol 1e-6).

Measured on an MI355X (profiles/masked_loss/parity.txt): see MEASURED below."""

import os

import pytest
import torch

import masked_loss_oracle as O
from test_gpu_trainer_depth_loss import _fatten
from test_gpu_trainer_pose import _trainer_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"

MEASURED = """first-step loss fused: masks 0.503560483 against
0.503560454 (err 2.9e-08, the float32 composition's own 3.0e-08, bar 6.0e-05),
random_bkgd err 1.6e-08, both 4.4e-09; the plain trainer's loss 0.465055.
Means gradient max|g| 1.373e-02, the alpha path's share 4.0e-03, unfused
run-to-run spread 4.7e-10, fused against unfused 3.0e-09, bar 1.4e-06;
opacities 2.390e-04, 1.4e-04, 7.3e-12, 8.2e-11, bar 2.4e-08.  Half-plane mask:
425 Gaussians under it with first moments exactly 0, 828 with a non-zero one.
Graph against eager after six steps: parameters within 7.9e-06 (the
opacities), first moments within 2.0e-08 (pose_opt 1.9e-06 / 7.3e-10, app_opt
1.5e-06 / 4.5e-10); captured step 40 kernel nodes with the options and
without (pose_opt 42, app_opt 46).  Resume: |B-A| at most 1.5e-08 (quats),
uninterrupted runs' own spread up to 1.2e-07."""


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


_CACHE = {}


def _scene():
    if "scene" not in _CACHE:
        scene = _trainer_scene()
        W, H = scene[4], scene[5]
        masks = torch.cat([O.disc_mask(1, H, W, 0.45), O.disc_mask(1, H, W, 0.35),
                           torch.ones(1, H, W, dtype=torch.bool), O.disc_mask(1, H, W, 0.25)])
        _CACHE["scene"] = (scene, masks)
    return _CACHE["scene"]


def _make(graph=False, **kw):
    from gsplat_hip.train_step import Trainer
    (means, rgbs, vm, K, W, H), _ = _scene()
    kw.setdefault("max_steps", 100)
    return _fatten(Trainer(means, rgbs, vm, K, W, H, device=DEV, graph=graph, **kw))


def _opts(which):
    _, masks = _scene()
    return {"masks": dict(masks=masks), "bkgd": dict(random_bkgd=True),
            "both": dict(masks=masks, random_bkgd=True)}[which]


def _expected_first_loss(tr, it=0):
    """(the oracle's loss of step `it` on tr's plain render, the float32 torch
    composition's own error against it)."""
    from gsplat_hip.losses import compose_masked
    from gsplat_hip.train_step import ssim
    ci = tr.camera_index(it)
    with torch.no_grad():
        colors, alphas, _ = tr.render(ci, tr.sh_degree_at(it))
    m = None if tr.masks is None else tr.masks[ci:ci + 1].bool()
    b = torch.tensor([tr.bkgd_at(it)], dtype=torch.float32, device=DEV) if tr.random_bkgd else None
    y = tr.targets[ci:ci + 1]
    lam = tr.ssim_lambda
    f64 = lambda t: None if t is None else t.double().cpu()  # noqa: E731
    want = float(O.loss_of(O.compose(f64(colors), None if m is None else m.cpu(), f64(alphas),
                                     f64(b)), f64(y), lam))
    with torch.no_grad():
        x = compose_masked(colors, m, alphas, b)
        l32 = (x - y).abs().mean() * (1 - lam) + (1 - ssim(x.permute(0, 3, 1, 2),
                                                           y.permute(0, 3, 1, 2))) * lam
    return want, abs(float(l32) - want)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("which", ["masks", "bkgd", "both"])
def test_first_step_loss_is_the_oracles(which, fused):
    tr = _make(fused=fused, **_opts(which))
    want, own = _expected_first_loss(tr)
    plain, _ = _expected_first_loss(_make())
    loss = float(tr.step(0).detach())
    tr.sync()
    bar = max(10.0 * own, 1e-4 * abs(want) + 1e-5)
    print(f"{which} fused={fused}: first-step loss {loss!r}, oracle {want!r} (plain trainer's "
          f"{plain!r}), err {abs(loss - want):.3e}, fp32 composition's own error {own:.3e}, "
          f"bar {bar:.3e}")
    assert abs(want - plain) > 100.0 * bar  # the options change the loss: a no-op build fails
    assert abs(loss - want) <= bar, (loss, want, bar)


def _unfused_grads(tr, ci, it, alpha_path=True):
    """d loss / d(means, raw opacities) through rasterization(), the torch
    composition and the existing loss."""
    from gsplat_hip import rasterization
    from gsplat_hip.losses import compose_masked, l1_ssim_loss
    p = tr.params
    means = p["means"].detach().clone().requires_grad_(True)
    opac = p["opacities"].detach().clone().requires_grad_(True)
    rc, ra, _ = rasterization(
        means, p["quats"].detach(), torch.exp(p["scales"].detach()), torch.sigmoid(opac),
        (p["sh0"].detach(), p["shN"].detach()), tr.viewmats[ci:ci + 1], tr.Ks[ci:ci + 1],
        tr.width, tr.height, sh_degree=tr.sh_degree_at(it), packed=False, near_plane=0.01,
        far_plane=1e10, radius_clip=0.0)
    b = torch.tensor([tr.bkgd_at(it)], dtype=torch.float32, device=DEV)
    x = compose_masked(rc, tr.masks[ci:ci + 1].bool(), ra if alpha_path else ra.detach(), b)
    loss = l1_ssim_loss(x, tr.targets[ci:ci + 1], tr.ssim_lambda)
    gm, go = torch.autograd.grad(loss, (means, opac))
    return gm.double().cpu(), go.double().cpu()


def test_one_step_gradients_match_the_unfused_composition():
    """After step 1 from zero state exp_avg / (1 - beta1) is the gradient.  The
    opacities are the parameter the alpha gradient reaches most directly: the
    unfused gradient with the alpha path cut differs by more than the bar."""
    it = 0
    tr = _make(**_opts("both"))
    ci = tr.camera_index(it)
    assert not bool(tr.masks[ci].bool().all())
    refs = [_unfused_grads(tr, ci, it) for _ in range(3)]
    cut = _unfused_grads(tr, ci, it, alpha_path=False)
    tr.step(it)
    tr.sync()
    mom = tr.moments()
    for k, name in enumerate(("means", "opacities")):
        g = mom[name][0].double().cpu() / 0.1
        ref = refs[0][k]
        spread = max(float((r[k] - ref).abs().max()) for r in refs[1:])
        top = float(ref.abs().max())
        bar = 10.0 * max(spread, 1e-5 * top)
        err = float((g.reshape(ref.shape) - ref).abs().max())
        part = float((ref - cut[k]).abs().max())
        print(f"{name} gradient: max|g| {top:.6e}, the alpha path's share max {part:.6e}, "
              f"unfused run-to-run spread {spread:.3e}, fused-vs-unfused err {err:.3e}, "
              f"bar {bar:.3e}")
        assert part > bar, (name, part, bar)
        assert err <= bar, (name, err, bar)


def test_gaussians_under_the_mask_get_no_gradient():
    """A half-plane mask on a tile border (columns < 32 masked), no background:
    a Gaussian whose footprint means2d +- radii lies in masked columns touches
    masked tiles only, and its first moments stay exactly 0."""
    (_, _, vm, _, W, H), _ = _scene()
    masks = torch.ones(len(vm), H, W, dtype=torch.bool)
    masks[:, :, :32] = False
    tr = _make(masks=masks)
    tr.step(0)
    tr.sync()
    meta = tr.last_meta
    x = meta["means2d"][0, :, 0].detach()
    radii = meta["radii"][0]
    rx = (radii[:, 0] if radii.dim() == 2 else radii).float()
    vis = (radii > 0).all(-1) if radii.dim() == 2 else radii > 0
    dead = vis & (x + rx + 1 < 32)
    mom = tr.moments()
    live = torch.zeros_like(dead)
    for k in ("sh0", "means", "opacities"):
        m = mom[k][0].reshape(dead.shape[0], -1)
        assert float(m[dead].abs().max()) == 0.0, k
        live |= (m != 0).any(-1)
    print(f"dead Gaussians {int(dead.sum())}, with a non-zero moment {int(live.sum())}")
    assert int(dead.sum()) >= 20 and int(live.sum()) >= 20
    assert not bool((live & dead).any())


def _run(graph, steps=6, **kw):
    tr = _make(graph, **kw)
    assert (tr._graph is not None) == graph
    losses = [tr.step(it) for it in range(steps)]
    tr.sync()
    assert tr.graph_fallback is None, tr.graph_fallback
    return dict(params={k: p.detach().clone() for k, p in tr.params.items()},
                exp_avg=[m.clone() for m in tr.opt.exp_avg],
                losses=torch.tensor([float(x.detach()) for x in losses]), tr=tr)


@pytest.mark.parametrize("variant", ["plain", "pose_opt", "app_opt"])
def test_graph_trainer_tracks_eager(variant):
    kw = dict({"plain": {}, "pose_opt": dict(pose_opt=True, pose_opt_lr=1e-3),
               "app_opt": dict(app_opt=True)}[variant], **_opts("both"))
    a, b = _run(False, **kw), _run(True, **kw)
    g = b["tr"]._graph
    assert g.replays >= 6
    assert set(g.census) <= {"kernel", "empty"}, g.census
    print(f"{variant}: captured step with masks and random_bkgd: {g.census}")
    assert sorted({b["tr"].camera_index(it) for it in range(6)}) == [0, 1, 2, 3]
    for k in a["params"]:
        print(f"{variant} {k}: graph-vs-eager max diff "
              f"{float((b['params'][k] - a['params'][k]).abs().max()):.3e}, max "
              f"{float(a['params'][k].abs().max()):.3e}")
    for x, y in zip(a["exp_avg"], b["exp_avg"]):
        print(f"{variant} exp_avg {tuple(x.shape)}: graph-vs-eager max diff "
              f"{float((y - x).abs().max()):.3e}, max {float(x.abs().max()):.3e}")
    print(f"{variant} losses eager {a['losses'].tolist()} graph {b['losses'].tolist()}")
    torch.testing.assert_close(b["losses"], a["losses"], rtol=1e-4, atol=1e-6)
    for k in a["params"]:
        torch.testing.assert_close(b["params"][k], a["params"][k], rtol=1e-3, atol=1e-5)
    for x, y in zip(a["exp_avg"], b["exp_avg"]):
        torch.testing.assert_close(y, x, rtol=1e-2, atol=1e-6)
    b["tr"].release_graph()


def test_options_off_leave_the_captured_step_unchanged():
    census = []
    for kw in ({}, dict(masks=None, random_bkgd=False), _opts("both")):
        tr = _make(True, **kw)
        for it in range(2):
            tr.step(it)
        tr.sync()
        assert tr.graph_fallback is None, tr.graph_fallback
        census.append(dict(tr._graph.census))
        tr.release_graph()
    print("census absent / off / on:", census)
    assert census[0] == census[1], census
    for c in census:
        assert set(c) <= {"kernel", "empty"}, c


def test_evaluate_zeroes_the_render_outside_the_masks():
    from gsplat_hip.losses import ssim_and_l1
    (_, _, vm, K, _, _), masks = _scene()
    tr = _make(**_opts("both"))
    got = tr.evaluate()
    psnr, ssim = [], []
    with torch.no_grad():
        for i in range(len(vm)):
            colors, _, _ = tr.render(i)
            colors = torch.where(masks[i:i + 1, ..., None].to(DEV), colors,
                                 torch.zeros((), device=DEV)).clamp(0.0, 1.0)
            gt = tr.targets[i:i + 1]
            psnr.append(float(-10.0 * torch.log10(torch.mean((colors - gt) ** 2))))
            ssim.append(float(ssim_and_l1(colors, gt)[0]))
    want = {"psnr": sum(psnr) / len(psnr), "ssim": sum(ssim) / len(ssim)}
    plain = _make().evaluate()
    print(f"evaluate: {got}, manual {want}, without masks {plain}")
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), (k, got, want)
        assert abs(got[k] - plain[k]) > 1e-4 * abs(plain[k]), (k, got, plain)
    explicit = _make().evaluate(viewmats=vm, Ks=K, images=tr.targets, masks=masks)
    for k in want:
        assert abs(explicit[k] - want[k]) <= 1e-6 * abs(want[k]), (k, explicit, want)


def test_resume_equals_not_stopping(tmp_path):
    """Three steps, save, load into a fresh trainer of another seed, four more:
    as close to the uninterrupted run as two uninterrupted runs are to each
    other (test_gpu_checkpoint's bar: max(4 x spread, 1e-5 max|A|))."""
    from gsplat_hip.train_step import Trainer
    from test_gpu_checkpoint import H, W, scalars, scene, tensors
    means, rgbs, vms, Ks, _ = scene()
    masks = torch.cat([O.disc_mask(1, H, W, f) for f in (0.45, 0.4, 0.3, 0.35)])

    def make(seed=42, **kw):
        kw = dict(dict(masks=masks, random_bkgd=True), **kw)
        return Trainer(means, rgbs, vms, Ks, W, H, device=DEV, seed=seed, max_steps=100, **kw)

    steps, half = 7, 3
    full = []
    for _ in range(2):
        tr = make()
        for it in range(steps):
            tr.step(it)
        full.append((tensors(tr), scalars(tr)))
    saver = make()
    for it in range(half):
        saver.step(it)
    path = os.path.join(str(tmp_path), f"ckpt_{half - 1}_rank0.pt")
    saver.save_checkpoint(path, half - 1)
    fresh = make(seed=7)
    assert fresh.bkgd_at(3) != saver.bkgd_at(3)
    assert fresh.load_checkpoint(path, resume=True) == half - 1
    assert fresh.bkgd_at(3) == saver.bkgd_at(3)
    for it in range(half, steps):
        fresh.step(it)
    tb, sb = tensors(fresh), scalars(fresh)
    (ta, sa), (ta2, _) = full
    assert sa["adam_step"] == sb["adam_step"] == steps
    bad = []
    for k in ta:
        a, a2, b = ta[k].double(), ta2[k].double(), tb[k].double()
        amax, spread = float(a.abs().max()), float((a2 - a).abs().max())
        err = float((b - a).abs().max())
        bar = max(4.0 * spread, 1e-5 * amax)
        print(f"{k:24s} |B-A| {err:.3e}  |A'-A| {spread:.3e}  max|A| {amax:.3e}  bar {bar:.3e}")
        if err > bar:
            bad.append((k, err, spread, amax))
    assert not bad, bad
    with pytest.raises(ValueError, match="random_bkgd"):
        make(seed=7, random_bkgd=False).load_checkpoint(path, resume=True)


def test_refusals_name_both_options():
    (means, rgbs, vm, K, W, H), masks = _scene()
    from gsplat_hip.train_step import Trainer
    for kw, word in ((dict(bilateral_grid=True), "bilateral_grid"),
                     (dict(depth_loss=True), "depth_loss"), (dict(model="2dgs"), "model='2dgs'"),
                     (dict(packed=True), "packed")):
        with pytest.raises(NotImplementedError, match="masks.*" + word):
            Trainer(means, rgbs, vm, K, W, H, device=DEV, masks=masks, **kw)
        with pytest.raises(NotImplementedError, match="random_bkgd.*" + word):
            Trainer(means, rgbs, vm, K, W, H, device=DEV, random_bkgd=True, **kw)
