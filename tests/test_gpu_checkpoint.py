"""GPU: Trainer.save_checkpoint / load_checkpoint / load_splats / save_ply on a
small scene (1,500 Gaussians, 128 x 80, 4 cameras).

Exact restore: a trainer built with another seed and loaded with resume=True
holds the saving trainer's state bit for bit.

Resume equals not stopping: run A is 8 uninterrupted steps, A' the same again
(together they measure the run-to-run spread of the step itself: the
rasterizer backward's float atomics; the code under test plays no part in
it), B is 4 steps, save, a fresh trainer of another seed, load, 4 steps.  Per
tensor  max|B - A| <= max(4 max|A' - A|, 1e-5 max|A|), the bar
tests/test_gpu_graph.py applies to eager against replayed steps; the Gaussian
counts of A, A' and B must be equal.  Every figure is printed before it is
asserted.  The runs of a configuration are made once and shared."""

import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, W, H, N_CAM = 1500, 128, 80, 4
STEPS, HALF = 8, 4
CONFIGS = ("plain", "default", "mcmc", "graph", "bil_pose_depth", "app_opt", "2dgs")


@functools.lru_cache(maxsize=None)
def scene():
    g = torch.Generator().manual_seed(11)
    means = (torch.rand(N, 3, generator=g) - 0.5) * torch.tensor([6.0, 4.0, 4.0])
    rgbs = torch.rand(N, 3, generator=g)
    vms = []
    for c in range(N_CAM):  # on a circle of radius 2.5 around the box, 0.3 rad apart
        a = 0.3 * (c - 1)
        eye = torch.tensor([2.5 * math.sin(a), 0.3 * c, -2.5 * math.cos(a)])
        fwd = torch.nn.functional.normalize(-eye, dim=0)
        right = torch.nn.functional.normalize(
            torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), fwd), dim=0)
        up = torch.linalg.cross(fwd, right)
        R = torch.stack([right, up, fwd])
        vm = torch.eye(4)
        vm[:3, :3] = R
        vm[:3, 3] = -R @ eye
        vms.append(vm)
    Ks = torch.tensor([[90.0, 0, W / 2], [0, 90.0, H / 2], [0, 0, 1]]).repeat(N_CAM, 1, 1)
    depth = []
    for c in range(N_CAM):
        xy = torch.rand(120 + 10 * c, 2, generator=g) * torch.tensor([W - 1.001, H - 1.001])
        depth.append((xy, torch.rand(len(xy), generator=g) * 3.0 + 1.0))
    return means, rgbs, torch.stack(vms), Ks, depth


def options(config):
    from gsplat_hip.densify import DefaultStrategyConfig
    from gsplat_hip.mcmc import MCMCStrategyConfig
    depth = scene()[4]
    return {
        "plain": {},
        # refines after steps 2, 4, 6, opacity resets after 0, 3, 6: one refine
        # and a reset before the save (after step 3), refines after it.  The
        # reset at step 0 puts every opacity at 0.01, which scales the 2D
        # gradients by about 0.02: grow_grad2d is lowered by as much, so the
        # refines after the save still grow; the screen radii are tracked
        "default": dict(strategy=DefaultStrategyConfig(refine_start_iter=0, refine_every=2,
                                                       reset_every=3, grow_grad2d=2e-6,
                                                       refine_scale2d_stop_iter=100)),
        # refines after steps 2, 4, 6.  min_opacity 0.2: a fifth of the
        # Gaussians start dead, and a relocated pair whose source was below
        # 0.36 is dead again at the next refine: relocations on both sides
        "mcmc": dict(strategy=MCMCStrategyConfig(cap_max=2000, refine_start_iter=0,
                                                 refine_every=2, min_opacity=0.2)),
        "graph": dict(graph=True),
        "bil_pose_depth": dict(bilateral_grid=True, pose_opt=True, pose_opt_lr=1e-3,
                               pose_noise=0.01, depth_loss=True, depth_points=depth),
        "app_opt": dict(app_opt=True),
        "2dgs": dict(model="2dgs"),
    }[config]


def make(config, seed=42):
    from gsplat_hip.train_step import Trainer
    means, rgbs, vms, Ks, _ = scene()
    tr = Trainer(means, rgbs, vms, Ks, W, H, device=DEV, seed=seed, max_steps=100,
                 **options(config))
    assert (tr._graph is not None) == (config == "graph")
    return tr


def tensors(tr):
    """Every tensor the next step reads, by name."""
    tr.sync()
    out = {"param." + k: p.detach() for k, p in tr.params.items()}
    for k, (m, v) in tr.moments().items():
        out["exp_avg." + k], out["exp_avg_sq." + k] = m, v
    out["grad2d"], out["count"] = tr.grad2d, tr.count
    if tr.radii2d is not None:
        out["radii2d"] = tr.radii2d
    if tr.bilateral_grid:
        out["bil_grids"] = tr.bil.grids.detach()
    if tr.pose_opt:
        out["pose_embeds"] = tr.pose.embeds
    if tr.pose_active and tr.pose.noise is not None:
        out["pose_noise_table"] = tr.pose.noise
    if tr.app_opt:
        out["app_embeds"], out["app_head"] = tr.app.embeds, tr.app.flat
    return {k: v.detach().clone() for k, v in out.items()}


def scalars(tr):
    tr.sync()
    return {"adam_step": tr.opt.step_count,
            "side_steps": {so.name: so.step_count for so in tr.side_opts},
            "refine_log": [tuple(r) for r in tr.refine_log],
            "rng": tr.rng.get_state().clone(), "noise_seed": tr._noise_seed,
            "split": (tr.split_div, tr.split_threshold, getattr(tr, "split_launch", None),
                      tr._split_tuned)}


def same_scalars(a, b):
    assert torch.equal(a.pop("rng"), b.pop("rng"))
    assert a == b, (a, b)


@functools.lru_cache(maxsize=None)
def runs(config):
    """A, A', the saver's state at the save, the fresh trainer's right after
    the load, and B's at the end; evaluate() of the saver (twice) and of the
    loaded trainer."""
    import tempfile
    out = {}
    for name in ("A", "A2"):
        tr = make(config)
        for it in range(STEPS):
            tr.step(it)
        out[name] = (tensors(tr), scalars(tr))
        assert tr.graph_fallback is None, tr.graph_fallback
        tr.release_graph()
        del tr
    saver = make(config)
    for it in range(HALF):
        saver.step(it)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"ckpt_{HALF - 1}_rank0.pt")
        gen = saver._param_gen
        saver.save_checkpoint(path, HALF - 1)
        assert saver._param_gen == gen  # the saving trainer is untouched
        out["saved"] = (tensors(saver), scalars(saver))
        out["eval_saved"] = (saver.evaluate(), saver.evaluate())
        fresh = make(config, seed=7)
        assert not torch.equal(fresh.params["quats"], saver.params["quats"])
        step = fresh.load_checkpoint(path, resume=True)
    assert step == HALF - 1
    out["loaded"] = (tensors(fresh), scalars(fresh))
    out["eval_loaded"] = fresh.evaluate()
    saver.release_graph()
    del saver
    for it in range(step + 1, STEPS):
        fresh.step(it)
    out["B"] = (tensors(fresh), scalars(fresh))
    assert fresh.graph_fallback is None, fresh.graph_fallback
    if config == "graph":
        assert fresh._graph is not None and fresh._graph.replays >= STEPS - HALF
    fresh.release_graph()
    return out


@pytest.mark.parametrize("config", CONFIGS)
def test_exact_restore(config):
    r = runs(config)
    (ta, sa), (tb, sb) = r["saved"], r["loaded"]
    assert set(ta) == set(tb)
    for k in ta:
        assert ta[k].shape == tb[k].shape and ta[k].dtype == tb[k].dtype, k
        assert torch.equal(ta[k].view(torch.int32) if ta[k].dtype == torch.float32 else ta[k],
                           tb[k].view(torch.int32) if tb[k].dtype == torch.float32 else tb[k]), k
    same_scalars(dict(sa), dict(sb))
    # evaluate(): as close as two calls on the saving trainer are, with a floor
    # of one float32 rounding of the metric (it is a float32 mean)
    (e1, e2), eb = r["eval_saved"], r["eval_loaded"]
    for k in ("psnr", "ssim"):
        spread, err = abs(e2[k] - e1[k]), abs(eb[k] - e1[k])
        print(f"{config} evaluate {k}: loaded-vs-saved {err:.3e}, two calls {spread:.3e}")
        assert err <= max(spread, 2.0 ** -23 * abs(e1[k])), (k, e1[k], e2[k], eb[k])


@pytest.mark.parametrize("config", CONFIGS)
def test_resume_equals_not_stopping(config):
    r = runs(config)
    (ta, sa), (ta2, sa2), (tb, sb) = r["A"], r["A2"], r["B"]
    n_a, n_a2, n_b = (t["param.means"].shape[0] for t in (ta, ta2, tb))
    print(f"{config}: Gaussians A {n_a} A' {n_a2} B {n_b}; refines {sa['refine_log']}")
    assert n_a == n_a2, (n_a, n_a2)
    assert n_b == n_a, (n_b, n_a)
    if config == "default":  # one refine and a reset before the save, refines after
        assert [x[0] for x in sa["refine_log"]] == [2, 4, 6]
        assert any(x[1] + x[2] + x[3] > 0 for x in sa["refine_log"][1:]), sa["refine_log"]
    if config == "mcmc":  # a relocation and an addition on each side of the save
        assert [x[0] for x in sa["refine_log"]] == [2, 4, 6]
        assert all(x[1] > 0 and x[2] > 0 for x in sa["refine_log"]), sa["refine_log"]
    assert sa["adam_step"] == sb["adam_step"] == STEPS
    assert sa["side_steps"] == sb["side_steps"]
    assert [x[0] for x in sb["refine_log"]] == [x[0] for x in sa["refine_log"]]
    bad = []
    for k in ta:
        a, a2, b = ta[k].double(), ta2[k].double(), tb[k].double()
        amax = float(a.abs().max()) if a.numel() else 0.0
        spread = float((a2 - a).abs().max()) if a.numel() else 0.0
        err = float((b - a).abs().max()) if a.numel() else 0.0
        bar = max(4.0 * spread, 1e-5 * amax)
        print(f"{config} {k:24s} |B-A| {err:.3e}  |A'-A| {spread:.3e}  max|A| {amax:.3e}  "
              f"bar {bar:.3e}")
        if err > bar:
            bad.append((k, err, spread, amax))
    assert not bad, bad


def test_reference_format_files_load(tmp_path):
    r = runs("plain")
    saver = make("plain")
    for it in range(HALF):
        saver.step(it)
    path = str(tmp_path / "full.pt")
    saver.save_checkpoint(path, HALF - 1)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    del ck["gsplat_hip"]
    half = N // 2
    pa, pb = str(tmp_path / "ckpt_3_rank0.pt"), str(tmp_path / "ckpt_3_rank1.pt")
    torch.save({"step": ck["step"], "splats": {k: v[:half].clone()
                                               for k, v in ck["splats"].items()}}, pa)
    torch.save({"step": ck["step"], "splats": {k: v[half:].clone()
                                               for k, v in ck["splats"].items()}}, pb)
    fresh = make("plain", seed=7)
    fresh.step(0)  # moments and statistics to be cleared
    assert fresh.load_checkpoint([pa, pb], resume=False) == HALF - 1
    for k, p in saver.params.items():
        assert torch.equal(p.detach(), fresh.params[k].detach()), k
        assert all(not m.any() for m in fresh.moments()[k]), k
    assert fresh.opt.step_count == 0 and not fresh.grad2d.any() and not fresh.count.any()
    e1, e2, eb = saver.evaluate(), saver.evaluate(), fresh.evaluate()
    for k in ("psnr", "ssim"):
        assert abs(eb[k] - e1[k]) <= max(abs(e2[k] - e1[k]), 2.0 ** -23 * abs(e1[k])), k
    fresh.step(HALF)  # and it trains on from there
    # the state the run-sharing fixture saw at the save is this trainer's too
    assert r["saved"][1]["adam_step"] == saver.opt.step_count == HALF


def test_load_splats_from_a_ply(tmp_path):
    import gsplat_hip
    saver = make("plain")
    saver.step(0)
    path = str(tmp_path / "point_cloud_0.ply")
    n = saver.save_ply(path)
    assert n == N
    direct = str(tmp_path / "direct.ply")
    gsplat_hip.save_ply({k: p.detach() for k, p in saver.synced_params().items()}, direct)
    assert open(path, "rb").read() == open(direct, "rb").read()
    fresh = make("plain", seed=7)
    fresh.load_splats(gsplat_hip.load_ply(path, device=DEV))
    for k, p in saver.params.items():
        assert torch.equal(p.detach(), fresh.params[k].detach()), k
    assert fresh.opt.step_count == 0
    fresh.step(1)


def test_save_ply_bakes_the_appearance(tmp_path):
    """The f_dc columns against the torch composition of
    simple_trainer.py:756-763 in float64 (tests/app_oracle.py: the module at
    the zero embedding and zero direction, `+ colors`, sigmoid), under the rule
    of tests/test_gpu_app.py: within 4 x the float32 composition's own error,
    floor 1e-6 on the colours.  f_dc = (c - 0.5) / C0 scales a colour error by
    1 / C0 and adds one rounding of a value below 1.8, hence the floor
    1e-6 / C0 + 2^-23."""
    import app_oracle as O
    import gsplat_hip
    tr = make("app_opt")
    for it in range(HALF):
        tr.step(it)
    C0 = 0.2820947917738781
    p = {k: v.detach().cpu() for k, v in tr.synced_params().items()}
    head = [t.detach().cpu() for t in tr.app.head]
    for deg in (None, 1):
        path = str(tmp_path / f"app_{deg}.ply")
        assert tr.save_ply(path, sh_degree=deg) == N
        back = gsplat_hip.load_ply(path)
        assert back["shN"].shape == (N, 0, 3)
        for k in ("means", "scales", "quats", "opacities"):
            assert torch.equal(back[k], p[k]), k
        f_dc = back["sh0"][:, 0, :].double()
        ref = {}
        for dt in (torch.float64, torch.float32):
            c = O.app_colors(p["features"].to(dt), p["colors"].to(dt), None,
                             torch.zeros(N, 3, dtype=dt), torch.zeros(1, 3, dtype=dt),
                             [t.to(dt) for t in head], 3 if deg is None else deg)[0]
            ref[dt] = ((c - 0.5) / C0).double()
        e_h = float((f_dc - ref[torch.float64]).abs().max())
        e_r = float((ref[torch.float32] - ref[torch.float64]).abs().max())
        print(f"save_ply app_opt deg={deg}: f_dc hip {e_h:.3e} fp32 {e_r:.3e}")
        assert e_h <= max(4.0 * e_r, 1e-6 / C0 + 2.0 ** -23), (e_h, e_r)
    assert np.isfinite(f_dc.numpy()).all()
