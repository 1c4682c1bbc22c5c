"""Time the sparse depth supervision at 1920x1080.

  op:   the depth term's kernel pair, forward + backward
        (gsplat_hip.depth_loss.table_depth_loss, csrc/depth_loss.hip: the
        RGB+D render's depth channel and the alphas read in place at the 4 M
        corners) against the torch composition of examples/simple_trainer.py
        (:647-664 with the RGB+ED render's cat and whole-image division, the
        slice / permute, F.grid_sample, where, F.l1_loss) on the same tensors,
        for M = 4,096 and 32,768 points.  Then the two arrangements of the
        training step's losses: the photometric loss and the depth term as
        one autograd node (depth_loss.l1_ssim_depth_loss: the scatter goes
        into the photometric gradient image) against two nodes whose
        4-channel gradient images autograd adds.  HIP events, the sides
        alternating in one process, two runs each.
  step: the graph-replayed M2 training step (garden scene_grid=3, 1,006,065
        Gaussians), images/s and ms: the option off; on with empty point
        tables (what the fourth rasterizer channel and the loss launches cost
        with nothing to sample); on with --points points per image sampled
        from the scene's own rendered depth.  The configurations alternate,
        two runs each.

Prints one JSON line per measurement.  For the kernel times run the `op` part
alone under `rocprofv3 --kernel-trace --stats` (no counters in the same run).

    python tools/depth_loss_bench.py [--part op|step|all] [--iters 50] [--steps 60]
                                     [--warmup 10] [--points 8192] [--only off|on]
"""

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat-triton_amd"))

W, H, GRID = 1920, 1080, 3


def timed(fn, iters):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def torch_term(rgbd, alphas, pts, dgt):
    """The reference's lines from the RGB+D render on: the RGB+ED division and
    cat (gsplat/rendering.py), then simple_trainer.py:649-664."""
    ed = torch.cat([rgbd[..., :-1], rgbd[..., -1:] / alphas.clamp(min=1e-10)], dim=-1)
    depths = ed[..., 3:4]
    points = torch.stack([pts[:, :, 0] / (W - 1) * 2 - 1, pts[:, :, 1] / (H - 1) * 2 - 1], dim=-1)
    grid = points.unsqueeze(2)
    d = F.grid_sample(depths.permute(0, 3, 1, 2), grid, align_corners=True)
    d = d.squeeze(3).squeeze(1)
    disp = torch.where(d > 0.0, 1.0 / d, torch.zeros_like(d))
    return F.l1_loss(disp, 1.0 / dgt)


def part_op(iters):
    from gsplat_hip.depth_loss import DepthPoints, l1_ssim_depth_loss, table_depth_loss
    from gsplat_hip.losses import l1_ssim_loss
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    alphas = (torch.rand(1, H, W, 1, generator=g) * 0.7 + 0.3).to(dev)
    rgbd = torch.rand(1, H, W, 4, generator=g).to(dev)
    rgbd[..., 3] = alphas[..., 0] * (rgbd[..., 3] * 2.0 + 1.0)
    rgbd.requires_grad_(True)
    alphas.requires_grad_(True)
    gt = torch.rand(1, H, W, 3, generator=g).to(dev)
    one = torch.ones((), device=dev)
    idx = torch.tensor([1], dtype=torch.int64, device=dev)
    for M in (4096, 32768):
        pts = (torch.rand(1, M, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])).to(dev)
        dgt = (torch.rand(1, M, generator=g) * 4.0 + 4.0).to(dev)
        # three images in the table; the middle one is the one timed
        tab = DepthPoints([(pts[0, :7].cpu(), dgt[0, :7].cpu()), (pts[0].cpu(), dgt[0].cpu()),
                           (pts[0, :99].cpu(), dgt[0, :99].cpu())], dev)

        def clear():
            rgbd.grad = alphas.grad = None

        def fused():
            clear()
            torch.autograd.backward(table_depth_loss(rgbd, alphas, tab, idx, 3), one)

        def composition():
            clear()
            torch.autograd.backward(torch_term(rgbd, alphas, pts, dgt), one)

        def one_node():
            clear()
            photo, term = l1_ssim_depth_loss(rgbd, alphas, gt, 0.2, tab, idx)
            torch.autograd.backward(photo + 0.01 * term, one)

        def two_nodes():
            clear()
            photo = l1_ssim_loss(rgbd, gt, 0.2, _channels=3)
            term = table_depth_loss(rgbd, alphas, tab, idx, 3)
            torch.autograd.backward(photo + 0.01 * term, one)

        fused()
        g_f = [rgbd.grad.clone(), alphas.grad.clone()]
        composition()
        g_c = [rgbd.grad.clone(), alphas.grad.clone()]
        one_node()
        g_1 = [rgbd.grad.clone(), alphas.grad.clone()]
        two_nodes()
        g_2 = [rgbd.grad.clone(), alphas.grad.clone()]
        print(json.dumps({
            "part": "op", "points": M, "check": "max abs gradient difference (v_rgbd, v_alphas)",
            "fused_vs_composition": [float((x - y).abs().max()) for x, y in zip(g_f, g_c)],
            "one_node_vs_two_nodes": [float((x - y).abs().max()) for x, y in zip(g_1, g_2)],
            "max_abs_grad": [float(y.abs().max()) for y in g_c]}), flush=True)
        for run in range(2):
            ms_f, ms_c = timed(fused, iters), timed(composition, iters)
            ms_1, ms_2 = timed(one_node, iters), timed(two_nodes, iters)
            print(json.dumps({
                "part": "op", "run": run, "pixels": W * H, "points": M,
                "fused_fwd_bwd_ms": round(ms_f, 4),
                "torch_composition_fwd_bwd_ms": round(ms_c, 4), "ratio": round(ms_c / ms_f, 2),
                "losses_one_node_fwd_bwd_ms": round(ms_1, 4),
                "losses_two_nodes_fwd_bwd_ms": round(ms_2, 4)}), flush=True)


def sample_points(tr, n_points, seed=0):
    """Per training image up to n_points positions in pixels whose alpha is
    above 0.5, with the expected depth of the trainer's own render there
    (5 % off, so the term is not zero)."""
    from gsplat_hip import rasterization
    p = tr.params
    out = []
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for ci in range(len(tr.viewmats)):
            rc, ra, _ = rasterization(
                p["means"], p["quats"], torch.exp(p["scales"]), torch.sigmoid(p["opacities"]),
                (p["sh0"], p["shN"]), tr.viewmats[ci:ci + 1], tr.Ks[ci:ci + 1], W, H,
                sh_degree=tr.sh_degree, packed=False, near_plane=0.01, far_plane=1e10,
                radius_clip=0.0, render_mode="RGB+ED")
            ok = (ra[0, :H - 1, :W - 1, 0] > 0.5).nonzero().cpu()
            if len(ok) == 0:
                out.append((torch.zeros(0, 2), torch.zeros(0)))
                continue
            pick = ok[torch.randint(len(ok), (n_points,), generator=g)]
            d = rc[0, :, :, 3].cpu()[pick[:, 0], pick[:, 1]] * 1.05
            xy = pick.flip(1).float() + torch.rand(n_points, 2, generator=g) * 0.999
            out.append((xy, d))
    return out


def part_step(steps, warmup, n_points, only=None):
    from gsplat_hip.train_step import Trainer, camera_pool, load_garden_scene
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(ROOT, "tests", "golden", "garden_scene.npz"), scene_grid=GRID)
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=8)
    probe = Trainer(means, rgbs, vm, K, W, H, sh_degree=3, device="cuda")
    points = sample_points(probe, n_points)
    del probe
    torch.cuda.empty_cache()
    empty = [(torch.zeros(0, 2), torch.zeros(0))] * len(vm)
    configs = (("off", {}), ("on, empty tables", dict(depth_loss=True, depth_points=empty)),
               ("on", dict(depth_loss=True, depth_points=points)))
    if only is not None:  # one configuration, once: a run under a kernel trace
        configs = tuple(c for c in configs if c[0] == only)
    for name, kw in (configs + configs if only is None else configs):
        tr = Trainer(means, rgbs, vm, K, W, H, sh_degree=3, device="cuda", graph=True, **kw)
        for it in range(warmup):
            tr.step(it)
        tr.sync()
        t0 = time.perf_counter()
        for it in range(warmup, warmup + steps):
            tr.step(it)
        tr.sync()
        dt = time.perf_counter() - t0
        g = tr._graph
        print(json.dumps({"part": "step", "depth_loss": name, "steps": steps,
                          "points_per_image": [len(d) for _, d in kw.get("depth_points", [])],
                          "images_per_s": round(steps / dt, 1),
                          "ms_per_step": round(1e3 * dt / steps, 3),
                          "graph": g is not None and tr.graph_fallback is None,
                          "kernel_nodes": None if g is None else g.census.get("kernel"),
                          "captures": None if g is None else g.recaptures}), flush=True)
        tr.release_graph()
        del tr
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("op", "step", "all"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--only", default=None, choices=("off", "on, empty tables", "on"),
                    help="step part: this configuration alone, once (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_loss_bench: needs a GPU (no CPU fall-back)")
    if args.part in ("op", "all"):
        part_op(args.iters)
    if args.part in ("step", "all"):
        part_step(args.steps, args.warmup, args.points, args.only)


if __name__ == "__main__":
    main()
