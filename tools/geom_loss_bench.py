"""Time the 2DGS geometry terms (normal consistency + distortion) at the M5
configuration (garden scene_grid=3, 1,006,065 surfels, 1920x1080).

  loss: the fused pair (gsplat_hip.geometry_loss_2dgs forward + backward,
        csrc/geom_loss.hip) against the torch composition a user of the
        previous release had to run on the same tensors (_Rotate3, then
        depth_to_normal, then torch ops; forward + backward), on the M5
        scene's render.  HIP events, the two sides alternating in one
        process, two runs each.
  step: the graph-replayed M5 training step, images/s and ms, in three
        states: colours only, normal term active, both terms active.

Prints one JSON line per measurement.  For the kernel times of the two new
kernels run the `loss` part alone under `rocprofv3 --kernel-trace --stats`
(no counters in the same run).

    python tools/geom_loss_bench.py [--part loss|step|all] [--iters 20] [--steps 30] [--warmup 5]
"""

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat-triton_amd"))

W, H, GRID = 1920, 1080, 3
NL, DL = 5e-2, 1e-2


def scene():
    from gsplat_hip.train_step import camera_pool, load_garden_scene
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(ROOT, "tests", "golden", "garden_scene.npz"), scene_grid=GRID)
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=8)
    return means, rgbs, vm, K


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


def part_loss(iters):
    from gsplat_hip import depth_to_normal, geometry_loss_2dgs
    from gsplat_hip.rendering import _Rotate3
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K = scene()
    tr = Trainer(means, rgbs, vm, K, W, H, sh_degree=3, device="cuda", model="2dgs")
    with torch.no_grad():
        _, ra, meta = tr.render(0, 3, geometry=(NL, DL))
        rn, _, rd = meta["_geometry"]
        rgbd, c2w = meta["_rgbd"].clone(), meta["camtoworlds"].clone()
        rn, ra, rd = rn.clone(), ra.clone(), rd.clone()
    del tr, meta
    torch.cuda.empty_cache()
    Ks = K[:1].to("cuda")
    n = rn.requires_grad_(True)
    img = rgbd.requires_grad_(True)
    dist = rd.requires_grad_(True)

    def clear():
        n.grad = img.grad = dist.grad = None

    def fused():
        clear()
        geometry_loss_2dgs(n, img[..., 3:4], ra, c2w, Ks, dist, normal_lambda=NL,
                           dist_lambda=DL).backward()

    def composition():
        clear()
        nw = _Rotate3.apply(c2w, n)
        nd = depth_to_normal(img[..., 3:4], c2w, Ks)
        loss = NL * (1.0 - (nw * (nd * ra)).sum(-1)).mean() + DL * dist.mean()
        loss.backward()

    fused()
    a = [float(geometry_loss_2dgs(n, img[..., 3:4], ra, c2w, Ks, dist, normal_lambda=NL,
                                  dist_lambda=DL).detach())]
    g_f = [t.grad.clone() for t in (n, img, dist)]
    composition()
    nw = _Rotate3.apply(c2w, n)
    nd = depth_to_normal(img[..., 3:4], c2w, Ks)
    a.append(float((NL * (1.0 - (nw * (nd * ra)).sum(-1)).mean() + DL * dist.mean()).detach()))
    g_c = [t.grad.clone() for t in (n, img, dist)]
    print(json.dumps({"part": "loss", "check": "fused vs composition",
                      "loss": a, "max_abs_grad_diff": [float((x - y).abs().max())
                                                       for x, y in zip(g_f, g_c)],
                      "max_abs_grad": [float(y.abs().max()) for y in g_c]}), flush=True)
    for run in range(2):
        ms_f = timed(fused, iters)
        ms_c = timed(composition, iters)
        print(json.dumps({"part": "loss", "run": run, "pixels": W * H,
                          "fused_fwd_bwd_ms": round(ms_f, 4),
                          "torch_composition_fwd_bwd_ms": round(ms_c, 4),
                          "ratio": round(ms_c / ms_f, 2)}), flush=True)


def part_step(steps, warmup):
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K = scene()
    states = (("colours only", {}),
              ("normal term", dict(normal_loss=True, normal_start_iter=-1)),
              ("both terms", dict(normal_loss=True, normal_start_iter=-1, dist_loss=True,
                                  dist_start_iter=-1)))
    for name, kw in states:
        tr = Trainer(means, rgbs, vm, K, W, H, sh_degree=3, device="cuda", model="2dgs",
                     graph=True, **kw)
        for it in range(warmup):
            tr.step(it)
        tr.sync()
        t0 = time.perf_counter()
        for it in range(warmup, warmup + steps):
            tr.step(it)
        tr.sync()
        dt = time.perf_counter() - t0
        g = tr._graph
        print(json.dumps({"part": "step", "state": name, "steps": steps,
                          "images_per_s": round(steps / dt, 1),
                          "ms_per_step": round(1e3 * dt / steps, 3),
                          "graph": g is not None and tr.graph_fallback is None,
                          "captures": None if g is None else g.recaptures}), flush=True)
        tr.release_graph()
        del tr
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("loss", "step", "all"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.part in ("loss", "all"):
        part_loss(args.iters)
    if args.part in ("step", "all"):
        part_step(args.steps, args.warmup)


if __name__ == "__main__":
    main()
