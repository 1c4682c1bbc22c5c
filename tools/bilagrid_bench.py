"""Time the bilateral-grid colour correction at 1920x1080 with N = 200 grids
of the default shape (16, 16, 8).

  op:   the fused slice + 10 x total variation, forward + backward
        (gsplat_hip.bilagrid._slice_tv, csrc/bilagrid.hip: one dense gradient
        write) against the torch composition of examples/lib_bilagrid.py
        (5-D grid_sample on the pixel meshgrid, the matmul, the index_select
        total variation) on the same tensors.  HIP events, the two sides
        alternating in one process, two runs each.
  step: the graph-replayed M2 training step (garden scene_grid=3, 1,006,065
        Gaussians), images/s and ms, with the option off and on.

Prints one JSON line per measurement.  For the kernel times run the `op` part
alone under `rocprofv3 --kernel-trace --stats` (no counters in the same run).

    python tools/bilagrid_bench.py [--part op|step|all] [--iters 20] [--steps 30] [--warmup 5]
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

W, H, GRID, N_GRIDS = 1920, 1080, 3, 200
TV_WEIGHT = 10.0


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


def torch_slice(grids, xy, rgb, idx):
    """lib_bilagrid.slice for one view: grid_sample + color_affine_transform."""
    gz = (rgb @ rgb.new_tensor([[0.299], [0.587], [0.114]])) * 2.0 - 1.0
    xyz = torch.cat([(xy - 0.5) * 2.0, gz], -1)[:, None]
    A = F.grid_sample(grids[idx], xyz, mode="bilinear", align_corners=True,
                      padding_mode="border")
    A = A.permute(0, 2, 3, 4, 1)[:, 0].reshape(*rgb.shape[:3], 3, 4)
    return torch.matmul(A[..., :3], rgb.unsqueeze(-1)).squeeze(-1) + A[..., 3]


def torch_tv(x):
    tv = 0.0
    for i in range(2, x.dim()):
        n = x.shape[i]
        x1 = x.index_select(i, torch.arange(1, n, device=x.device))
        x2 = x.index_select(i, torch.arange(0, n - 1, device=x.device))
        tv = tv + ((x1 - x2) ** 2).sum() / x1[0].numel()
    return tv / x.shape[0]


def part_op(iters):
    import gsplat_hip
    from gsplat_hip.bilagrid import _slice_tv
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    grids = gsplat_hip.bilagrid_identity(N_GRIDS, device=dev)
    grids = (grids + 0.1 * torch.randn(grids.shape, generator=g).to(dev)).requires_grad_(True)
    rgb = (torch.rand(1, H, W, 3, generator=g) * 1.2 - 0.1).to(dev).requires_grad_(True)
    v_out = (torch.randn(1, H, W, 3, generator=g) / (H * W)).to(dev)
    idx = torch.tensor([17], device=dev)
    # the reference trainer's meshgrid, built once outside the timed region
    ys, xs = torch.meshgrid((torch.arange(H, device=dev) + 0.5) / H,
                            (torch.arange(W, device=dev) + 0.5) / W, indexing="ij")
    xy = torch.stack([xs, ys], -1)[None]

    def clear():
        grids.grad = rgb.grad = None

    def fused():
        clear()
        out, tv = _slice_tv(grids, rgb, idx, TV_WEIGHT)
        torch.autograd.backward([out, tv], [v_out, torch.ones_like(tv)])

    def composition():
        clear()
        out = torch_slice(grids, xy, rgb, idx)
        tv = TV_WEIGHT * torch_tv(grids)
        torch.autograd.backward([out, tv], [v_out, torch.ones_like(tv)])

    fused()
    g_f = [grids.grad.clone(), rgb.grad.clone()]
    composition()
    g_c = [grids.grad.clone(), rgb.grad.clone()]
    print(json.dumps({"part": "op", "check": "fused vs composition (v_grids, v_rgb)",
                      "max_abs_grad_diff": [float((x - y).abs().max()) for x, y in zip(g_f, g_c)],
                      "max_abs_grad": [float(y.abs().max()) for y in g_c]}), flush=True)
    for run in range(2):
        ms_f = timed(fused, iters)
        ms_c = timed(composition, iters)
        print(json.dumps({"part": "op", "run": run, "pixels": W * H, "grids": N_GRIDS,
                          "fused_fwd_bwd_ms": round(ms_f, 4),
                          "torch_composition_fwd_bwd_ms": round(ms_c, 4),
                          "ratio": round(ms_c / ms_f, 2)}), flush=True)


def part_step(steps, warmup):
    from gsplat_hip.train_step import Trainer, camera_pool, load_garden_scene
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(ROOT, "tests", "golden", "garden_scene.npz"), scene_grid=GRID)
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=8)
    for name, kw in (("off", {}), ("on", dict(bilateral_grid=True)), ("off", {}),
                     ("on", dict(bilateral_grid=True))):
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
        print(json.dumps({"part": "step", "bilateral_grid": name, "steps": steps,
                          "grids": len(vm) if kw else 0,
                          "images_per_s": round(steps / dt, 1),
                          "ms_per_step": round(1e3 * dt / steps, 3),
                          "graph": g is not None and tr.graph_fallback is None,
                          "captures": None if g is None else g.recaptures}), flush=True)
        tr.release_graph()
        del tr
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("op", "step", "all"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.part in ("op", "all"):
        part_op(args.iters)
    if args.part in ("step", "all"):
        part_step(args.steps, args.warmup)


if __name__ == "__main__":
    main()
