"""Time the masked / composited photometric loss at 1920x1080 RGB.

  op:   forward + backward of
        (a) the plain fused loss (l1_ssim_loss, ssim::fused_kernel<3,4,3,3>),
        (b) the masked loss with a disc mask and a background, composed in the
            kernel (l1_ssim_loss(masks=, alphas=, backgrounds=),
            ssim::fused_masked_kernel<3,4>),
        (c) the torch composition in front of the plain fused loss
            (losses.compose_masked: a where and a composite, with their
            autograd backward) -- what the fusion replaces,
        on the same tensors, seeded with the trainer's constant 1.0 gradient.
        HIP events, the three alternating in one process, two rounds each;
        the launches of one forward + backward are counted with
        torch.profiler.
  step: the graph-replayed M2 training step (garden scene_grid=3, 1,006,065
        Gaussians), images/s and ms, with masks and random_bkgd both off and
        both on, alternating, two runs each.

Prints one JSON line per measurement.  For the kernel times run the `op` part
alone under `rocprofv3 --kernel-trace --stats` (no counters in the same run).

    python tools/masked_loss_bench.py [--part op|step|all] [--iters 50] [--steps 60]
                                      [--warmup 10] [--only off|on]
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


def disc(n, frac=0.45):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32),
                            torch.arange(W, dtype=torch.float32), indexing="ij")
    r = frac * min(H, W)
    m = (yy - (H - 1) / 2) ** 2 + (xx - (W - 1) / 2) ** 2 <= r * r
    return m[None].repeat(n, 1, 1)


def launches(fn):
    """Device kernels of one call of fn."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)


def part_op(iters):
    from gsplat_hip.losses import compose_masked, l1_ssim_loss
    from gsplat_hip.train_step import _one_grad
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    img = torch.rand(1, H, W, 3, generator=g).to(dev).requires_grad_(True)
    alphas = (torch.rand(1, H, W, 1, generator=g) * 0.7 + 0.3).to(dev).requires_grad_(True)
    gt = torch.rand(1, H, W, 3, generator=g).to(dev)
    mask = disc(1).to(dev)
    back = torch.tensor([[0.2, 0.5, 0.9]], device=dev)
    one = _one_grad(torch.device(dev, torch.cuda.current_device()))

    def clear():
        img.grad = alphas.grad = None

    def plain():
        clear()
        torch.autograd.backward(l1_ssim_loss(img, gt, 0.2), one)

    def masked():
        clear()
        torch.autograd.backward(l1_ssim_loss(img, gt, 0.2, masks=mask, alphas=alphas,
                                             backgrounds=back), one)

    def composition():
        clear()
        torch.autograd.backward(l1_ssim_loss(compose_masked(img, mask, alphas, back), gt, 0.2),
                                one)

    masked()
    g_m = [img.grad.clone(), alphas.grad.clone()]
    composition()
    g_c = [img.grad.clone(), alphas.grad.clone()]
    print(json.dumps({
        "part": "op", "check": "max abs gradient difference (img, alphas), fused vs composition",
        "diff": [float((x - y).abs().max()) for x, y in zip(g_m, g_c)],
        "max_abs_grad": [float(y.abs().max()) for y in g_c],
        "launches_fwd_bwd": {"plain": launches(plain), "masked": launches(masked),
                             "torch_composition": launches(composition)}}), flush=True)
    for run in range(2):
        ms_p, ms_m, ms_c = timed(plain, iters), timed(masked, iters), timed(composition, iters)
        print(json.dumps({
            "part": "op", "run": run, "pixels": W * H,
            "plain_fwd_bwd_ms": round(ms_p, 4), "masked_fwd_bwd_ms": round(ms_m, 4),
            "torch_composition_fwd_bwd_ms": round(ms_c, 4),
            "composition_over_masked": round(ms_c / ms_m, 2),
            "masked_over_plain": round(ms_m / ms_p, 2)}), flush=True)


def part_step(steps, warmup, only=None):
    from gsplat_hip.train_step import Trainer, camera_pool, load_garden_scene
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(ROOT, "tests", "golden", "garden_scene.npz"), scene_grid=GRID)
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=8)
    configs = (("off", {}), ("on", dict(masks=disc(len(vm)), random_bkgd=True)))
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
        print(json.dumps({"part": "step", "masks_and_random_bkgd": name, "steps": steps,
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
    ap.add_argument("--only", default=None, choices=("off", "on"),
                    help="step part: this configuration alone, once (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("masked_loss_bench: needs a GPU (no CPU fall-back)")
    if args.part in ("op", "all"):
        part_op(args.iters)
    if args.part in ("step", "all"):
        part_step(args.steps, args.warmup, args.only)


if __name__ == "__main__":
    main()
