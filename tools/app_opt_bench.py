"""Time the appearance MLP at the benchmark scene's size (N = 1,006,065, C = 1).

  op:  the kernel pair of gsplat_hip.appearance (csrc/appearance.hip) --
       forward alone, and forward + backward + the ordered reduction of the
       workspace -- against the torch composition of examples/utils.py
       AppearanceOptModule and simple_trainer.py:389-410 (normalize, the SH
       bases, cat, three Linear layers, sigmoid, autograd) on the same tensors.
       HIP events, the sides alternating in one process, two runs each.  Also
       with --visible of the rows hidden (a random mask; the trainer's radii
       mask hides the Gaussians outside the view).
       The achieved fraction of the fp32 MFMA peak (157.3 TFLOP/s) counts the
       matrix products only: forward 2 x 64 x 64 x 2 FLOP per row, backward
       that again (the recomputation) plus dW and dX of both layers.

  scene: the benchmark scene itself (garden scene_grid=3, 1920x1080, the
       eight cameras of the pool): the share of the Gaussians each camera
       sees (radii > 0), the share of 32-row waves with a visible row (what
       the kernels cannot skip), and the pair's times with that mask, the
       scene's means and the camera's centre.

  step: the benchmark's training step (bench.py's M2: that scene, 1920x1080,
       eight cameras, graph replays) with and without `app_opt`, alternating
       in one process, two runs each: ms per step between HIP events over
       --steps steps after --warmup, and the host's wall clock over the same
       steps.

Prints one JSON line per measurement.  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats` (no counters in the same run).

    python tools/app_opt_bench.py [--part op|scene|step|all] [--n 1006065] [--iters 20]
                                  [--visible 0.35] [--steps 100] [--warmup 20]
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

PEAK_TFLOPS = 157.3
FWD_FLOP = 2 * 2 * 64 * 64            # per visible row: two 64x64 layers
BWD_FLOP = FWD_FLOP + 4 * 2 * 64 * 64  # recomputation, dW2, dW1, dH1, dX


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


def sh_bases(d):
    x, y, z = d.unbind(-1)
    zz = z * z
    g2, h2 = 2 * x * y, x * x - y * y
    g3, h3 = x * g2 + y * h2, x * h2 - y * g2
    c31 = -2.285228997322329 * zz + 0.4570457994644658
    return torch.stack([
        torch.full_like(x, 0.2820947917738781), -0.48860251190292 * y, 0.48860251190292 * z,
        -0.48860251190292 * x, 0.5462742152960395 * g2, -1.092548430592079 * z * y,
        0.9461746957575601 * zz - 0.3153915652525201, -1.092548430592079 * z * x,
        0.5462742152960395 * h2, -0.5900435899266435 * g3, 1.445305721320277 * z * g2, c31 * y,
        z * (1.865881662950577 * zz - 1.119528997770346), c31 * x, 1.445305721320277 * z * h2,
        -0.5900435899266435 * h3], dim=-1)


def torch_colors(t, head):
    C, N = t["campos"].shape[0], t["features"].shape[0]
    dirs = F.normalize(t["means"][None] - t["campos"][:, None], dim=-1)
    h = torch.cat([t["embeds"][:, None, :].expand(-1, N, -1),
                   t["features"][None].expand(C, -1, -1), sh_bases(dirs)], dim=-1)
    h = torch.relu(F.linear(h, head[0], head[1]))
    h = torch.relu(F.linear(h, head[2], head[3]))
    return torch.sigmoid(F.linear(h, head[4], head[5]) + t["base_colors"])


def part_scene(iters):
    import gsplat_hip
    from gsplat_hip import appearance as A
    from gsplat_hip.train_step import Trainer, camera_pool, load_garden_scene
    W, H = 1920, 1080
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(ROOT, "tests", "golden", "garden_scene.npz"), scene_grid=3)
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=8)
    tr = Trainer(means, rgbs, vm, K, W, H, sh_degree=3, device="cuda")
    N = tr.params["means"].shape[0]
    g = torch.Generator().manual_seed(0)
    feats = torch.rand(N, 32, generator=g).cuda().requires_grad_(True)
    base = torch.randn(N, 3, generator=g).cuda().requires_grad_(True)
    emb = torch.randn(1, 16, generator=g).cuda().requires_grad_(True)
    head = [((torch.rand(*s, generator=g) * 2 - 1) * 0.125).cuda().requires_grad_(True)
            for s in A.HEAD_SHAPES]
    v = torch.randn(1, N, 3, generator=g).cuda()
    mu = tr.params["means"].detach().clone().requires_grad_(True)
    leaves = [feats, base, emb, mu] + head
    for ci in range(len(vm)):
        with torch.no_grad():
            _, _, meta = tr.render(ci)
        radii = meta["radii"]
        mask = ((radii > 0).all(-1) if radii.dim() == 3 else radii > 0).reshape(1, N)
        campos = tr.camtoworld(ci)[:, :3, 3].contiguous()
        pad = (-N) % 32
        waves = torch.nn.functional.pad(mask[0], (0, pad)).view(-1, 32).any(1)

        def both():
            c = gsplat_hip.appearance_colors(feats, base, emb, mu, campos, head, 3, masks=mask)
            torch.autograd.grad(c, leaves, v)

        def fwd():
            with torch.no_grad():
                gsplat_hip.appearance_colors(feats, base, emb, mu, campos, head, 3, masks=mask)

        print(json.dumps(dict(measure="scene", camera=ci, N=N,
                              visible=round(float(mask.float().mean()), 4),
                              waves_with_a_visible_row=round(float(waves.float().mean()), 4),
                              fwd_ms=round(timed(fwd, iters), 4),
                              fwd_bwd_reduce_ms=round(timed(both, iters), 4))), flush=True)


def part_step(steps, warmup, graph=True):
    from gsplat_hip.train_step import Trainer, camera_pool, load_garden_scene
    W, H = 1920, 1080
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(ROOT, "tests", "golden", "garden_scene.npz"), scene_grid=3)
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=8)
    for run in (1, 2):
        res = {}
        for on in (False, True):
            tr = Trainer(means, rgbs, vm, K, W, H, sh_degree=3, device="cuda", graph=graph,
                         app_opt=on)
            if on:  # a trained module's last layer is not zero
                g = torch.Generator().manual_seed(0)
                tr.app.head[4].copy_((torch.randn(3, 64, generator=g) * 0.1).cuda())
            for it in range(warmup):
                tr.step(it)
            tr.sync()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.record()
            for it in range(warmup, warmup + steps):
                loss = tr.step(it)
            e.record()
            tr.sync()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3 / steps
            res[on] = s.elapsed_time(e) / steps
            print(json.dumps(dict(measure="M2 step", app_opt=on, run=run, graph=graph,
                                  replayed=tr._graph is not None, fallback=tr.graph_fallback,
                                  N=tr.params["means"].shape[0], steps=steps,
                                  ms_per_step=round(res[on], 4), wall_ms_per_step=round(wall, 4),
                                  loss=round(float(loss), 6))), flush=True)
            tr.release_graph()
            del tr
            torch.cuda.empty_cache()
        print(json.dumps(dict(measure="M2 step, app_opt on - off", run=run,
                              ms=round(res[True] - res[False], 4),
                              ratio=round(res[True] / res[False], 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("op", "scene", "step", "all"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--n", type=int, default=1006065)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--visible", type=float, default=0.35)
    a = ap.parse_args()
    if a.part in ("scene", "all"):
        part_scene(a.iters)
    if a.part in ("step", "all"):
        part_step(a.steps, a.warmup)
    if a.part in ("scene", "step"):
        return
    import gsplat_hip
    from gsplat_hip import appearance as A
    dev, N = "cuda", a.n
    g = torch.Generator().manual_seed(0)
    t = dict(features=torch.rand(N, 32, generator=g), base_colors=torch.randn(N, 3, generator=g),
             means=torch.randn(N, 3, generator=g), campos=torch.randn(1, 3, generator=g) * 3,
             embeds=torch.randn(1, 16, generator=g))
    t = {k: v.to(dev).requires_grad_(k != "campos") for k, v in t.items()}
    head = [((torch.rand(*s, generator=g) * 2 - 1) * 0.125).to(dev).requires_grad_(True)
            for s in A.HEAD_SHAPES]
    v = torch.randn(1, N, 3, generator=g).to(dev)
    mask = (torch.rand(1, N, generator=g) < a.visible).to(dev)
    leaves = [x for x in t.values() if x.requires_grad] + head

    def hip_fwd(m=None):
        with torch.no_grad():
            gsplat_hip.appearance_colors(t["features"], t["base_colors"], t["embeds"], t["means"],
                                         t["campos"], head, 3, masks=m)

    def hip_both(m=None):
        c = gsplat_hip.appearance_colors(t["features"], t["base_colors"], t["embeds"], t["means"],
                                         t["campos"], head, 3, masks=m)
        torch.autograd.grad(c, leaves, v)

    def torch_fwd():
        with torch.no_grad():
            torch_colors(t, head)

    def torch_both():
        torch.autograd.grad(torch_colors(t, head), leaves, v)

    def out(name, ms, flop_rows=None, flop=0, **kw):
        d = dict(measure=name, N=N, ms=round(ms, 4), **kw)
        if flop_rows:
            tf = flop_rows * flop / (ms * 1e-3) / 1e12
            d.update(mfma_tflops=round(tf, 2), frac_of_fp32_mfma_peak=round(tf / PEAK_TFLOPS, 4))
        print(json.dumps(d), flush=True)
        return ms

    nvis = int(mask.sum())
    for run in (1, 2):
        hf = out("hip fwd", timed(hip_fwd, a.iters), N, FWD_FLOP, run=run)
        tf = out("torch fwd", timed(torch_fwd, a.iters), run=run)
        hb = out("hip fwd+bwd+reduce", timed(hip_both, a.iters), N, FWD_FLOP + BWD_FLOP, run=run)
        tb = out("torch fwd+bwd", timed(torch_both, a.iters), run=run)
        print(json.dumps(dict(measure="torch / hip", fwd=round(tf / hf, 2),
                              fwd_bwd=round(tb / hb, 2), run=run)), flush=True)
        out("hip fwd masked", timed(lambda: hip_fwd(mask), a.iters), nvis, FWD_FLOP, run=run,
            visible=round(nvis / N, 4))
        out("hip fwd+bwd+reduce masked", timed(lambda: hip_both(mask), a.iters), nvis,
            FWD_FLOP + BWD_FLOP, run=run, visible=round(nvis / N, 4))


if __name__ == "__main__":
    main()
