"""Time camera pose optimisation at M2 (garden scene_grid=3, 1,006,065
Gaussians, 1920x1080).

  op:   the three launches of a pose_opt step, HIP events:
        (a) gsplat_hip_pose_apply,
        (b) gsplat_hip_projection_bwd_adam_pose against the plain
            gsplat_hip_projection_bwd_adam on the same inputs (alternating,
            two runs each): what the pose partials add to the fused backward,
        (c) gsplat_hip_pose_bwd_adam over the backward's 3,930 workspace rows
            and a table of 200 images.
  step: the graph-replayed M2 training step, images/s and ms, with the option
        off and on (alternating, two runs each), and the captured step's node
        census of both.

Prints one JSON line per measurement.  For the kernel times run the `op` part
alone under `rocprofv3 --kernel-trace --stats` (no counters in the same run).

    python tools/pose_opt_bench.py [--part op|step|all] [--iters 50] [--steps 30] [--warmup 5]
"""

import argparse
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat-triton_amd"))

W, H, GRID, N_IMAGES = 1920, 1080, 3, 200


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
    return 1e3 * s.elapsed_time(e) / iters  # us


def scene(n_cams=8):
    from gsplat_hip.train_step import camera_pool, load_garden_scene
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(ROOT, "tests", "golden", "garden_scene.npz"), scene_grid=GRID)
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=n_cams)
    return means, rgbs, vm.float(), K.float()


def part_op(iters):
    import gsplat_hip
    from gsplat_hip import _wrapper
    from gsplat_hip.pose import pose_apply, pose_bwd_adam, pose_workspace
    from gsplat_hip.train_step import Trainer
    dev = "cuda"
    means, rgbs, vm, K = scene()
    tr = Trainer(means, rgbs, vm, K, W, H, sh_degree=3, device=dev)
    N = tr.params["means"].shape[0]
    g = torch.Generator().manual_seed(0)
    p = [tr.params[k].data for k in tr.GEOM]
    scales, opac = torch.exp(p[1]), torch.sigmoid(p[3])
    vm0, K0 = tr.viewmats[:1].contiguous(), tr.Ks[:1].contiguous()
    radii, _, _, conics, _ = gsplat_hip.fully_fused_projection(
        p[0], None, p[2], scales, vm0, K0, W, H, packed=False, near_plane=0.01, far_plane=1e10)
    vis = (radii[0] > 0).float()

    def rnd(*shape, scale=1e-4):
        return (torch.randn(*shape, generator=g) * scale).to(dev)

    fusion = types.SimpleNamespace(v_dirs=(rnd(N, 3) * vis[:, None]).contiguous(),
                                   v_opac_in=rnd(1, N), opac_act=opac)
    grads = (rnd(1, N, 2), rnd(1, N), rnd(1, N, 3))
    ws = pose_workspace(N, dev)

    def backward(pose):
        m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
        ga = _wrapper.GeomAdamInBackward([t.clone() for t in p], m, v, [0.0] * 4, (0.9, 0.999),
                                         1e-15, 1)
        ga.pose_ws = ws if pose else None
        return lambda: ga.run(ga.params[0], ga.params[2], scales, vm0, K0, W, H, 0.3, radii,
                              conics.contiguous(), *grads, fusion)

    plain, posed = backward(False), backward(True)
    for run in range(2):
        us_p, us_q = timed(plain, iters), timed(posed, iters)
        print(json.dumps({"part": "op", "launch": "b", "run": run, "gaussians": N,
                          "visible": int(vis.sum()),
                          "projection_bwd_adam_us": round(us_p, 2),
                          "projection_bwd_adam_pose_us": round(us_q, 2),
                          "added_us": round(us_q - us_p, 2)}), flush=True)
    emb = rnd(N_IMAGES, 9, scale=1e-2)
    m, v = torch.zeros_like(emb), torch.zeros_like(emb)
    cam = torch.tensor([17], device=dev)
    out = torch.empty(1, 4, 4, device=dev)
    us_a = timed(lambda: pose_apply(vm0, cam, emb, None, out=out), iters)
    us_c = timed(lambda: pose_bwd_adam(ws, N, vm0, cam, emb, m, v, 1e-5, 1e-6, 1), iters)
    print(json.dumps({"part": "op", "launch": "a", "pose_apply_us": round(us_a, 2),
                      "note": "event time of back-to-back launches: launch-bound"}), flush=True)
    print(json.dumps({"part": "op", "launch": "c", "workspace_rows": (N + 255) // 256,
                      "images": N_IMAGES, "pose_bwd_adam_us": round(us_c, 2)}), flush=True)


def part_step(steps, warmup):
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K = scene()
    for name, kw in (("off", {}), ("on", dict(pose_opt=True)), ("off", {}),
                     ("on", dict(pose_opt=True))):
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
        print(json.dumps({"part": "step", "pose_opt": name, "steps": steps,
                          "images_per_s": round(steps / dt, 1),
                          "ms_per_step": round(1e3 * dt / steps, 3),
                          "graph": g is not None and tr.graph_fallback is None,
                          "captures": None if g is None else g.recaptures,
                          "census": None if g is None else dict(g.census)}), flush=True)
        tr.release_graph()
        del tr
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("op", "step", "all"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.part in ("op", "all"):
        part_op(args.iters)
    if args.part in ("step", "all"):
        part_step(args.steps, args.warmup)


if __name__ == "__main__":
    main()
