"""Time the projection from covariances at M2 (garden scene_grid=3, 1,006,065
Gaussians, one 1920x1080 camera), HIP events, in one process:

  fused:   fully_fused_projection(covars=[N,6]) forward and backward against
           the quats / scales forward and backward on the same Gaussians
           (alternating, two runs each).  Bytes the kernels must move per
           Gaussian: forward 9 input floats against 10, backward 6 gradient
           floats against 7 (+ the shared outputs / cotangents), so parity is
           the expectation; the achieved bytes/s of each are printed.
  stages:  world_to_cam + proj (pinhole), forward and forward+backward,
           against the same composition written with torch matmuls, as a
           user without these kernels would run it.
  models:  proj alone, pinhole / ortho / fisheye, forward and
           forward+backward.
  packed:  the packed forward (count, scan, write) of both fused paths; not
           part of `all`, it only gives rocprofv3 the packed kernels to time.

Every figure is event time per Python call: the larger of the host's issue
time (wrapper, allocations, launches) and the GPU's time, not kernel time.
Prints one JSON line per measurement and appends them to
profiles/covars/covar_proj_bench.txt (--out).  For kernel times run under
`rocprofv3 --kernel-trace --stats` (no counters in the same run).

    python tools/covar_proj_bench.py [--part fused|stages|models|packed|all] [--iters 300]
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat-triton_amd"))

W, H, GRID = 1920, 1080, 3
_OUT = None


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if _OUT:
        with open(_OUT, "a") as f:
            f.write(line + "\n")


def timed(fn, iters):
    for _ in range(5):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1e3 * s.elapsed_time(e) / iters  # us


def scene():
    """The trainer's initial Gaussians of the M2 scene and its first camera."""
    from gsplat_hip.train_step import Trainer, camera_pool, load_garden_scene
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(ROOT, "tests", "golden", "garden_scene.npz"), scene_grid=GRID)
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=8)
    tr = Trainer(means, rgbs, vm.float(), K.float(), W, H, sh_degree=3, device="cuda")
    p = [tr.params[k].data.clone() for k in tr.GEOM]  # means, log-scales, quats, logits
    vm0, K0 = tr.viewmats[:1].contiguous().clone(), tr.Ks[:1].contiguous().clone()
    del tr
    torch.cuda.empty_cache()
    return p[0], p[2], torch.exp(p[1]), vm0, K0


def part_fused(iters):
    import gsplat_hip
    from gsplat_hip import _wrapper, _wrapper_covar
    means, quats, scales, vm, K = scene()
    N = means.shape[0]
    covars = gsplat_hip.quat_scale_to_covar_preci(quats, scales, compute_preci=False, triu=True)[0]
    kw = dict(eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0)
    g = torch.Generator(device="cuda").manual_seed(0)
    cot = [torch.randn(s, device="cuda", generator=g) * 1e-3
           for s in ((1, N, 2), (1, N), (1, N, 3))]

    def fwd_q():
        return gsplat_hip.fully_fused_projection(means, None, quats, scales, vm, K, W, H, **kw)

    def fwd_c():
        return gsplat_hip.fully_fused_projection(means, covars, None, None, vm, K, W, H, **kw)

    rq, rc = fwd_q(), fwd_c()
    vis = int((rq[0] > 0).sum())
    same = float((rq[0] == rc[0]).float().mean())

    # the backward alone: the autograd node's backward on saved tensors
    def make_bwd(fn, leaves):
        leaves = [t.detach().requires_grad_(True) for t in leaves]
        out = fn(*leaves)
        outs, gr = [out[1], out[2], out[3]], cot
        return lambda: torch.autograd.grad(outs, leaves, gr, retain_graph=True)

    bwd_q = make_bwd(lambda m, q, s: gsplat_hip.fully_fused_projection(
        m, None, q, s, vm, K, W, H, **kw), (means, quats, scales))
    bwd_c = make_bwd(lambda m, c: gsplat_hip.fully_fused_projection(
        m, c, None, None, vm, K, W, H, **kw), (means, covars))
    # bytes per Gaussian the kernels must move (one camera): inputs + outputs
    fwd_bytes = {"quats_scales": 4 * (10 + 8), "covars": 4 * (9 + 8)}   # radii, means2d, depths, conics
    bwd_bytes = {"quats_scales": 4 * (10 + 1 + 3 + 6 + 10), "covars": 4 * (9 + 1 + 3 + 6 + 9)}
    for run in range(2):
        us = {"fwd_quats_scales": timed(fwd_q, iters), "fwd_covars": timed(fwd_c, iters),
              "bwd_quats_scales": timed(bwd_q, iters), "bwd_covars": timed(bwd_c, iters)}
        emit({"part": "fused", "run": run, "gaussians": N, "visible": vis,
              "radii_equal_share": round(same, 6), "iters": iters,
              **{k + "_us": round(v, 2) for k, v in us.items()},
              "fwd_covars_over_quats": round(us["fwd_covars"] / us["fwd_quats_scales"], 3),
              "bwd_covars_over_quats": round(us["bwd_covars"] / us["bwd_quats_scales"], 3),
              "fwd_GBps": {k: round(N * b / us["fwd_" + k] / 1e3, 1) for k, b in fwd_bytes.items()},
              "bwd_GBps": {k: round(N * b / us["bwd_" + k] / 1e3, 1) for k, b in bwd_bytes.items()},
              "note": "event time per call: launch(es), wrapper and allocations included"})


def torch_stages(means, covars, viewmats, Ks, width, height):
    """world_to_cam then the pinhole proj, written with torch matmuls the way
    csrc/projection_covar.hip computes them: camera-space mean R m + t and
    covariance R S R^T, the screen coordinates clamped to the image plus
    persp()'s 15 % margin, the two Jacobian rows, J S J^T."""
    R = viewmats[:, None, :3, :3]                                   # [C,1,3,3]
    p = (R @ means[None, :, :, None]).squeeze(-1) + viewmats[:, None, :3, 3]
    S = R @ covars[None] @ R.transpose(-1, -2)                      # [C,N,3,3]
    f = torch.stack([Ks[:, 0, 0], Ks[:, 1, 1]], -1)[:, None]        # [C,1,2]
    c = Ks[:, None, :2, 2]                                          # [C,1,2]
    size = torch.tensor([float(width), float(height)], device=means.device)
    iz = 1.0 / p[..., 2:3]
    margin = 0.15 * size / f
    s = torch.maximum(torch.minimum(p[..., :2] * iz, margin + (size - c) / f), -margin - c / f)
    J = torch.cat([torch.diag_embed(f * iz), (-f * s * iz)[..., None]], -1)  # [C,N,2,3]
    return f * p[..., :2] * iz + c, J @ S @ J.transpose(-1, -2)


def part_stages(iters):
    import gsplat_hip
    means, quats, scales, vm, K = scene()
    N = means.shape[0]
    covars = gsplat_hip.quat_scale_to_covar_preci(quats, scales, compute_preci=False)[0]  # [N,3,3]
    g = torch.Generator(device="cuda").manual_seed(1)
    v_m2 = torch.randn(1, N, 2, device="cuda", generator=g)
    v_c2 = torch.randn(1, N, 2, 2, device="cuda", generator=g)

    def hip_fwd(m, c):
        return gsplat_hip.proj(*gsplat_hip.world_to_cam(m, c, vm), K, W, H)

    def torch_fwd(m, c):
        return torch_stages(m, c, vm, K, W, H)

    def fwd_bwd(fn):
        m, c = means.detach().requires_grad_(True), covars.detach().requires_grad_(True)

        def run():
            m2, c2 = fn(m, c)
            return torch.autograd.grad([m2, c2], [m, c], [v_m2, v_c2])
        return run

    a, b = hip_fwd(means, covars), torch_fwd(means, covars)
    agree = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b)]
    for run in range(2):
        us = {"hip_fwd": timed(lambda: hip_fwd(means, covars), iters),
              "torch_fwd": timed(lambda: torch_fwd(means, covars), iters),
              "hip_fwd_bwd": timed(fwd_bwd(hip_fwd), iters),
              "torch_fwd_bwd": timed(fwd_bwd(torch_fwd), iters)}
        emit({"part": "stages", "run": run, "gaussians": N, "iters": iters,
              **{k + "_us": round(v, 2) for k, v in us.items()},
              "fwd_speedup": round(us["torch_fwd"] / us["hip_fwd"], 2),
              "fwd_bwd_speedup": round(us["torch_fwd_bwd"] / us["hip_fwd_bwd"], 2),
              "max_rel_diff_means2d_covars2d": [float(f"{x:.3e}") for x in agree]})


def part_models(iters):
    """proj alone for the three camera models (the fisheye scalar chain runs
    in float64), forward and forward + backward."""
    import gsplat_hip
    means, quats, scales, vm, K = scene()
    N = means.shape[0]
    covars = gsplat_hip.quat_scale_to_covar_preci(quats, scales, compute_preci=False)[0]
    mc, cc = gsplat_hip.world_to_cam(means, covars, vm)
    g = torch.Generator(device="cuda").manual_seed(2)
    v_m2 = torch.randn(1, N, 2, device="cuda", generator=g)
    v_c2 = torch.randn(1, N, 2, 2, device="cuda", generator=g)
    for run in range(2):
        row = {"part": "models", "run": run, "gaussians": N, "iters": iters}
        for model in ("pinhole", "ortho", "fisheye"):
            m, c = mc.detach().requires_grad_(True), cc.detach().requires_grad_(True)

            def fwd_bwd():
                m2, c2 = gsplat_hip.proj(m, c, K, W, H, camera_model=model)
                return torch.autograd.grad([m2, c2], [m, c], [v_m2, v_c2])

            row[model + "_fwd_us"] = round(timed(
                lambda: gsplat_hip.proj(mc, cc, K, W, H, camera_model=model), iters), 2)
            row[model + "_fwd_bwd_us"] = round(timed(fwd_bwd, iters), 2)
        emit(row)


def part_packed(iters):
    import gsplat_hip
    means, quats, scales, vm, K = scene()
    covars = gsplat_hip.quat_scale_to_covar_preci(quats, scales, compute_preci=False, triu=True)[0]
    kw = dict(eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0, packed=True)
    us = {"fwd_quats_scales": timed(lambda: gsplat_hip.fully_fused_projection(
              means, None, quats, scales, vm, K, W, H, **kw), iters),
          "fwd_covars": timed(lambda: gsplat_hip.fully_fused_projection(
              means, covars, None, None, vm, K, W, H, **kw), iters)}
    emit({"part": "packed", "gaussians": means.shape[0], "iters": iters,
          **{k + "_us": round(v, 2) for k, v in us.items()},
          "note": "event time per call: two kernels, the scan, a host read of nnz"})


def main():
    global _OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("fused", "stages", "models", "packed", "all"))
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covars",
                                                  "covar_proj_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times kernels: it needs the GPU"
    _OUT = args.out
    if _OUT:
        os.makedirs(os.path.dirname(os.path.abspath(_OUT)), exist_ok=True)
    if args.part in ("fused", "all"):
        part_fused(args.iters)
    if args.part in ("stages", "all"):
        part_stages(args.iters)
    if args.part in ("models", "all"):
        part_models(args.iters)
    if args.part == "packed":
        part_packed(args.iters)


if __name__ == "__main__":
    main()
