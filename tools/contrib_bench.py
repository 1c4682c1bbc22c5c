"""Time the contribution-score pass (csrc/rasterize_score.hip), HIP events, in
one process:

  forward:      at M2 (garden scene_grid=3, 1,006,065 Gaussians, one 1920x1080
                camera) `rasterize_to_contributions` beside the
                `rasterize_to_pixels` forward at D=3 on the same isects,
                alternating, two runs each.  Both walk the same records; the
                score pass adds the reductions over the pixels and one atomic
                per (record, tile) that some pixel blended, and drops the
                colours.
  composition:  on a scene small enough for it (scene_grid=1, 480x270), the
                same scores composed from `rasterize_to_indices_in_range` and
                the `accumulate` weights, which write every (pixel, Gaussian)
                pair to memory first; the pairs and their bytes are printed,
                and the two results compared.

Every figure is event time per Python call (wrapper, allocations and launches
included), not kernel time: for kernel times run this tool under
`rocprofv3 --kernel-trace --stats` (no counters in the same run).  Prints one
JSON line per measurement and appends them to profiles/contrib/contrib_bench.txt
(--out).

    python tools/contrib_bench.py [--part forward|composition|all] [--iters 100]
"""

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat-triton_amd"))

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


def projected(grid, W, H):
    """The trainer's initial Gaussians of the garden scene, projected to its
    first camera and intersected with 16-pixel tiles."""
    import gsplat_hip
    from gsplat_hip.train_step import Trainer, camera_pool, load_garden_scene
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(ROOT, "tests", "golden", "garden_scene.npz"), scene_grid=grid)
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=8)
    tr = Trainer(means, rgbs, vm.float(), K.float(), W, H, sh_degree=3, device="cuda")
    p = {k: v.data.clone() for k, v in tr.params.items()}
    vm0, K0 = tr.viewmats[:1].contiguous().clone(), tr.Ks[:1].contiguous().clone()
    del tr
    torch.cuda.empty_cache()
    radii, m2, d, cn, _ = gsplat_hip.fully_fused_projection(
        p["means"], None, p["quats"], torch.exp(p["scales"]), vm0, K0, W, H)
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    _, ids, fids = gsplat_hip.isect_tiles(m2, radii, d, 16, tw, th)
    off = gsplat_hip.isect_offset_encode(ids, 1, tw, th)
    return m2, cn, torch.sigmoid(p["opacities"])[None].contiguous(), off, fids


def part_forward(iters):
    import gsplat_hip
    W, H = 1920, 1080
    m2, cn, op, off, fids = projected(3, W, H)
    N = m2.shape[1]
    colors = torch.rand(1, N, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(0))

    def fwd():
        with torch.no_grad():
            return gsplat_hip.rasterize_to_pixels(m2, cn, colors, op, W, H, 16, off, fids)

    def score():
        return gsplat_hip.rasterize_to_contributions(m2, cn, op, W, H, 16, off, fids)

    s, m, n = score()
    _, alphas = fwd()
    for run in range(2):
        us = {"forward_d3": timed(fwd, iters), "scores": timed(score, iters)}
        emit({"part": "forward", "run": run, "gaussians": N, "isects": fids.numel(),
              "blended_pairs": int(n.sum()), "scored_gaussians": int((n > 0).sum()),
              "iters": iters, **{k + "_us": round(v, 2) for k, v in us.items()},
              "scores_over_forward": round(us["scores"] / us["forward_d3"], 3),
              # every blended pair is in exactly one sum and one pixel's alpha
              "sum_w_rel_diff_to_alphas": float(f"{abs(float(s.sum() / alphas.sum()) - 1):.3e}"),
              "note": "event time per call: launch(es), wrapper and allocations included"})


def composed_scores(m2, cn, op, W, H, off, fids):
    """The scores from the per-pixel contributor lists: every blended (pixel,
    Gaussian) pair is written out, then reduced per Gaussian with torch."""
    import gsplat_hip
    from gsplat_hip._wrapper_indices import _num_batches, _render_weights
    N = m2.shape[1]
    trans = torch.ones(1, H, W, device="cuda")
    gs, pix, cam = gsplat_hip.rasterize_to_indices_in_range(
        0, _num_batches(off, len(fids), 16), trans, m2, cn, op, W, H, 16, off, fids)
    d = torch.stack([pix % W, pix // W], -1) + 0.5 - m2[cam, gs]
    c = cn[cam, gs]
    sig = 0.5 * (c[:, 0] * d[:, 0] ** 2 + c[:, 2] * d[:, 1] ** 2) + c[:, 1] * d[:, 0] * d[:, 1]
    w = _render_weights(torch.clamp_max(op[cam, gs] * torch.exp(-sig), 0.999), cam * H * W + pix)
    s = torch.zeros(N, device="cuda").index_add_(0, gs, w)
    m = torch.zeros(N, device="cuda").scatter_reduce_(0, gs, w, "amax")
    return s, m, torch.bincount(gs, minlength=N), gs.numel()


def part_composition(iters):
    import gsplat_hip
    W, H = 480, 270
    m2, cn, op, off, fids = projected(1, W, H)
    s, m, n = gsplat_hip.rasterize_to_contributions(m2, cn, op, W, H, 16, off, fids)
    rs, rm, rn, pairs = composed_scores(m2, cn, op, W, H, off, fids)
    for run in range(2):
        us = {"scores": timed(lambda: gsplat_hip.rasterize_to_contributions(
                  m2, cn, op, W, H, 16, off, fids), iters),
              "composition": timed(lambda: composed_scores(m2, cn, op, W, H, off, fids),
                                   max(3, iters // 10))}
        emit({"part": "composition", "run": run, "gaussians": m2.shape[1],
              "isects": fids.numel(), "pairs": pairs,
              "pair_bytes_written": pairs * 16,  # two int64 lists, before any weight
              "iters": iters, **{k + "_us": round(v, 2) for k, v in us.items()},
              "speedup": round(us["composition"] / us["scores"], 1),
              "max_abs_diff": {"sum": float((s[0] - rs).abs().max()),
                               "max": float((m[0] - rm).abs().max()),
                               "count": int((n[0] - rn).abs().max())}})


def main():
    global _OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("forward", "composition", "all"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrib",
                                                  "contrib_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times kernels: it needs the GPU"
    _OUT = args.out
    if _OUT:
        os.makedirs(os.path.dirname(os.path.abspath(_OUT)), exist_ok=True)
    if args.part in ("forward", "all"):
        part_forward(args.iters)
    if args.part in ("composition", "all"):
        part_composition(args.iters)


if __name__ == "__main__":
    main()
