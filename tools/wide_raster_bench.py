"""Time the wide-channel rasterizer (csrc/rasterize_wide.hip, `wide=True`)
against the chunked path (D / 32 renders of 32 channels) on the same isects,
HIP events, in one process.

A 1920x1080 view of the garden scene's geometry at M2 (scene_grid=3,
1,006,065 Gaussians: colours [N, 512] and their gradients are 2 GB each),
random feature colours with D in --dims.  Per D, alternating, two runs each:

  forward            rasterize_to_pixels under no_grad
  forward+backward   with a loss on colours and alphas, gradients of means2d,
                     conics, colours and opacities

Every figure is event time per Python call (wrapper, allocations and launches
included), not kernel time: for kernel times run this tool under
`rocprofv3 --kernel-trace --stats` (no counters in the same run; kernels
wide_fwd_kernel / wide_bwd_kernel).  `product_flop`: the three matrix
products over every isect of every tile, 2 * 256 * n_isects * D each (the
forward's one, the backward's two) -- an upper bound on what the kernels
issue, which skip Gaussians no pixel takes and tiles that terminated.
Prints one JSON line per measurement and appends them to
profiles/wide_raster/wide_raster.txt (--out).

    python tools/wide_raster_bench.py [--dims 64 128 256 512] [--iters 5]
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat-triton_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from contrib_bench import projected, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 128, 256, 512])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_raster",
                                                  "wide_raster.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times kernels: it needs the GPU"
    import gsplat_hip
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    W, H = 1920, 1080
    m2, cn, op, off, fids = projected(3, W, H)
    N = m2.shape[1]
    gen = torch.Generator("cuda").manual_seed(0)
    for D in args.dims:
        colors = torch.rand(1, N, D, device="cuda", generator=gen)
        vc = torch.randn(1, H, W, D, device="cuda", generator=gen)
        va = torch.randn(1, H, W, 1, device="cuda", generator=gen)

        def fwd(wide):
            with torch.no_grad():
                return gsplat_hip.rasterize_to_pixels(m2, cn, colors, op, W, H, 16, off, fids,
                                                      wide=wide)

        def fwd_bwd(wide):
            ins = [x.detach().requires_grad_(True) for x in (m2, cn, colors, op)]
            rc, ra = gsplat_hip.rasterize_to_pixels(*ins, W, H, 16, off, fids, wide=wide)
            return torch.autograd.grad((rc * vc).sum() + (ra * va).sum(), ins)

        # the two paths agree before they are timed
        diff = {"colors": float((fwd(True)[0] - fwd(False)[0]).abs().max())}
        for k, a, b in zip(("v_means2d", "v_conics", "v_colors", "v_opacities"), fwd_bwd(True),
                           fwd_bwd(False)):
            diff[k] = float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))
        for run in range(2):
            us = {f"{n}_{p}": timed(lambda: f(p == "wide"), args.iters)
                  for n, f in (("fwd", fwd), ("fwd_bwd", fwd_bwd)) for p in ("chunked", "wide")}
            line = json.dumps({
                "D": D, "run": run, "gaussians": N, "isects": fids.numel(), "iters": args.iters,
                **{k + "_us": round(v, 1) for k, v in us.items()},
                "fwd_speedup": round(us["fwd_chunked"] / us["fwd_wide"], 2),
                "fwd_bwd_speedup": round(us["fwd_bwd_chunked"] / us["fwd_bwd_wide"], 2),
                "product_flop": 2 * 256 * fids.numel() * D,
                "max_abs_diff_colors": diff["colors"],
                "max_diff_over_max_grad": {k: v for k, v in diff.items() if k != "colors"},
                "note": "event time per call: launches, wrapper and allocations included"})
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        del colors, vc, va
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
