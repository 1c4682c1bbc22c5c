"""Time the undistortion of one camera's images at a capture's size: one
4000x3000 OPENCV camera, B = 8 uint8 images sharing its map.

  kernel: gsplat_hip.undistort_images (csrc/undistort.hip, the analytic map)
       and gsplat_hip.remap_bilinear (the same remap from map tensors), by HIP
       events around --iters back-to-back launches after a warm-up, --reps
       times, the two taking turns; min / median / max over the repetitions.
       GB/s is against the byte model: per output pixel and image 3 B read
       (every source byte is needed once; its reuse by the neighbouring
       output pixels comes from the caches) and 12 B written; the table form
       also reads its 8 B of map per output pixel once for the B images.  The
       kernel is memory-bound: the share is of the 8.0 TB/s HBM peak.
  host: colmap.undistort_host (numpy, the map tables already built) on ONE of
       the images, wall clock on the same machine, and colmap.undistort_maps
       (building the tables, once per camera).
  check: the kernel's first image against the host path's.

One JSON line per measurement, also written to --out.

    python tools/undistort_bench.py [--width 4000] [--height 3000] [--batch 8] [--iters 5]
        [--reps 5] [--out profiles/undistort/undistort.txt]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat-triton_amd"))

HBM_PEAK_GBS = 8000.0


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def spread(ms):
    return dict(ms_min=round(min(ms), 4), ms_median=round(statistics.median(ms), 4),
                ms_max=round(max(ms), 4), reps=len(ms))


class Log:
    def __init__(self, path):
        self.path = path
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            open(path, "w").close()  # a run replaces the record

    def __call__(self, **kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if self.path:
            with open(self.path, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort", "undistort.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "undistort_bench.py measures on the GPU"
    from gsplat_hip import colmap as M
    from gsplat_hip import remap_bilinear, undistort_images
    log = Log(a.out)
    log(measure="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)

    W, H, B = a.width, a.height, a.batch
    f = 0.75 * W
    K = np.array([[f, 0.0, 0.5025 * W], [0.0, 0.997 * f, 0.49 * H], [0.0, 0.0, 1.0]])
    params = [-0.15, 0.03, 0.004, -0.003]
    K_new, roi = M.optimal_new_camera_matrix(K, params, (W, H))
    t0 = time.perf_counter()
    mapx, mapy = M.undistort_maps(K, params, K_new, (W, H), "perspective")
    t_maps = time.perf_counter() - t0
    x, y, w, h = roi
    rng = np.random.default_rng(0)
    # a smooth image plus noise, one per batch entry (the content does not change the traffic)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32),
                         indexing="ij")
    base = 127.5 + 100.0 * np.sin(0.01 * xx) * np.cos(0.013 * yy)
    imgs = np.stack([np.clip(base[..., None] + rng.normal(0, 8, (H, W, 3)), 0, 255).astype(np.uint8)
                     for _ in range(B)])
    u8 = torch.from_numpy(imgs).cuda()
    out = torch.empty((B, h, w, 3), device="cuda")
    mx = torch.from_numpy(np.ascontiguousarray(mapx[y:y + h, x:x + w])).cuda()
    my = torch.from_numpy(np.ascontiguousarray(mapy[y:y + h, x:x + w])).cuda()
    log(measure="case", model="OPENCV", width=W, height=H, batch=B, params=params, roi=list(roi),
        source_MB=round(u8.numel() / 1e6, 1), output_MB=round(out.numel() * 4 / 1e6, 1))

    sides = {"analytic": lambda: undistort_images(u8, K, params, K_new, roi, scale=1 / 255.0,
                                                  out=out),
             "table": lambda: remap_bilinear(u8, mx, my, scale=1 / 255.0, out=out)}
    for fn in sides.values():  # warm-up: code objects, allocator
        fn()
    ms = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, fn in sides.items():
            ms[k].append(timed(fn, a.iters))
    npx = float(h) * w
    model = {"analytic": B * npx * 15.0, "table": B * npx * 15.0 + npx * 8.0}
    for k, what in (("analytic", "kernel, analytic map (undistort_images)"),
                    ("table", "kernel, map tables (remap_bilinear)")):
        med = statistics.median(ms[k])
        gbs = model[k] / (med * 1e-3) / 1e9
        log(measure=what, **spread(ms[k]), ms_per_image=round(med / B, 4),
            model_bytes=int(model[k]), GBps=round(gbs, 1),
            frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 3))

    t0 = time.perf_counter()
    host = M.undistort_host(imgs[0], mapx, mapy, roi)
    t_host = time.perf_counter() - t0
    log(measure="host, undistort_host (numpy), ONE image", wall_s=round(t_host, 3),
        maps_once_per_camera_wall_s=round(t_maps, 3))
    med = statistics.median(ms["analytic"])
    log(measure="host / kernel, per image", ratio=round(t_host / (med * 1e-3 / B), 0))
    got = undistort_images(u8[:1], K, params, K_new, roi)[0].cpu().numpy()
    log(measure="max |kernel - host| on the first image (levels)",
        value=float(np.abs(got - host).max()))


if __name__ == "__main__":
    main()
