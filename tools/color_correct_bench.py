"""Time gsplat_hip.color_correct on one 1920x1080 image, 5 iterations.

  call:      event time per call of the kernels (csrc/color_correct.hip)
             against two torch compositions of the same algebra on the same
             device tensors, the sides taking turns, --reps repetitions of
             --iters back-to-back calls after a warm-up:
               lstsq   per iteration and channel torch.linalg.lstsq on the
                       masked [P,10] float32 matrix, as the reference's
                       examples/lib_bilagrid.py does (skipped, and said so, if
                       torch refuses the shape on this device)
               normal  the masked normal equations in torch float64 and a
                       Cholesky solve
             and the kernels' result against the `normal` composition.
             GB/s is against the byte model: per pixel and iteration the sums
             read x, ref and img (36 B; 24 B in the first iteration, where x
             is img) and the warp reads and writes x (24 B); the three channel
             blocks' re-reads are left to the caches.
  resources: the accumulate kernel's registers and spills, from
             `hipcc -Rpass-analysis=kernel-resource-usage` (no GPU needed).
  kernels:   --iters calls and nothing else, for
             `rocprofv3 --kernel-trace --stats -- python tools/color_correct_bench.py
             --part kernels` in a run of its own;
  stats:     reads that run's kernel stats CSV (--stats-csv) and records the
             three kernels' mean times.

One JSON line per measurement, appended to --out (`call` starts the file).

    python tools/color_correct_bench.py [--part call|resources|kernels|stats] [--iters 20]
        [--reps 5] [--out profiles/color_correct/color_correct.txt] [--stats-csv FILE]
"""

import argparse
import csv
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat-triton_amd"))

W, H, NUM_ITERS, EPS = 1920, 1080, 5, 0.5 / 255
HBM_PEAK_GBS = 8000.0
KERNELS = ("accumulate_kernel", "solve_kernel", "warp_kernel")


class Log:
    def __init__(self, path, fresh):
        self.path = path
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            if fresh:
                open(path, "w").close()  # a `call` run replaces the record

    def __call__(self, **kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if self.path:
            with open(self.path, "a") as f:
                f.write(line + "\n")


def scene(torch, dev):
    """A smooth textured reference plus noise and its image under a gain and a
    gamma per channel with the highlights clipped, [H,W,3] float32."""
    g = torch.Generator().manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, indexing="ij")
    tex = torch.stack([0.5 + 0.25 * torch.sin(6.0 * xs + 1.0 + c) * torch.cos(5.0 * ys - c)
                       + 0.15 * torch.sin(23.0 * (xs + ys) + 2.0 * c) for c in range(3)], -1)
    ref = (tex + 0.02 * torch.randn(H, W, 3, generator=g)).clamp(0.0, 1.0)
    gain = torch.tensor([1.25, 1.1, 0.95])
    gamma = torch.tensor([1.3, 1.5, 1.7])
    img = (gain * ref.clamp_min(1e-3) ** gamma
           + 0.01 * torch.randn(H, W, 3, generator=g)).clamp(0.0, 1.0)
    return img.to(dev), ref.to(dev)


def features(torch, x):
    x0, x1, x2 = x[:, 0], x[:, 1], x[:, 2]
    return torch.stack([x0 * x0, x0 * x1, x0 * x2, x1 * x1, x1 * x2, x2 * x2, x0, x1, x2,
                        torch.ones_like(x0)], 1)


def torch_composition(torch, img, ref, solver):
    """The definition of include/gsplat_hip.h's color_correct in torch ops:
    solver "lstsq" (float32, the masked matrix) or "normal" (float64)."""
    lo = torch.tensor(EPS, dtype=torch.float32, device=img.device)
    hi = torch.tensor(1.0 - EPS, dtype=torch.float32, device=img.device)
    dt = torch.float32 if solver == "lstsq" else torch.float64
    x = img.reshape(-1, 3)
    r = ref.reshape(-1, 3)
    m0 = (x >= lo) & (x <= hi)
    mr = (r >= lo) & (r <= hi)
    for _ in range(NUM_ITERS):
        a = features(torch, x.to(dt))
        m = m0 & (x >= lo) & (x <= hi) & mr
        cols = []
        for c in range(3):
            am = a * m[:, c:c + 1].to(dt)
            b = r[:, c].to(dt) * m[:, c].to(dt)
            if solver == "lstsq":
                cols.append(torch.linalg.lstsq(am, b[:, None]).solution[:, 0])
            else:
                L = torch.linalg.cholesky(am.T @ am)
                cols.append(torch.cholesky_solve((am.T @ b)[:, None], L)[:, 0])
        x = (a @ torch.stack(cols, 1)).clamp(0.0, 1.0).float()
    return x.reshape(img.shape)


def timed(torch, fn, iters):
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


def part_call(log, iters, reps):
    import torch
    assert torch.cuda.is_available(), "color_correct_bench.py measures on the GPU"
    import gsplat_hip
    log(measure="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)
    img, ref = scene(torch, "cuda")
    P = W * H
    log(measure="case", width=W, height=H, num_iters=NUM_ITERS,
        saturated_share=round(float((img >= 1.0).float().mean()), 4))
    sides = {"kernels": lambda: gsplat_hip.color_correct(img, ref, NUM_ITERS, EPS)}
    try:
        torch_composition(torch, img, ref, "lstsq")
        torch.cuda.synchronize()
        sides["lstsq"] = lambda: torch_composition(torch, img, ref, "lstsq")
    except Exception as ex:  # noqa: BLE001 -- recorded, the other composition stands in
        log(measure="torch.linalg.lstsq refused the shape; the float64 normal equations in torch "
                    "are the comparison", error=f"{type(ex).__name__}: {str(ex)[:200]}")
    sides["normal"] = lambda: torch_composition(torch, img, ref, "normal")
    got, info = gsplat_hip.color_correct(img, ref, NUM_ITERS, EPS, return_info=True)
    want = torch_composition(torch, img, ref, "normal")
    log(measure="max |kernels - torch float64 normal equations|",
        value=float((got - want).abs().max()), fallbacks=int(info["fallbacks"].sum()),
        psnr_before=round(float(-10 * torch.log10(((img - ref) ** 2).mean())), 2),
        psnr_after=round(float(-10 * torch.log10(((got - ref) ** 2).mean())), 2))
    for fn in sides.values():  # warm-up: code objects, allocator, solver handles
        fn()
    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            ms[k].append(timed(torch, fn, iters if k == "kernels" else max(iters // 10, 2)))
    model = P * (60.0 * NUM_ITERS - 12.0)
    med = statistics.median(ms["kernels"])
    gbs = model / (med * 1e-3) / 1e9
    log(measure="kernels, gsplat_hip.color_correct, per call", **spread(ms["kernels"]),
        launches=3 * NUM_ITERS, model_bytes=int(model), GBps=round(gbs, 1),
        frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 3))
    names = {"lstsq": "torch composition, float32 lstsq on the masked matrix, per call",
             "normal": "torch composition, float64 masked normal equations, per call"}
    for k in ("lstsq", "normal"):
        if k in ms:
            log(measure=names[k], **spread(ms[k]),
                ratio_to_kernels=round(statistics.median(ms[k]) / med, 1))


def part_resources(log):
    src = os.path.join(ROOT, "gsplat-triton_amd", "csrc", "color_correct.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950",
                          "-munsafe-fp-atomics", "-Rpass-analysis=kernel-resource-usage",
                          "--cuda-device-only", "-c", src, "-o", os.devnull],
                         capture_output=True, text=True, check=True).stderr
    cur, res = None, {}
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and cur:
            res.setdefault(cur, {})[m.group(1).strip()] = m.group(2)
    for name, r in res.items():
        short = next((k for k in KERNELS if k in name), None)
        if short:
            log(measure=f"resources, {short}", VGPRs=int(r["VGPRs"]), AGPRs=int(r["AGPRs"]),
                VGPR_spills=int(r["VGPRs Spill"]), SGPR_spills=int(r["SGPRs Spill"]),
                scratch_bytes_per_lane=int(r["ScratchSize"]),
                waves_per_SIMD=int(r["Occupancy"]), LDS_bytes=int(r["LDS Size"]))


def part_kernels(iters):
    import torch
    assert torch.cuda.is_available(), "color_correct_bench.py measures on the GPU"
    import gsplat_hip
    img, ref = scene(torch, "cuda")
    for _ in range(iters):
        gsplat_hip.color_correct(img, ref, NUM_ITERS, EPS)
    torch.cuda.synchronize()


def part_stats(log, path):
    rows = list(csv.DictReader(open(path)))
    for k in KERNELS:
        for r in rows:
            if k in r["Name"]:
                log(measure=f"kernel time, {k}", calls=int(r["Calls"]),
                    mean_us=round(float(r["AverageNs"]) / 1e3, 2),
                    min_us=round(float(r["MinNs"]) / 1e3, 2),
                    max_us=round(float(r["MaxNs"]) / 1e3, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="call", choices=("call", "resources", "kernels", "stats"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_correct",
                                                  "color_correct.txt"))
    ap.add_argument("--stats-csv")
    a = ap.parse_args()
    log = Log(a.out, fresh=a.part == "call")
    if a.part == "call":
        part_call(log, a.iters, a.reps)
    elif a.part == "resources":
        part_resources(log)
    elif a.part == "kernels":
        part_kernels(a.iters)
    else:
        part_stats(log, a.stats_csv)


if __name__ == "__main__":
    main()
