"""Time gsplat_hip.knn(points, 4) and the SfM scale initialisation it serves,
at the benchmark scene's 1,006,065 points and on a clustered cloud of the same
size (99 % of the points in 1 % of the box).

  call:     per cloud, --reps repetitions after a warm-up of
              device   event time of knn(points, 4, validate=False), --iters
                       back-to-back calls (csrc/knn.hip, every launch of it)
              hip      wall clock of knn_log_scales(points.to(device),
                       backend="hip").cpu() from host points to host scales,
                       ending in the copy back (a synchronise)
              host     wall clock of knn_log_scales(points), today's k-d tree
            the sides taking turns, and the largest difference of the two
            log-scales.
  kernels:  --iters calls on the scene cloud and nothing else, for
            `rocprofv3 --kernel-trace --stats -- python tools/knn_bench.py
            --part kernels` in a run of its own;
  stats:    reads that run's kernel stats CSV (--stats-csv) and records the
            time per call of the stages: box+keys, sort, gather, search.

One JSON line per measurement, appended to --out (`call` starts the file).

    python tools/knn_bench.py [--part call|kernels|stats] [--iters 10] [--reps 5]
        [--out profiles/knn/knn.txt] [--stats-csv FILE]
"""

import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat-triton_amd"))

K = 4
# kernel-name fragment -> stage (keys_hi gathers through the first permutation
# but is a key pass: it re-derives the key from the point)
STAGES = (("box_partial", "box+keys"), ("box_final", "box+keys"), ("keys_lo", "box+keys"),
          ("keys_hi", "box+keys"), ("hist_kernel", "sort"), ("scan_kernel", "sort"),
          ("scatter_kernel", "sort"), ("gather_kernel", "gather"), ("search_kernel", "search"))


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


def clouds(torch):
    from gsplat_hip.train_step import load_garden_scene
    scene = load_garden_scene(os.path.join(ROOT, "tests", "golden", "garden_scene.npz"),
                              scene_grid=3)[0].float().contiguous()
    N = scene.shape[0]
    g = torch.Generator().manual_seed(0)
    n_core = N * 99 // 100
    core = 0.4 + torch.rand(n_core, 3, generator=g) * 0.01 ** (1.0 / 3.0)
    clustered = torch.cat([core, torch.rand(N - n_core, 3, generator=g)])
    return {"scene": scene, "clustered": clustered[torch.randperm(N, generator=g)].contiguous()}


def spread(ms):
    return dict(ms_min=round(min(ms), 3), ms_median=round(statistics.median(ms), 3),
                ms_max=round(max(ms), 3), reps=len(ms))


def part_call(log, iters, reps):
    import torch
    assert torch.cuda.is_available(), "knn_bench.py measures on the GPU"
    import gsplat_hip
    from gsplat_hip.train_step import knn_log_scales
    log(measure="device", name=torch.cuda.get_device_name(0), torch=torch.__version__,
        host_cpus=len(os.sched_getaffinity(0)))
    for name, pts in clouds(torch).items():
        dev = pts.to("cuda")
        log(measure="case", cloud=name, points=pts.shape[0], k=K)

        def device():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(iters):
                gsplat_hip.knn(dev, K, validate=False)
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) / iters

        def wall(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            return (time.perf_counter() - t) * 1e3, out

        sides = {"device": device,
                 "hip": lambda: wall(lambda: knn_log_scales(pts.to("cuda"), backend="hip").cpu()),
                 "host": lambda: wall(lambda: knn_log_scales(pts))}
        gsplat_hip.knn(dev, K)  # warm-up: code objects, allocator
        ms, out = {k: [] for k in sides}, {}
        for _ in range(reps):
            for k, fn in sides.items():
                r = fn()
                ms[k].append(r if k == "device" else r[0])
                if k != "device":
                    out[k] = r[1]
        log(measure="max |log-scale hip - host|", cloud=name,
            value=float((out["hip"] - out["host"]).abs().max()))
        log(measure="device: knn(points, 4, validate=False), event time per call", cloud=name,
            **spread(ms["device"]))
        log(measure="hip: knn_log_scales(backend='hip'), host points to host scales, wall clock",
            cloud=name, **spread(ms["hip"]))
        log(measure="host: knn_log_scales(backend='host'), k-d tree, wall clock", cloud=name,
            **spread(ms["host"]),
            ratio_to_hip=round(statistics.median(ms["host"]) / statistics.median(ms["hip"]), 2))


def part_kernels(iters):
    import torch
    assert torch.cuda.is_available(), "knn_bench.py measures on the GPU"
    import gsplat_hip
    dev = clouds(torch)["scene"].to("cuda")
    for _ in range(iters):
        gsplat_hip.knn(dev, K, validate=False)
    torch.cuda.synchronize()


def part_stats(log, path, iters):
    total = {}
    for r in csv.DictReader(open(path)):
        stage = next((s for frag, s in STAGES if frag in r["Name"]), None)
        if stage:
            t = total.setdefault(stage, [0, 0.0])
            t[0] += int(r["Calls"])
            t[1] += int(r["Calls"]) * float(r["AverageNs"])
    for stage, (calls, ns) in total.items():
        log(measure=f"kernel time per call, {stage}", cloud="scene", launches_per_call=calls // iters,
            ms=round(ns / iters / 1e6, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="call", choices=("call", "kernels", "stats"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn", "knn.txt"))
    ap.add_argument("--stats-csv")
    a = ap.parse_args()
    log = Log(a.out, fresh=a.part == "call")
    if a.part == "call":
        part_call(log, a.iters, a.reps)
    elif a.part == "kernels":
        part_kernels(a.iters)
    else:
        part_stats(log, a.stats_csv, a.iters)


if __name__ == "__main__":
    main()
