"""Time the k-means passes of the splat compression at the benchmark scene's
size (N = 1,006,065 rows of D = 45, K = 65,536 centroids; random data).

  assign: gsplat_hip_kmeans_l1_assign (csrc/compress.hip) against the chunked
       torch composition `torch.cdist(x_chunk, c, p=1).argmin(1)`.  Chunks
       sized to fit: torch's cdist launches one 256-thread workgroup per
       output element and HIP refuses a launch of 2^32 threads or more
       ("invalid configuration argument"), so a chunk has at most
       (2^32 - 1) / (256 K) rows -- 255 at K = 65,536 (--chunk 0: that limit).
       The composition is a loop over equal, independent chunks;
       --torch-chunks of them are timed (0: all) and the whole pass is that
       time x N / rows timed, reported as such next to the measured figure.
       The labels of the timed rows are compared.
       The kernel's arithmetic is one subtract and one add per point, centroid
       and dimension: 2 N K D vector operations.  The fp32 vector peak of
       157.3 TFLOP/s counts an FMA as two, so the peak for these one-FLOP
       instructions is 78.65 T operations/s; the achieved fraction is against
       that.
  update: gsplat_hip_kmeans_update (label sort + ordered segment means) against
       `index_add_` sums, `bincount` and a divide.
  files: PngCompression.compress of N random splats of degree 3 into a
       temporary directory: the size of each file and the bytes per Gaussian.
       File sizes only -- random parameters neither cluster nor deflate like a
       trained scene's.

HIP events around --iters back-to-back launches after a warm-up, --reps times,
the two sides alternating; min / median / max over the repetitions.  One JSON
line per measurement, also appended to --out.

    python tools/kmeans_bench.py [--part assign|update|files|all] [--n 1006065] [--k 65536]
        [--d 45] [--iters 3] [--reps 5] [--chunk 0] [--torch-chunks 64]
        [--out profiles/compression/kmeans.txt]
"""

import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat-triton_amd"))

PEAK_VALU_TOPS = 157.3 / 2  # one-FLOP vector instructions, T/s


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


def alternate(sides, iters, reps):
    """{name: [ms per call] * reps}, the sides taking turns."""
    for fn in sides.values():  # warm-up: code objects, allocator
        fn()
    out = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            out[k].append(timed(fn, iters))
    return out


def part_assign(a, log):
    from gsplat_hip import compression as C
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.n, a.d, generator=g).cuda()
    c = x[torch.randperm(a.n, generator=g)[:a.k].cuda()].contiguous()
    labels = torch.full((a.n,), -1, dtype=torch.int32, device="cuda")
    dist = torch.empty(a.n, device="cuda")
    fit = (2 ** 32 - 1) // (256 * a.k)
    a.chunk = fit if a.chunk <= 0 else min(a.chunk, fit)
    n_chunks = -(-a.n // a.chunk)
    t_chunks = n_chunks if a.torch_chunks <= 0 else min(a.torch_chunks, n_chunks)
    rows = min(t_chunks * a.chunk, a.n)
    ref = torch.empty(rows, dtype=torch.int64, device="cuda")

    def hip():
        C.kmeans_assign(x, c, labels, dist)

    def composition():
        for s in range(0, rows, a.chunk):
            ref[s:s + a.chunk] = torch.cdist(x[s:min(s + a.chunk, rows)], c, p=1).argmin(1)

    ms = alternate({"hip": hip, "torch": composition}, a.iters, a.reps)
    ops = 2.0 * a.n * a.k * a.d
    med = statistics.median(ms["hip"])
    log(measure="assign, hip kernel", N=a.n, K=a.k, D=a.d, **spread(ms["hip"]),
        vector_tops=round(ops / (med * 1e-3) / 1e12, 2),
        frac_of_fp32_valu_peak=round(ops / (med * 1e-3) / 1e12 / PEAK_VALU_TOPS, 4))
    scale = a.n / rows
    log(measure="assign, torch cdist(p=1).argmin composition", rows_timed=rows, chunk=a.chunk,
        **spread(ms["torch"]),
        whole_pass_ms=round(statistics.median(ms["torch"]) * scale, 2),
        whole_pass_is="measured" if rows == a.n else f"rows_timed x {scale:.2f}")
    log(measure="assign, torch / hip", ratio=round(statistics.median(ms["torch"]) * scale / med, 1))
    diff = int((labels[:rows].long() != ref).sum())
    log(measure="assign, labels differing from the composition's", rows=rows, differing=diff)


def part_update(a, log):
    from gsplat_hip import compression as C
    g = torch.Generator().manual_seed(1)
    x = torch.randn(a.n, a.d, generator=g).cuda()
    labels = torch.randint(0, a.k, (a.n,), generator=g, dtype=torch.int32).cuda()
    long_labels = labels.long()
    c0 = torch.randn(a.k, a.d, generator=g).cuda()
    cents = c0.clone()
    counts = torch.empty(a.k, dtype=torch.int32, device="cuda")
    ws = C.kmeans_workspace(a.n, "cuda")
    out = {}

    def hip():
        C.kmeans_update(x, labels, cents, counts, ws)

    def composition():
        sums = torch.zeros(a.k, a.d, device="cuda").index_add_(0, long_labels, x)
        n = torch.bincount(long_labels, minlength=a.k)
        out["c"] = torch.where(n[:, None] > 0, sums / n[:, None].clamp(min=1), c0)

    ms = alternate({"hip": hip, "torch": composition}, a.iters, a.reps)
    log(measure="update, hip (sort + ordered means)", N=a.n, K=a.k, D=a.d, **spread(ms["hip"]))
    log(measure="update, torch index_add_ / bincount composition", **spread(ms["torch"]))
    log(measure="update, torch / hip",
        ratio=round(statistics.median(ms["torch"]) / statistics.median(ms["hip"]), 2))
    log(measure="update, max |hip - composition|", value=float((cents - out["c"]).abs().max()))


def part_files(a, log):
    from gsplat_hip import PngCompression
    g = torch.Generator().manual_seed(2)
    N = a.n
    sp = {"means": torch.randn(N, 3, generator=g) * 3, "scales": torch.randn(N, 3, generator=g),
          "quats": torch.randn(N, 4, generator=g), "opacities": torch.randn(N, generator=g),
          "sh0": torch.randn(N, 1, 3, generator=g) * 0.5,
          "shN": torch.randn(N, (a.d // 3), 3, generator=g) * 0.1}
    sp = {k: v.cuda() for k, v in sp.items()}
    with tempfile.TemporaryDirectory() as d:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        PngCompression(verbose=False, n_clusters=a.k).compress(d, sp)
        e.record()
        torch.cuda.synchronize()
        sizes = {f: os.path.getsize(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    n = int(N ** 0.5) ** 2
    raw = sum(v.numel() * 4 for v in sp.values()) / N
    log(measure="files, random splats (file sizes only)", N=N, num_GS=n, files=sizes,
        total_bytes=sum(sizes.values()), bytes_per_gaussian=round(sum(sizes.values()) / n, 2),
        fp32_bytes_per_gaussian=raw, compress_wall_ms=round(s.elapsed_time(e), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("assign", "update", "files", "all"))
    ap.add_argument("--n", type=int, default=1006065)
    ap.add_argument("--k", type=int, default=65536)
    ap.add_argument("--d", type=int, default=45)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--torch-chunks", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compression", "kmeans.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kmeans_bench.py measures on the GPU"
    log = Log(a.out)
    log(measure="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)
    if a.part in ("assign", "all"):
        part_assign(a, log)
    if a.part in ("update", "all"):
        part_update(a, log)
    if a.part in ("files", "all"):
        part_files(a, log)


if __name__ == "__main__":
    main()
