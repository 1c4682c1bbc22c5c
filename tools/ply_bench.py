"""Time the PLY export at the size of a trained scene: N = 1,006,065 Gaussians
at SH degree 3 (F = 62 floats per row, a 250 MB file), 1 % of the rows invalid.

  kernel: gsplat_hip_ply_count and gsplat_hip_ply_pack (csrc/ply.hip) on the
       whole N in one call each, by HIP events around --iters back-to-back
       launches after a warm-up, --reps times, taking turns with the torch
       composition; min / median / max over the repetitions.  GB/s of the pack
       is against the byte model 2 * 4 * F * N (every kept float read once and
       written once); the kernel is memory-bound: the share is of the 8.0 TB/s
       HBM peak.
  torch: the same rows built by torch: `cat` of the permuted views plus a
       boolean index with the finite-row mask (what a device path without the
       kernel would be).
  check: the kernel's rows equal the torch composition's bit for bit.
  end to end: gsplat_hip.save_ply and load_ply, wall clock, the tensors on the
       GPU against the same tensors on the CPU (the numpy path), into --tmp.

One JSON line per measurement, also written to --out.

    python tools/ply_bench.py [--n 1006065] [--iters 5] [--reps 5]
        [--out profiles/ply/ply.txt] [--tmp /tmp]
"""

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1006065)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ply", "ply.txt"))
    ap.add_argument("--tmp", default=tempfile.gettempdir())
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ply_bench.py measures on the GPU"
    from gsplat_hip import _lib, load_ply, save_ply
    from gsplat_hip._wrapper import _stream
    log = Log(a.out)
    log(measure="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)

    N, K1 = a.n, 15
    F = 17 + 3 * K1
    g = torch.Generator().manual_seed(0)
    s = dict(means=torch.randn(N, 3, generator=g), scales=torch.randn(N, 3, generator=g),
             quats=torch.randn(N, 4, generator=g), opacities=torch.randn(N, generator=g),
             sh0=torch.randn(N, 1, 3, generator=g), shN=torch.randn(N, K1, 3, generator=g))
    bad = torch.randperm(N, generator=g)[:N // 100]
    s["means"][bad[::2], 0] = float("nan")
    s["shN"][bad[1::2], 7, 1] = float("inf")
    d = {k: v.cuda() for k, v in s.items()}
    log(measure="case", n=N, sh_degree=3, floats_per_row=F, invalid_rows=int(bad.numel()),
        file_MB=round(4 * F * (N - bad.numel()) / 1e6, 1))

    ws = torch.empty(int(_lib.query("gsplat_hip_ply_workspace_bytes", N)), dtype=torch.uint8,
                     device="cuda")
    n_valid = torch.zeros(1, dtype=torch.int64, device="cuda")
    rows = torch.empty(N * F, device="cuda")
    ptrs = [d[k].data_ptr() for k in ("means", "scales", "quats", "opacities", "sh0", "shN")]

    def count():
        _lib.call("gsplat_hip_ply_count", N, K1, *ptrs, 0, ws.data_ptr(), n_valid.data_ptr(),
                  _stream())

    def pack():
        _lib.call("gsplat_hip_ply_pack", N, K1, *ptrs, 0, ws.data_ptr(), rows.data_ptr(),
                  _stream())

    def composition():
        r = torch.cat([d["means"], torch.zeros_like(d["means"]),
                       d["sh0"].permute(0, 2, 1).reshape(N, -1),
                       d["shN"].permute(0, 2, 1).reshape(N, -1), d["opacities"][:, None],
                       d["scales"], d["quats"]], dim=1)
        return r[torch.isfinite(r).all(dim=1)]

    sides = {"count": count, "pack": pack, "torch": composition}
    for fn in sides.values():  # warm-up: code objects, allocator
        fn()
    ms = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, fn in sides.items():
            ms[k].append(timed(fn, a.iters))
    nv = int(n_valid.item())
    model = 2.0 * 4.0 * F * nv
    for k, what in (("count", "kernel, validity + counts + scan (gsplat_hip_ply_count)"),
                    ("pack", "kernel, pack (gsplat_hip_ply_pack)"),
                    ("torch", "torch composition (cat of permuted views + boolean index)")):
        med = statistics.median(ms[k])
        extra = {}
        if k == "pack":
            gbs = model / (med * 1e-3) / 1e9
            extra = dict(model_bytes=int(model), GBps=round(gbs, 1),
                         frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 3))
        log(measure=what, **spread(ms[k]), **extra)
    both = statistics.median(ms["count"]) + statistics.median(ms["pack"])
    log(measure="torch composition / (count + pack)",
        ratio=round(statistics.median(ms["torch"]) / both, 2))
    ref = composition()
    log(measure="kernel rows == torch composition rows (bitwise)", rows=nv,
        equal=bool(ref.shape[0] == nv and torch.equal(rows[:nv * F].view(torch.int32),
                                                      ref.reshape(-1).view(torch.int32))))
    del ref, rows

    with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
        p_dev, p_cpu = os.path.join(tmp, "dev.ply"), os.path.join(tmp, "cpu.ply")
        save_ply(d, p_dev)  # warm-up: the pinned buffer's first allocation
        t_dev, _ = wall(lambda: save_ply(d, p_dev))
        t_cpu, _ = wall(lambda: save_ply(s, p_cpu))
        same = open(p_dev, "rb").read() == open(p_cpu, "rb").read()
        log(measure="save_ply end to end", device_wall_s=round(t_dev, 3),
            numpy_wall_s=round(t_cpu, 3), ratio=round(t_cpu / t_dev, 2), same_bytes=same,
            file_bytes=os.path.getsize(p_dev))
        load_ply(p_dev, device="cuda")
        t_dev, _ = wall(lambda: load_ply(p_dev, device="cuda"))
        t_cpu, _ = wall(lambda: load_ply(p_dev))
        log(measure="load_ply end to end", device_wall_s=round(t_dev, 3),
            numpy_wall_s=round(t_cpu, 3), ratio=round(t_cpu / t_dev, 2))


if __name__ == "__main__":
    main()
