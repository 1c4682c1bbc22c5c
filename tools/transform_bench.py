"""Time the similarity transform of a splat scene at the size of a trained one:
N = 1,006,065 Gaussians at SH degree 3, one segment, and 4,096 segments with
clustered (sorted) and with random ids.

  kernel: gsplat_hip_splat_xform_apply (csrc/transform.hip) on the whole N, by
       HIP events around back-to-back launches after a warm-up, as many as
       fill --window-ms (sized from a short calibration run, recorded as
       `iters`), --reps times, taking turns with the torch composition; min /
       median / max over the repetitions.  The prepare kernel is timed apart
       (its launches are short enough that the figure is the host's issue rate;
       the kernel trace has its own time).  GB/s against the byte model
       2 * (12 + 16 + 12 + 12 (K-1)) B per Gaussian (every float read once and
       written once) plus 8 B with ids; the kernel is memory-bound: the share is
       of the 8.0 TB/s HBM peak.  One launch streams about 440 MB, more
       than the 256 MiB Infinity Cache, but back-to-back launches over the same
       tensors are partly cache-fed.
  torch: the same result composed on the device: one einsum per degree with the
       gathered blocks, the quaternion product and the affine map (what a user
       without the kernel would write).
  check: the kernel's result against the torch composition.

One JSON line per measurement, also written to --out.  `--kernels-only` runs
--launches prepare + apply pairs per case and nothing else, for a separate
`rocprofv3 --kernel-trace --stats` run.

    python tools/transform_bench.py [--n 1006065] [--window-ms 250] [--reps 5]
        [--out profiles/transform/transform.txt] [--kernels-only --launches 5]
"""

import argparse
import json
import math
import os
import statistics
import sys

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


def random_similarities(S, g):
    q = torch.randn(S, 4, generator=g, dtype=torch.float64)
    w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
                    1).reshape(S, 3, 3)
    T = torch.zeros(S, 4, 4, dtype=torch.float64)
    T[:, :3, :3] = R * (0.5 + torch.rand(S, 1, 1, generator=g, dtype=torch.float64))
    T[:, :3, 3] = torch.randn(S, 3, generator=g, dtype=torch.float64)
    T[:, 3, 3] = 1
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1006065)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transform", "transform.txt"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "transform_bench.py measures on the GPU"
    from gsplat_hip import transform as X
    log = Log(None if a.kernels_only else a.out)
    log(measure="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)

    N, deg, K1 = a.n, 3, 15
    g = torch.Generator().manual_seed(0)
    d = {k: v.cuda() for k, v in dict(
        means=torch.randn(N, 3, generator=g), quats=torch.randn(N, 4, generator=g),
        scales=torch.randn(N, 3, generator=g), shN=torch.randn(N, K1, 3, generator=g)).items()}
    keys = ("means", "quats", "scales", "shN")
    src = tuple(d[k] for k in keys)
    dst = tuple(torch.empty_like(t) for t in src)
    row_bytes = 2 * (12 + 16 + 12 + 12 * K1)
    log(measure="case", n=N, sh_degree=deg, model_bytes_per_gaussian=row_bytes,
        note="one launch streams more than the 256 MiB Infinity Cache, but back-to-back "
             "launches over the same tensors are partly cache-fed")

    cases = [("S=1, no ids", 1, None),
             ("S=4096, clustered ids", 4096, "sorted"),
             ("S=4096, random ids", 4096, "random")]
    for label, S, kind in cases:
        T = random_similarities(S, g).cuda()
        ids = None
        if kind:
            ids = torch.randint(0, S, (N,), generator=g)
            ids = (ids.sort().values if kind == "sorted" else ids).cuda()
        rec, flags = X._prepare_device(T, deg)

        def prepare():
            X._prepare_device(T, deg)

        def apply():
            X._apply_device(N, deg, S, rec, flags, ids, src, dst)

        def composition():
            seg = ids if ids is not None else torch.zeros(N, dtype=torch.int64, device="cuda")
            hdr = rec[seg, :X.HEADER_FLOATS]
            A, t = hdr[:, :9].reshape(N, 3, 3), hdr[:, 9:12]
            out = [torch.einsum("nij,nj->ni", A, d["means"]) + t,
                   X._quat_mul(hdr[:, 12:16], d["quats"]), d["scales"] + hdr[:, 16:17]]
            sh, at, off = [], 0, X.HEADER_FLOATS
            for l in range(1, deg + 1):
                n = 2 * l + 1
                M = rec[seg, off:off + n * n].reshape(N, n, n)
                sh.append(torch.einsum("nij,njc->nic", M, d["shN"][:, at:at + n]))
                at, off = at + n, off + n * n
            return out + [torch.cat(sh, 1)]

        if a.kernels_only:
            for _ in range(a.launches):
                prepare()
                apply()
            torch.cuda.synchronize()
            continue
        sides = {"prepare": prepare, "apply": apply, "torch": composition}
        for fn in sides.values():  # warm-up: code objects, allocator
            fn()
        # enough launches to fill the window, from a short calibration run
        iters = {k: max(3, math.ceil(a.window_ms / timed(fn, 3))) for k, fn in sides.items()}
        ms = {k: [] for k in sides}
        for _ in range(a.reps):
            for k, fn in sides.items():
                ms[k].append(timed(fn, iters[k]))
        model = float(N) * (row_bytes + (8 if ids is not None else 0))
        med = statistics.median(ms["apply"])
        gbs = model / (med * 1e-3) / 1e9
        log(measure=f"{label}: kernel, apply (gsplat_hip_splat_xform_apply)", **spread(ms["apply"]),
            iters=iters["apply"], model_bytes=int(model), GBps=round(gbs, 1),
            frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 3))
        log(measure=f"{label}: kernel, prepare (gsplat_hip_splat_xform_prepare)",
            **spread(ms["prepare"]), iters=iters["prepare"])
        log(measure=f"{label}: torch composition (einsum per degree, quaternion product, affine)",
            **spread(ms["torch"]), iters=iters["torch"])
        log(measure=f"{label}: torch composition / apply",
            ratio=round(statistics.median(ms["torch"]) / med, 2))
        ref = composition()
        err = max(float((r - o).abs().max() / r.abs().max()) for r, o in zip(ref, dst))
        oob = int(flags[:2].cpu().view(torch.int64)[0])
        log(measure=f"{label}: kernel against the torch composition", max_rel_err=float(f"{err:.3g}"),
            ids_out_of_range=oob, refused_segments=int((flags[2:] != 0).sum()))
        del ref


if __name__ == "__main__":
    main()
