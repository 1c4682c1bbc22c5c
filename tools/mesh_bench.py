"""Time the mesh export on a 512^3 volume with colours: 2.7 GB of state, far
past the 256 MiB Infinity Cache, so the rates are HBM rates.

  integrate: gsplat_hip_tsdf_integrate (csrc/tsdf.hip) with C = 1 and C = 8
       views of 1920 x 1080 (a sphere seen from cameras around it), by HIP
       events around --iters back-to-back launches after a warm-up, --reps
       times, taking turns with the torch composition; min / median / max.
       GB/s against the byte model 2 * 20 B per voxel per launch (five planes
       read and written once) plus each image once (depth, alpha, colours:
       20 B per pixel); the share is of the 8.0 TB/s HBM peak.
  torch: the same update as torch ops (projection, gather by index, running
       mean under a mask), one camera after the other.
  check: the voxels whose weight or tsdf differs between the kernel and the
       torch composition, counted (a pair within rounding of a pixel boundary
       reads the neighbouring pixel on one side only).
  extract: gsplat_hip_mc_count (classify + edges + the two scans) and
       gsplat_hip_mc_emit (vertices + faces) on an analytic sphere and on the
       volume fused from the 8 views; GB/s of the count against 8 B per voxel
       per classifying pass (two passes); extract_mesh() end to end (with its
       host read and allocations) as wall clock.
  --resources: no GPU needed: each kernel's registers, LDS, scratch and
       occupancy from hipcc -Rpass-analysis=kernel-resource-usage.

One JSON line per measurement, also written to --out.

    python tools/mesh_bench.py [--n 512] [--iters 3] [--reps 3]
        [--out profiles/mesh/mesh.txt] [--resources profiles/mesh/resources.txt]
"""

import argparse
import json
import math
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsplat-triton_amd"))

HBM_PEAK_GBS = 8000.0
VOXEL_BYTES = 2 * 20   # five float planes read and written once per launch
PIXEL_BYTES = 20       # depth + alpha + three colour floats
CLASSIFY_BYTES = 8     # tsdf + weight per voxel per classifying pass


def resources(path):
    csrc = os.path.join(ROOT, "gsplat-triton_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950",
                          "-munsafe-fp-atomics", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "tsdf.hip", "-o",
                          os.devnull], cwd=csrc, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?): (.*?) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if k == "Function Name":
            cur = {"kernel": subprocess.run(["c++filt", v], capture_output=True,
                                            text=True).stdout.strip() or v}
            rows.append(cur)
        elif cur is not None and k in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]",
                                       "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
            cur[k] = int(v)
    rows = [r for r in rows if "tsdf::" in r["kernel"]]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh", "mesh.txt"))
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    if a.resources:
        return resources(a.resources)

    import torch
    assert torch.cuda.is_available(), "mesh_bench.py measures on the GPU"
    from gsplat_hip import TSDFVolume, _lib
    from gsplat_hip._wrapper import _stream
    dev = "cuda"

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

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()

    def log(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    log(measure="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)
    n, W, H, C = a.n, 1920, 1080, 8
    h = 2.0 / (n - 1)
    origin, radius = (-1.0, -1.0, -1.0), 0.6
    nvox = n ** 3
    log(measure="case", dims=[n, n, n], voxels=nvox, state_GB=round(20 * nvox / 1e9, 2),
        image=[W, H], cameras=C)

    # C cameras on a circle of radius 3 around the sphere, looking at its centre
    vms, f = [], 1400.0
    for k in range(C):
        p = 2 * math.pi * k / C + 0.1
        eye = torch.tensor([3 * math.cos(p), 3 * math.sin(p), 0.8], dtype=torch.float64)
        z = -eye / eye.norm()
        x = torch.linalg.cross(z, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
        x = x / x.norm()
        y = torch.linalg.cross(z, x)
        V = torch.eye(4, dtype=torch.float64)
        V[:3, :3] = torch.stack([x, y, z])
        V[:3, 3] = -V[:3, :3] @ eye
        vms.append(V)
    vms = torch.stack(vms).float().to(dev)
    Ks = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]).repeat(C, 1, 1).to(dev)
    # the sphere's z-depth at the pixel centres (the ray parameter with d_z = 1)
    py, px = torch.meshgrid(torch.arange(H, device=dev) + 0.5, torch.arange(W, device=dev) + 0.5,
                            indexing="ij")
    dc = torch.stack([(px - W / 2) / f, (py - H / 2) / f, torch.ones_like(px)], -1)
    depths = []
    for k in range(C):
        R, t = vms[k, :3, :3], vms[k, :3, 3]
        o, d = -R.T @ t, dc @ R
        qa, qb, qc = (d * d).sum(-1), 2 * (d @ o), o @ o - radius * radius
        disc = qb * qb - 4 * qa * qc
        s = (-qb - disc.clamp_min(0).sqrt()) / (2 * qa)
        depths.append(torch.where(disc > 0, s, torch.zeros_like(s)))
    depths = torch.stack(depths).contiguous()
    alphas = (depths > 0).float()
    colors = torch.rand(C, H, W, 3, device=dev)

    vol = TSDFVolume(origin, h, (n, n, n), device=dev, colors=True)
    trunc = vol.sdf_trunc

    def kernel(c):
        return lambda: vol.integrate(depths[:c], vms[:c], Ks[:c], colors=colors[:c],
                                     alphas=alphas[:c])

    ax = torch.arange(n, device=dev, dtype=torch.float32)
    ref = torch.zeros(5, n, n, n, device=dev)

    def composition(c):
        def run():
            X = (origin[0] + h * ax)[None, None, :]
            Y = (origin[1] + h * ax)[None, :, None]
            Z = (origin[2] + h * ax)[:, None, None]
            tsdf, w, col = ref[0], ref[1], ref[2:5]
            for k in range(c):
                V = vms[k]
                pc = [V[r, 0] * X + V[r, 1] * Y + V[r, 2] * Z + V[r, 3] for r in range(3)]
                u = Ks[k, 0, 0] * pc[0] / pc[2] + Ks[k, 0, 2]
                v = Ks[k, 1, 1] * pc[1] / pc[2] + Ks[k, 1, 2]
                ok = (pc[2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
                pix = torch.where(ok, v.floor().long() * W + u.floor().long(),
                                  torch.zeros((), dtype=torch.long, device=dev))
                dd = depths[k].reshape(-1)[pix]
                ok &= (dd > 0) & (alphas[k].reshape(-1)[pix] >= 0.5)
                sdf = dd - pc[2]
                ok &= sdf >= -trunc
                s = (sdf / trunc).clamp_max(1.0)
                w1 = w + 1
                tsdf.copy_(torch.where(ok, (tsdf * w + s) / w1, tsdf))
                rgb = colors[k].reshape(-1, 3)[pix]
                for ch in range(3):
                    col[ch].copy_(torch.where(ok, (col[ch] * w + rgb[..., ch]) / w1, col[ch]))
                w.copy_(torch.where(ok, w1, w))
        return run

    for c in (1, C):
        sides = {"kernel": kernel(c), "torch": composition(c)}
        for fn in sides.values():
            fn()
        ms = {k: [] for k in sides}
        for _ in range(a.reps):
            for k, fn in sides.items():
                ms[k].append(timed(fn, a.iters))
        model = VOXEL_BYTES * nvox + PIXEL_BYTES * c * H * W
        med = statistics.median(ms["kernel"])
        gbs = model / (med * 1e-3) / 1e9
        log(measure=f"integrate C={c}: kernel (gsplat_hip_tsdf_integrate)", **spread(ms["kernel"]),
            model_bytes=int(model), GBps=round(gbs, 1), frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 3))
        tmed = statistics.median(ms["torch"])
        log(measure=f"integrate C={c}: torch composition (gather + running mean)",
            **spread(ms["torch"]), ratio_to_kernel=round(tmed / med, 1))

    # check: one fusion of the C views by either side
    vol.reset()
    ref.zero_()
    kernel(C)()
    composition(C)()
    # (a pair within rounding of a pixel boundary reads the neighbouring pixel on one
    # side only: another weight at a silhouette, another depth elsewhere)
    dw = (vol.weight - ref[1]).abs()
    dt = (vol.tsdf - ref[0]).abs()
    log(measure="kernel vs torch composition after one fusion of 8 views",
        fused_voxels=int((ref[1] > 0).sum()), voxels_with_another_weight=int((dw > 0).sum()),
        max_weight_diff=float(dw.max()), voxels_with_tsdf_off_by_1e_5=int((dt > 1e-5).sum()),
        median_tsdf_diff=float(dt[ref[1] > 0].median()))
    del ref

    # extraction: the fused scene, then an analytic sphere in the same volume
    def extract_case(name):
        nx = ny = nz = n
        state = vol._state
        ws = torch.empty(int(_lib.query("gsplat_hip_mc_workspace_bytes", nx, ny, nz)) + 16,
                         dtype=torch.uint8, device=dev)
        base = ws.data_ptr() + (-ws.data_ptr()) % 16
        totals = torch.zeros(2, dtype=torch.int64, device=dev)

        def count():
            _lib.call("gsplat_hip_mc_count", nx, ny, nz, state[0].data_ptr(), state[1].data_ptr(),
                      0.0, base, totals.data_ptr(), _stream())

        count()
        V, F = (int(v) for v in totals.cpu())
        verts = torch.empty(V, 3, device=dev)
        vcol = torch.empty(V, 3, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)

        def emit():
            _lib.call("gsplat_hip_mc_emit", nx, ny, nz, *origin, h, state[0].data_ptr(),
                      state[2].data_ptr(), vol._stride, base, V, F, verts.data_ptr(),
                      vcol.data_ptr(), faces.data_ptr(), _stream())

        emit()
        ms = {"count": [], "emit": []}
        for _ in range(a.reps):
            ms["count"].append(timed(count, a.iters))
            ms["emit"].append(timed(emit, a.iters))
        med = statistics.median(ms["count"])
        gbs = 2 * CLASSIFY_BYTES * nvox / (med * 1e-3) / 1e9
        log(measure=f"extract {name}: count (classify + edges + scans)", **spread(ms["count"]),
            model_bytes=2 * CLASSIFY_BYTES * nvox, GBps=round(gbs, 1),
            frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 3))
        log(measure=f"extract {name}: emit (vertices + faces)", **spread(ms["emit"]),
            vertices=V, faces=F)
        del ws, verts, vcol, faces
        vol.extract_mesh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = vol.extract_mesh()
        torch.cuda.synchronize()
        log(measure=f"extract {name}: extract_mesh() end to end", wall_ms=round(
            (time.perf_counter() - t0) * 1e3, 3), vertices=int(out[0].shape[0]),
            faces=int(out[1].shape[0]))

    extract_case("fused scene (8 views of a sphere)")
    g = origin[0] + h * ax
    r = (g[None, None, :] ** 2 + g[None, :, None] ** 2 + g[:, None, None] ** 2).sqrt()
    vol.tsdf.copy_(((r - radius) / trunc).clamp(-1.0, 1.0))
    vol.weight.fill_(1.0)
    del r
    extract_case("analytic sphere")


if __name__ == "__main__":
    main()
