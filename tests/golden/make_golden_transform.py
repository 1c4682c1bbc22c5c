#!/usr/bin/env python3
"""Writes tests/golden/transform_<case>.npz and transform_checks.npz from the
float64 oracle of tests/transform_cases.py.

Per case: the float32 inputs, the float64 outputs (`out_*`) and, per compared
output, `bar_*` = the error of the same oracle run in float32, as
max err / max |oracle|.

transform_checks.npz:
  blocks_*      M_1..M_4 of one generic rotation and their float32 bars
  sh_eval_bar   the float32-vs-float64 error of  SH(L, d, rotated coefficients)
                against  SH(L, R^T d, coefficients)  on 1,000 Gaussians, both
                sides evaluated by the numpy oracle in float32
  render_*      the similarity of the render check (float64), the float32 bar of the
                oracle's render against its float64 render (the larger of the
                original and the moved scene, flips of the alpha threshold
                excluded up to raster_cases.close_most's default allowance,
                which this script asserts is enough), and the float64
                difference between the two renders

Usage: python tests/golden/make_golden_transform.py   (CPU only)
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import raster_cases  # noqa: E402
import transform_cases as TC  # noqa: E402
from oracle import gsplat_oracle as O  # noqa: E402


def case_file(name):
    case = TC.make_case(name)
    want = TC.oracle(case, np.float64)
    got32 = TC.oracle(case, np.float32)
    wv, gv = TC.views(want), TC.views(got32)
    out = {"means": case.means, "quats": case.quats, "scales": case.scales, "shN": case.shN,
           "transforms": case.transforms}
    if case.ids is not None:
        out["ids"] = case.ids
    for k in ("means", "quats", "scales", "shN"):
        out["out_" + k] = want[k]
    for k in TC.OUTPUTS:
        out["bar_" + k] = np.float64(TC.rel_err(gv[k], wv[k]))
    path = os.path.join(HERE, f"transform_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name:22s} {os.path.getsize(path) / 1024:7.1f} KiB  " +
          "  ".join(f"{k} {float(out['bar_' + k]):.2e}" for k in TC.OUTPUTS))


def sh_eval(dtype, L=4, n=1000):
    rng = np.random.default_rng(TC.seed_of("sh_eval"))
    R = TC.rotation("generic", rng).astype(np.float32).astype(dtype)
    dirs = rng.normal(size=(n, 3)).astype(np.float32).astype(dtype)
    coeffs = (rng.normal(size=(n, (L + 1) ** 2, 3)) * 0.3).astype(np.float32).astype(dtype)
    U, _, Vt = np.linalg.svd(R)
    R = (U @ Vt).astype(dtype)
    rot = coeffs.copy()
    at = 1
    for l, M in enumerate(TC.sh_blocks(R, L), start=1):
        k = 2 * l + 1
        rot[:, at:at + k] = np.einsum("ij,njc->nic", M, coeffs[:, at:at + k])
        at += k
    with O.precision(dtype):
        return O.sh_fwd(L, dirs, rot), O.sh_fwd(L, (dirs @ R).astype(dtype), coeffs)


def excluding_flips(a, b):
    """max |a - b| / max |b| without the largest `allowed` elements."""
    allowed = max(2, int(1e-4 * a.size))
    err = np.sort(np.abs(a - b).reshape(-1))
    return float(err[-1 - allowed] / np.abs(b).max())


def render_checks():
    splats, vm, K, W, H = TC.render_scene()
    deg = 3
    T = TC.similarity(2.5, "generic", 5.0, TC.seed_of("render"))
    vm2, s = TC.move_camera(vm, T)
    near, far = 0.01, 1e10
    imgs, bars = {}, []
    for dtype in (np.float64, np.float32):   # the float32 run moves by the rounded matrix
        case = TC.SimpleNamespace(N=len(splats["means"]), deg=deg, ids=None,
                                  transforms=T.astype(dtype)[None],
                                  **{k: splats[k] for k in ("means", "quats", "scales", "shN")})
        moved = dict(splats, **TC.oracle(case, dtype))
        imgs[dtype, 0] = TC.render(splats, vm, K, W, H, deg, near, far, dtype)
        imgs[dtype, 1] = TC.render(moved, vm2, K, W, H, deg, near * s, far * s, dtype)
    diff64 = float(np.abs(imgs[np.float64, 0] - imgs[np.float64, 1]).max())
    for i in (0, 1):
        bars.append(excluding_flips(imgs[np.float32, i], imgs[np.float64, i]))
    bar = max(bars)
    top = float(np.abs(imgs[np.float64, 0]).max())
    for i in (0, 1):   # the float32 oracle stays inside the flip allowance
        raster_cases.close_most(imgs[np.float32, i], imgs[np.float64, i], rtol=0.0,
                                atol=TC.FACTOR * bar * top, what=f"float32 oracle render {i}")
    print(f"render: N {case.N}  float64 difference {diff64:.2e}  float32 bars "
          f"{bars[0]:.2e} {bars[1]:.2e}  max {top:.3f}")
    return {"render_T": T, "render_bar": np.float64(bar), "render_diff64": np.float64(diff64),
            "render_max": np.float64(top)}


def main():
    for name in TC.NAMES:
        case_file(name)
    out = {}
    rng = np.random.default_rng(TC.seed_of("blocks"))
    R = TC.rotation("generic", rng).astype(np.float32)
    out["blocks_R"] = R
    R64 = TC.decompose(np.block([[R.astype(np.float64), np.zeros((3, 1))],
                                 [np.zeros((1, 3)), np.ones((1, 1))]]))[3]
    R32 = TC.decompose(np.block([[R, np.zeros((3, 1), np.float32)],
                                 [np.zeros((1, 3), np.float32), np.ones((1, 1), np.float32)]]))[3]
    for l, (M, M32) in enumerate(zip(TC.sh_blocks(R64, 4), TC.sh_blocks(R32, 4)), start=1):
        out[f"blocks_M{l}"] = M
        out[f"blocks_bar{l}"] = np.float64(TC.rel_err(M32.astype(np.float64), M))
    a64, b64 = sh_eval(np.float64)
    a32, b32 = sh_eval(np.float32)
    out["sh_eval_bar"] = np.float64(np.abs(a32.astype(np.float64) - b32).max() / np.abs(b64).max())
    print(f"sh_eval: float64 {np.abs(a64 - b64).max():.2e}  float32 bar "
          f"{float(out['sh_eval_bar']):.2e}")
    out.update(render_checks())
    np.savez_compressed(os.path.join(HERE, "transform_checks.npz"), **out)


if __name__ == "__main__":
    main()
