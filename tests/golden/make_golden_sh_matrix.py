"""Bars for the SH colour test matrix (tests/sh_cases.py), from the
REFERENCE's own torch implementation (gsplat/cuda/_torch_impl.py:
`_spherical_harmonics`) with the rendering.py glue of the fused colour path
(`torch.inverse`, masking, `clamp_min(colors + 0.5, 0)`) and, for the Adam
cases, `torch.optim.Adam`.  Run in the build container only:

    python tests/golden/make_golden_sh_matrix.py

Every case of sh_cases.ALL_NAMES runs on the CPU in float64 and in float32
from the same float32 inputs.  Written to sh_matrix.npz (numbers only):

    bar_names, bar_values   per "<case>:<output>", max |fp32 - fp64| / max |fp64|:
                            the reference's own float32 error, which the
                            tests scale their bounds from
    sample_<output>         the reference's float64 outputs of sh_cases.SAMPLE,
                            so the oracle can be checked against them without
                            the reference present
"""

import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))

import sh_cases as SC  # noqa: E402


def _impl():
    pkg = types.ModuleType("gsplat")
    pkg.__path__ = [os.path.join(REF, "gsplat")]
    sys.modules["gsplat"] = pkg
    from gsplat.cuda import _torch_impl
    return _torch_impl


def bar(a32, a64):
    a64 = np.asarray(a64, np.float64)
    return float(np.abs(np.asarray(a32, np.float64) - a64).max() / max(np.abs(a64).max(), 1e-300))


def T(a, dtype, grad=False):
    return torch.from_numpy(np.array(a)).to(dtype).requires_grad_(grad)


def grads(loss, ins):
    gs = torch.autograd.grad(loss, ins, allow_unused=True)
    return [torch.zeros_like(i) if g is None else g for g, i in zip(gs, ins)]


def run_nf(R, c, dtype):
    dirs, coeffs = T(c.dirs, dtype, True), T(c.coeffs, dtype, True)
    col = R._spherical_harmonics(c.deg, dirs, coeffs.expand(*dirs.shape[:-1], -1, -1))
    if c.masks is not None:  # the wrapper's `colors[~masks] = 0`
        col = torch.where(T(c.masks, torch.bool)[..., None], col, torch.zeros_like(col))
    vc, vd = grads((col * T(c.v_colors, dtype)).sum(), (coeffs, dirs))
    norm = T(c.dirs, torch.float64).norm(dim=-1, keepdim=True).to(dtype)
    return {"colors": col.detach().numpy(), "v_coeffs": vc.numpy(), "v_dirs": (vd * norm).numpy()}


def fused_colors(R, c, means, coeffs, dtype):
    """rendering.py's colour path for unpacked Gaussians."""
    C, N = c.radii.shape
    camtoworlds = torch.inverse(T(c.viewmats, dtype))
    dirs = means[None, :, :] - camtoworlds[:, None, :3, 3]
    masks = T(c.radii, torch.int32) > 0
    shs = coeffs.expand(C, -1, -1, -1) if coeffs.dim() == 3 else coeffs
    col = R._spherical_harmonics(c.deg, dirs, shs)
    col = torch.where(masks[..., None], col, torch.zeros_like(col))
    return torch.clamp_min(col + 0.5, 0.0)


def run_fz(R, c, dtype):
    means, coeffs = T(c.means, dtype, True), T(c.coeffs, dtype, True)
    col = fused_colors(R, c, means, coeffs, dtype)
    vc, vm = grads((col * T(c.v_colors, dtype)).sum(), (coeffs, means))
    return {"colors": col.detach().numpy(), "v_coeffs": vc.numpy(), "v_means": vm.numpy()}


def run_adam(R, c, dtype):
    a = SC.ADAM
    sh0 = T(c.coeffs[:, :1], dtype, True)
    shN = T(c.coeffs[:, 1:], dtype, True)
    opt = torch.optim.Adam([{"params": [sh0], "lr": a["lr0"]}, {"params": [shN], "lr": a["lr_rest"]}],
                           betas=a["betas"], eps=a["eps"])
    out = {}
    for step in range(a["steps"]):
        means = T(c.means, dtype, True)
        opt.zero_grad(set_to_none=True)
        col = fused_colors(R, c, means, torch.cat([sh0, shN], 1), dtype)
        (col * T(c.v_colors, dtype)).sum().backward()
        if step == 0:
            out["v_coeffs"] = torch.cat([sh0.grad, shN.grad], 1).numpy().copy()
        opt.step()
    st0, stN = opt.state[sh0], opt.state[shN]
    out["m"] = torch.cat([st0["exp_avg"], stN["exp_avg"]], 1).numpy()
    out["v"] = torch.cat([st0["exp_avg_sq"], stN["exp_avg_sq"]], 1).numpy()
    out["p"] = torch.cat([sh0, shN], 1).detach().numpy()
    out["v_means"] = (torch.zeros_like(means) if means.grad is None else means.grad).detach().numpy()
    return out


def main():
    R = _impl()
    run = {"nf": run_nf, "fz": run_fz, "adam": run_adam}
    names, values, sample = [], [], {}
    for name in SC.ALL_NAMES:
        c = SC.build(name)
        r64, r32 = run[c.kind](R, c, torch.float64), run[c.kind](R, c, torch.float32)
        for k in SC.OUTPUTS[c.kind]:
            names.append(f"{name}:{k}")
            values.append(bar(r32[k], r64[k]))
        if name == SC.SAMPLE:
            sample = {"sample_" + k: r64[k] for k in SC.OUTPUTS[c.kind]}
    assert sample
    values = np.array(values, np.float64)
    for kind in run:
        for k in SC.OUTPUTS[kind]:
            v = np.array([b for n, b in zip(names, values) if n.startswith(kind) and n.endswith(":" + k)])
            print(f"{kind:5s} {k:9s} bars: min {v.min():.2e}  median {np.median(v):.2e}  max {v.max():.2e}")
    path = os.path.join(OUT, "sh_matrix.npz")
    np.savez_compressed(path, bar_names=np.array(names), bar_values=values, **sample)
    size = os.path.getsize(path)
    print(f"sh_matrix: {len(names)} bars, {size} bytes")
    assert size < 100_000, size


if __name__ == "__main__":
    main()
