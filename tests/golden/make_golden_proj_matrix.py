"""Bars for the projection test matrix (tests/proj_cases.py) and its
cross-check against the REFERENCE's torch implementation
(gsplat/cuda/_torch_impl.py: `_quat_scale_to_covar_preci` +
`_fully_fused_projection` + autograd).  Run in the build container only, on
the CPU:

    python tests/golden/make_golden_proj_matrix.py

Written to proj_matrix.npz (numbers only; the inputs are rebuilt from the
seed and the float64 oracle runs at test time):

    bar_names, bar_values   per "<case>:<variant>:<output>", the larger of two
                            float32 errors against the float64 oracle, as max
                            error / max |float64|: the oracle's own torch
                            formulation run in float32, and oracle/
                            gsplat_oracle.py's numpy proj_fwd / proj_bwd in
                            their native float32 (the same algebra in another
                            operation order).  The per-pair rows pp_* and the
                            Adam outputs have the torch run only (the numpy
                            oracle returns neither); a pp_* bar is no smaller
                            than its dense output's.
    ref_<case>_<output>     the reference's float64 outputs and gradients of
                            the two smallest cases that exercise neither of
                            the oracle's two conventions, so the oracle can be
                            checked against them without the reference present

Before writing, every case with no clamped valid pair and radius_clip 0 (the
reference has none) is run through the reference in float64, compensations
off: radii identical, outputs and gradients within 1e-10 relative.
"""

import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(OUT), os.path.dirname(os.path.dirname(OUT))]

import proj_cases as PC  # noqa: E402


def _impl():
    pkg = types.ModuleType("gsplat")
    pkg.__path__ = [os.path.join(REF, "gsplat")]
    sys.modules["gsplat"] = pkg
    from gsplat.cuda import _torch_impl
    return _torch_impl


def T(a, grad=False):
    return torch.from_numpy(np.array(a)).double().requires_grad_(grad)


def run_reference(R, c):
    """Forward and gradients of the reference in float64, compensations off;
    invalid entries zeroed as the oracle's are."""
    means, quats, scales, vm = T(c.means, True), T(c.quats, True), T(c.scales, True), T(c.viewmats, True)
    covars, _ = R._quat_scale_to_covar_preci(quats, scales, True, False, triu=False)
    radii, m2, depths, conics, _ = R._fully_fused_projection(
        means, covars, vm, T(c.Ks), c.W, c.H, c.eps2d, c.near, c.far, False)
    on = (radii > 0).double()
    loss = (m2 * T(c.v_means2d) * on[..., None]).sum() + (depths * T(c.v_depths) * on).sum() \
        + (conics * T(c.v_conics) * on[..., None]).sum()
    zeros = [torch.zeros_like(x) for x in (means, quats, scales, vm)]
    gs = torch.autograd.grad(loss, (means, quats, scales, vm), allow_unused=True) if on.any() else zeros
    gs = [z if g is None else g for g, z in zip(gs, zeros)]
    out = {"radii": radii.numpy().astype(np.int32), "means2d": (m2 * on[..., None]).detach().numpy(),
           "depths": depths.detach().numpy(), "conics": (conics * on[..., None]).detach().numpy()}
    out.update({k: g.numpy() for k, g in zip(PC.BWD_OUT, gs)})
    return out


REF_OUT = ("means2d", "depths", "conics") + PC.BWD_OUT


def exercises_no_convention(c):
    p = PC.gates(c)
    clamped = torch.stack(list(p.clamp.values())).any(0)
    return c.radius_clip == 0.0 and not bool((clamped & p.valid).any())


def cross_check(R):
    """-> {ref_<case>_<output>: array} of the two smallest cases checked."""
    checked = []
    for name in PC.ALL_NAMES:
        c = PC.build(name)
        if not exercises_no_convention(c):
            continue
        ref, f64, b64 = run_reference(R, c), PC.fwd64(name), PC.bwd64(name)
        assert np.array_equal(ref["radii"], f64["radii"]), name
        ours = {**f64, **b64}
        worst = max(PC.rel_err(ours[k], ref[k]) for k in REF_OUT)
        assert worst <= 1e-10, (name, worst)
        checked.append((c.C * c.N, name, ref, worst))
    print(f"reference cross-check: {len(checked)} cases, largest relative difference "
          f"{max(w for *_, w in checked):.2e}")
    fixture = {}
    live = [x for x in checked if (x[2]["radii"] > 0).any()]
    for _, name, ref, _ in sorted(live, key=lambda x: x[0])[:2]:
        fixture["ref_names"] = np.array(list(fixture.get("ref_names", [])) + [name])
        for k in ("radii",) + REF_OUT:
            fixture[f"ref_{name}_{k}"] = ref[k]
    return fixture


def case_bars(name):
    c = PC.build(name)
    f64 = PC.fwd64(name)
    valid = f64["radii"] > 0
    t32, n32 = PC.oracle_fwd(c, torch.float32), PC.numpy_fwd(c)
    assert np.array_equal(t32["radii"], f64["radii"]) and np.array_equal(n32["radii"], f64["radii"]), name
    bars = {}
    for k in PC.FWD_OUT:
        bars[f"{name}:fwd:{k}"] = max(PC.rel_err(t32[k], f64[k]), PC.rel_err(n32[k], f64[k]))
    for comps, depths in PC.BWD_VARIANTS:
        key = PC.bwd_key(comps, depths)
        b64 = PC.bwd64(name, comps, depths)
        bt = PC.oracle_bwd(c, torch.float32, comps, depths, valid=valid)
        bn = PC.numpy_bwd(c, n32, np.float32, comps, depths)
        for k in PC.BWD_OUT:
            bars[f"{name}:{key}:{k}"] = max(PC.rel_err(bt[k], b64[k]), PC.rel_err(bn[k], b64[k]))
            bars[f"{name}:{key}:pp_{k}"] = max(PC.rel_err(bt["pp_" + k], b64["pp_" + k]),
                                               bars[f"{name}:{key}:{k}"])
    if name in PC.ADAM_NAMES:
        for dirs, opac in PC.ADAM_VARIANTS:
            a64 = PC.adam64(name, dirs, opac)
            a32 = PC.oracle_adam(c, torch.float32, dirs, opac, valid=valid)
            for k in PC.ADAM_OUT:
                bars[f"{name}:{PC.adam_key(dirs, opac)}:{k}"] = PC.rel_err(a32[k], a64[k])
    return bars


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same bytes every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    fixture = cross_check(_impl())
    assert len(fixture["ref_names"]) == 2
    bars = {}
    for name in PC.ALL_NAMES:
        bars.update(case_bars(name))
    names = sorted(bars)
    values = np.array([bars[k] for k in names], np.float64)
    assert np.isfinite(values).all()
    for part in ("fwd", "bwd", "bwd_comp", "adam"):
        outs = sorted({n.split(":")[2] for n in names if n.split(":")[1] == part})
        for k in outs:
            v = np.array([bars[n] for n in names if n.split(":")[1:] == [part, k]])
            print(f"{part:9s} {k:14s} bars: min {v.min():.2e}  median {np.median(v):.2e}  max {v.max():.2e}")
    print("largest share of redrawn pairs:", max(PC.build(n).redrawn for n in PC.ALL_NAMES))
    path = os.path.join(OUT, "proj_matrix.npz")
    save_npz(path, dict(bar_names=np.array(names), bar_values=values, **fixture))
    size = os.path.getsize(path)
    print(f"proj_matrix: {len(names)} bars, fixture {list(fixture['ref_names'])}, {size} bytes")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
