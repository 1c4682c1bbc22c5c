"""Golden vectors for the covariance-input projection, `world_to_cam` and
`proj`, from the REFERENCE's own torch implementations
(gsplat/cuda/_torch_impl.py: `_fully_fused_projection`, `_world_to_cam`,
`_persp_proj`, `_ortho_proj`, `_fisheye_proj`) run in float64.  Run in the
build container only:

    python tests/golden/make_golden_covar.py

Every input and cotangent is drawn in float32 and cast up, so the float32
kernels under test read exactly the numbers the float64 oracle read.
Gradients come from torch autograd with seeded cotangents.  The same functions
also run in float32; per output and per gradient the file stores
`bar_<name>` = max |fp32 - fp64| / max |fp64|, the reference's own float32
error, which the GPU tests scale their bounds from.  Only arrays are written.

Files (each below 1 MB):
    covar_proj.npz             fused projection from [N,6] covariances
    world_to_cam.npz           world -> camera transform
    proj_models.npz            inputs and cotangents of the three camera models,
                               and the whole fisheye near-axis set
    proj_models_<model>.npz    float64 outputs, gradients and bars per model
                               (one file per model: together they pass 1 MB)
"""

import math
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
TRIU = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])


def _impl():
    pkg = types.ModuleType("gsplat")
    pkg.__path__ = [os.path.join(REF, "gsplat")]
    sys.modules["gsplat"] = pkg
    from gsplat.cuda import _torch_impl
    return _torch_impl


def bar(a32, a64):
    a64 = np.asarray(a64, np.float64)
    return float(np.abs(np.asarray(a32, np.float64) - a64).max() / max(np.abs(a64).max(), 1e-300))


def sym3(c6):
    """[N,6] upper triangle -> symmetric [N,3,3]; autograd through it yields
    the v_covars convention of the fused kernels (off-diagonals summed)."""
    i = torch.tensor([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    return c6[:, i]


def save(name, arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print(f"{name}: {size} bytes")
    assert size < 1_000_000, (name, size)


# ------------------------------------------------------------ covar_proj --
def covar_scene(seed):
    g = torch.Generator().manual_seed(seed)
    N, C, W, H = 1500, 3, 128, 80
    means = (torch.rand(N, 3, generator=g) - 0.5) * torch.tensor([6.0, 4.0, 4.0])
    quats = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=-1)
    scales = torch.exp(torch.rand(N, 3, generator=g) * 3.0 - 4.5)
    w, x, y, z = quats.double().unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
                    -1).reshape(N, 3, 3)
    M = R * scales.double()[:, None, :]
    covars = (M @ M.transpose(1, 2))[:, TRIU[0], TRIU[1]].float()  # [N,6], fp32 numbers
    vms = []
    for c in range(C):  # on a circle of radius 2.5 around the box, 0.3 rad apart
        a = 0.3 * (c - 1)
        eye = torch.tensor([2.5 * math.sin(a), 0.3 * c, -2.5 * math.cos(a)])
        fwd = torch.nn.functional.normalize(-eye, dim=0)
        right = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), fwd),
                                              dim=0)
        up = torch.linalg.cross(fwd, right)
        Rm = torch.stack([right, up, fwd])
        vm = torch.eye(4)
        vm[:3, :3] = Rm
        vm[:3, 3] = -Rm @ eye
        vms.append(vm)
    viewmats = torch.stack(vms)
    Ks = torch.tensor([[90.0, 0, W / 2], [0, 90.0, H / 2], [0, 0, 1]]).repeat(C, 1, 1)
    cot = dict(v_means2d=torch.randn(C, N, 2, generator=g), v_depths=torch.randn(C, N, generator=g),
               v_conics=torch.randn(C, N, 3, generator=g), v_comps=torch.randn(C, N, generator=g))
    return means, covars, viewmats, Ks, W, H, cot


def run_covar(T, dtype, means, covars, viewmats, Ks, W, H, cot, comp, near, far):
    m = means.clone().to(dtype).requires_grad_(True)
    c6 = covars.clone().to(dtype).requires_grad_(True)
    vm = viewmats.clone().to(dtype).requires_grad_(True)
    radii, m2, d, cn, cp = T._fully_fused_projection(
        m, sym3(c6), vm, Ks.to(dtype), W, H, eps2d=0.3, near_plane=near, far_plane=far,
        calc_compensations=comp)
    sel = radii > 0
    C = vm.shape[0]
    loss = (m2[sel] * cot["v_means2d"][:C].to(dtype)[sel]).sum() \
        + (d[sel] * cot["v_depths"][:C].to(dtype)[sel]).sum() \
        + (cn[sel] * cot["v_conics"][:C].to(dtype)[sel]).sum()
    if comp:
        loss = loss + (cp[sel] * cot["v_comps"][:C].to(dtype)[sel]).sum()
    vmn, vc, vv = torch.autograd.grad(loss, (m, c6, vm))
    out = dict(radii=radii, means2d=m2, depths=d, conics=cn)
    if comp:
        out["comps"] = cp
    out = {k: v.detach().numpy() for k, v in out.items()}
    grads = dict(v_means=vmn.numpy(), v_covars=vc.numpy(), v_viewmats=vv.numpy())
    return out, grads


def gen_covar_proj(T):
    near, far = 0.2, 100.0
    for seed in range(11, 40):
        means, covars, viewmats, Ks, W, H, cot = covar_scene(seed)
        o64, _ = run_covar(T, torch.float64, means, covars, viewmats, Ks, W, H, cot, True, near, far)
        o32, _ = run_covar(T, torch.float32, means, covars, viewmats, Ks, W, H, cot, True, near, far)
        if np.array_equal(o64["radii"], o32["radii"]):
            break
    else:
        raise SystemExit("no seed with equal fp32 / fp64 radii")
    vis = o64["radii"] > 0
    print(f"covar_proj: seed {seed}, visible {vis.mean():.3f}")
    arrs = dict(means=means.numpy(), covars=covars.numpy(), viewmats=viewmats.numpy(),
                Ks=Ks.numpy(), width=W, height=H, eps2d=0.3, near=near, far=far, seed=seed,
                radii=o64["radii"].astype(np.int32), radii_fp32=o32["radii"].astype(np.int32),
                **{k: v.numpy() for k, v in cot.items()})
    for k in ("means2d", "depths", "conics", "comps"):
        arrs[k] = o64[k]
        arrs["bar_" + k] = bar(o32[k][vis], o64[k][vis])
    for C in (3, 1):
        for comp in (False, True):
            tag = f"_c{C}" + ("_comp" if comp else "")
            _, g64 = run_covar(T, torch.float64, means, covars, viewmats[:C], Ks[:C], W, H, cot,
                               comp, near, far)
            _, g32 = run_covar(T, torch.float32, means, covars, viewmats[:C], Ks[:C], W, H, cot,
                               comp, near, far)
            for k in g64:
                arrs[k + tag] = g64[k]
                arrs["bar_" + k + tag] = bar(g32[k], g64[k])
                print(f"  bar_{k}{tag} = {arrs['bar_' + k + tag]:.2e}")
    save("covar_proj", arrs)


# ---------------------------------------------------------- world_to_cam --
def gen_world_to_cam(T):
    g = torch.Generator().manual_seed(21)
    C, N = 3, 1000
    means = torch.randn(N, 3, generator=g)
    A = torch.randn(N, 3, 3, generator=g) * 0.3
    covars = A @ A.transpose(1, 2) + 0.01 * torch.eye(3)
    vms = []
    for c in range(C):
        vm = torch.eye(4)
        Q = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
        vm[:3, :3] = torch.eye(3) * 0.9 + Q * 0.1  # near the identity, not orthonormal
        vm[:3, 3] = torch.randn(3, generator=g) * 0.2
        vms.append(vm)
    viewmats = torch.stack(vms)
    v_mc = torch.randn(C, N, 3, generator=g)
    v_cc = torch.randn(C, N, 3, 3, generator=g)

    def run(dtype):
        ins = [t.clone().to(dtype).requires_grad_(True) for t in (means, covars, viewmats)]
        mc, cc = T._world_to_cam(*ins)
        gr = torch.autograd.grad((mc * v_mc.to(dtype)).sum() + (cc * v_cc.to(dtype)).sum(), ins)
        return dict(means_c=mc.detach().numpy(), covars_c=cc.detach().numpy(),
                    v_means=gr[0].numpy(), v_covars=gr[1].numpy(), v_viewmats=gr[2].numpy())

    r64, r32 = run(torch.float64), run(torch.float32)
    arrs = dict(means=means.numpy(), covars=covars.numpy(), viewmats=viewmats.numpy(),
                v_means_c=v_mc.numpy(), v_covars_c=v_cc.numpy())
    for k in r64:
        arrs[k] = r64[k]
        arrs["bar_" + k] = bar(r32[k], r64[k])
        print(f"  world_to_cam bar_{k} = {arrs['bar_' + k]:.2e}")
    save("world_to_cam", arrs)


# ----------------------------------------------------------- proj models --
def run_proj(fn, dtype, means, covars, Ks, W, H, v_m2, v_c2):
    m = means.clone().to(dtype).requires_grad_(True)
    c = covars.clone().to(dtype).requires_grad_(True)
    m2, c2 = fn(m, c, Ks.to(dtype), W, H)
    vm, vc = torch.autograd.grad((m2 * v_m2.to(dtype)).sum() + (c2 * v_c2.to(dtype)).sum(), (m, c))
    return dict(means2d=m2.detach().numpy(), covars2d=c2.detach().numpy(), v_means=vm.numpy(),
                v_covars=vc.numpy())


def gen_proj_models(T):
    g = torch.Generator().manual_seed(31)
    C, N, W, H = 2, 2048, 128, 80
    z = torch.rand(C, N, generator=g) * 4.5 + 0.5
    xy = (torch.rand(C, N, 2, generator=g) * 2 - 1) * 1.2 * z[..., None]  # some past the clamp
    means = torch.cat([xy, z[..., None]], -1)
    means_fe = means.clone()  # fisheye: 10 % behind the camera, away from the axis
    back = torch.rand(C, N, generator=g) < 0.1
    ang = torch.rand(C, N, generator=g) * 2 * math.pi
    rad = torch.rand(C, N, generator=g) * 2.0 + 0.2
    means_fe[..., 0] = torch.where(back, rad * torch.cos(ang), means_fe[..., 0])
    means_fe[..., 1] = torch.where(back, rad * torch.sin(ang), means_fe[..., 1])
    means_fe[..., 2] = torch.where(back, -means_fe[..., 2], means_fe[..., 2])
    A = torch.randn(C, N, 3, 3, generator=g) * 0.2
    covars = A @ A.transpose(-1, -2) + 0.005 * torch.eye(3)
    covars = (covars + covars.transpose(-1, -2)) / 2
    Ks = torch.tensor([[[100.0, 0, 64.0], [0, 110.0, 40.0], [0, 0, 1]],
                       [[80.0, 0, 60.0], [0, 85.0, 44.0], [0, 0, 1]]])
    v_m2 = torch.randn(C, N, 2, generator=g)
    v_c2 = torch.randn(C, N, 2, 2, generator=g)  # not symmetric
    # near-axis fisheye set: 256 points with |xy| / z in [1e-3, 1e-2]
    Cn, Nn = 2, 128
    zn = torch.rand(Cn, Nn, generator=g) * 4.5 + 0.5
    rn = torch.exp(torch.rand(Cn, Nn, generator=g) * math.log(10.0) + math.log(1e-3)) * zn
    an = torch.rand(Cn, Nn, generator=g) * 2 * math.pi
    means_ax = torch.stack([rn * torch.cos(an), rn * torch.sin(an), zn], -1)
    An = torch.randn(Cn, Nn, 3, 3, generator=g) * 0.2
    covars_ax = An @ An.transpose(-1, -2) + 0.005 * torch.eye(3)
    covars_ax = (covars_ax + covars_ax.transpose(-1, -2)) / 2
    v_m2_ax = torch.randn(Cn, Nn, 2, generator=g)
    v_c2_ax = torch.randn(Cn, Nn, 2, 2, generator=g)

    shared = dict(means=means.numpy(), means_fisheye=means_fe.numpy(), covars=covars.numpy(),
                  Ks=Ks.numpy(), width=W, height=H, v_means2d=v_m2.numpy(),
                  v_covars2d=v_c2.numpy(), axis_means=means_ax.numpy(),
                  axis_covars=covars_ax.numpy(), axis_v_means2d=v_m2_ax.numpy(),
                  axis_v_covars2d=v_c2_ax.numpy())
    r64 = run_proj(T._fisheye_proj, torch.float64, means_ax, covars_ax, Ks, W, H, v_m2_ax, v_c2_ax)
    r32 = run_proj(T._fisheye_proj, torch.float32, means_ax, covars_ax, Ks, W, H, v_m2_ax, v_c2_ax)
    for k in r64:
        shared["axis_" + k] = r64[k]
        shared["bar_axis_" + k] = bar(r32[k], r64[k])
        print(f"  fisheye near-axis bar_{k} = {shared['bar_axis_' + k]:.2e}")
    save("proj_models", shared)

    fns = dict(pinhole=T._persp_proj, ortho=T._ortho_proj, fisheye=T._fisheye_proj)
    for model, fn in fns.items():
        mm = means_fe if model == "fisheye" else means
        r64 = run_proj(fn, torch.float64, mm, covars, Ks, W, H, v_m2, v_c2)
        r32 = run_proj(fn, torch.float32, mm, covars, Ks, W, H, v_m2, v_c2)
        arrs = {}
        for k in r64:
            arrs[k] = r64[k]
            arrs["bar_" + k] = bar(r32[k], r64[k])
            print(f"  {model} bar_{k} = {arrs['bar_' + k]:.2e}")
        save("proj_models_" + model, arrs)


def main():
    T = _impl()
    gen_covar_proj(T)
    gen_world_to_cam(T)
    gen_proj_models(T)


if __name__ == "__main__":
    main()
