"""GPU checks of the projection stage for Gaussians given by covariances
(csrc/projection_covar.hip): the fused projection from covars [N,6] (dense
and packed), `world_to_cam`, `proj` (pinhole / ortho / fisheye) and
`rasterization(covars=...)`.

The oracle is the reference's torch implementation run in float64
(tests/golden/make_golden_covar.py).  Every bound is 4 x the error of the
reference's own float32 run against that oracle (`bar_*`, stored with the
goldens, max error / max |golden|); for the fused projection the bound is
floored at 1e-6.  The factor 4 covers fma contraction and the atomic summation
order over cameras, which the float32 torch run does not have.  Achieved
values are recorded beside the end-to-end test's, by its recorder
(test_gpu_parity._record_errors), under "covar_<case>"."""

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_parity import E2E_TOL, _e2e_check, _record_errors

pytestmark = pytest.mark.gpu
DEV = "cuda"
RADII_CAP = 0.002  # share of pairs whose radius may differ (by at most 1)
FACTOR = 4.0
FLOOR = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401  (fails loudly if the .so is missing)


def T(x, dtype=torch.float32):
    return torch.from_numpy(np.array(x, copy=True)).to(DEV).to(dtype)  # the goldens stay read-only


def npy(t):
    return t.detach().cpu().numpy().astype(np.float64)


_GOLD = {}


def gold(name):
    """The goldens, loaded once and shared (read-only) by the tests."""
    if name not in _GOLD:
        g = load_golden(name)
        for v in g.values():
            v.setflags(write=False)
        _GOLD[name] = g
    return _GOLD[name]


def _record(name, errs):
    _record_errors("covar_" + name, errs)


def rel_err(ours, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(ours, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def check_all(name, pairs, floor):
    """pairs: {what: (ours, golden, bar)}.  Prints and records every figure,
    then asserts each against max(4 x bar, floor)."""
    errs, bad = {}, []
    for what, (ours, ref, bar) in pairs.items():
        e = rel_err(ours, ref)
        bound = max(FACTOR * float(bar), floor)
        errs[what] = {"err": e, "bar": float(bar), "bound": bound}
        print(f"{name}: {what}: err {e:.3e}  bound {bound:.3e}  (bar {float(bar):.3e})")
        if not e <= bound:
            bad.append((what, e, bound))
    _record(name, errs)
    assert not bad, (name, bad)


def check_radii(ours, ref):
    """At most 0.2 % of the pairs differ, and by at most 1; returns the mask
    of the pairs that differ."""
    ours = np.asarray(ours, np.int64)
    ref = np.asarray(ref, np.int64)
    assert ours.shape == ref.shape, (ours.shape, ref.shape)
    diff = ours != ref
    if ours.size:
        assert diff.mean() <= RADII_CAP, diff.mean()
        assert np.abs(ours - ref).max() <= 1, np.abs(ours - ref).max()
    return diff


# ================================================== dense, vs the float64 run
@pytest.mark.parametrize("comp", [False, True])
@pytest.mark.parametrize("C", [3, 1])
def test_dense_projection_from_covars_vs_float64(C, comp):
    from gsplat_hip import fully_fused_projection
    g = gold("covar_proj")
    tag = f"_c{C}" + ("_comp" if comp else "")
    means = T(g["means"]).requires_grad_(True)
    covars = T(g["covars"]).requires_grad_(True)
    vm = T(g["viewmats"][:C]).requires_grad_(True)
    radii, m2, d, cn, cp = fully_fused_projection(
        means, covars, None, None, vm, T(g["Ks"][:C]), int(g["width"]), int(g["height"]),
        eps2d=float(g["eps2d"]), near_plane=float(g["near"]), far_plane=float(g["far"]),
        calc_compensations=comp)
    assert radii.dtype == torch.int32 and radii.shape == (C, means.shape[0])
    assert (cp is not None) == comp
    r = radii.cpu().numpy()
    diff = check_radii(r, g["radii"][:C])
    v = (r > 0) & (g["radii"][:C] > 0)
    # invalid entries are written as zeros
    inv = torch.from_numpy(r == 0).to(DEV)
    assert not m2[inv].any() and not cn[inv].any()
    if comp:
        assert not cp[inv].any()
    pairs = {"means2d": (npy(m2)[v], g["means2d"][:C][v], g["bar_means2d"]),
             "depths": (npy(d)[v], g["depths"][:C][v], g["bar_depths"]),
             "conics": (npy(cn)[v], g["conics"][:C][v], g["bar_conics"])}
    if comp:
        pairs["comps"] = (npy(cp)[v], g["comps"][:C][v], g["bar_comps"])
    sel = radii > 0
    loss = (m2[sel] * T(g["v_means2d"][:C])[sel]).sum() + (d[sel] * T(g["v_depths"][:C])[sel]).sum() \
        + (cn[sel] * T(g["v_conics"][:C])[sel]).sum()
    if comp:
        loss = loss + (cp[sel] * T(g["v_comps"][:C])[sel]).sum()
    v_means, v_covars, v_vm = torch.autograd.grad(loss, (means, covars, vm))
    assert v_covars.shape == covars.shape
    keep = ~diff.any(0)  # Gaussians whose radii differ are left out
    assert (~keep).mean() <= RADII_CAP
    pairs["v_means"] = (npy(v_means)[keep], g["v_means" + tag][keep], g["bar_v_means" + tag])
    pairs["v_covars"] = (npy(v_covars)[keep], g["v_covars" + tag][keep], g["bar_v_covars" + tag])
    pairs["v_viewmats"] = (npy(v_vm), g["v_viewmats" + tag], g["bar_v_viewmats" + tag])
    check_all("dense" + tag, pairs, FLOOR)


# ==================================================================== packed
def scene(N=3000, C=3, W=160, H=120, seed=0):
    """test_gpu_packed.py's scene, with the covariances of its quats / scales."""
    from gsplat_hip import quat_scale_to_covar_preci
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(N, 3, generator=g) * torch.tensor([1.0, 0.8, 0.6])
    means[:, 2] += 4.0
    if N == 1:
        means[0] = torch.tensor([0.1, -0.1, 4.0])  # the single lane is a visible one
    quats = torch.randn(N, 4, generator=g)
    scales = torch.rand(N, 3, generator=g) * 0.08 + 0.005
    vms = torch.eye(4).repeat(C, 1, 1)
    for c in range(C):
        vms[c, 0, 3] = 0.3 * c
        vms[c, 1, 3] = -0.1 * c
    K = torch.tensor([[150.0, 0, W / 2], [0, 150.0, H / 2], [0, 0, 1]]).repeat(C, 1, 1)
    means, quats, scales, vms, K = (x.to(DEV) for x in (means, quats, scales, vms, K))
    covars = quat_scale_to_covar_preci(quats, scales, compute_preci=False, triu=True)[0]
    return means, covars, vms, K, W, H


@pytest.mark.parametrize("N,C,comp,clip", [(3000, 3, True, 0.0), (3000, 1, False, 0.0),
                                            (257, 3, False, 0.0), (1, 1, True, 0.0),
                                            (3000, 3, False, 4.0)])
def test_packed_fwd_is_dense_compacted(N, C, comp, clip):
    from gsplat_hip import fully_fused_projection
    means, covars, vms, K, W, H = scene(N=N, C=C)
    r, dm2, dd, dcn, dcp = fully_fused_projection(means, covars, None, None, vms, K, W, H,
                                                  calc_compensations=comp, radius_clip=clip)
    cid, gid, radii, m2, d, cn, cp = fully_fused_projection(
        means, covars, None, None, vms, K, W, H, packed=True, calc_compensations=comp,
        radius_clip=clip)
    sel = r > 0
    assert sel.any()
    if clip > 0:  # the clip removes pairs, and the same ones in both
        r0 = fully_fused_projection(means, covars, None, None, vms, K, W, H)[0]
        assert int((r0 > 0).sum()) > int(sel.sum())
        assert int(r[sel].min()) > clip
    ec, eg = torch.where(sel)
    assert cid.dtype == torch.int64 and gid.dtype == torch.int64
    assert torch.equal(cid, ec) and torch.equal(gid, eg)
    assert torch.equal(radii, r[sel])
    torch.testing.assert_close(m2, dm2[sel], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(d, dd[sel], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(cn, dcn[sel], rtol=1e-5, atol=1e-5)
    if comp:
        torch.testing.assert_close(cp, dcp[sel], rtol=1e-5, atol=1e-5)
    else:
        assert cp is None


@pytest.mark.parametrize("N,C,sparse", [(3000, 1, False), (3000, 3, False), (3000, 3, True),
                                        (257, 3, True), (1, 1, False)])
def test_packed_bwd_matches_dense(N, C, sparse):
    from gsplat_hip import fully_fused_projection
    means, covars, vms, K, W, H = scene(N=N, C=C, seed=1)

    def grads(packed):
        ins = [x.clone().requires_grad_(True) for x in (means, covars, vms)]
        out = fully_fused_projection(ins[0], ins[1], None, None, ins[2], K, W, H, packed=packed,
                                     sparse_grad=sparse and packed, calc_compensations=True)
        if packed:
            cid, gid, radii, m2, d, cn, cp = out
        else:
            radii, m2, d, cn, cp = out
        # cotangents drawn densely [C, N, ...], then gathered for the packed pairs
        g = torch.Generator(device=DEV).manual_seed(5)
        w = [torch.randn((C, N) + s, device=DEV, generator=g) for s in ((2,), (), (3,), ())]
        if packed:
            w = [wi[cid, gid] for wi in w]
            loss = sum((t * wi).sum() for t, wi in zip((m2, d, cn, cp), w))
        else:  # the kept pairs only
            sel = radii > 0
            loss = sum((t[sel] * wi[sel]).sum() for t, wi in zip((m2, d, cn, cp), w))
        return torch.autograd.grad(loss, ins)

    gm_d, gc_d, gv_d = grads(False)
    gm_p, gc_p, gv_p = grads(True)
    if sparse:
        assert gm_p.is_sparse and gc_p.is_sparse
        gm_p, gc_p = (x.coalesce().to_dense() for x in (gm_p, gc_p))
    assert gc_p.shape == (N, 6)
    for a, b in ((gm_p, gm_d), (gc_p, gc_d), (gv_p, gv_d)):
        assert float(b.abs().max()) > 0
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4 * float(b.abs().max()))


# =========================================== agreement with the quats / scales
def _allclose_tol(ours, ref, key, what):
    rtol, atol = E2E_TOL[key]
    ref = npy(ref)
    np.testing.assert_allclose(npy(ours), ref, rtol=rtol, atol=atol * np.abs(ref).max(),
                               err_msg=what)


@pytest.mark.parametrize("C,comp", [(3, True), (1, False)])
def test_covars_path_agrees_with_quats_scales_path(C, comp):
    """The fixture's means and cameras with fresh quaternions and scales drawn
    as its covariances were (scales over e^3).

    Unlike the float64 comparison above, the two paths here do not read the
    same numbers: the covars path reads the covariance rounded to fp32 (6e-8
    relative), the quats / scales path forms it in registers.  A relative
    perturbation d of the covariance moves det(cov2d), and with it the
    compensation sqrt(det / det_blurred), by about d * k / 2, k being the
    ratio of cov2d's eigenvalues.  That is 2e-6 at k = 55 and 1.2e-5 at the
    k = 400 this draw reaches, above the 6.8e-6 bound of comps whatever the
    kernels do (measured over all pairs: 7.4e-6).  So comps is asserted on
    the pairs with k <= 55, which must be most of them; radii, means2d,
    depths, conics and the gradients are asserted on every pair.

    Gradients: v_covars pushed through quat_scale_to_covar_preci's backward
    against the existing v_quats / v_scales.  v_means is not compared: for
    means outside the screen-margin clamp the existing path (as the Triton
    reference) uses the clamped x / z in the z-gradient of means2d, the covars
    path (as the CUDA reference and the float64 oracle) the unclamped one."""
    from gsplat_hip import fully_fused_projection, quat_scale_to_covar_preci
    g = gold("covar_proj")
    N = g["means"].shape[0]
    gen = torch.Generator().manual_seed(77)
    quats = torch.randn(N, 4, generator=gen).to(DEV).requires_grad_(True)
    scales = torch.exp(torch.rand(N, 3, generator=gen) * 3.0 - 4.5).to(DEV).requires_grad_(True)
    means = T(g["means"]).requires_grad_(True)
    vm, K = T(g["viewmats"][:C]), T(g["Ks"][:C])
    kw = dict(eps2d=float(g["eps2d"]), near_plane=float(g["near"]), far_plane=float(g["far"]),
              calc_compensations=comp)
    W, H = int(g["width"]), int(g["height"])
    ref = fully_fused_projection(means, None, quats, scales, vm, K, W, H, **kw)
    covars = quat_scale_to_covar_preci(quats, scales, compute_preci=False, triu=True)[0]
    out = fully_fused_projection(means, covars, None, None, vm, K, W, H, **kw)
    diff = check_radii(out[0].cpu().numpy(), ref[0].cpu().numpy())
    v = ((out[0] > 0) & (ref[0] > 0)).cpu().numpy()
    names = ["means2d", "depths", "conics"] + (["comps"] if comp else [])
    pairs = {k: (npy(o)[v], npy(r)[v], g["bar_" + k]) for k, o, r in zip(names, out[1:], ref[1:])}
    if comp:
        # eigenvalue ratio of cov2d = conic^-1 - eps I, in float64 from the existing path
        a, b, c = (npy(ref[3])[..., i] for i in range(3))
        det = a * c - b * b
        with np.errstate(all="ignore"):
            sxx, sxy, syy = c / det - kw["eps2d"], -b / det, a / det - kw["eps2d"]
            mid, rad = 0.5 * (sxx + syy), np.hypot(0.5 * (sxx - syy), sxy)
            k2d = np.where(mid - rad > 0, (mid + rad) / (mid - rad), np.inf)
        mild = v & (k2d <= 55.0)
        assert mild.sum() >= 0.5 * v.sum(), (mild.sum(), v.sum())
        assert (v & ~mild).any()  # the wide draw does reach past it
        pairs["comps"] = (npy(out[4])[mild], npy(ref[4])[mild], g["bar_comps"])
    check_all(f"vs_quats_c{C}" + ("_comp" if comp else ""), pairs, FLOOR)
    # v_covars pushed through quat_scale_to_covar_preci's backward
    gen = torch.Generator(device=DEV).manual_seed(3)
    w = [torch.randn(t.shape, device=DEV, generator=gen) for t in ref[1:1 + len(names)]]
    sel = torch.from_numpy(v).to(DEV)

    def loss(o):
        return sum((t[sel] * wi[sel]).sum() for t, wi in zip(o[1:1 + len(names)], w))

    gq_r, gs_r = torch.autograd.grad(loss(ref), (quats, scales))
    gq_c, gs_c = torch.autograd.grad(loss(out), (quats, scales))
    keep = ~diff.any(0)
    assert (~keep).mean() <= RADII_CAP
    _allclose_tol(gq_c[keep], gq_r[keep], "v_quats", "v_quats")
    _allclose_tol(gs_c[keep], gs_r[keep], "v_scales", "v_scales")


# ==================================================== world_to_cam and proj
def test_world_to_cam_vs_float64():
    from gsplat_hip import world_to_cam
    g = gold("world_to_cam")
    ins = [T(g[k]).requires_grad_(True) for k in ("means", "covars", "viewmats")]
    mc, cc = world_to_cam(*ins)
    loss = (mc * T(g["v_means_c"])).sum() + (cc * T(g["v_covars_c"])).sum()
    grads = torch.autograd.grad(loss, ins)
    pairs = {"means_c": (npy(mc), g["means_c"], g["bar_means_c"]),
             "covars_c": (npy(cc), g["covars_c"], g["bar_covars_c"])}
    for k, gr in zip(("v_means", "v_covars", "v_viewmats"), grads):
        pairs[k] = (npy(gr), g[k], g["bar_" + k])
    check_all("world_to_cam", pairs, 0.0)


@pytest.mark.parametrize("model", ["pinhole", "ortho", "fisheye"])
def test_proj_vs_float64(model):
    from gsplat_hip import proj
    s, g = gold("proj_models"), gold("proj_models_" + model)
    means = T(s["means_fisheye" if model == "fisheye" else "means"]).requires_grad_(True)
    covars = T(s["covars"]).requires_grad_(True)
    m2, c2 = proj(means, covars, T(s["Ks"]), int(s["width"]), int(s["height"]), camera_model=model)
    loss = (m2 * T(s["v_means2d"])).sum() + (c2 * T(s["v_covars2d"])).sum()  # not symmetric
    vm, vc = torch.autograd.grad(loss, (means, covars))
    pairs = {"means2d": (npy(m2), g["means2d"], g["bar_means2d"]),
             "covars2d": (npy(c2), g["covars2d"], g["bar_covars2d"]),
             "v_means": (npy(vm), g["v_means"], g["bar_v_means"]),
             "v_covars": (npy(vc), g["v_covars"], g["bar_v_covars"])}
    check_all("proj_" + model, pairs, 0.0)


def test_proj_fisheye_near_axis_vs_float64():
    """|xy| / z in [1e-3, 1e-2]: where the closed-form VJP cancels in fp32."""
    from gsplat_hip import proj
    s = gold("proj_models")
    means = T(s["axis_means"]).requires_grad_(True)
    covars = T(s["axis_covars"]).requires_grad_(True)
    m2, c2 = proj(means, covars, T(s["Ks"]), int(s["width"]), int(s["height"]),
                  camera_model="fisheye")
    loss = (m2 * T(s["axis_v_means2d"])).sum() + (c2 * T(s["axis_v_covars2d"])).sum()
    vm, vc = torch.autograd.grad(loss, (means, covars))
    pairs = {k: (npy(o), s["axis_" + k], s["bar_axis_" + k])
             for k, o in (("means2d", m2), ("covars2d", c2), ("v_means", vm), ("v_covars", vc))}
    check_all("proj_fisheye_near_axis", pairs, 0.0)
    # bar_axis_v_means is the reference's fp32 closed form cancelling (8.6e-5): a
    # kernel as inaccurate would pass the bound above.  Away from the axis
    # that form is at bar_v_means of the regular fisheye set; a VJP that stays
    # accurate on the axis meets 4 x that here too.
    tight = FACTOR * float(gold("proj_models_fisheye")["bar_v_means"])
    e = rel_err(npy(vm), s["axis_v_means"])
    print(f"proj_fisheye_near_axis: v_means err {e:.3e}  tight bound {tight:.3e}")
    assert e <= tight, (e, tight)


def test_gradients_are_computed_only_when_needed(monkeypatch):
    """requires_grad on means alone: the other gradient buffers are not
    allocated (null pointers reach the kernels) and come back as None."""
    from gsplat_hip import _lib, _wrapper_covar, proj, world_to_cam
    g = gold("world_to_cam")
    seen = {}
    real = _lib.call

    def spy(name, *a):
        seen[name] = a
        return real(name, *a)

    monkeypatch.setattr(_wrapper_covar._lib, "call", spy)
    means = T(g["means"]).requires_grad_(True)
    covars, vm = T(g["covars"]), T(g["viewmats"])
    mc, cc = world_to_cam(means, covars, vm)
    (mc.sum() + cc.sum()).backward()
    # (C, N, means, covars, viewmats, v_means_c, v_covars_c, v_means, v_covars, v_viewmats, stream)
    a = seen["gsplat_hip_world_to_cam_bwd"]
    assert a[7] != 0 and a[8] == 0 and a[9] == 0
    assert means.grad is not None and covars.grad is None and vm.grad is None
    ref = torch.einsum("cij,cni->nj", vm[:, :3, :3], torch.ones_like(mc))
    torch.testing.assert_close(means.grad, ref, rtol=1e-5, atol=1e-5)

    s = gold("proj_models")
    pm = T(s["means"]).requires_grad_(True)
    m2, c2 = proj(pm, T(s["covars"]), T(s["Ks"]), int(s["width"]), int(s["height"]))
    m2.sum().backward()  # covars2d unused: its cotangent is None
    # (C, N, model, means, covars, Ks, W, H, v_means2d, v_covars2d, v_means, v_covars, stream)
    a = seen["gsplat_hip_proj_bwd"]
    assert a[8] != 0 and a[9] == 0 and a[10] != 0 and a[11] == 0
    assert pm.grad is not None and torch.isfinite(pm.grad).all()
    # and covars alone
    pc = T(s["covars"]).requires_grad_(True)
    m2, c2 = proj(T(s["means"]), pc, T(s["Ks"]), int(s["width"]), int(s["height"]))
    c2.sum().backward()
    a = seen["gsplat_hip_proj_bwd"]
    assert a[10] == 0 and a[11] != 0 and pc.grad is not None


# =============================================================== composition
@pytest.mark.parametrize("comp", [False, True])
def test_unfused_stages_compose_to_the_fused_projection(comp):
    from gsplat_hip import fully_fused_projection, proj, world_to_cam
    g = gold("covar_proj")
    means, c6 = T(g["means"]), T(g["covars"])
    vm, K = T(g["viewmats"]), T(g["Ks"])
    W, H, eps2d = int(g["width"]), int(g["height"]), float(g["eps2d"])
    radii, m2, d, cn, cp = fully_fused_projection(
        means, c6, None, None, vm, K, W, H, eps2d=eps2d, near_plane=float(g["near"]),
        far_plane=float(g["far"]), calc_compensations=comp)
    idx = torch.tensor([[0, 1, 2], [1, 3, 4], [2, 4, 5]], device=DEV)
    means_c, covars_c = world_to_cam(means, c6[:, idx], vm)
    u2, c2 = proj(means_c, covars_c, K, W, H, camera_model="pinhole")
    # the blur and the inverse in float64 on the host: conic = sym((S + eps I)^-1),
    # compensation = sqrt(det S / det(S + eps I))
    S2 = c2.detach().double().cpu()
    blurred = S2 + eps2d * torch.eye(2, dtype=torch.float64)
    inv = torch.linalg.inv(blurred)
    inv = 0.5 * (inv + inv.transpose(-1, -2))
    conics = torch.stack([inv[..., 0, 0], inv[..., 0, 1], inv[..., 1, 1]], -1)
    v = (radii > 0).cpu().numpy()
    assert v.any()
    pairs = {"means2d": (npy(u2)[v], npy(m2)[v], g["bar_means2d"]),
             "depths": (npy(means_c[..., 2])[v], npy(d)[v], g["bar_depths"]),
             "conics": (npy(conics)[v], npy(cn)[v], g["bar_conics"])}
    if comp:
        ratio = torch.linalg.det(S2) / torch.linalg.det(blurred)
        pairs["comps"] = (npy(ratio.clamp(min=0.0).sqrt())[v], npy(cp)[v], g["bar_comps"])
    check_all("composition" + ("_comp" if comp else ""), pairs, FLOOR)


# ================================================================ end to end
def _e2e_inputs(name):
    from gsplat_hip import quat_scale_to_covar_preci
    g = load_golden(name)
    ins = [T(g[k]).requires_grad_(True) for k in ("means", "quats", "scales", "opacities", "sh")]
    # [N,3,3]; its gradient flows back to quats / scales, where the goldens are
    covars = quat_scale_to_covar_preci(ins[1], ins[2], compute_preci=False, triu=False)[0]
    return g, ins, covars


@pytest.mark.parametrize("packed", [False, True])
def test_rasterization_from_covars_vs_reference(packed):
    import gsplat_hip
    g, ins, covars = _e2e_inputs("e2e_m1_rgb")
    assert covars.shape == (ins[0].shape[0], 3, 3)
    rc, ra, meta = gsplat_hip.rasterization(
        ins[0], None, None, ins[3], ins[4], T(g["viewmats"]), T(g["Ks"]), int(g["width"]),
        int(g["height"]), sh_degree=3, packed=packed, render_mode=str(g["render_mode"]),
        backgrounds=T(g["backgrounds"]), covars=covars)
    radii = meta["radii"].cpu().numpy()
    if packed:
        cam = meta["camera_ids"].cpu().numpy()
        gid = meta["gaussian_ids"].cpu().numpy()
        dense = np.zeros_like(g["radii"])
        dense[cam, gid] = radii
        radii = dense
    check_radii(radii, g["radii"])
    _e2e_check("covars_e2e_m1_rgb" + ("_packed" if packed else ""), g, rc, ra, ins)


def test_rasterization_from_covars_antialiased_vs_reference():
    import gsplat_hip
    g, ins, covars = _e2e_inputs("e2e_m1_aa")
    rc, ra, meta = gsplat_hip.rasterization(
        ins[0], None, None, ins[3], ins[4], T(g["viewmats"]), T(g["Ks"]), int(g["width"]),
        int(g["height"]), sh_degree=3, packed=False, rasterize_mode="antialiased", covars=covars)
    check_radii(meta["radii"].cpu().numpy(), g["radii"])
    _e2e_check("covars_e2e_m1_aa", g, rc, ra, ins)


# =============================================================== edge shapes
@pytest.mark.parametrize("N,C", [(0, 2), (5, 0), (0, 0)])
@pytest.mark.parametrize("packed", [False, True])
def test_empty_shapes(N, C, packed):
    from gsplat_hip import fully_fused_projection, proj, world_to_cam
    means = torch.zeros(N, 3, device=DEV).requires_grad_(True)
    covars = (torch.ones(N, 6, device=DEV) * 0.01).requires_grad_(True)
    vm = torch.eye(4, device=DEV).repeat(C, 1, 1).requires_grad_(True)
    K = torch.eye(3, device=DEV).repeat(C, 1, 1)
    out = fully_fused_projection(means, covars, None, None, vm, K, 16, 16, packed=packed,
                                 calc_compensations=True)
    if packed:
        assert all(o.shape[0] == 0 for o in out)
        m2, d, cn, cp = out[3:]
    else:
        assert out[0].shape == (C, N)
        m2, d, cn, cp = out[1:]
    gm, gc, gv = torch.autograd.grad(m2.sum() + d.sum() + cn.sum() + cp.sum(), (means, covars, vm))
    assert gm.shape == (N, 3) and gc.shape == (N, 6) and gv.shape == (C, 4, 4)
    assert not gm.any() and not gc.any() and not gv.any()
    if not packed:
        c33 = torch.eye(3, device=DEV).repeat(N, 1, 1).requires_grad_(True)
        mc, cc = world_to_cam(means, c33, vm)
        assert mc.shape == (C, N, 3) and cc.shape == (C, N, 3, 3)
        u2, c2 = proj(mc, cc, K, 16, 16)
        assert u2.shape == (C, N, 2) and c2.shape == (C, N, 2, 2)
        gm, gc, gv = torch.autograd.grad(u2.sum() + c2.sum(), (means, c33, vm))
        assert gm.shape == (N, 3) and gc.shape == (N, 3, 3) and gv.shape == (C, 4, 4)
        assert not gm.any() and not gc.any() and not gv.any()
    torch.cuda.synchronize()


def test_non_contiguous_covars_view():
    from gsplat_hip import fully_fused_projection
    means, covars, vms, K, W, H = scene(N=300, C=2)
    wide = torch.zeros(300, 9, device=DEV)
    wide[:, 1:7] = covars
    view = wide[:, 1:7]  # row stride 9, offset 4 B: neither contiguous nor 8-B aligned
    assert not view.is_contiguous()
    a = fully_fused_projection(means, covars, None, None, vms, K, W, H)
    b = fully_fused_projection(means, view, None, None, vms, K, W, H)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    view = view.detach().requires_grad_(True)
    out = fully_fused_projection(means, view, None, None, vms, K, W, H)
    (gv,) = torch.autograd.grad(out[3].sum(), (view,))
    assert gv.shape == (300, 6) and torch.isfinite(gv).all() and gv.any()
