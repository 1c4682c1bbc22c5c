"""GPU: the camera pose kernels (csrc/pose.hip and the pose variant of the
fused projection backward) against float64 torch compositions written here
from the formulas of the reference's CameraOptModule, the CPU oracle's
projection backward, and torch.optim.Adam."""

import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401  (fails loudly if the .so is missing)


# ------------------------------------------------------------ float64 reference
def _normalize(x):
    return x / torch.clamp(x.norm(dim=-1, keepdim=True), min=1e-12)


def pose_T(e):
    """T(e) [..., 4, 4] of rows e [..., 9] = (dx, d6), in e's dtype."""
    dx, d6 = e[..., :3], e[..., 3:]
    one = torch.tensor([1.0, 0, 0, 0, 1.0, 0], dtype=e.dtype, device=e.device)
    a1, a2 = (d6 + one)[..., :3], (d6 + one)[..., 3:]
    b1 = _normalize(a1)
    b2 = _normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1)
    b3 = torch.cross(b1, b2, dim=-1)
    R = torch.stack([b1, b2, b3], dim=-2)
    top = torch.cat([R, dx[..., None]], dim=-1)
    bot = torch.tensor([0.0, 0, 0, 1.0], dtype=e.dtype,
                       device=e.device).expand(e.shape[:-1] + (1, 4))
    return torch.cat([top, bot], dim=-2)


def rigid(batch, g):
    """Random rigid camera-to-world matrices [*batch, 4, 4], float64."""
    q, _ = torch.linalg.qr(torch.randn(*batch, 3, 3, generator=g, dtype=torch.float64))
    m = torch.zeros(*batch, 4, 4, dtype=torch.float64)
    m[..., :3, :3] = q
    m[..., :3, 3] = torch.randn(*batch, 3, generator=g, dtype=torch.float64) * 2.0
    m[..., 3, 3] = 1.0
    return m


def within(got, ref, what):
    """|got - ref| <= 1e-5 max|ref|, per tensor."""
    ref = ref.detach().double().cpu()
    err = float((got.detach().double().cpu() - ref).abs().max())
    bound = 1e-5 * float(ref.abs().max())
    print(f"{what}: max err {err:.3e}  bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


# ------------------------------------------------------------------ pose_adjust
@pytest.mark.parametrize("batch", [(), (1,), (5,)], ids=["scalar", "one", "five"])
@pytest.mark.parametrize("std", [0.0, 0.1, 1.0])
def test_pose_adjust_forward_and_backward(batch, std):
    import gsplat_hip
    g = torch.Generator().manual_seed(11 + len(batch) + int(std * 100))
    c2w = rigid(batch, g)
    e = torch.randn(*batch, 9, generator=g, dtype=torch.float64) * std
    w = torch.randn(*batch, 4, 4, generator=g, dtype=torch.float64)
    c32 = c2w.float().to(DEV)
    e_dev = e.float().to(DEV).requires_grad_(True)
    out = gsplat_hip.pose_adjust(c32, e_dev)
    assert out.shape == c32.shape and out.dtype == torch.float32
    (g_dev,) = torch.autograd.grad((out * w.float().to(DEV)).sum(), e_dev)
    assert g_dev.shape == e_dev.shape
    # the reference evaluated at the float32 inputs the kernel saw
    e_in = e.float().double().requires_grad_(True)
    out_in = c2w.float().double() @ pose_T(e_in)
    (g_in,) = torch.autograd.grad((out_in * w.float().double()).sum(), e_in)
    within(out, out_in, "camtoworlds'")
    within(g_dev, g_in, "v_deltas")
    if std == 0.0:  # the identity adjustment returns its input bit for bit
        assert torch.equal(out, c32)


def test_pose_adjust_gives_no_camera_gradient():
    import gsplat_hip
    g = torch.Generator().manual_seed(3)
    c = rigid((2,), g).float().to(DEV).requires_grad_(True)
    e = torch.zeros(2, 9, device=DEV, requires_grad=True)
    gsplat_hip.pose_adjust(c, e).sum().backward()
    assert c.grad is None and e.grad is not None


def test_pose_apply_matches_the_inverse_of_the_adjusted_camera():
    """viewmat' = T_adj^-1 T_noise^-1 viewmat is inv(c2w T_noise T_adj); a zero
    row reproduces the base bit for bit; the index is clamped."""
    from gsplat_hip.pose import pose_apply
    g = torch.Generator().manual_seed(5)
    n = 4
    c2w = rigid((n,), g)
    vms = torch.linalg.inv(c2w).float().contiguous()
    emb = (torch.randn(n, 9, generator=g) * 0.1).float()
    noi = (torch.randn(n, 9, generator=g) * 0.05).float()
    vd, ed, nd = vms.to(DEV), emb.to(DEV), noi.to(DEV)
    idx = torch.arange(n, device=DEV)
    for ci in range(n):
        for use_e, use_n in ((True, False), (False, True), (True, True)):
            c2w_out = torch.empty(4, 4, device=DEV)
            out = pose_apply(vd[ci:ci + 1], idx[ci:ci + 1], ed if use_e else None,
                             nd if use_n else None, camtoworld_out=c2w_out)
            ref = torch.linalg.inv(vms[ci].double())
            if use_n:
                ref = ref @ pose_T(noi[ci].double())
            if use_e:
                ref = ref @ pose_T(emb[ci].double())
            within(out[0], torch.linalg.inv(ref), "viewmat'")
            within(c2w_out, ref, "camtoworld'")
    zero = torch.zeros(n, 9, device=DEV)
    for ci in range(n):
        assert torch.equal(pose_apply(vd[ci:ci + 1], idx[ci:ci + 1], zero, zero)[0], vd[ci])
    far = torch.tensor([99], device=DEV)
    assert torch.equal(pose_apply(vd[:1], far, ed), pose_apply(vd[:1], idx[n - 1:], ed))


# ------------------------------------------- pose variant of the projection bwd
W_IMG, H_IMG = 64, 48


def _proj_case(N, culled=False, seed=0):
    """Inputs of gsplat_hip_projection_bwd_adam for N Gaussians and one camera."""
    import gsplat_hip
    g = torch.Generator().manual_seed(100 + N + seed)
    means = torch.randn(N, 3, generator=g) * 0.8
    means[:, 2] += -4.0 if culled else 4.0
    if not culled and N > 4:
        means[::5, 2] -= 8.0  # some behind the camera: radii 0 inside the blocks
    quats = torch.randn(N, 4, generator=g)
    log_scales = torch.log(torch.rand(N, 3, generator=g) * 0.2 + 0.02)
    logits = torch.randn(N, generator=g)
    vm = torch.eye(4)
    vm[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    if torch.det(vm[:3, :3]) < 0:
        vm[:3, 0] = -vm[:3, 0]
    vm[:3, :3] = torch.eye(3) * 0.9 + vm[:3, :3] * 0.1  # near the identity, not orthonormal
    vm[:3, 3] = torch.tensor([0.1, -0.05, 0.2])
    K = torch.tensor([[60.0, 0, W_IMG / 2], [0, 60.0, H_IMG / 2], [0, 0, 1]])
    d = dict(means=means, quats=quats, log_scales=log_scales, logits=logits, vm=vm[None],
             K=K[None])
    d = {k: v.to(DEV).contiguous() for k, v in d.items()}
    d["scales"] = torch.exp(d["log_scales"])
    d["opac"] = torch.sigmoid(d["logits"])
    radii, _, _, conics, _ = gsplat_hip.fully_fused_projection(
        d["means"], None, d["quats"], d["scales"], d["vm"], d["K"], W_IMG, H_IMG, packed=False,
        near_plane=0.01, far_plane=1e10)
    d["radii"], d["conics"] = radii, conics.contiguous()
    vis = (radii[0] > 0).float()
    d["v_means2d"] = torch.randn(1, N, 2, generator=g).to(DEV)
    d["v_depths"] = torch.randn(1, N, generator=g).to(DEV)
    d["v_conics"] = torch.randn(1, N, 3, generator=g).to(DEV)
    # the SH-colour backward writes zero rows for the culled Gaussians
    d["v_dirs"] = (torch.randn(N, 3, generator=g).to(DEV) * vis[:, None]).contiguous()
    d["v_opac"] = torch.randn(1, N, generator=g).to(DEV)
    d["m"] = [(torch.randn(*s, generator=g) * 0.01).to(DEV) for s in ((N, 3), (N, 3), (N, 4), (N,))]
    d["v"] = [(torch.rand(*s, generator=g) * 1e-4).to(DEV) for s in ((N, 3), (N, 3), (N, 4), (N,))]
    return d


def _run_bwd_adam(d, pose):
    """One launch on clones of the parameters and moments; returns them and
    the pose workspace (None for the existing entry)."""
    from gsplat_hip import _wrapper
    from gsplat_hip.pose import pose_workspace
    N = d["means"].shape[0]
    p = [d[k].clone() for k in ("means", "log_scales", "quats", "logits")]
    m, v = [t.clone() for t in d["m"]], [t.clone() for t in d["v"]]
    ga = _wrapper.GeomAdamInBackward(p, m, v, [1.6e-4, 5e-3, 1e-3, 5e-2], (0.9, 0.999), 1e-15, 3)
    ws = None
    if pose:
        ws = pose_workspace(N, DEV)
        ws.fill_(float("nan"))  # every row must be written
        ga.pose_ws = ws
    fusion = types.SimpleNamespace(v_dirs=d["v_dirs"], v_opac_in=d["v_opac"], opac_act=d["opac"])
    ga.run(p[0], p[2], d["scales"], d["vm"], d["K"], W_IMG, H_IMG, 0.3, d["radii"], d["conics"],
           d["v_means2d"], d["v_depths"], d["v_conics"], fusion)
    torch.cuda.synchronize()
    return p, m, v, ws


@pytest.mark.parametrize("N", [1, 255, 257, 1000])
def test_projection_pose_variant(N):
    from oracle import gsplat_oracle as O
    d = _proj_case(N)
    assert int((d["radii"] > 0).sum()) > 0
    p0, m0, v0, _ = _run_bwd_adam(d, pose=False)
    p1, m1, v1, ws = _run_bwd_adam(d, pose=True)
    p2, m2, v2, ws2 = _run_bwd_adam(d, pose=True)
    nb = (N + 255) // 256
    rows = ws[:16 * nb].view(nb, 16)
    assert torch.isfinite(rows).all() and not rows[:, 15].any()
    # the update is the existing entry's, bit for bit, and two runs agree
    for a, b, c in zip(p0 + m0 + v0, p1 + m1 + v1, p2 + m2 + v2):
        assert torch.equal(a, b) and torch.equal(b, c)
    assert torch.equal(ws[:16 * nb], ws2[:16 * nb])
    for a, b in zip(p0, (d["means"], d["log_scales"], d["quats"], d["logits"])):
        assert not torch.equal(a, b)  # (an update did happen)

    sums = rows.double().sum(0).cpu().numpy()
    c = lambda t: t.detach().cpu().numpy()  # noqa: E731
    _, _, _, ref = O.proj_bwd(c(d["means"]), c(d["quats"]), c(d["scales"]), c(d["vm"]), c(d["K"]),
                              W_IMG, H_IMG, 0.3, c(d["radii"]), c(d["conics"]), None,
                              c(d["v_means2d"]), c(d["v_depths"]), c(d["v_conics"]), None)
    ref = ref[0, :3, :].reshape(-1).astype(np.float64)
    err = np.abs(sums[:12] - ref)
    print(f"N={N}: v_viewmat max err {err.max():.3e}, max|ref| {np.abs(ref).max():.3e}")
    # tests/test_gpu_parity.py's v_viewmats tolerance, in both readings
    assert (err <= 5e-3 + 1e-4 * np.abs(ref)).all(), (sums[:12], ref)
    assert (err <= 1e-4 + 5e-3 * np.abs(ref)).all(), (sums[:12], ref)
    # sum v_dirs: any fp32 summation order of n values is within
    # (n - 1) 2^-24 sum|x| of the exact sum
    vd = d["v_dirs"].double().cpu()
    bound = (N - 1) * 2.0 ** -24 * vd.abs().sum(0).numpy() + 1e-30
    errd = np.abs(sums[12:15] - vd.sum(0).numpy())
    print(f"N={N}: sum v_dirs err {errd}, bound {bound}")
    assert (errd <= bound).all(), (errd, bound)


def test_projection_pose_variant_all_culled():
    d = _proj_case(300, culled=True)
    assert int((d["radii"] > 0).sum()) == 0
    _, _, _, ws = _run_bwd_adam(d, pose=True)
    assert torch.equal(ws[:32], torch.zeros(32, device=DEV))


# ------------------------------------------------------------------ pose_bwd_adam
def _grad_ref(tot, vm, e, noise_row):
    """d/de of sum(G * V'(e)[:3]) - s . campos(e) in float64: G the 3x4
    view-matrix gradient, s the summed v_dirs, V' = T(e)^-1 T(noise)^-1 V,
    campos the translation of inv(V')."""
    G = torch.tensor(tot[:12], dtype=torch.float64).view(3, 4)
    s = torch.tensor(tot[12:15], dtype=torch.float64)
    e = e.clone().requires_grad_(True)
    c2w = torch.linalg.inv(vm.double())
    if noise_row is not None:
        c2w = c2w @ pose_T(noise_row.double())
    c2w = c2w @ pose_T(e)
    V = torch.linalg.inv(c2w)
    loss = (G * V[:3]).sum() - (s * c2w[:3, 3]).sum()
    (g,) = torch.autograd.grad(loss, e)
    return g


@pytest.mark.parametrize("n_images,with_noise", [(1, False), (3, True), (300, False)])
def test_pose_bwd_adam_matches_torch_adam(n_images, with_noise):
    from gsplat_hip.pose import pose_bwd_adam
    g = torch.Generator().manual_seed(40 + n_images)
    lr, wd = 1e-3, 1e-2
    N = 20000  # 79 workspace rows: more than the 64 row groups of the kernel
    nb = (N + 255) // 256
    table = torch.randn(n_images, 9, generator=g, dtype=torch.float64) * 0.1
    table = table.float().double()
    noise = (torch.randn(n_images, 9, generator=g) * 0.05) if with_noise else None
    vms = torch.linalg.inv(rigid((n_images,), g)).float().contiguous()
    ref_p = table.clone().requires_grad_(True)
    # the float32 hyper-parameters the C ABI carries (1 - float32(0.999) is
    # 1.3e-5 off 0.001 in relative terms: an input, not the kernel's error)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    opt = torch.optim.Adam([ref_p], lr=f32(lr), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8),
                           weight_decay=f32(wd))
    emb = table.float().to(DEV)
    m, v = torch.zeros_like(emb), torch.zeros_like(emb)
    vd = vms.to(DEV)
    nd = None if noise is None else noise.to(DEV)
    idx = torch.arange(n_images, device=DEV)
    cams = [0, 0, 0] if n_images == 1 else ([0, 1, 2] if n_images == 3 else [7, 150, 299])
    for step, ci in enumerate(cams, 1):
        # multiples of 1/256: the kernel's fp32 sums of the rows are exact
        ws = torch.randint(-2048, 2048, (nb, 16), generator=g).float() / 256.0
        tot = ws.double().sum(0).numpy()
        ref_p.grad = torch.zeros_like(ref_p)
        ref_p.grad[ci] = _grad_ref(tot, vms[ci], ref_p.detach()[ci],
                                   None if noise is None else noise[ci])
        before = ref_p.detach().clone()
        opt.step()
        pose_bwd_adam(ws.to(DEV).reshape(-1), N, vd[ci:ci + 1], idx[ci:ci + 1], emb, m, v, lr, wd,
                      step, noise=nd)
        torch.cuda.synchronize()
        within(emb, ref_p, f"embeds after step {step}")
        within(m, opt.state[ref_p]["exp_avg"], f"exp_avg after step {step}")
        within(v, opt.state[ref_p]["exp_avg_sq"], f"exp_avg_sq after step {step}")
        # the rows of the other cameras: weight decay and moment decay only
        # (the reference's dense Adam; they do move, and the selected row
        # moves differently from what decay alone would give)
        if n_images > 1:
            others = [r for r in range(n_images) if r != ci]
            moved = (ref_p.detach() - before)[others].abs().max()
            assert float(moved) > 0.0


def test_pose_bwd_adam_void_step_and_device_factors():
    from gsplat_hip.losses import adam_factors
    from gsplat_hip.pose import BETAS, pose_bwd_adam
    g = torch.Generator().manual_seed(9)
    n, N = 5, 1000
    nb = (N + 255) // 256
    emb0 = (torch.randn(n, 9, generator=g) * 0.1).to(DEV)
    m0 = (torch.randn(n, 9, generator=g) * 0.01).to(DEV)
    v0 = (torch.rand(n, 9, generator=g) * 1e-4).to(DEV)
    ws = torch.randn(nb * 16, generator=g).to(DEV)
    vm = torch.linalg.inv(rigid((1,), g)).float().contiguous().to(DEV)
    cam = torch.tensor([3], device=DEV)
    lr, wd, step = 2e-3, 1e-6, 4

    def run(**kw):
        e, m, v = emb0.clone(), m0.clone(), v0.clone()
        pose_bwd_adam(ws, N, vm, cam, e, m, v, lr, wd, step, **kw)
        torch.cuda.synchronize()
        return e, m, v

    host = run()
    assert not torch.equal(host[0], emb0)
    for a, b in zip(host, run()):  # the ordered reduction: identical between calls
        assert torch.equal(a, b)
    void = run(skip=torch.ones(1, dtype=torch.int32, device=DEV))
    for a, b in zip(void, (emb0, m0, v0)):
        assert torch.equal(a, b)
    live = run(skip=torch.zeros(1, dtype=torch.int32, device=DEV))
    hyper = torch.tensor(adam_factors([lr], BETAS, step)[0], device=DEV)
    dev = run(hyper=hyper)
    for a, b, c in zip(host, live, dev):  # the captured step's factors: the same update
        assert torch.equal(a, b) and torch.equal(a, c)
