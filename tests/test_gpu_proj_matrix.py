"""GPU: every instantiation and entry point of the quat / scale EWA projection
(csrc/projection.hip, csrc/proj_math.h) against the float64 oracle of
tests/proj_cases.py.

Cases (N 1 / 255 / 257 / 600, cameras 1 / 3; depth bands, a non-orthonormal
view, unnormalised quaternions, isotropic and anisotropic Gaussians, clamped
ones, each cull test alone, all culled, a dead wave, the packed tail, and
the at-the-gate cases) and the oracle: proj_cases.py.  Radii, validity, nnz
and ids are compared exactly; every other output is bounded by max(FACTOR x
bar, FLOOR) relative to the largest |oracle value|, bar being the larger
float32 error of two float32 evaluations of the same case (tests/golden/
proj_matrix.npz); tests/test_proj_cases_host.py shows on the CPU that plain
float32 arithmetic meets it.

  a  projection_fwd_kernel<0> (fully_fused_projection), compensations off / on
  b  projection_fwd_kernel<1> (count), packed_scan_kernel, projection_fwd_
     kernel<2> (write): packed=True
  c  projection_bwd_kernel<false>, dense: store mode (C = 1) and atomic mode
     (C = 3); with / without v_viewmats, v_depths, compensations
  d  projection_bwd_kernel<false>, packed: dense gradients and sparse_grad COO
  e  projection_bwd_kernel<true>: the geometry Adam in the backward
     (_wrapper.GeomAdamInBackward.run), lrs / step and hyper forms, skip
  f  projection_bwd_kernel<true, true>: the pose partials beside it
  g  the at-the-gate cases through a, b and c

The largest error of every output per group, with its bar and bound, is
printed as one JSON line when the module finishes (pytest -s shows it).
"""

import json
import math
import os
import types

import numpy as np
import pytest
import torch

import proj_cases as PC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERRORS = {}  # group -> output -> the entry with the largest err / bound
BARS = PC.load_bars(os.path.join(GOLDEN, "proj_matrix.npz"))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401  (fails loudly if the .so is missing)
    yield
    line = {g: {k: {f: float(f"{r[f]:.3g}") for f in ("err", "bar", "bound")} for k, r in o.items()}
            for g, o in ERRORS.items()}
    print("\nproj_matrix_errors " + json.dumps(line, sort_keys=True, separators=(",", ":")))
    for g, o in sorted(ERRORS.items()):
        k = max(o, key=lambda k: o[k]["ratio"])
        print(f"proj_matrix group {g}: largest err / bound {o[k]['ratio']:.3f} ({k}, {o[k]['case']})")


def T(x, grad=False):
    return torch.from_numpy(np.array(x)).to(DEV).requires_grad_(grad)  # the cases stay read-only


def npy(t):
    return t.detach().cpu().numpy()


def _gpu(fn):
    """fn() and a synchronize; a HIP error (a fault on the card) ends the
    session: no further kernel is launched on a card that has faulted."""
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"GPU fault, stopping: {e}", returncode=3)
        raise


def check(group, name, what, variant, pairs):
    """pairs: {output: (ours, oracle)} or {output: (ours, oracle, bar output)};
    the bar is that of "<name>:<variant>:<bar output>".  Prints and records
    every figure, then asserts each against max(FACTOR x bar, FLOOR)."""
    bad = []
    for k, pr in pairs.items():
        ours, ref = pr[0], pr[1]
        bar = BARS[f"{name}:{variant}:{pr[2] if len(pr) > 2 else k}"]
        assert ours.shape == ref.shape, (name, what, k, ours.shape, ref.shape)
        assert np.isfinite(ours).all(), (name, what, k)
        e, b = PC.rel_err(ours, ref), PC.bound(bar)
        print(f"{name} {what}: {k}: err {e:.3e}  bound {b:.3e}  (bar {bar:.3e})")
        rec = ERRORS.setdefault(group, {})
        if k not in rec or e / b > rec[k]["ratio"]:
            rec[k] = {"err": e, "bar": bar, "bound": b, "ratio": e / b, "case": f"{name} {what}"}
        if not e <= b:
            bad.append((k, e, b))
    assert not bad, (name, what, bad)


def _project(c, comps, packed=False, sparse=False, grad=(), vm_grad=False):
    import gsplat_hip
    ins = {k: T(getattr(c, k), k in grad) for k in ("means", "quats", "scales")}
    ins["viewmats"] = T(c.viewmats, vm_grad)
    out = gsplat_hip.fully_fused_projection(
        ins["means"], None, ins["quats"], ins["scales"], ins["viewmats"], T(c.Ks), c.W, c.H,
        eps2d=c.eps2d, near_plane=c.near, far_plane=c.far, radius_clip=c.radius_clip,
        packed=packed, sparse_grad=sparse, calc_compensations=comps)
    return ins, out


# ------------------------------------------------------------ a: dense forward
def _check_dense_forward(group, name):
    c, ref = PC.build(name), PC.fwd64(name)
    off = ~(ref["radii"] > 0)
    for comps in (False, True):
        _, out = _gpu(lambda: _project(c, comps))
        radii, means2d, depths, conics = (npy(t) for t in out[:4])
        assert radii.shape == (c.C, c.N) and radii.dtype == np.int32
        assert np.array_equal(radii, ref["radii"]), np.nonzero(radii != ref["radii"])
        got = {"means2d": means2d, "depths": depths, "conics": conics}
        if comps:
            got["comps"] = npy(out[4])
        else:
            assert out[4] is None
        check(group, name, "comps" if comps else "plain", "fwd", {k: (v, ref[k]) for k, v in got.items()})
        for k in ("means2d", "conics", "comps"):
            if k in got:
                assert not got[k][off].any(), k  # invalid entries: exact zeros


@pytest.mark.parametrize("name", PC.SEEDED_NAMES)
def test_dense_forward_vs_float64_oracle(name):
    _check_dense_forward("a", name)


# ----------------------------------------------------------- b: packed forward
def _check_packed_forward(group, name):
    c, ref = PC.build(name), PC.fwd64(name)
    ci, ni = np.nonzero(ref["radii"] > 0)  # (camera, Gaussian) order
    for comps in (False, True):
        _, out = _gpu(lambda: _project(c, comps, packed=True))
        cam, gau, radii = (npy(t) for t in out[:3])
        assert cam.shape == gau.shape == radii.shape == (len(ci),), (cam.shape, len(ci))  # nnz
        assert np.array_equal(cam, ci) and np.array_equal(gau, ni)
        assert np.array_equal(radii, ref["radii"][ci, ni])
        got = {"means2d": npy(out[3]), "depths": npy(out[4]), "conics": npy(out[5])}
        if comps:
            got["comps"] = npy(out[6])
        check(group, name, "packed" + (" comps" if comps else ""), "fwd",
              {k: (v, ref[k][ci, ni]) for k, v in got.items()})


@pytest.mark.parametrize("name", PC.SEEDED_NAMES)
def test_packed_forward_vs_float64_oracle(name):
    _check_packed_forward("b", name)


def test_packed_cases_include_the_tail_the_dead_wave_and_nnz_zero():
    pops = {PC.SPECS[n][0] for n in PC.SEEDED_NAMES}
    assert {"tail", "deadwave", "allculled"} <= pops
    assert not (PC.fwd64("allculled_n257_c3")["radii"] > 0).any()


# ---------------------------------------------------------- c: dense backward
def _loss(c, m2, depths, conics, comps, sel, use_depths):
    cot = lambda a: T(a)[sel] if sel is not None else T(a)  # noqa: E731
    loss = (m2 * cot(c.v_means2d)).sum() + (conics * cot(c.v_conics)).sum()
    if use_depths:
        loss = loss + (depths * cot(c.v_depths)).sum()
    if comps is not None:
        loss = loss + (comps * cot(c.v_comps)).sum()
    return loss


def _check_dense_backward(group, name):
    c, fwd = PC.build(name), PC.fwd64(name)
    unseen = ~(fwd["radii"] > 0).any(0)
    for comps, use_depths in PC.BWD_VARIANTS:
        ref = PC.bwd64(name, comps, use_depths)
        for want_vm in (True, False):
            def run():
                ins, out = _project(c, comps, grad=("means", "quats", "scales"), vm_grad=want_vm)
                assert np.array_equal(npy(out[0]), fwd["radii"])
                loss = _loss(c, out[1], out[2], out[3], out[4], None, use_depths)
                leaves = [ins[k] for k in ("means", "quats", "scales")] + ([ins["viewmats"]] if want_vm else [])
                return torch.autograd.grad(loss, leaves)
            gr = _gpu(run)
            got = dict(zip(PC.BWD_OUT, (npy(g) for g in gr)))
            what = PC.bwd_key(comps, use_depths) + ("" if want_vm else " no-v_viewmats")
            check(group, name, what, PC.bwd_key(comps, use_depths), {k: (v, ref[k]) for k, v in got.items()})
            for k in ("v_means", "v_quats", "v_scales"):
                assert not got[k][unseen].any(), k  # valid in no camera: exact zeros
            if want_vm:
                assert not got["v_viewmats"][:, 3].any()


@pytest.mark.parametrize("name", PC.SEEDED_NAMES)
def test_dense_backward_vs_float64_oracle(name):
    """C = 1: store mode; C = 3: atomic mode."""
    _check_dense_backward("c", name)


# --------------------------------------------------------- d: packed backward
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("name", PC.SEEDED_NAMES)
def test_packed_backward_vs_float64_oracle(name, sparse):
    c, fwd = PC.build(name), PC.fwd64(name)
    ci, ni = np.nonzero(fwd["radii"] > 0)
    sel = (torch.from_numpy(ci).to(DEV), torch.from_numpy(ni).to(DEV))
    unseen = ~(fwd["radii"] > 0).any(0)
    for comps, use_depths in PC.BWD_VARIANTS[:3]:
        ref = PC.bwd64(name, comps, use_depths)

        def run():
            ins, out = _project(c, comps, packed=True, sparse=sparse,
                                grad=("means", "quats", "scales"), vm_grad=True)
            assert np.array_equal(npy(out[0]), ci) and np.array_equal(npy(out[1]), ni)
            loss = _loss(c, out[3], out[4], out[5], out[6], sel, use_depths)
            return torch.autograd.grad(loss, [ins[k] for k in ("means", "quats", "scales", "viewmats")])
        gr = _gpu(run)
        what = ("sparse " if sparse else "packed ") + PC.bwd_key(comps, use_depths)
        key = PC.bwd_key(comps, use_depths)
        if sparse:
            got = {}
            for k, g, like in zip(PC.BWD_OUT[:3], gr[:3], (c.means, c.quats, c.scales)):
                assert g.is_sparse and tuple(g.shape) == like.shape
                assert np.array_equal(npy(g._indices()), ni[None])  # gaussian_ids, per pair
                got["pp_" + k] = npy(g._values())
            check("d", name, what, key, {k: (v, ref[k]) for k, v in got.items()})
        else:
            got = dict(zip(PC.BWD_OUT[:3], (npy(g) for g in gr[:3])))
            check("d", name, what, key, {k: (v, ref[k]) for k, v in got.items()})
            for v in got.values():
                assert not v[unseen].any()
        check("d", name, what, key, {"v_viewmats": (npy(gr[3]), ref["v_viewmats"])})


# ------------------------------------------------------- e, f: geometry Adam
def _hyper(step):
    """f32[8]: (lr_i / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) per group."""
    b1, b2 = PC.ADAM["betas"]
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return [x for lr in PC.ADAM["lrs"] for x in (lr / bc1, 1 / math.sqrt(bc2))]


_FWD = {}  # case -> (radii, conics) of the GPU's dense forward, shared read-only


def _gpu_forward(name):
    if name not in _FWD:
        c = PC.build(name)
        _, out = _gpu(lambda: _project(c, False))
        assert np.array_equal(npy(out[0]), PC.fwd64(name)["radii"])
        _FWD[name] = (out[0], out[3].contiguous())
    return _FWD[name]


def _run_adam(name, step, zero_moments=False, dirs=True, opac=True, hyper=False, skip=None,
              pose=False):
    """One launch on fresh copies of the parameters and moments; returns
    (params, exp_avgs, exp_avg_sqs) as numpy lists and the pose rows."""
    from gsplat_hip import _wrapper
    from gsplat_hip.pose import pose_workspace
    c = PC.build(name)
    N = c.N
    radii, conics = _gpu_forward(name)
    p = [T(getattr(c, k)) for k in PC.GROUPS]
    m = [torch.zeros_like(t) if zero_moments else T(a) for t, a in zip(p, c.m_init)]
    v = [torch.zeros_like(t) if zero_moments else T(a) for t, a in zip(p, c.v_init)]
    # every buffer the entry point reads or writes, sized from the case
    widths = ((N, 3), (N, 3), (N, 4), (N,))
    for group in (p, m, v):
        assert [tuple(t.shape) for t in group] == list(widths)
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in group)
    scales, vm, Ks = T(c.scales), T(c.viewmats), T(c.Ks)
    vm2, vdep, vcon = T(c.v_means2d), T(c.v_depths), T(c.v_conics)
    fusion = types.SimpleNamespace(v_dirs=T(c.v_dirs) if dirs else None,
                                   v_opac_in=T(c.v_opac)[None] if opac else None, opac_act=T(c.opac))
    assert tuple(scales.shape) == (N, 3) and tuple(vm.shape) == (1, 4, 4) and tuple(Ks.shape) == (1, 3, 3)
    assert tuple(radii.shape) == (1, N) and radii.dtype == torch.int32
    assert tuple(conics.shape) == (1, N, 3) and tuple(vm2.shape) == (1, N, 2)
    assert tuple(vdep.shape) == (1, N) and tuple(vcon.shape) == (1, N, 3)
    assert tuple(fusion.opac_act.shape) == (N,)
    assert fusion.v_dirs is None or tuple(fusion.v_dirs.shape) == (N, 3)
    assert fusion.v_opac_in is None or tuple(fusion.v_opac_in.shape) == (1, N)
    hy = torch.tensor(_hyper(step), dtype=torch.float32, device=DEV) if hyper else None
    sk = None if skip is None else torch.tensor([skip], dtype=torch.int32, device=DEV)
    assert hy is None or tuple(hy.shape) == (8,)
    ga = _wrapper.GeomAdamInBackward(p, m, v, list(PC.ADAM["lrs"]), PC.ADAM["betas"], PC.ADAM["eps"],
                                     step, hyper=hy, skip=sk)
    nb = (N + 255) // 256
    ws = None
    if pose:
        ws = pose_workspace(N, DEV)
        assert ws.dtype == torch.float32 and ws.numel() >= 16 * nb
        ws.fill_(float("nan"))  # every row must be written
        ga.pose_ws = ws
    _gpu(lambda: ga.run(p[0], p[2], scales, vm, Ks, c.W, c.H, c.eps2d, radii, conics, vm2, vdep, vcon,
                        fusion))
    rows = None if ws is None else npy(ws[:16 * nb].view(nb, 16))
    return [npy(t) for t in p], [npy(t) for t in m], [npy(t) for t in v], rows


_STEP3 = {}  # case -> the step-3 update of the (v_dirs, v_opac, lrs / step) form, for group f


def _step3(name):
    if name not in _STEP3:
        _STEP3[name] = _run_adam(name, PC.ADAM["step"])[:3]
    return _STEP3[name]


def _named(prefix, arrays):
    return {f"{prefix}_{k}": a for k, a in zip(PC.GROUPS, arrays)}


@pytest.mark.parametrize("name", PC.ADAM_NAMES)
def test_adam_in_backward_gradients_vs_float64_oracle(name):
    """Step 1 from zero moments: exp_avg = 0.1 x gradient, every one of the
    eleven gradients (the exp and sigmoid chain rules included) at the
    gradients' bars; with and without v_dirs and v_opac."""
    culled = ~(PC.fwd64(name)["radii"][0] > 0)
    for dirs, opac in PC.ADAM_VARIANTS:
        ref = PC.adam64(name, dirs, opac)
        _, m1, _, _ = _run_adam(name, 1, zero_moments=True, dirs=dirs, opac=opac)
        key = PC.adam_key(dirs, opac)
        check("e", name, key + " step 1", key,
              {"m1_" + k: (a, ref["m1_" + k], "g_" + k) for k, a in zip(PC.GROUPS, m1)})
        for a in m1:
            assert not a[culled].any()  # culled Gaussians: a zero gradient
        if not opac:
            assert not m1[3].any()


@pytest.mark.parametrize("form", ["lrs", "hyper"])
@pytest.mark.parametrize("name", PC.ADAM_NAMES)
def test_adam_in_backward_update_vs_float64_oracle(name, form):
    """One update at step 3 from seeded moments: the parameters and exp_avg
    against torch.optim.Adam's update in float64 at betas (0.9, 0.999);
    exp_avg_sq against the same oracle at the betas the entry point receives,
    float32(0.9) and float32(0.999) (its ABI type is float; diagnosed in
    tests/test_gpu_sh_matrix.py, whose kernels share adam_update).  Culled
    Gaussians have a zero gradient and only decay: the oracle's dense Adam."""
    c = PC.build(name)
    variants = PC.ADAM_VARIANTS if form == "lrs" else PC.ADAM_VARIANTS[:1]
    for dirs, opac in variants:
        ref, ref32 = PC.adam64(name, dirs, opac), PC.adam64(name, dirs, opac, True)
        if form == "lrs" and dirs and opac:
            p, m, v = _step3(name)
        else:
            p, m, v, _ = _run_adam(name, PC.ADAM["step"], dirs=dirs, opac=opac, hyper=form == "hyper")
        key = PC.adam_key(dirs, opac)
        what = f"{key} {form} step 3"
        check("e", name, what, key, {k: (a, ref[k]) for k, a in {**_named("p", p), **_named("m", m)}.items()})
        check("e", name, what, key, {k: (a, ref32[k]) for k, a in _named("v", v).items()})
        moved = [not np.array_equal(a, getattr(c, k)) for a, k in zip(p, PC.GROUPS)]
        assert all(moved)  # from non-zero moments every row moves, the culled ones too


@pytest.mark.parametrize("name", ["z3_n255_c1", "tail_n257_c1", "allculled_n1_c1"])
def test_adam_in_backward_skip_leaves_every_row_bit_unchanged(name):
    c = PC.build(name)
    p, m, v, rows = _run_adam(name, PC.ADAM["step"], hyper=True, skip=1)
    for a, k in zip(p, PC.GROUPS):
        assert np.array_equal(a, getattr(c, k)), k
    for got, init in ((m, c.m_init), (v, c.v_init)):
        for a, b in zip(got, init):
            assert np.array_equal(a, b)
    # the flag cleared: the update of the hyper form
    p0, m0, v0, _ = _run_adam(name, PC.ADAM["step"], hyper=True, skip=0)
    p1, m1, v1, _ = _run_adam(name, PC.ADAM["step"], hyper=True)
    for a, b in zip(p0 + m0 + v0, p1 + m1 + v1):
        assert np.array_equal(a, b)
    assert not np.array_equal(p0[0], c.means)


@pytest.mark.parametrize("name", PC.ADAM_NAMES)
def test_pose_partials_vs_float64_oracle(name):
    """projection_bwd_kernel<true, true>: the per-block rows of the pose
    workspace summed in float64 against the oracle's v_viewmats[0, :3, :] at
    that output's measured bar (pose_partials is a second hand-written
    derivation: the clamped and non-orthonormal cases are among these); the
    sum of v_dirs over the visible Gaussians; column 15 zero and every row
    written; the update bit-equal to projection_bwd_kernel<true>'s."""
    c = PC.build(name)
    p, m, v, rows = _run_adam(name, PC.ADAM["step"], pose=True)
    nb = (c.N + 255) // 256
    assert rows.shape == (nb, 16) and np.isfinite(rows).all() and not rows[:, 15].any()
    for a, b in zip(p + m + v, sum(_step3(name), [])):
        assert np.array_equal(a, b)
    sums = rows.astype(np.float64).sum(0)
    ref = PC.bwd64(name)["v_viewmats"][0, :3, :]
    check("f", name, "pose", "bwd", {"v_viewmats": (sums[:12].reshape(3, 4), ref)})
    # any float32 summation order of n values is within (n - 1) 2^-24 sum |x|
    # of the exact sum (v_dirs rows of culled Gaussians are zero)
    vd = c.v_dirs.astype(np.float64)
    bound = (c.N - 1) * 2.0 ** -24 * np.abs(vd).sum(0) + 1e-30
    errd = np.abs(sums[12:15] - vd.sum(0))
    print(f"{name}: sum v_dirs err {errd}, bound {bound}")
    assert (errd <= bound).all(), (errd, bound)
    if not (PC.fwd64(name)["radii"] > 0).any():
        assert not rows.any()


# ------------------------------------------------ g: the at-the-gate cases
@pytest.mark.parametrize("name", PC.GATE_NAMES)
def test_at_the_gate_cases(name):
    """z == near_plane exactly is culled, its nextafter kept; radius 3 is
    culled at radius_clip 3 and radius 4 kept; means2d +- radius 2e-5 beyond
    each image edge is culled, 2e-5 inside kept: through the dense forward,
    the packed forward and the dense backward."""
    want = {"gate_near": [False, True], "gate_clip": [False, True],
            "gate_frustum": [False] * 4 + [True] * 4}[name]
    assert ((PC.fwd64(name)["radii"][0] > 0) == np.array(want)).all()
    _check_dense_forward("g", name)
    _check_packed_forward("g", name)
    _check_dense_backward("g", name)
