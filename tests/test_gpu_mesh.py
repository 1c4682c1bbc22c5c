"""GPU: mesh export -- TSDFVolume.integrate / extract_mesh (csrc/tsdf.hip)
against the float64 oracle of mesh_cases.py, and Trainer.extract_mesh.

Integrate bar: bar = max |oracle in float32 - oracle in float64| over the
voxels none of whose (voxel, camera) pairs may flip in float32 (mesh_cases
NEAR_PIX / NEAR_CUT); the kernel is within max(4 bar, 1e-6) there (the factor 4
covers fma contraction and operation order, as in test_gpu_covar.py), and its
weight is exact there and within 1 elsewhere.
Extract bar: faces exactly equal, in order; positions within
8 * 2^-24 * (voxel_size + max |coordinate|): on a sign-changing edge va and vb
have opposite signs, so t = va / (va - vb) has no cancellation and lies in
[0, 1]; colours within 8 * 2^-24 * max |colour|.
Shapes: x no multiple of 4 or 64, several workgroups, a dimension of 1, a
single cell, and one volume of 2^31 + 2^21 grid points for the 64-bit indices."""

import math

import numpy as np
import pytest
import torch

import mesh_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


@pytest.fixture(scope="module")
def table():
    from gsplat_hip.mesh import mc_table
    return mc_table()


@pytest.fixture(scope="module")
def scene():
    sc = M.IntegrateScene()
    out = {"scene": sc}
    for name, views in (("one", [sc.first]), ("two", [sc.first, sc.second])):
        s64, _, near = sc.oracle(views, np.float64)
        s32, _, _ = sc.oracle(views, np.float32)
        out[name] = (s64, s32, near.any(0))
    return out


def _dev(v):
    return {k: torch.from_numpy(a).to(DEV) for k, a in v.items()}


def _integrate(vol, sc, v, colors=True, cams=None):
    t = _dev(v)
    sl = slice(None) if cams is None else cams
    vol.integrate(t["depths"][sl], t["viewmats"][sl], t["Ks"][sl],
                  colors=t["colors"][sl] if colors else None, alphas=t["alphas"][sl],
                  depth_trunc=sc.depth_trunc, alpha_min=sc.alpha_min)
    return vol


def _volume(sc, colors=True):
    from gsplat_hip import TSDFVolume
    return TSDFVolume(sc.origin, sc.h, sc.dims, sdf_trunc=sc.sdf_trunc, device=DEV, colors=colors)


def _check_state(vol, s64, s32, excluded, what):
    ok = ~excluded
    w = vol.weight.cpu().numpy().ravel().astype(np.float64)
    dw = np.abs(w - s64["weight"])
    assert dw[ok].max() == 0.0, what
    assert dw.max() <= 1.0, what
    got = {"tsdf": vol.tsdf.cpu().numpy().ravel()[None],
           "color": vol.color.cpu().numpy().reshape(3, -1)}
    for k in ("tsdf", "color"):
        ref64, ref32 = np.atleast_2d(s64[k]), np.atleast_2d(s32[k])
        bar = float(np.abs(ref32.astype(np.float64) - ref64)[:, ok].max())
        err = float(np.abs(got[k].astype(np.float64) - ref64)[:, ok].max())
        print(f"{what} {k}: err {err:.3e}, float32 oracle bar {bar:.3e}, bound "
              f"{max(4 * bar, 1e-6):.3e}; {int(excluded.sum())} of {excluded.size} voxels excluded, "
              f"{int((dw > 0).sum())} weights differ")
        assert err <= max(4.0 * bar, 1e-6), (what, k, err, bar)


def test_integrate_matches_the_oracle(scene):
    sc = scene["scene"]
    vol = _integrate(_volume(sc), sc, sc.first)
    s64, s32, excluded = scene["one"]
    assert tuple(vol.tsdf.shape) == sc.dims[::-1] and tuple(vol.color.shape) == (3,) + sc.dims[::-1]
    assert 0.05 < (s64["weight"] > 0).mean() < 1.0 and s64["weight"].max() == 2.0
    _check_state(vol, s64, s32, excluded, "three cameras")


def test_batching_changes_no_bits(scene):
    sc = scene["scene"]
    a = _integrate(_volume(sc), sc, sc.first)
    b = _volume(sc)
    for c in range(3):
        _integrate(b, sc, sc.first, cams=slice(c, c + 1))
    again = _integrate(_volume(sc), sc, sc.first)
    assert torch.equal(a._state, b._state) and torch.equal(a._state, again._state)
    assert float(a.weight.sum()) > 0
    # a second integrate on top of the first: the oracle's six-camera sequence
    _integrate(a, sc, sc.second)
    s64, s32, excluded = scene["two"]
    assert s64["weight"].max() >= 4.0
    _check_state(a, s64, s32, excluded, "six cameras")
    # a volume without colours fuses the same tsdf and weight
    c = _integrate(_integrate(_volume(sc, colors=False), sc, sc.first, colors=False), sc,
                   sc.second, colors=False)
    assert c.color is None and tuple(c._state.shape[:1]) == (2,)
    assert torch.equal(c.tsdf, a.tsdf) and torch.equal(c.weight, a.weight)
    a.reset()
    assert float(a._state.abs().sum()) == 0.0


def _set_volume(tsdf, weight, color, origin, h):
    from gsplat_hip import TSDFVolume
    nz, ny, nx = tsdf.shape
    vol = TSDFVolume(origin, h, (nx, ny, nz), device=DEV, colors=color is not None)
    vol.tsdf.copy_(torch.from_numpy(np.ascontiguousarray(tsdf)))
    vol.weight.copy_(torch.from_numpy(np.ascontiguousarray(weight)))
    if color is not None:
        vol.color.copy_(torch.from_numpy(np.ascontiguousarray(color)))
    return vol


def _check_mesh(mesh, ref, h, what):
    v, f, c = mesh
    V, F, C = ref[:3]
    assert v.dtype == torch.float32 and f.dtype in (torch.int32, torch.int64)
    assert tuple(v.shape) == (len(V), 3) and tuple(f.shape) == (len(F), 3), what
    assert np.array_equal(f.cpu().numpy().astype(np.int64), F), what
    if len(V) == 0:
        return
    bound = 8 * EPS * (float(np.float32(h)) + np.abs(V).max())
    err = np.abs(v.cpu().numpy().astype(np.float64) - V).max()
    print(f"{what}: {len(V)} vertices, {len(F)} faces, position err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (what, err, bound)
    assert set(F.ravel().tolist()) == set(range(len(V))), what  # no unreferenced vertex
    if C is None:
        assert c is None
    else:
        cerr = np.abs(c.cpu().numpy().astype(np.float64) - C).max()
        cb = 8 * EPS * np.abs(C).max()
        print(f"{what}: colour err {cerr:.3e} (bound {cb:.3e})")
        assert cerr <= cb, (what, cerr, cb)


def test_extract_matches_the_oracle(table):
    tsdf, color, weight = M.random_field()
    assert 0.05 < (weight == 0).mean() < 0.15
    origin, h = (0.3, -1.2, 2.0), 0.07
    vol = _set_volume(tsdf, weight, color, origin, h)
    ref = M.extract_oracle(table, tsdf, weight, origin, h, color=color)
    full = M.extract_oracle(table, tsdf, np.ones_like(weight), origin, h)
    assert 0 < len(ref[1]) < len(full[1])  # the zero weights cut cells out
    mesh = vol.extract_mesh()
    _check_mesh(mesh, ref, h, "random field")
    again = vol.extract_mesh()
    for a, b in zip(mesh, again):
        assert torch.equal(a, b)
    # min_weight: cells with a corner weight <= 1 drop out as well
    ref1 = M.extract_oracle(table, tsdf, weight, origin, h, color=color, min_weight=1.0)
    assert 0 < len(ref1[1]) < len(ref[1])
    _check_mesh(vol.extract_mesh(min_weight=1.0), ref1, h, "min_weight=1")


def test_gpu_mesh_is_manifold(table):
    tsdf, _, weight = M.random_field()
    ones = np.ones_like(weight)
    vol = _set_volume(tsdf, ones, None, (0.0, 0.0, 0.0), 1.0)
    v, f, c = vol.extract_mesh()
    _, F, _, owners, cases = M.extract_oracle(table, tsdf, ones, (0, 0, 0), 1.0)
    assert c is None and len(set(cases.tolist())) == 256
    f = f.cpu().numpy().astype(np.int64)
    assert v.shape[0] == len(owners) and f.shape == F.shape
    repeated, bad = M.half_edges(f, owners, (21, 21, 21))
    assert repeated == 0 and bad == 0, (repeated, bad)


def test_sphere():
    tsdf, origin, h, r, centre = M.sphere_field()
    vol = _set_volume(tsdf, np.ones_like(tsdf), None, origin, h)
    v, f, _ = vol.extract_mesh()
    v, f = v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64)
    he = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = he[:, 0] * len(v) + he[:, 1]
    assert len(np.unique(key)) == len(key)  # every directed half-edge once
    assert np.isin(he[:, 1] * len(v) + he[:, 0], key).all()  # ... with its opposite: closed
    E = len(he) // 2
    assert len(v) - E + len(f) == 2, (len(v), E, len(f))
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    volume = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
    exact = 4.0 / 3.0 * math.pi * r ** 3
    dist = np.abs(np.linalg.norm(v - centre, axis=1) - r).max()
    bound = h * h / (8.0 * (r - 2.0 * h)) + 8 * EPS * (h + np.abs(v).max())
    print(f"sphere: {len(v)} vertices, {len(f)} faces, volume {volume:.5f} (exact {exact:.5f}), "
          f"max distance {dist:.3e} (bound {bound:.3e})")
    assert volume > 0.0 and abs(volume - exact) < 0.05 * exact
    assert dist <= bound, (dist, bound)


def test_edge_shapes(table, scene):
    from gsplat_hip import TSDFVolume
    sc = scene["scene"]
    for colors in (True, False):
        v, f, c = TSDFVolume((0, 0, 0), 0.1, (9, 7, 5), device=DEV, colors=colors).extract_mesh()
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
        assert (c is None) if not colors else tuple(c.shape) == (0, 3)
    rng = np.random.default_rng(5)
    for dims in ((9, 1, 5), (1, 6, 7), (8, 5, 1), (1, 1, 1)):  # a dimension of 1: no cells
        t = M.f32(rng.standard_normal(dims[::-1]))
        v, f, _ = _set_volume(t, np.ones_like(t), None, (0, 0, 0), 0.1).extract_mesh()
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3), dims
    for dims in ((17, 9, 5), (2, 2, 2), (300, 2, 3)):
        t = M.f32(rng.standard_normal(dims[::-1]))
        col = M.f32(rng.random((3,) + dims[::-1]))
        w = np.ones_like(t)
        origin, h = (-0.4, 0.2, 0.1), 0.03
        ref = M.extract_oracle(table, t, w, origin, h, color=col)
        _check_mesh(_set_volume(t, w, col, origin, h).extract_mesh(), ref, h, f"dims {dims}")
    # colors=False: the geometry of the colour volume, no colours
    a = _integrate(_volume(sc), sc, sc.first).extract_mesh()
    b = _integrate(_volume(sc, colors=False), sc, sc.first, colors=False).extract_mesh()
    assert b[2] is None and a[0].shape[0] > 0 and a[2].shape == a[0].shape
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_linear_indices_past_2_31(table):
    """2048 x 1024 x 1025 grid points: the top layer's linear indices lie past
    2^31 (and every byte offset of the upper half past 2^33).  h = 2^-10 and
    the origin 0 make every coordinate exact in float32, so the oracle on a
    crop of the volume (its origin shifted) sees the kernel's numbers: the
    bars are those of the small tests.  Extraction and integration are local,
    so the crop's mesh is the volume's, indices included."""
    from gsplat_hip import TSDFVolume
    dims, h = (2048, 1024, 1025), 2.0 ** -10
    assert dims[0] * dims[1] * (dims[2] - 1) == 1 << 31
    vol = TSDFVolume((0.0, 0.0, 0.0), h, dims, sdf_trunc=4 * h, device=DEV, colors=False)
    # integrate: a small camera above the top layer, looking down at a constant depth
    I0, J0 = 1500, 700
    eye = (I0 * h + 0.0004, J0 * h + 0.0003, 1.0 + 0.05)
    V = M.f32(M.look_at(eye, (eye[0], eye[1], 0.0), up=(0, 1, 0)))[None]
    K = M.f32(M.intrinsics(40.0, 16, 12))[None]
    depth = np.full((1, 12, 16), 0.0522, np.float32)
    depth[0, 3, 5] = 0.0  # a hole
    vol.integrate(*(torch.from_numpy(a).to(DEV) for a in (depth, V, K)))
    ci, cj, ck = (I0 - 40, I0 + 40), (J0 - 40, J0 + 40), (985, 1025)
    cdims = (ci[1] - ci[0], cj[1] - cj[0], ck[1] - ck[0])
    corigin = (ci[0] * h, cj[0] * h, ck[0] * h)
    out = {}
    for dt in (np.float64, np.float32):
        st = M.empty_state(cdims, False, dt)
        _, near = M.integrate_oracle(st, corigin, h, cdims, depth, V, K, sdf_trunc=4 * h, dtype=dt)
        out[dt] = st
    s64, s32, ok = out[np.float64], out[np.float32], ~near[0]
    sl = (slice(*ck), slice(*cj), slice(*ci))
    w = vol.weight[sl].cpu().numpy().ravel().astype(np.float64)
    t = vol.tsdf[sl].cpu().numpy().ravel().astype(np.float64)
    top = s64["weight"].reshape(cdims[::-1])[-1]
    assert top.sum() >= 100 and s64["weight"].reshape(cdims[::-1])[:5].sum() == 0
    assert np.abs(w - s64["weight"])[ok].max() == 0 and np.abs(w - s64["weight"]).max() <= 1
    bar = np.abs(s32["tsdf"].astype(np.float64) - s64["tsdf"])[ok].max()
    err = np.abs(t - s64["tsdf"])[ok].max()
    print(f"2^31: {int(s64['weight'].sum())} voxels fused, {int(top.sum())} of them past 2^31; "
          f"tsdf err {err:.3e}, float32 oracle bar {bar:.3e}")
    assert err <= max(4 * bar, 1e-6)
    assert float(vol.weight.sum()) == w.sum()  # nothing fused outside the crop
    # extract: a random field in a crop that reaches the top layer, weight 0 elsewhere
    vol.reset()
    rng = np.random.default_rng(11)
    ci, cj, ck = (1800, 1812), (900, 909), (1021, 1025)
    field = M.f32(rng.standard_normal((ck[1] - ck[0], cj[1] - cj[0], ci[1] - ci[0])))
    sl = (slice(*ck), slice(*cj), slice(*ci))
    vol.tsdf[sl] = torch.from_numpy(field).to(DEV)
    vol.weight[sl] = 1.0
    ref = M.extract_oracle(table, field, np.ones_like(field), (ci[0] * h, cj[0] * h, ck[0] * h), h)
    assert len(ref[1]) > 100
    _check_mesh(vol.extract_mesh(), ref, h, "crop past 2^31")


# ------------------------------------------------------------------ Trainer
PLANE_H = 0.08  # the voxel size of the trainer test


def _plane_trainer(model, graph=False):
    """Surfels (or flat Gaussians) tiling the square [-1, 1]^2 of the plane
    z = 0 every 0.05, and six 64 x 48 cameras (f = 60) 3 away, 20 degrees off
    the normal.  Half a pixel's footprint (0.5 * 3.2 / 60 = 0.027 at the far
    rim) times the steepest depth slope (tan 35 deg = 0.7 at the image corner)
    is 0.019 < PLANE_H / 4."""
    from gsplat_hip.train_step import Trainer
    g = torch.arange(-20, 21, dtype=torch.float32) * 0.05
    x, y = torch.meshgrid(g, g, indexing="ij")
    means = torch.stack([x.reshape(-1), y.reshape(-1), torch.zeros(x.numel())], -1)
    rgbs = torch.stack([0.5 + 0.4 * torch.sin(3 * means[:, 0]), 0.5 + 0.4 * torch.cos(2 * means[:, 1]),
                        torch.full((len(means),), 0.3)], -1)
    th = math.radians(20.0)
    vms = [M.look_at((3 * math.sin(th) * math.cos(p), 3 * math.sin(th) * math.sin(p),
                      3 * math.cos(th)), (0, 0, 0), up=(0, 1, 0))
           for p in (math.radians(60.0 * k + 10.0) for k in range(6))]
    W, H = 64, 48
    vm = torch.from_numpy(np.stack(vms)).float()
    K = torch.from_numpy(M.intrinsics(60.0, W, H)).float()[None].repeat(6, 1, 1)
    tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, model=model, graph=graph, max_steps=100)
    n = len(means)
    thin = 0.05 if model == "2dgs" else 0.005
    with torch.no_grad():
        tr.params["scales"].copy_(torch.log(torch.tensor([0.05, 0.05, thin])).repeat(n, 1))
        tr.params["quats"].copy_(torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(n, 1))
        tr.params["opacities"].fill_(float(torch.logit(torch.tensor(0.95))))
    return tr


def _plane_check(mesh, what):
    v, f, c = mesh
    assert v.shape[0] > 0 and f.shape[0] > 0 and c.shape == v.shape
    v = v.cpu().numpy().astype(np.float64)
    inner = (np.abs(v[:, :2]) <= 1.0 - 2 * PLANE_H).all(1)
    assert inner.sum() >= 200, inner.sum()
    dist = np.abs(v[inner, 2]).max()
    print(f"{what}: {len(v)} vertices, {int(inner.sum())} inside the rim, max distance to the "
          f"plane {dist:.4f} (h = {PLANE_H})")
    assert dist <= PLANE_H, dist
    # the inner vertices span the square: no hole the size of the plane
    assert v[inner, 0].min() < -0.7 and v[inner, 0].max() > 0.7
    assert v[inner, 1].min() < -0.7 and v[inner, 1].max() > 0.7


def test_trainer_extract_mesh_2dgs(tmp_path):
    from test_mesh_host import parse_mesh_ply
    tr = _plane_trainer("2dgs", graph=True)
    assert tr._graph is not None, tr.graph_fallback
    path = str(tmp_path / "plane.ply")
    mesh = tr.extract_mesh(voxel_size=PLANE_H, path=path)
    _plane_check(mesh, "2dgs median")
    pv, pc, pf = parse_mesh_ply(path)
    assert np.array_equal(pv, mesh[0].cpu().numpy()) and np.array_equal(pf, mesh[1].cpu().numpy())
    assert pc is not None and pc.shape == pv.shape
    _plane_check(tr.extract_mesh(voxel_size=PLANE_H, depth_mode="expected", camera_batch=4,
                                 cameras=[0, 2, 3, 5]), "2dgs expected, 4 cameras")
    # with the step captured: parameters, moments and the graph are left alone
    tr.step(0)
    tr.sync()
    g = tr._graph
    assert g is not None and tr.graph_fallback is None, tr.graph_fallback
    params = {k: p.detach().clone() for k, p in tr.params.items()}
    ptrs = {k: p.data_ptr() for k, p in tr.params.items()}
    moms = {k: [m.clone() for m in mv] for k, mv in tr.moments().items()}
    replays, recaptures, steps = g.replays, g.recaptures, tr.opt.step_count
    geo = tr.extract_mesh(voxel_size=PLANE_H, colors=False)
    assert geo[2] is None and geo[0].shape[0] > 0
    tr.sync()
    assert tr._graph is g and (g.replays, g.recaptures) == (replays, recaptures)
    assert tr.opt.step_count == steps
    for k, p in tr.params.items():
        assert p.data_ptr() == ptrs[k] and torch.equal(p.detach(), params[k]), k
    now = tr.moments()
    for k in moms:
        assert all(torch.equal(a, b) for a, b in zip(now[k], moms[k])), k
    loss = float(tr.step(1).detach())
    tr.sync()
    assert np.isfinite(loss) and tr._graph is g and g.replays > replays, tr.graph_fallback
    tr.release_graph()


def test_trainer_extract_mesh_3dgs(tmp_path):
    from test_mesh_host import parse_mesh_ply
    tr = _plane_trainer("3dgs")
    with pytest.raises(ValueError, match="expected depth only"):
        tr.extract_mesh(voxel_size=PLANE_H)
    with pytest.raises(ValueError, match="max_voxels"):
        tr.extract_mesh(voxel_size=PLANE_H, depth_mode="expected", max_voxels=1000)
    path = str(tmp_path / "plane3.ply")
    v, f, c = tr.extract_mesh(resolution=40, depth_mode="expected", path=path)
    assert v.shape[0] > 0 and f.shape[0] > 0 and c.shape == v.shape
    pv, pc, pf = parse_mesh_ply(path)
    assert len(pv) == v.shape[0] and len(pf) == f.shape[0]
    inner = (v[:, :2].abs() <= 0.8).all(1)
    print(f"3dgs expected: {v.shape[0]} vertices, max distance to the plane inside the rim "
          f"{float(v[inner, 2].abs().max()):.4f}")
