"""GPU checks of the similarity transform of splat scenes (csrc/transform.hip
through gsplat_hip/transform.py) against the float64 fixtures of
tests/transform_cases.py."""

import os

import numpy as np
import pytest
import torch

import raster_cases
import transform_cases as TC
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MOVED = ("means", "quats", "scales", "shN")


def _views(res):
    return TC.views({k: res[k].cpu().numpy() for k in MOVED})


def _bits_equal(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in MOVED)


@pytest.mark.parametrize("name", TC.NAMES)
def test_fixture_cases(name):
    import gsplat_hip
    case, g = TC.make_case(name), load_golden(f"transform_{name}")
    splats, T, ids = TC.splats_of(case, torch, DEV)
    res = gsplat_hip.transform_splats(splats, T, segment_ids=ids)
    assert set(res) == set(splats)
    for k in ("sh0", "opacities"):
        assert res[k] is splats[k]
    got = _views(res)
    want = TC.views({k: g["out_" + k] for k in MOVED})
    for k in TC.OUTPUTS:
        err, lim = TC.rel_err(got[k], want[k]), TC.bound(g["bar_" + k])
        print(f"hip {name:20s} {k:9s} err {err:.2e}  bound {lim:.2e}")
        assert err <= lim, (name, k, err, lim)
    # two runs, in place, and the transforms given on the host: the same bits
    again = gsplat_hip.transform_splats(splats, T.cpu().numpy(), segment_ids=ids, validate=False)
    assert _bits_equal(res, again)
    mine = {k: v.clone() for k, v in splats.items()}
    same = gsplat_hip.transform_splats(mine, T, segment_ids=ids, inplace=True)
    assert all(same[k] is mine[k] for k in MOVED) and _bits_equal(res, same)
    if case.deg:   # the SH part alone, given A / s: against the oracle at the bar
        R = T[:, :3, :3].double()
        R = R / torch.linalg.det(R).pow(1 / 3)[:, None, None]
        sh = gsplat_hip.rotate_sh(splats["shN"], R, segment_ids=ids)
        err = TC.rel_err(sh.cpu().numpy().astype(np.float64), g["out_shN"])
        assert err <= TC.bound(g["bar_shN"]), (name, err)
        buf = splats["shN"].clone()   # the same call into its own input: the same bits
        assert gsplat_hip.rotate_sh(buf, R, segment_ids=ids, out=buf) is buf
        assert torch.equal(buf, sh)
    if case.S == 1:     # no ids and all-zero ids: the same bits
        zeros = torch.zeros(case.N, dtype=torch.int64, device=DEV)
        assert _bits_equal(res, gsplat_hip.transform_splats(splats, T, segment_ids=zeros))


def test_sh_rotation_matrices_on_the_device():
    import gsplat_hip
    g = load_golden("transform_checks")
    Ms = gsplat_hip.sh_rotation_matrices(torch.from_numpy(g["blocks_R"]).to(DEV), 4)
    for l, M in enumerate(Ms, start=1):
        assert M.shape == (1, 2 * l + 1, 2 * l + 1) and M.dtype == torch.float32
        err = TC.rel_err(M[0].cpu().numpy().astype(np.float64), g[f"blocks_M{l}"])
        print(f"M_{l} err {err:.2e}")
        assert err <= TC.bound(g[f"blocks_bar{l}"]), (l, err)
    with pytest.raises(ValueError, match="det"):
        gsplat_hip.sh_rotation_matrices(-torch.eye(3, device=DEV), 2)


def test_out_of_range_ids_and_refused_segments():
    import gsplat_hip
    case = TC.make_case("n257_d4_s3")
    splats, T, ids = TC.splats_of(case, torch, DEV)
    good = gsplat_hip.transform_splats(splats, T, segment_ids=ids)
    bad_rows = torch.tensor([0, 63, 64, 200, 256], device=DEV)
    bad_ids = ids.clone()
    bad_ids[bad_rows] = torch.tensor([-1, 3, 1 << 40, -(1 << 62), 3], device=DEV)
    with pytest.raises(ValueError, match="5 of 257"):
        gsplat_hip.transform_splats(splats, T, segment_ids=bad_ids)
    res = gsplat_hip.transform_splats(splats, T, segment_ids=bad_ids, validate=False)
    keep = torch.ones(case.N, dtype=torch.bool, device=DEV)
    keep[bad_rows] = False
    for k in MOVED:
        assert torch.equal(res[k][bad_rows], splats[k][bad_rows]), k
        assert torch.equal(res[k][keep], good[k][keep]), k
    # a refused segment (a shear in segment 2, given on the device so that only
    # the kernel sees it): its rows come back unchanged, the others move
    Tb = T.clone()
    Tb[2, 0, 1] += 0.01
    with pytest.raises(ValueError, match=r"segment 2.*max\|A\^T A"):
        gsplat_hip.transform_splats(splats, Tb, segment_ids=ids)
    res = gsplat_hip.transform_splats(splats, Tb, segment_ids=ids, validate=False)
    seg2 = ids == 2
    assert bool(seg2.any()) and bool((~seg2).any())
    for k in MOVED:
        assert torch.equal(res[k][seg2], splats[k][seg2]), k
        assert torch.equal(res[k][~seg2], good[k][~seg2]), k
    Tr = T.clone()
    Tr[0, :3, 0] *= -1
    with pytest.raises(ValueError, match="segment 0.*det"):
        gsplat_hip.transform_splats(splats, Tr, segment_ids=ids)
    # a NaN or an infinite entry is refused like any other matrix that is no similarity
    for bad in (float("nan"), float("inf")):
        Tn = T.clone()
        Tn[0, 1, 2] = bad
        with pytest.raises(ValueError, match="segment 0"):
            gsplat_hip.transform_splats(splats, Tn, segment_ids=ids)
        res = gsplat_hip.transform_splats(splats, Tn, segment_ids=ids, validate=False)
        seg0 = ids == 0
        for k in MOVED:
            assert torch.equal(res[k][seg0], splats[k][seg0]), k
            assert torch.equal(res[k][~seg0], good[k][~seg0]), k
    mixed = dict(splats, means=splats["means"].cpu())
    with pytest.raises(gsplat_hip._lib.GsplatHipError):
        gsplat_hip.transform_splats(mixed, T, segment_ids=ids)


def test_rotated_coefficients_through_the_sh_kernel():
    """spherical_harmonics(L, d, rotated coefficients) against
    spherical_harmonics(L, d R, coefficients), which evaluates at R^T d: both
    sides through the existing kernel, 4 x the float32 bar of that comparison."""
    import gsplat_hip
    L, n = 4, 1000
    rng = np.random.default_rng(TC.seed_of("sh_eval"))
    R = torch.from_numpy(TC.rotation("generic", rng).astype(np.float32)).to(DEV)
    dirs = torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32)).to(DEV)
    coeffs = torch.from_numpy((rng.normal(size=(n, (L + 1) ** 2, 3)) * 0.3)
                              .astype(np.float32)).to(DEV)
    rot = torch.cat([coeffs[:, :1], gsplat_hip.rotate_sh(coeffs[:, 1:], R)], 1)
    a = gsplat_hip.spherical_harmonics(L, dirs, rot)
    b = gsplat_hip.spherical_harmonics(L, dirs @ R, coeffs)
    err = float((a - b).abs().max() / b.abs().max())
    lim = TC.bound(load_golden("transform_checks")["sh_eval_bar"])
    print(f"sh eval err {err:.2e}  bound {lim:.2e}")
    assert err <= lim
    # unrotated coefficients are far off: the check sees the rotation
    c = gsplat_hip.spherical_harmonics(L, dirs, coeffs)
    assert float((c - b).abs().max() / b.abs().max()) > 0.1


def test_render_is_unchanged_by_a_similarity():
    import gsplat_hip
    g = load_golden("transform_checks")
    splats, vm, K, W, H = TC.render_scene()
    T = g["render_T"]
    vm2, s = TC.move_camera(vm, T)
    sp = {k: torch.from_numpy(v).to(DEV) for k, v in splats.items()}
    moved = gsplat_hip.transform_splats(sp, T)

    def render(p, viewmat, scale):
        colors = torch.cat([p["sh0"], p["shN"]], 1)
        img, _, _ = gsplat_hip.rasterization(
            p["means"], p["quats"], p["scales"].exp(), p["opacities"].sigmoid(), colors,
            torch.from_numpy(viewmat).float()[None].to(DEV),
            torch.from_numpy(K).float()[None].to(DEV), W, H, near_plane=0.01 * scale,
            far_plane=1e10 * scale, sh_degree=3, packed=False)
        return img[0]

    a, b = render(sp, vm, 1.0), render(moved, vm2, s)
    assert float(a.std()) > 0.05
    atol = 2 * TC.FACTOR * float(g["render_bar"]) * float(g["render_max"])
    print(f"render max diff {float((a - b).abs().max()):.2e}  atol {atol:.2e}")
    raster_cases.close_most(b, a, rtol=0.0, atol=atol, what="moved scene, moved camera")
    naive = dict(moved, shN=sp["shN"])
    assert float((render(naive, vm2, s) - a).abs().max()) > 1e-3


def _trainer(**kw):
    from gsplat_hip.train_step import Trainer, camera_pool, load_garden_scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(root, "tests", "golden", "garden_scene.npz"), scene_grid=1)
    means, rgbs = means[::56].contiguous(), rgbs[::56].contiguous()
    vm, K = camera_pool(vms, Ks, sw, sh_, 64, 64, n=3)
    tr = Trainer(means, rgbs, vm.float(), K.float(), 64, 64, device=DEV, max_steps=100, **kw)
    if "shN" in tr.params:
        with torch.no_grad():   # a view-dependent colour to carry along
            tr.params["shN"].normal_(0.0, 0.2, generator=torch.Generator(DEV).manual_seed(1))
    return tr


def test_trainer_save_ply_with_and_without_a_transform(tmp_path):
    import gsplat_hip
    tr = _trainer()
    plain, moved, direct = (str(tmp_path / n) for n in ("plain.ply", "moved.ply", "direct.ply"))
    n = tr.save_ply(plain)
    params = {k: v.data for k, v in tr.synced_params().items()}
    assert gsplat_hip.save_ply(params, direct) == n
    assert open(plain, "rb").read() == open(direct, "rb").read()
    T = TC.similarity(2.5, "generic", 5.0, 4)
    assert tr.save_ply(moved, transform=T) == n
    got = gsplat_hip.load_ply(moved, device=DEV)
    want = gsplat_hip.transform_splats(gsplat_hip.load_ply(plain, device=DEV), T)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["shN"], params["shN"])


def test_app_opt_trainer_save_ply_moves_the_geometry_only(tmp_path):
    """app_opt bakes view-independent colours: with a transform the file holds
    the moved means, quaternions and scales and the plain export's colours."""
    import gsplat_hip
    tr = _trainer(app_opt=True)
    plain, moved = str(tmp_path / "plain.ply"), str(tmp_path / "moved.ply")
    n = tr.save_ply(plain)
    T = TC.similarity(0.4, "generic", 3.0, 9)
    assert tr.save_ply(moved, transform=T) == n
    a, b = gsplat_hip.load_ply(plain, device=DEV), gsplat_hip.load_ply(moved, device=DEV)
    assert set(a) == set(b)
    want = gsplat_hip.transform_splats({k: a[k] for k in ("means", "quats", "scales")}, T)
    for k in a:
        assert torch.equal(b[k], want[k] if k in want else a[k]), k
    assert not torch.equal(b["means"], a["means"])
