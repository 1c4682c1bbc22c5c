"""CPU checks of the similarity transform of splat scenes: the oracle's own
properties, the fixtures, the torch path of gsplat_hip/transform.py against
the fixtures, render invariance in float64, the argument checks that come
before any device work, merge_splats, and the ABI surface."""

import os
import re

import numpy as np
import pytest
import torch

import transform_cases as TC
from conftest import GOLDEN, ROOT, load_golden


@pytest.fixture
def no_device_work(monkeypatch):
    """Any call into the library fails the test: the errors below must be
    raised from the arguments alone."""
    from gsplat_hip import _lib

    def boom(name, *a):
        raise AssertionError(f"device work before the argument check: {name}")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "query", boom)


def _rot(kind, seed):
    return TC.rotation(kind, np.random.default_rng(seed))


def _blockdiag(Ms):
    n = sum(len(M) for M in Ms)
    out = np.zeros((n, n))
    at = 0
    for M in Ms:
        out[at:at + len(M), at:at + len(M)] = M
        at += len(M)
    return out


# -------------------------------------------------------------- the oracle
def test_oracle_basis_is_the_kernels_basis():
    """The restated constants against oracle/gsplat_oracle.py's sh_fwd, which
    the colour kernels are tested against: a one-hot coefficient picks Y_k."""
    from oracle import gsplat_oracle as O
    d = TC.unit_dirs(50, 7)
    K = 25
    with O.precision(np.float64):
        Y = np.stack([O.sh_fwd(4, d, np.tile(np.eye(K)[k][None, :, None], (50, 1, 1)))[:, 0]
                      for k in range(K)], -1)
    assert np.abs(Y - TC.basis(d, 4)).max() < 1e-12


@pytest.mark.parametrize("kind", ["generic", "axis_x", "axis_z", "pi", "identity"])
def test_oracle_properties(kind):
    R1, R2 = _rot(kind, 1), _rot("generic", 2)
    M1, M2, M21 = TC.sh_blocks(R1, 4), TC.sh_blocks(R2, 4), TC.sh_blocks(R2 @ R1, 4)
    d = TC.unit_dirs(1000, 99)
    for l in range(1, 5):
        a, b, c = M1[l - 1], M2[l - 1], M21[l - 1]
        assert np.abs(a @ a.T - np.eye(2 * l + 1)).max() < 1e-12          # orthogonal
        assert np.abs(c - b @ a).max() < 1e-12                             # composition
        coef = np.random.default_rng(l).normal(size=2 * l + 1)
        lhs = TC.basis(d, l)[:, l * l:] @ (a @ coef)
        rhs = TC.basis(d @ R1, l)[:, l * l:] @ coef                        # Y(R^T d)
        assert np.abs(lhs - rhs).max() < 1e-12                             # the definition
    if kind == "identity":
        assert np.abs(_blockdiag(M1) - np.eye(24)).max() < 1e-12
    # matrix -> quaternion -> matrix
    q = TC.rotmat_to_quat(R1)
    assert abs(np.linalg.norm(q) - 1) < 1e-12
    assert np.abs(TC.quat_to_rotmat(q) - R1).max() < 1e-12
    if kind == "pi":
        assert abs(q[0]) < 1e-12           # the w = 0 branch


def test_fixtures_are_whole_and_small():
    for name in TC.NAMES:
        path = os.path.join(GOLDEN, f"transform_{name}.npz")
        assert os.path.getsize(path) < 1_000_000, name
        g = load_golden(f"transform_{name}")
        case = TC.make_case(name)
        for k in ("means", "quats", "scales", "shN", "transforms"):
            assert g[k].dtype == np.float32 and np.array_equal(g[k], getattr(case, k)), (name, k)
        assert ("ids" in g) == (case.ids is not None)
        if case.ids is not None:
            assert np.array_equal(g["ids"], case.ids)
        for k in ("means", "quats", "scales", "shN"):
            assert g["out_" + k].dtype == np.float64 and np.isfinite(g["out_" + k]).all()
        for k in TC.OUTPUTS:
            assert 0 <= float(g["bar_" + k]) < 1e-5, (name, k)
    assert os.path.getsize(os.path.join(GOLDEN, "transform_checks.npz")) < 1_000_000
    # the cases the suite is meant to hold
    specs = {s[0]: s for s in TC.SPECS}
    assert {s[1] for s in TC.SPECS} == {1, 63, 64, 65, 257, 1000}
    assert {s[2] for s in TC.SPECS} == {0, 1, 2, 3, 4}
    assert {s[3] for s in TC.SPECS} == {1, 3, 300}
    ids = TC.make_case("n257_d4_s3").ids
    assert set(ids.tolist()) == {0, 2} and (np.diff(ids) < 0).any()      # unsorted, 1 empty
    assert {s[6] for s in TC.SPECS if s[6]} == {0.01, 1.0, 37.0}
    assert specs["n64_d2_pi"][5] == ("pi",)


# ------------------------------------------------------------ the CPU path
def _check(name, res, g, factor=1.0, what="cpu"):
    got = TC.views({k: res[k].cpu().numpy() for k in ("means", "quats", "scales", "shN")})
    want = TC.views({k: g["out_" + k] for k in ("means", "quats", "scales", "shN")})
    for k in TC.OUTPUTS:
        err, lim = TC.rel_err(got[k], want[k]), factor * TC.bound(g["bar_" + k])
        print(f"{what} {name:20s} {k:9s} err {err:.2e}  bound {lim:.2e}")
        assert err <= lim, (name, k, err, lim)


@pytest.mark.parametrize("name", TC.NAMES)
def test_cpu_path_against_fixtures(name):
    import gsplat_hip
    case, g = TC.make_case(name), load_golden(f"transform_{name}")
    splats, T, ids = TC.splats_of(case, torch)
    res = gsplat_hip.transform_splats(splats, T, segment_ids=ids)
    assert set(res) == set(splats)
    for k in ("sh0", "opacities"):
        assert res[k] is splats[k]
    for k in ("means", "quats", "scales", "shN"):
        assert res[k].dtype == torch.float32 and res[k] is not splats[k]
    _check(name, res, g)
    if case.deg:
        R = case.transforms[:, :3, :3].astype(np.float64)
        R = R / np.cbrt(np.linalg.det(R))[:, None, None]
        sh = gsplat_hip.rotate_sh(splats["shN"], torch.from_numpy(R), segment_ids=ids)
        err = TC.rel_err(sh.numpy().astype(np.float64), g["out_shN"])
        assert err <= TC.bound(g["bar_shN"]), (name, err)
    # in place: the same values, written into the given tensors
    mine = {k: v.clone() for k, v in splats.items()}
    same = gsplat_hip.transform_splats(mine, T.numpy(), segment_ids=ids, inplace=True)
    for k in ("means", "quats", "scales", "shN"):
        assert same[k] is mine[k] and torch.equal(same[k], res[k])


def test_sh_rotation_matrices_against_fixture():
    import gsplat_hip
    g = load_golden("transform_checks")
    Ms = gsplat_hip.sh_rotation_matrices(torch.from_numpy(g["blocks_R"]), 4)
    assert [tuple(M.shape) for M in Ms] == [(1, 3, 3), (1, 5, 5), (1, 7, 7), (1, 9, 9)]
    for l, M in enumerate(Ms, start=1):
        err = TC.rel_err(M[0].numpy().astype(np.float64), g[f"blocks_M{l}"])
        assert err <= TC.bound(g[f"blocks_bar{l}"]), (l, err)
    two = gsplat_hip.sh_rotation_matrices(np.stack([_rot("generic", 5), np.eye(3)]), 2)
    assert two[1].shape == (2, 5, 5) and two[1].dtype == torch.float64
    assert (two[1][1] - torch.eye(5)).abs().max() < 1e-14


def _well_conditioned(name):
    """The way back divides lengths by s, so the forward rounding of the moved
    means, eps (s |m| + |t|), comes back as eps (1 + |t| / (s |m|)) relative to
    |m|.  Twice the bar against the original scene (the issue's bound) leaves
    room for a factor of about ten; the means are drawn with sigma = 3 and span
    about +-10, so the means' round trip is checked where |t| <= 10 s.  Where
    the translation dominates (s = 0.01 with |t| up to 1e3) float32 cannot
    bring the means back to that bound whatever the code does; those cases
    check the other outputs, whose round trip does not depend on t."""
    _, _, _, _, _, _, scale, tmax = TC.SPECS[TC.NAMES.index(name)]
    return scale is not None and tmax <= 10 * scale


def test_round_trip_cases():
    assert [n for n in TC.NAMES if _well_conditioned(n)] == [
        "n1_d3_generic", "n257_d0_generic", "n257_d4_s3", "n1000_d3_identity", "n1000_d2_axis_y"]


@pytest.mark.parametrize("name", TC.NAMES)
def test_round_trip(name):
    """T^-1 after T gives the input back at twice the bar, max err / max
    |original| (two roundings to float32); the means where `_well_conditioned`."""
    import gsplat_hip
    case, g = TC.make_case(name), load_golden(f"transform_{name}")
    splats, T, ids = TC.splats_of(case, torch)
    T = T.double()
    fwd = gsplat_hip.transform_splats(splats, T, segment_ids=ids)
    back = gsplat_hip.transform_splats(fwd, torch.linalg.inv(T), segment_ids=ids)
    got = TC.views({k: back[k].numpy() for k in ("means", "quats", "scales", "shN")})
    want = TC.views({k: splats[k].numpy() for k in ("means", "quats", "scales", "shN")})
    for k in TC.OUTPUTS:
        if k == "means" and not _well_conditioned(name):
            continue
        err = TC.rel_err(got[k], want[k])
        assert err <= 2 * TC.bound(g["bar_" + k]), (name, k, err)


@pytest.mark.parametrize("name", ["n65_d4_generic", "n257_d4_s3", "n1000_d3_s300"])
def test_composition(name):
    """T2 o T1 in one call equals two calls at twice the bar, max err / max
    |the one call's result|."""
    import gsplat_hip
    case, g = TC.make_case(name), load_golden(f"transform_{name}")
    splats, T, ids = TC.splats_of(case, torch)
    T = T.double()
    fwd = gsplat_hip.transform_splats(splats, T, segment_ids=ids)
    T2 = torch.from_numpy(np.stack([TC.similarity(1.7, "generic", 3.0, 11 + i)
                                    for i in range(len(T))]))
    once = gsplat_hip.transform_splats(splats, T2 @ T, segment_ids=ids)
    twice = gsplat_hip.transform_splats(fwd, T2, segment_ids=ids)
    a = TC.views({k: once[k].numpy() for k in ("means", "quats", "scales", "shN")})
    b = TC.views({k: twice[k].numpy() for k in ("means", "quats", "scales", "shN")})
    for k in TC.OUTPUTS:
        assert TC.rel_err(b[k], a[k]) <= 2 * TC.bound(g["bar_" + k]), (name, k)


def test_render_invariance_float64():
    """The oracle's float64 render of the moved scene from the moved camera is
    the render of the original: measured 3.2e-15, bound 1e-12.  Moving means,
    quaternions and scales but copying shN changes the picture by far more
    than 1e-3, so the check sees the SH rotation."""
    import gsplat_hip
    splats, vm, K, W, H = TC.render_scene()
    T = load_golden("transform_checks")["render_T"]
    assert T.dtype == np.float64
    vm2, s = TC.move_camera(vm, T)
    tsplats = {k: torch.from_numpy(v) for k, v in splats.items()}
    # float64 through the package's CPU algebra (its float32 rounding skipped)
    from gsplat_hip import transform as X
    d = X._decompose(torch.from_numpy(T)[None])
    seg = torch.zeros(len(splats["means"]), dtype=torch.int64)
    m, q, sc = (tsplats[k].double() for k in ("means", "quats", "scales"))
    moved = dict(splats)
    moved["means"] = ((d["A"][0] @ m.T).T + d["t"][0]).numpy()
    moved["quats"] = X._quat_mul(X._rotmat_to_quat(d["R"]), q).numpy()
    moved["scales"] = (sc + d["s"].log()).numpy()
    sh = tsplats["shN"].double().clone()
    at = 0
    for l, M in enumerate(X._host_blocks(d["R"], 3), start=1):
        n = 2 * l + 1
        sh[:, at:at + n] = torch.einsum("nij,njc->nic", M[seg], sh[:, at:at + n])
        at += n
    moved["shN"] = sh.numpy()
    a = TC.render(splats, vm, K, W, H, 3, 0.01, 1e10, np.float64)
    b = TC.render(moved, vm2, K, W, H, 3, 0.01 * s, 1e10 * s, np.float64)
    assert a.std() > 0.05
    diff = float(np.abs(a - b).max())
    print(f"float64 render difference {diff:.2e}")
    assert diff <= 1e-12
    naive = dict(moved, shN=splats["shN"])
    c = TC.render(naive, vm2, K, W, H, 3, 0.01 * s, 1e10 * s, np.float64)
    assert float(np.abs(a - c).max()) > 1e-3
    # and the public float32 result renders the same picture to float32 accuracy
    res = gsplat_hip.transform_splats(tsplats, T)
    f32 = {k: v.numpy() for k, v in res.items()}
    e = TC.render(f32, vm2, K, W, H, 3, 0.01 * s, 1e10 * s, np.float64)
    assert float(np.abs(a - e).max()) < 1e-4


# ------------------------------------------------------- argument checks
def _tiny(N=5, K1=3):
    g = torch.Generator().manual_seed(0)
    return {"means": torch.randn(N, 3, generator=g), "quats": torch.randn(N, 4, generator=g),
            "scales": torch.randn(N, 3, generator=g), "opacities": torch.randn(N, generator=g),
            "sh0": torch.randn(N, 1, 3, generator=g), "shN": torch.randn(N, K1, 3, generator=g)}


def test_argument_checks_come_first(no_device_work):
    import gsplat_hip
    from gsplat_hip._lib import GsplatHipError
    sp, eye = _tiny(), torch.eye(4)
    refl = eye.clone()
    refl[0, 0] = -1
    with pytest.raises(ValueError, match="segment 0.*det"):
        gsplat_hip.transform_splats(sp, refl)
    shear = eye.clone()
    shear[0, 1] = 0.01
    with pytest.raises(ValueError, match=r"segment 0.*max\|A\^T A"):
        gsplat_hip.transform_splats(sp, shear.numpy())
    both = torch.stack([eye, shear])
    with pytest.raises(ValueError, match="segment 1"):
        gsplat_hip.transform_splats(sp, both, segment_ids=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="no degree"):
        gsplat_hip.transform_splats(_tiny(K1=4), eye)
    with pytest.raises(ValueError, match="segment_ids"):
        gsplat_hip.transform_splats(sp, eye, segment_ids=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        gsplat_hip.transform_splats(sp, eye, segment_ids=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="need segment_ids"):
        gsplat_hip.transform_splats(sp, both)
    with pytest.raises(NotImplementedError):
        gsplat_hip.transform_splats(sp, eye.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        gsplat_hip.rotate_sh(sp["shN"], torch.eye(3, requires_grad=True))
    with pytest.raises(ValueError):
        gsplat_hip.sh_rotation_matrices(-torch.eye(3), 2)
    with pytest.raises(ValueError):
        gsplat_hip.transform_splats(sp, torch.eye(3))
    meta = dict(sp, means=sp["means"].to("meta"))
    with pytest.raises(GsplatHipError):
        gsplat_hip.transform_splats(meta, eye)
    # out-of-range ids on the CPU path: counted and refused, or copied through
    ids = torch.tensor([0, -1, 1, 0, 1 << 40])
    with pytest.raises(ValueError, match="3 of 5"):
        gsplat_hip.transform_splats(sp, eye[None], segment_ids=ids)
    mv = eye.clone()
    mv[:3, 3] = 1.0
    res = gsplat_hip.transform_splats(sp, mv[None], segment_ids=ids, validate=False)
    assert torch.equal(res["means"][[1, 2, 4]], sp["means"][[1, 2, 4]])
    assert torch.equal(res["means"][[0, 3]], sp["means"][[0, 3]] + 1.0)


def test_merge_splats():
    import gsplat_hip
    a, b, c = _tiny(4, 3), _tiny(3, 15), _tiny(2, 0)
    m = gsplat_hip.merge_splats([a, b, c])
    assert set(m) == set(a) and m["shN"].shape == (9, 15, 3) and m["means"].shape == (9, 3)
    assert torch.equal(m["shN"][:4, :3], a["shN"]) and not m["shN"][:4, 3:].any()
    assert torch.equal(m["shN"][4:7], b["shN"]) and not m["shN"][7:].any()
    assert torch.equal(m["quats"], torch.cat([a["quats"], b["quats"], c["quats"]]))
    extra = dict(_tiny(), features=torch.zeros(5, 2))
    with pytest.raises(ValueError, match="keys"):
        gsplat_hip.merge_splats([a, extra])
    with pytest.raises(ValueError, match="devices"):
        gsplat_hip.merge_splats([a, {k: v.to("meta") for k, v in b.items()}])
    with pytest.raises(ValueError):
        gsplat_hip.merge_splats([])


# ----------------------------------------------------------------- surface
def test_abi_and_exports():
    import gsplat_hip
    from gsplat_hip import _lib
    names = ["gsplat_hip_splat_xform_record_floats", "gsplat_hip_splat_xform_prepare",
             "gsplat_hip_splat_xform_apply", "gsplat_hip_splat_xform_rotate_sh"]
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for n in names:
        assert n in _lib.EXPORTED and re.search(rf"\b{n}\s*\(", header)
    assert _lib.ABI_VERSION == 38
    for n in ("transform_splats", "rotate_sh", "sh_rotation_matrices", "merge_splats"):
        assert n in gsplat_hip.__all__ and callable(getattr(gsplat_hip, n))
    lib = _lib.load()   # host-only queries, no kernel launch
    assert [lib.gsplat_hip_splat_xform_record_floats(d) for d in range(-1, 6)] == \
        [0, 20, 29, 54, 103, 184, 0]
    # null pointers are refused with status 1 before anything is launched
    assert lib.gsplat_hip_splat_xform_prepare(1, 3, None, None, None, None) == 1
    assert lib.gsplat_hip_splat_xform_apply(4, 0, 1, *([None] * 13)) == 1
    assert b"null" in lib.gsplat_hip_last_error()


def test_generated_table_is_current():
    """The committed header holds what the generator computes, to 1e-12 (the
    text of a float64 inverse depends on the LAPACK build, its value does
    not), and the inverse is the inverse of the basis at its directions."""
    import subprocess
    import sys
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_sh_rot_table.py"),
                    "--check"], check=True)
    text = open(os.path.join(ROOT, "gsplat-triton_amd", "csrc", "sh_rot_table.h")).read()
    for l in range(1, 5):
        n = 2 * l + 1
        arr = {k: np.array([float(v) for v in re.search(
            rf"{k}{l}\[\d+\] = \{{([^}}]*)\}}", text).group(1).split(",")]) for k in ("P", "YINV")}
        P, Yinv = arr["P"].reshape(n, 3), arr["YINV"].reshape(n, n)
        assert np.abs(np.linalg.norm(P, axis=1) - 1).max() < 1e-14
        Y = TC.basis(P, l)[:, l * l:]
        assert np.abs(Yinv @ Y - np.eye(n)).max() < 1e-12
        assert np.linalg.cond(Y) < 4.0


def test_trainer_save_ply_takes_a_transform():
    import inspect
    from gsplat_hip.train_step import Trainer
    p = inspect.signature(Trainer.save_ply).parameters
    assert list(p) == ["self", "path", "sh_degree", "transform"]
    assert p["transform"].default is None
    assert "np.linalg.inv(parser.transform)" in Trainer.save_ply.__doc__
