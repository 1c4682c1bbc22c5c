"""Host-side contract of the covariance-input projection, `proj` and
`world_to_cam` (no GPU): the reference's signatures, the unchanged ABI
version, argument errors raised before any device work, and the
self-consistency of the float64 fixtures the GPU tests scale their bounds
from (tests/golden/make_golden_covar.py)."""

import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

SIGS = json.load(open(os.path.join(GOLDEN, "signatures_proj.json")))


@pytest.mark.parametrize("name", sorted(SIGS))
def test_signature_matches_reference(name):
    """The rule of test_signatures.py: the reference's parameters first, with
    its names, kinds and defaults; extensions only after them, with defaults."""
    import gsplat_hip
    assert name in gsplat_hip.__all__
    ref = SIGS[name]["params"]
    ours = list(inspect.signature(getattr(gsplat_hip, name)).parameters.values())
    assert len(ours) >= len(ref), (name, [p.name for p in ours])
    for (rname, rkind, rdef), p in zip(ref, ours):
        assert p.name == rname, (name, rname, p.name)
        assert p.kind.name == rkind, (name, rname, rkind, p.kind.name)
        ours_def = None if p.default is inspect.Parameter.empty else repr(p.default)
        assert ours_def == rdef, (name, rname, rdef, ours_def)
    for p in ours[len(ref):]:
        assert p.default is not inspect.Parameter.empty, (name, "extension without default",
                                                         p.name)


def test_abi_version_unchanged():
    from gsplat_hip import _lib
    assert _lib.ABI_VERSION == 38
    for name in ("gsplat_hip_projection_covar_fwd", "gsplat_hip_projection_covar_bwd",
                 "gsplat_hip_projection_covar_packed_count",
                 "gsplat_hip_projection_covar_packed_fwd",
                 "gsplat_hip_projection_covar_packed_bwd", "gsplat_hip_world_to_cam_fwd",
                 "gsplat_hip_world_to_cam_bwd", "gsplat_hip_proj_fwd", "gsplat_hip_proj_bwd"):
        assert name in _lib.EXPORTED, name


@pytest.fixture()
def no_device_work(monkeypatch):
    """Any call into the library fails the test: the errors below must be
    raised from the arguments alone (CPU tensors here)."""
    from gsplat_hip import _lib

    def boom(name, *a):
        raise AssertionError(f"device work before the argument check: {name}")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "query", boom)


def _cams(C=1):
    return torch.eye(4).repeat(C, 1, 1), torch.eye(3).repeat(C, 1, 1)


def test_wrong_covars_shape(no_device_work):
    import gsplat_hip
    N = 5
    vm, K = _cams()
    for bad in (torch.zeros(N, 3, 3), torch.zeros(N, 5), torch.zeros(N + 1, 6)):
        with pytest.raises(AssertionError):
            gsplat_hip.fully_fused_projection(torch.zeros(N, 3), bad, None, None, vm, K, 8, 8)
    for bad in (torch.zeros(N, 6), torch.zeros(N, 3, 2), torch.zeros(N + 1, 3, 3)):
        with pytest.raises(AssertionError):
            gsplat_hip.rasterization(torch.zeros(N, 3), None, None, torch.zeros(N),
                                     torch.zeros(N, 3), vm, K, 8, 8, covars=bad)
    with pytest.raises(AssertionError):  # sparse_grad needs packed, as for quats / scales
        gsplat_hip.fully_fused_projection(torch.zeros(N, 3), torch.zeros(N, 6), None, None, vm,
                                          K, 8, 8, packed=False, sparse_grad=True)
    with pytest.raises(AssertionError):
        gsplat_hip.world_to_cam(torch.zeros(N, 3), torch.zeros(N, 6), vm)
    with pytest.raises(AssertionError):
        gsplat_hip.proj(torch.zeros(1, N, 3), torch.zeros(1, N, 6), K, 8, 8)


def test_covars_distributed_not_implemented(no_device_work):
    import gsplat_hip
    N = 5
    vm, K = _cams()
    with pytest.raises(NotImplementedError) as e:
        gsplat_hip.rasterization(torch.zeros(N, 3), None, None, torch.zeros(N),
                                 torch.zeros(N, 3), vm, K, 8, 8, covars=torch.zeros(N, 3, 3),
                                 distributed=True)
    assert "covars" in str(e.value) and "distributed" in str(e.value)


@pytest.mark.parametrize("with_covars", [False, True])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("model", ["ortho", "fisheye", "nonsense"])
def test_projection_camera_model_still_not_implemented(no_device_work, with_covars, packed, model):
    import gsplat_hip
    N = 5
    vm, K = _cams()
    covars = torch.zeros(N, 6) if with_covars else None
    quats = None if with_covars else torch.zeros(N, 4)
    scales = None if with_covars else torch.zeros(N, 3)
    with pytest.raises(NotImplementedError):
        gsplat_hip.fully_fused_projection(torch.zeros(N, 3), covars, quats, scales, vm, K, 8, 8,
                                          packed=packed, camera_model=model)


def test_proj_unknown_camera_model(no_device_work):
    import gsplat_hip
    _, K = _cams()
    with pytest.raises(ValueError):
        gsplat_hip.proj(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3, 3), K, 8, 8,
                        camera_model="equirect")


def test_cpu_tensors_are_refused():
    import gsplat_hip
    from gsplat_hip._lib import GsplatHipError
    vm, K = _cams()
    with pytest.raises(GsplatHipError):
        gsplat_hip.fully_fused_projection(torch.zeros(4, 3), torch.zeros(4, 6), None, None, vm,
                                          K, 8, 8)
    with pytest.raises(GsplatHipError):
        gsplat_hip.world_to_cam(torch.zeros(4, 3), torch.zeros(4, 3, 3), vm)
    with pytest.raises(GsplatHipError):
        gsplat_hip.proj(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3, 3), K, 8, 8)


# ---------------------------------------------------------------- fixtures --
FILES = ["covar_proj", "world_to_cam", "proj_models", "proj_models_pinhole", "proj_models_ortho",
         "proj_models_fisheye"]


@pytest.mark.parametrize("name", FILES)
def test_fixture_bars_are_finite(name):
    g = load_golden(name)
    bars = {k: float(v) for k, v in g.items() if k.startswith("bar_")}
    assert bars, name
    for k, v in bars.items():
        # a float32 run of well-conditioned algebra: some rounding, far from 1
        assert np.isfinite(v) and 0.0 <= v < 1e-2, (name, k, v)
        assert k[len("bar_"):] in g, (name, k)
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1_000_000


def test_covar_proj_fixture_is_self_consistent():
    g = load_golden("covar_proj")
    N, C = 1500, 3
    assert g["means"].shape == (N, 3) and g["covars"].shape == (N, 6)
    assert g["viewmats"].shape == (C, 4, 4) and g["radii"].shape == (C, N)
    assert g["means"].dtype == np.float32 and g["covars"].dtype == np.float32
    assert g["means2d"].dtype == np.float64 and g["v_covars_c3"].dtype == np.float64
    # the reference's own float32 run sees the same Gaussians with the same radii
    assert np.array_equal(g["radii_fp32"], g["radii"])
    vis = (g["radii"] > 0).mean()
    assert 0.3 < vis < 0.9, vis  # both culled and visible pairs
    assert (g["radii"][0] > 0).any() and (g["radii"] == 0).any()
    for tag in ("_c3", "_c3_comp", "_c1", "_c1_comp"):
        assert g["v_means" + tag].shape == (N, 3)
        assert g["v_covars" + tag].shape == (N, 6)
        Cn = int(tag[2])
        assert g["v_viewmats" + tag].shape == (Cn, 4, 4)
        # Gaussians no camera sees have no gradient
        unseen = ~(g["radii"][:Cn] > 0).any(0)
        assert unseen.any()
        assert not g["v_means" + tag][unseen].any() and not g["v_covars" + tag][unseen].any()
    # covariances are positive definite
    c = g["covars"].astype(np.float64)
    S = np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], 1)
    assert np.linalg.eigvalsh(S).min() > 0


def test_proj_models_fixture_covers_its_cases():
    g = load_golden("proj_models")
    C, N = 2, 2048
    assert g["means"].shape == (C, N, 3) and g["covars"].shape == (C, N, 3, 3)
    z = g["means"][..., 2]
    assert z.min() >= 0.5 and z.max() <= 5.0
    fe = g["means_fisheye"]
    back = fe[..., 2] < 0
    assert 0.05 < back.mean() < 0.15
    assert np.hypot(fe[..., 0], fe[..., 1])[back].min() >= 0.2 - 1e-6
    ax = g["axis_means"]
    assert ax.shape[0] * ax.shape[1] == 256
    s = np.hypot(ax[..., 0].astype(np.float64), ax[..., 1]) / ax[..., 2]
    assert s.min() >= 1e-3 * (1 - 1e-6) and s.max() <= 1e-2 * (1 + 1e-6)
    v = g["v_covars2d"]
    assert np.abs(v - np.swapaxes(v, -1, -2)).max() > 0.1  # not symmetric
    # pinhole: points on both sides of the screen-margin clamp
    K, W, H = g["Ks"], int(g["width"]), int(g["height"])
    sx = g["means"][..., 0] / z
    lim = (W - K[:, 0, 2]) / K[:, 0, 0] + 0.15 * W / K[:, 0, 0]
    assert (sx > lim[:, None]).any() and (sx < lim[:, None]).any()
    w2c = load_golden("world_to_cam")
    R = w2c["viewmats"][:, :3, :3].astype(np.float64)
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() > 1e-2  # not orthonormal
