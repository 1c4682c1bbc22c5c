"""CPU: the host side of camera pose optimisation -- the constructor's
gating, the learning-rate schedule, the state a pose_opt trainer holds, and
the ABI version."""

import math

import pytest
import torch


def _trainer(**kw):
    from gsplat_hip.train_step import Trainer
    g = torch.Generator().manual_seed(0)
    pts, rgbs = torch.rand(8, 3, generator=g), torch.rand(8, 3, generator=g)
    vm, K = torch.eye(4)[None].repeat(3, 1, 1), torch.eye(3)[None].repeat(3, 1, 1)
    return Trainer(pts, rgbs, vm, K, 16, 16, device="cpu", **kw)


UNSUPPORTED = {
    "model='2dgs'": dict(model="2dgs"),
    "packed": dict(packed=True),
    "sparse_grad": dict(packed=True, sparse_grad=True),
    "visible_adam": dict(visible_adam=True),
    "antialiased": dict(antialiased=True),
    "opacity_reg": dict(opacity_reg=0.01),
    "scale_reg": dict(scale_reg=0.01),
    "gaussian_shard": dict(gaussian_shard=True, world_size=2),
    "sharded_optimizer": dict(sharded_optimizer=True),
    "world_size": dict(world_size=2),
}


@pytest.mark.parametrize("name", sorted(UNSUPPORTED))
@pytest.mark.parametrize("opt", ["pose_opt", "pose_noise"])
def test_trainer_refuses_unsupported_combinations(name, opt):
    """Checked before anything touches the device; the message names the option."""
    kw = dict(pose_opt=True) if opt == "pose_opt" else dict(pose_noise=0.01)
    with pytest.raises(NotImplementedError, match=name.split("=")[0]):
        _trainer(**kw, **UNSUPPORTED[name])


def test_trainer_refuses_geom_in_proj_off(monkeypatch):
    monkeypatch.setenv("GSPLAT_HIP_GEOM_IN_PROJ", "0")
    with pytest.raises(NotImplementedError, match="GSPLAT_HIP_GEOM_IN_PROJ=0"):
        _trainer(pose_opt=True)
    _trainer()  # a plain trainer is not concerned


def test_pose_noise_must_not_be_negative():
    with pytest.raises(ValueError):
        _trainer(pose_noise=-1.0)


def test_lr_schedule():
    """ExponentialLR(0.01 ** (1 / max_steps)) on lr = pose_opt_lr sqrt(BS)."""
    tr = _trainer(pose_opt=True, pose_opt_lr=3e-4, max_steps=1000)
    assert tr.pose_lr_at(0) == pytest.approx(3e-4, rel=1e-12)
    assert tr.pose_lr_at(500) == pytest.approx(3e-5, rel=1e-12)
    assert tr.pose_lr_at(1000) == pytest.approx(3e-6, rel=1e-12)
    gamma = 0.01 ** (1.0 / 1000)
    assert tr.pose_lr_at(137) == pytest.approx(3e-4 * gamma ** 137, rel=1e-12)
    tr = _trainer(pose_opt=True)  # the defaults; no schedule without max_steps
    for it in (0, 17, 5000):
        assert tr.pose_lr_at(it) == 1e-5
    assert tr.pose_opt_reg == 1e-6


def test_state_of_a_pose_opt_trainer():
    tr = _trainer(pose_opt=True, pose_noise=0.05, seed=7)
    assert tr.pose.embeds.shape == (3, 9) and tr.pose.embeds.dtype == torch.float32
    assert not tr.pose.embeds.any()
    m, v = tr.moments()["pose_embeds"]
    assert m.shape == v.shape == (3, 9) and not m.any() and not v.any()
    # the fixed perturbation: from the trainer's seed, N(0, pose_noise)
    again = _trainer(pose_opt=True, pose_noise=0.05, seed=7)
    assert torch.equal(tr.pose.noise, again.pose.noise)
    assert not torch.equal(tr.pose.noise,
                           _trainer(pose_noise=0.05, seed=8).pose.noise)
    assert 0.0 < float(tr.pose.noise.abs().max()) < 0.05 * 6
    # the pose draws leave the Gaussians' initialisation alone
    plain = _trainer(seed=7)
    for k in plain.params:
        assert torch.equal(plain.params[k], tr.params[k]), k
    assert "pose_embeds" not in plain.moments()
    assert not plain.pose_active and tr.pose_active


def test_pose_adjust_argument_checks_without_a_gpu():
    import gsplat_hip
    from gsplat_hip._lib import GsplatHipError
    with pytest.raises(ValueError):
        gsplat_hip.pose_adjust(torch.eye(4)[None], torch.zeros(2, 9))
    with pytest.raises(ValueError):
        gsplat_hip.pose_adjust(torch.eye(3), torch.zeros(9))
    with pytest.raises(GsplatHipError):  # no CPU fall-back
        gsplat_hip.pose_adjust(torch.eye(4), torch.zeros(9))


def test_abi_version_is_38():
    from gsplat_hip import _lib
    assert _lib.ABI_VERSION == 38
    assert _lib.load().gsplat_hip_abi_version() == 38
    for name in ("gsplat_hip_pose_apply", "gsplat_hip_pose_bwd_adam",
                 "gsplat_hip_pose_workspace_bytes", "gsplat_hip_projection_bwd_adam_pose",
                 "gsplat_hip_pose_adjust_fwd", "gsplat_hip_pose_adjust_bwd"):
        assert name in _lib.EXPORTED
    q = _lib.query
    assert q("gsplat_hip_pose_workspace_bytes", 1) == 64
    assert q("gsplat_hip_pose_workspace_bytes", 256) == 64
    assert q("gsplat_hip_pose_workspace_bytes", 257) == 128
    assert q("gsplat_hip_pose_workspace_bytes", 1006065) == 64 * math.ceil(1006065 / 256)
