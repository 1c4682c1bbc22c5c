"""CPU: the host side of the bilateral grid -- the learning-rate schedule
against torch's chained schedulers, the identity parameter, and the argument
checks that need no GPU."""

import pytest
import torch


def test_lr_matches_the_chained_torch_schedulers():
    """simple_trainer.py: ChainedScheduler([LinearLR(start_factor=0.01,
    total_iters=1000), ExponentialLR(gamma=0.01 ** (1 / max_steps))]) on
    Adam(lr=2e-3); the lr of step `it` is the one in force after `it`
    scheduler steps."""
    from gsplat_hip import bilagrid_lr
    max_steps, base = 30000, 2e-3
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=base)
    sched = torch.optim.lr_scheduler.ChainedScheduler([
        torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.01, total_iters=1000),
        torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.01 ** (1.0 / max_steps))])
    want = {}
    for it in range(5001):
        if it in (0, 1, 999, 1000, 1001, 5000):
            want[it] = opt.param_groups[0]["lr"]
        opt.step()
        sched.step()
    assert sorted(want) == [0, 1, 999, 1000, 1001, 5000]
    for it, lr in want.items():
        got = bilagrid_lr(it, max_steps, base)
        assert abs(got - lr) <= 1e-12 * lr, (it, got, lr)
    assert bilagrid_lr(0, max_steps) == pytest.approx(2e-5, rel=1e-12)
    for it in (0, 17, 5000):  # no schedule without max_steps (as the means')
        assert bilagrid_lr(it, None, base) == base


def test_identity_shape_layout_and_values():
    from gsplat_hip import bilagrid_identity
    g = bilagrid_identity(3, (5, 4, 2))  # (X, Y, W) -> Wg, Hg, L
    assert g.shape == (3, 12, 2, 4, 5) and g.dtype == torch.float32
    eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
    assert torch.equal(g, eye.view(1, 12, 1, 1, 1).expand_as(g))
    # channel c = 4 i + j is element (i, j) of the 3x4 matrix: the identity
    A = g[0, :, 0, 0, 0].view(3, 4)
    assert torch.equal(A[:, :3], torch.eye(3)) and torch.equal(A[:, 3], torch.zeros(3))
    assert bilagrid_identity(1).shape == (1, 12, 8, 16, 16)
    for bad in ((1, 4, 4), (4, 1, 4), (4, 4, 1)):
        with pytest.raises(ValueError):
            bilagrid_identity(1, bad)
    with pytest.raises(ValueError):
        bilagrid_identity(0)


def test_argument_checks_without_a_gpu():
    import gsplat_hip
    from gsplat_hip._lib import GsplatHipError
    rgb = torch.rand(1, 8, 8, 3)
    for shape in ((1, 12, 1, 4, 4), (1, 12, 4, 1, 4), (1, 12, 4, 4, 1), (1, 11, 4, 4, 4)):
        with pytest.raises(ValueError):
            gsplat_hip.bilagrid_slice(torch.zeros(shape), rgb, 0)
        with pytest.raises(ValueError):
            gsplat_hip.bilagrid_tv_loss(torch.zeros(shape))
    with pytest.raises(ValueError):
        gsplat_hip.bilagrid_slice(gsplat_hip.bilagrid_identity(1), torch.rand(1, 8, 8, 4), 0)
    with pytest.raises(GsplatHipError):  # no CPU fall-back
        gsplat_hip.bilagrid_slice(gsplat_hip.bilagrid_identity(1), rgb, 0)
    with pytest.raises(GsplatHipError):
        gsplat_hip.bilagrid_tv_loss(gsplat_hip.bilagrid_identity(1))


def test_trainer_refuses_unsupported_combinations():
    """Checked before anything touches the device."""
    from gsplat_hip.train_step import Trainer
    pts, rgbs = torch.rand(8, 3), torch.rand(8, 3)
    vm, K = torch.eye(4)[None], torch.eye(3)[None]
    for kw in (dict(model="2dgs"), dict(packed=True), dict(packed=True, sparse_grad=True),
               dict(visible_adam=True), dict(gaussian_shard=True, world_size=2),
               dict(sharded_optimizer=True), dict(world_size=2)):
        with pytest.raises(NotImplementedError):
            Trainer(pts, rgbs, vm, K, 16, 16, device="cpu", bilateral_grid=True, **kw)
    for shape in ((16, 16, 1), (1, 16, 8), (16, 16)):
        with pytest.raises(ValueError):
            Trainer(pts, rgbs, vm, K, 16, 16, device="cpu", bilateral_grid=True,
                    bilateral_grid_shape=shape)
