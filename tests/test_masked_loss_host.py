"""Host: the pieces of Trainer(masks=..., random_bkgd=True) that need no GPU --
the float64 oracle's closed forms against its own autograd, the background
colour as a function of (seed, step), the captured step's block field, the
refusals and the checkpoint fingerprint."""

import numpy as np
import pytest
import torch

import masked_loss_oracle as O
from test_checkpoint_host import N_IMG, skeleton


@pytest.mark.parametrize("B,H,W,C", [(1, 37, 45, 3), (2, 12, 33, 1)])
def test_oracle_closed_forms_equal_its_autograd(B, H, W, C):
    """dL/dc = m ? u : 0 and dL/da = -sum_ch b_ch u_ch (u = dL/dx), to 1e-12."""
    g = torch.Generator().manual_seed(H * W + C)
    c = torch.rand(B, H, W, C, generator=g, dtype=torch.float64)
    y = torch.rand(B, H, W, C, generator=g, dtype=torch.float64)
    a = torch.rand(B, H, W, 1, generator=g, dtype=torch.float64)
    b = torch.rand(B, C, generator=g, dtype=torch.float64) * 0.8 + 0.1
    m = O.disc_mask(B, H, W)
    assert 0 < int(m.sum()) < m.numel()
    _, gc, ga = O.loss_and_grads(c, y, 0.2, m, a, b)
    fc, fa = O.closed_forms(c, y, 0.2, m, a, b)
    assert float(gc.abs().max()) > 0 and float(ga.abs().max()) > 0
    assert float((gc - fc).abs().max()) <= 1e-12
    assert float((ga - fa).abs().max()) <= 1e-12
    assert float(gc[~m].abs().max()) == 0.0
    assert float(ga[~m].abs().max()) > 0.0  # the alpha gradient lives under the mask too


def _keyed(seed):
    """A trainer that did not go through __init__, with Trainer.__init__'s noise key."""
    from gsplat_hip.train_step import Trainer
    tr = Trainer.__new__(Trainer)
    tr._noise_seed = ((seed + 1) * 0x9E3779B97F4A7C15) % (1 << 64)
    return tr


def test_bkgd_at_is_a_function_of_seed_and_step():
    a, a2, b = _keyed(42), _keyed(42), _keyed(43)
    table = [a.bkgd_at(it) for it in range(3000)]
    assert all(len(v) == 3 and all(type(x) is float for x in v) for v in table)
    assert table == [a.bkgd_at(it) for it in range(3000)]  # no stream state
    assert table[:50] == [a2.bkgd_at(it) for it in range(50)]  # another trainer, same seed
    assert all(table[it] != table[it + 1] for it in range(2999))
    assert all(a.bkgd_at(it) != b.bkgd_at(it) for it in range(50))
    t = np.array(table)
    assert t.min() >= 0.0 and t.max() < 1.0
    assert np.array_equal(t.astype(np.float32).astype(np.float64), t)  # float32 values
    # 0.03 is 5.7 standard errors of a uniform's mean at n = 3000
    assert np.abs(t.mean(0) - 0.5).max() < 0.03, t.mean(0)


def test_bkgd_at_of_a_constructed_trainer_and_rng_untouched():
    tr = skeleton(seed=5, random_bkgd=True)
    state = tr.rng.get_state().clone()
    assert tr.bkgd_at(7) == _keyed(5).bkgd_at(7)
    assert torch.equal(tr.rng.get_state(), state)


def test_block_has_the_background_field():
    """BLOCK's own field set is pinned by test_step_block_host.py, so the
    option's field sits in BLOCK_OPTIONS, in the same block and under the same
    overlap check."""
    from gsplat_hip import graph_step as G
    G._check_block()
    (field,) = [f for f in G.BLOCK_OPTIONS if f[0] == "bkgd"]
    assert field[2:] == ("float32", 3)
    end_scale = [off + 4 for name, off, _, _ in G.BLOCK if name == "mcmc_scale"][0]
    start_vm = [off for name, off, _, _ in G.BLOCK if name == "viewmats"][0]
    assert end_scale <= field[1] and field[1] + 12 <= start_vm
    buf = np.zeros(G.SLOT, dtype=np.uint8)
    G.option_views(buf, np)["bkgd"][:] = (0.25, 0.5, 0.75)
    assert list(buf[field[1]:field[1] + 12].view(np.float32)) == [0.25, 0.5, 0.75]
    assert not any(name == "bkgd" for name, _, _, _ in G.BLOCK)


COMPANIONS = ("model='2dgs'", "packed", "sparse_grad", "visible_adam", "gaussian_shard",
              "sharded_optimizer", "world_size", "bilateral_grid", "depth_loss")


@pytest.mark.parametrize("option", ["masks", "random_bkgd"])
def test_refusal_rows(option):
    from gsplat_hip.train_step import _REFUSALS, _refuse
    assert set(_REFUSALS[option][1]) == set(COMPANIONS)
    off = {c: False for c in COMPANIONS}
    _refuse(option, off)  # nothing asked: no refusal
    for c in COMPANIONS:
        with pytest.raises(NotImplementedError) as e:
            _refuse(option, dict(off, **{c: True}))
        assert option in str(e.value) and c in str(e.value)


PARENT_KEYS = {"model", "sh_degree", "fused", "n_images", "width", "height", "params", "strategy",
               "bilateral_grid", "pose_opt", "depth_loss", "app_opt", "normal_loss", "dist_loss",
               "packed", "sparse_grad", "visible_adam", "pose_noise", "opacity_reg", "scale_reg",
               "ssim_lambda", "scene_scale", "rasterize_mode", "max_steps", "sh_degree_interval"}


def test_fingerprint_gains_the_options_only_when_on(tmp_path):
    from gsplat_hip import checkpoint as ck
    from gsplat_hip.train_step import Trainer
    assert Trainer.masks is None and Trainer.random_bkgd is False
    off = skeleton(masks=None, random_bkgd=False)
    assert set(ck.fingerprint(off)) == PARENT_KEYS
    masks = torch.ones(N_IMG, 16, 32, dtype=torch.bool)
    masks[:, :, :5] = False
    on = skeleton(masks=masks, random_bkgd=True)
    assert on.masks.dtype == torch.uint8 and tuple(on.masks.shape) == (N_IMG, 16, 32)
    fp = ck.fingerprint(on)
    assert set(fp) == PARENT_KEYS | {"masks", "random_bkgd"}
    assert fp["masks"] is True and fp["random_bkgd"] is True
    with pytest.raises(ValueError, match="random_bkgd"):
        ck._check_fingerprint(off, fp)
    with pytest.raises(ValueError, match="random_bkgd"):
        ck._check_fingerprint(on, ck.fingerprint(off))
    ck._check_fingerprint(on, fp)
    # a file of a trainer without the options still loads into one
    path = str(tmp_path / "c.pt")
    off.save_checkpoint(path, 2)
    assert skeleton(seed=9).load_checkpoint(path, resume=True) == 2
    with pytest.raises(ValueError, match="masks"):
        skeleton(masks=masks).load_checkpoint(path, resume=True)


def test_constructor_refuses_and_checks_masks():
    masks = torch.ones(N_IMG, 16, 32, dtype=torch.bool)
    for kw, word in ((dict(bilateral_grid=True), "bilateral_grid"),
                     (dict(model="2dgs"), "model='2dgs'"), (dict(packed=True), "packed")):
        with pytest.raises(NotImplementedError, match="masks.*" + word):
            skeleton(masks=masks, **kw)
        with pytest.raises(NotImplementedError, match="random_bkgd.*" + word):
            skeleton(random_bkgd=True, **kw)
    with pytest.raises(ValueError, match="masks"):
        skeleton(masks=masks[:, :8])
    with pytest.raises(ValueError, match="masks"):
        skeleton(masks=masks.float())
