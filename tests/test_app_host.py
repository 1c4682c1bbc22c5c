"""CPU: the host side of appearance optimisation -- the ABI entries, the
public function's argument checks and CPU refusal, the workspace size, the
state and the refusals of Trainer(app_opt=True), and the torch oracle (tests/app_oracle.py) against the fixture recorded from the
reference's own AppearanceOptModule (tests/golden/make_golden_app.py)."""

import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import app_oracle as O
from conftest import ROOT, load_golden

NEW = ("gsplat_hip_app_colors_fwd", "gsplat_hip_app_colors_bwd", "gsplat_hip_app_reduce_adam",
       "gsplat_hip_app_workspace_bytes")


def test_new_entries_are_bound_declared_and_exported():
    from gsplat_hip import _lib
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (gsplat_hip_\w+)", out))
    for name in NEW:
        assert name in _lib.EXPORTED, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported, name
    # new entries only: the ABI number stays
    assert _lib.ABI_VERSION == 38
    assert _lib.load().gsplat_hip_abi_version() == 38


def test_public_name():
    import gsplat_hip
    assert "appearance_colors" in gsplat_hip.__all__
    assert callable(gsplat_hip.appearance_colors)


def test_workspace_bytes():
    """One row of 8515 + 16 C floats per workgroup; a workgroup pass is 128
    rows and the grid is persistent, 256 workgroups at the most."""
    from gsplat_hip import _lib
    q = lambda n, c: _lib.query("gsplat_hip_app_workspace_bytes", n, c)
    row = lambda c: 4 * (8515 + 16 * c)
    assert q(1, 1) == row(1)
    assert q(128, 1) == row(1)
    assert q(129, 1) == 2 * row(1)
    assert q(129, 2) == 2 * row(2)
    assert q(0, 1) == row(1)  # the empty scene still gets its (zero) row
    assert q(256 * 128, 1) == 256 * row(1)
    assert q(256 * 128 + 1, 1) == 256 * row(1)
    assert math.ceil(1006065 / 128) > 256
    assert q(1006065, 1) == 256 * row(1) == 8735744  # 8.7 MB at the benchmark scene


def _args(N=4, C=1):
    g = torch.Generator().manual_seed(0)
    head = [torch.zeros(s) for s in ((64, 64), (64,), (64, 64), (64,), (3, 64), (3,))]
    return dict(features=torch.rand(N, 32, generator=g), base_colors=torch.zeros(N, 3),
                embeds=torch.zeros(C, 16), means=torch.randn(N, 3, generator=g),
                campos=torch.zeros(C, 3), head=head, sh_degree=3)


def _call(**kw):
    import gsplat_hip
    a = _args()
    a.update(kw)
    return gsplat_hip.appearance_colors(a["features"], a["base_colors"], a["embeds"], a["means"],
                                        a["campos"], a["head"], a["sh_degree"],
                                        masks=a.get("masks"))


@pytest.mark.parametrize("bad", [
    dict(features=torch.zeros(4, 16)),          # feature_dim is 32
    dict(embeds=torch.zeros(1, 8)),             # embed_dim is 16
    dict(embeds=torch.zeros(2, 16)),            # one row per camera
    dict(base_colors=torch.zeros(5, 3)),
    dict(means=torch.zeros(4, 2)),
    dict(campos=torch.zeros(3)),
    dict(sh_degree=4),                          # the module's degree is 3
    dict(sh_degree=-1),
    dict(masks=torch.ones(2, 4, dtype=torch.bool)),
    dict(head=[torch.zeros(64, 64)] * 5),
    dict(head=[torch.zeros(32, 64), torch.zeros(32), torch.zeros(64, 32), torch.zeros(64),
               torch.zeros(3, 64), torch.zeros(3)]),  # another width
    dict(head={"color_head.0.weight": torch.zeros(64, 64)}),
], ids=lambda d: next(iter(d)))
def test_argument_checks(bad):
    with pytest.raises(ValueError):
        _call(**bad)


def test_campos_gradient_is_refused():
    with pytest.raises(NotImplementedError, match="campos"):
        _call(campos=torch.zeros(1, 3, requires_grad=True))


def test_cpu_tensors_are_refused():
    from gsplat_hip._lib import GsplatHipError
    with pytest.raises(GsplatHipError):  # no CPU fall-back
        _call()
    with pytest.raises(GsplatHipError):
        _call(embeds=None)


def test_head_layouts():
    """Six tensors, the reference module's state dict (with or without the
    `color_head.` prefix) or a module with a `color_head`."""
    from gsplat_hip.appearance import HEAD_KEYS, head_tensors
    seq = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64),
                              torch.nn.ReLU(), torch.nn.Linear(64, 3))

    class Mod(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.embeds = torch.nn.Embedding(5, 16)
            self.color_head = seq

    want = [seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias, seq[4].weight, seq[4].bias]
    sd = Mod().state_dict()
    assert set(HEAD_KEYS) | {"embeds.weight"} == set(sd)
    for form in (want, sd, seq.state_dict(), Mod()):
        got = head_tensors(form)
        assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_low_level_calls_check_layout():
    """app_colors_fwd / _bwd take caller tensors: float32, contiguous, the
    feature rows 16-byte aligned -- checked before any launch."""
    from gsplat_hip import appearance as A
    head = [torch.zeros(sh) for sh in A.HEAD_SHAPES]
    f, b, m, cp = torch.zeros(4, 32), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(1, 3)
    with pytest.raises(ValueError, match="features"):
        A._check_rows(features=torch.zeros(5, 33)[1:, 1:])  # a sliced view
    with pytest.raises(ValueError, match="16-byte"):
        A._check_rows(features=torch.zeros(4 * 32 + 1)[1:].view(4, 32))
    with pytest.raises(ValueError, match="means"):
        A._check_rows(features=f, means=m.double())
    with pytest.raises(ValueError, match="radii"):
        A._check_masks(None, torch.zeros(1, 4, dtype=torch.int64))
    A._check_rows(features=f, base_colors=b, means=m, campos=cp, embeds=None,
                  **{f"head[{i}]": t for i, t in enumerate(head)})


# ------------------------------------------------------------------ Trainer
def _trainer(**kw):
    from gsplat_hip.train_step import Trainer
    g = torch.Generator().manual_seed(0)
    pts, rgbs = torch.rand(8, 3, generator=g), torch.rand(8, 3, generator=g)
    rgbs[0], rgbs[1] = 0.0, 1.0  # pure black and white SfM points
    vm, K = torch.eye(4)[None].repeat(3, 1, 1), torch.eye(3)[None].repeat(3, 1, 1)
    return Trainer(pts, rgbs, vm, K, 16, 16, device="cpu", **kw), rgbs


@pytest.mark.parametrize("init", ["random", "sfm"])
def test_trainer_state(init):
    from gsplat_hip.appearance import HEAD_KEYS, HEAD_SHAPES
    tr, rgbs = _trainer(app_opt=True, init=init)
    plain, _ = _trainer(init=init)
    off, _ = _trainer(app_opt=False, init=init)
    assert list(tr.params) == ["means", "scales", "quats", "opacities", "features", "colors"]
    assert "sh0" not in tr.params and "shN" not in tr.params
    assert tr.params["features"].shape == (8, 32) and tr.params["colors"].shape == (8, 3)
    f = tr.params["features"].detach()
    assert 0.0 <= float(f.min()) and float(f.max()) < 1.0 and float(f.std()) > 0.1
    # logit of the clamped colours: finite for pure black / white
    c = tr.params["colors"].detach()
    assert torch.isfinite(c).all()
    torch.testing.assert_close(torch.sigmoid(c), rgbs.clamp(1 / 512, 1 - 1 / 512))
    # the geometry is a plain trainer's, bit for bit; option off is the plain trainer
    for k in ("means", "scales", "quats", "opacities"):
        assert torch.equal(tr.params[k], plain.params[k]), k
    assert list(off.params) == list(plain.params)
    assert all(torch.equal(off.params[k], plain.params[k]) for k in plain.params)
    assert plain.app is None
    # the module: N(0,1) table, Linear default init, zero last layer
    assert tr.app.embeds.shape == (3, 16) and float(tr.app.embeds.std()) > 0.5
    assert [tuple(t.shape) for t in tr.app.head] == list(HEAD_SHAPES)
    bound = 1.0 / 8.0
    for t in tr.app.head[:4]:
        assert float(t.abs().max()) <= bound and float(t.abs().max()) > 0.5 * bound
    assert not tr.app.head[4].any() and not tr.app.head[5].any()
    sd = tr.app_state_dict()
    assert set(sd) == {"embeds.weight"} | set(HEAD_KEYS)
    assert torch.equal(sd["embeds.weight"], tr.app.embeds)
    for k, t in zip(HEAD_KEYS, tr.app.head):
        assert torch.equal(sd[k], t)
    # ordinary optimizer groups with the reference's learning rates
    assert tr.lrs[4] == tr.lrs[5] == 2.5e-3
    assert tr.app.lr == 1e-3 and tr.app_opt_reg == 1e-6
    assert not tr.sh_adam_in_bwd
    moms = tr.moments()
    assert set(moms) == set(tr.params) | {"app_embeds", "app_head"}
    assert moms["app_embeds"][0].shape == (3, 16) and moms["app_head"][0].shape == (8515,)
    assert moms["features"][0].shape == (8, 32)


UNSUPPORTED = {
    "pose_opt": dict(pose_opt=True),
    "pose_noise": dict(pose_noise=0.01),
    "model='2dgs'": dict(model="2dgs"),
    "packed": dict(packed=True),
    "sparse_grad": dict(packed=True, sparse_grad=True),
    "visible_adam": dict(visible_adam=True),
    "gaussian_shard": dict(gaussian_shard=True, world_size=2),
    "sharded_optimizer": dict(sharded_optimizer=True),
    "world_size": dict(world_size=2),
    "fused=False": dict(fused=False),
}


@pytest.mark.parametrize("name", sorted(UNSUPPORTED))
def test_trainer_refuses_unsupported_combinations(name):
    """Checked before anything touches the device; the message names both options."""
    with pytest.raises(NotImplementedError, match="app_opt.*" + name.split("=")[0]):
        _trainer(app_opt=True, **UNSUPPORTED[name])


def test_trainer_fixed_dimensions():
    with pytest.raises(ValueError, match="app_embed_dim"):
        _trainer(app_opt=True, app_embed_dim=32)
    with pytest.raises(ValueError, match="sh_degree"):
        _trainer(app_opt=True, sh_degree=2)
    _trainer(app_embed_dim=32)  # ignored with the option off, as the reference does


# ------------------------------------------------------------------ the oracle
def fixture_inputs(z, C):
    inp = {k: torch.from_numpy(z[k]) for k in ("features", "base_colors", "means") + O.HEAD_NAMES}
    inp["campos"] = torch.from_numpy(z["campos"][:C])
    inp["embeds"] = torch.from_numpy(z["embeds_table"][z["embed_ids"][:C]])
    return inp


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_oracle_reproduces_the_fixture_colours(C, deg):
    z = load_golden("app_opt")
    col, _ = O.run(fixture_inputs(z, C), z["v_colors"][:C], deg, torch.float32)
    np.testing.assert_allclose(col.numpy(), z[f"colors_c{C}d{deg}"], rtol=0, atol=2e-7)


@pytest.mark.parametrize("tag,C,deg,use", [("c2d3", 2, 3, True), ("c1d1none", 1, 1, False),
                                           ("c2d3none", 2, 3, False)])
def test_oracle_reproduces_the_fixture_gradients(tag, C, deg, use):
    """The same fp32 torch operations in the same order: equal up to the last
    bits (the basis is spelled differently), on gradients of order 1."""
    z = load_golden("app_opt")
    col, g = O.run(fixture_inputs(z, C), z["v_colors"][:C], deg, torch.float32, use_embeds=use)
    np.testing.assert_allclose(col.numpy(), z[f"colors_{tag}"], rtol=0, atol=2e-7)
    if f"{tag}_v_W1" not in z:
        return
    for k, v in g.items():
        ref = (z[f"{tag}_v_embeds_table"][z["embed_ids"][:C]] if k == "embeds"
               else z[f"{tag}_v_{k}"])
        np.testing.assert_allclose(v.numpy(), ref, rtol=1e-6, atol=1e-6, err_msg=k)
    if use:  # the images the step does not show get no gradient
        others = np.setdiff1d(np.arange(5), z["embed_ids"][:C])
        assert not z[f"{tag}_v_embeds_table"][others].any()


def test_oracle_fp64_agrees_with_fp32():
    z = load_golden("app_opt")
    inp = fixture_inputs(z, 2)
    c32, g32 = O.run(inp, z["v_colors"], 3, torch.float32)
    c64, g64 = O.run(inp, z["v_colors"], 3, torch.float64)
    assert c64.dtype == torch.float64
    assert float((c32.double() - c64).abs().max()) < 1e-6
    for k in g64:
        scale = float(g64[k].abs().max())
        assert float((g32[k].double() - g64[k]).abs().max()) < 1e-5 * max(scale, 1.0), k


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "app_opt.npz")) < 256 * 1024
