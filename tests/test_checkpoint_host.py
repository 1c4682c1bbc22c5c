"""CPU: the checkpoint dict of Trainer.save_checkpoint (gsplat_hip/checkpoint.py)
on skeleton trainers that hold their tensors on the CPU and launch nothing: the
multi-rank refusals, the reference's keys and shapes, the weights_only round
trip and the fingerprint check."""

import pytest
import torch

N, N_IMG = 60, 3


def skeleton(seed=42, **kw):
    from gsplat_hip.train_step import Trainer
    g = torch.Generator().manual_seed(1)
    return Trainer(torch.randn(N, 3, generator=g), torch.rand(N, 3, generator=g),
                   torch.eye(4)[None].repeat(N_IMG, 1, 1), torch.eye(3)[None].repeat(N_IMG, 1, 1),
                   32, 16, device="cpu", seed=seed, **kw)


@pytest.mark.parametrize("option", ["gaussian_shard", "sharded_optimizer", "world_size"])
@pytest.mark.parametrize("method", ["save_checkpoint", "load_checkpoint", "load_splats",
                                    "save_ply"])
def test_multi_rank_options_are_refused(tmp_path, option, method):
    from gsplat_hip.train_step import _REFUSALS, Trainer
    assert _REFUSALS["checkpoint"][1] == ("gaussian_shard", "sharded_optimizer", "world_size")
    tr = Trainer.__new__(Trainer)  # no tensors at all: the refusal comes before any work
    tr.gshard, tr.sharded, tr.world_size = False, False, 1
    if option == "world_size":
        tr.world_size = 2
    else:
        setattr(tr, {"gaussian_shard": "gshard", "sharded_optimizer": "sharded"}[option], True)
    args = {"save_checkpoint": (str(tmp_path / "c.pt"), 0),
            "load_checkpoint": (str(tmp_path / "missing.pt"),),
            "load_splats": ({},), "save_ply": (str(tmp_path / "c.ply"),)}[method]
    with pytest.raises(NotImplementedError, match="checkpoint.*" + option):
        getattr(tr, method)(*args)
    assert not list(tmp_path.iterdir())


def plain_only(x):
    if isinstance(x, dict):
        assert all(isinstance(k, str) for k in x)
        return all(plain_only(v) for v in x.values())
    if isinstance(x, list):
        return all(plain_only(v) for v in x)
    if torch.is_tensor(x):
        return x.device.type == "cpu"
    return x is None or isinstance(x, (bool, int, float, str))


def test_reference_keys_and_shapes(tmp_path):
    from gsplat_hip.densify import DefaultStrategyConfig
    tr = skeleton(pose_opt=True, bilateral_grid=True, strategy=DefaultStrategyConfig())
    path = str(tmp_path / "ckpt_6_rank0.pt")
    tr.save_checkpoint(path, 6)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert plain_only(ck)
    assert set(ck) == {"step", "splats", "pose_adjust", "gsplat_hip"} and ck["step"] == 6
    shapes = {k: tuple(v.shape) for k, v in ck["splats"].items()}
    assert shapes == {"means": (N, 3), "scales": (N, 3), "quats": (N, 4), "opacities": (N,),
                      "sh0": (N, 1, 3), "shN": (N, 15, 3)}
    assert list(ck["splats"]) == ["means", "scales", "quats", "opacities", "sh0", "shN"]
    assert {k: tuple(v.shape) for k, v in ck["pose_adjust"].items()} == \
        {"embeds.weight": (N_IMG, 9)}
    gs = ck["gsplat_hip"]
    for k in ("format", "fingerprint", "moments", "adam_step", "side_steps", "bil_grids",
              "grad2d", "count", "radii2d", "refine_log", "rng", "noise_seed", "split"):
        assert k in gs, k
    assert set(gs["moments"]) == set(shapes) | {"bil_grids", "pose_embeds"}
    assert gs["side_steps"] == {"bil": 0, "pose": 0}
    assert set(gs["split"]) >= {"split_div", "split_threshold", "split_launch", "_split_tuned"}
    fp = gs["fingerprint"]
    assert fp["model"] == "3dgs" and fp["sh_degree"] == 3 and fp["n_images"] == N_IMG
    assert (fp["width"], fp["height"]) == (32, 16) and fp["strategy"] == "DefaultStrategyConfig"
    assert fp["strategy.refine_every"] == 100 and fp["pose_opt"] is True


def test_app_opt_keys_are_the_reference_modules(tmp_path):
    tr = skeleton(app_opt=True)
    path = str(tmp_path / "c.pt")
    tr.save_checkpoint(path, 0)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert {k: tuple(v.shape) for k, v in ck["splats"].items()} == {
        "means": (N, 3), "scales": (N, 3), "quats": (N, 4), "opacities": (N,),
        "features": (N, 32), "colors": (N, 3)}
    assert {k: tuple(v.shape) for k, v in ck["app_module"].items()} == {
        "embeds.weight": (N_IMG, 16), "color_head.0.weight": (64, 64), "color_head.0.bias": (64,),
        "color_head.2.weight": (64, 64), "color_head.2.bias": (64,),
        "color_head.4.weight": (3, 64), "color_head.4.bias": (3,)}
    assert set(ck["gsplat_hip"]["moments"]) == set(ck["splats"]) | {"app_embeds", "app_head"}


def test_round_trip_restores_a_trainer_of_another_seed(tmp_path):
    from gsplat_hip.mcmc import MCMCStrategyConfig
    a = skeleton(seed=1, strategy=MCMCStrategyConfig(), pose_noise=0.01)
    # a state no fresh trainer has
    g = torch.Generator().manual_seed(9)
    for m, v in a.moments().values():
        m.copy_(torch.randn(m.shape, generator=g))
        v.copy_(torch.rand(v.shape, generator=g))
    a.opt.step_count = 11
    a.grad2d += 2.0
    a.refine_log = [(5, 1, 2, N)]
    torch.randn(7, generator=a.rng)
    a.split_div, a.split_threshold, a.split_launch, a._split_tuned = 1100, 640, 1, True
    path = str(tmp_path / "c.pt")
    a.save_checkpoint(path, 10)
    b = skeleton(seed=2, strategy=MCMCStrategyConfig(), pose_noise=0.01)
    assert not torch.equal(a.params["quats"], b.params["quats"])
    assert a._noise_seed != b._noise_seed
    gen = b._param_gen
    assert b.load_checkpoint(path) == 10
    assert b._param_gen == gen + 1
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]), k
        assert isinstance(b.params[k], torch.nn.Parameter)
        for x, y in zip(a.moments()[k], b.moments()[k]):
            assert torch.equal(x, y), k
    assert b.opt.step_count == 11 and b.opt.params == list(b.params.values())
    assert torch.equal(a.grad2d, b.grad2d) and torch.equal(a.count, b.count)
    assert b.refine_log == [(5, 1, 2, N)] and b._noise_seed == a._noise_seed
    assert torch.equal(a.rng.get_state(), b.rng.get_state())
    assert torch.equal(a.pose.noise, b.pose.noise)
    assert (b.split_div, b.split_threshold, b.split_launch, b._split_tuned) == (1100, 640, 1, True)
    # the saving trainer is untouched
    assert a.opt.step_count == 11 and a._param_gen == 0


def test_fingerprint_mismatch_names_every_field(tmp_path):
    from gsplat_hip.densify import DefaultStrategyConfig
    a = skeleton(strategy=DefaultStrategyConfig(refine_every=50))
    path = str(tmp_path / "c.pt")
    a.save_checkpoint(path, 3)
    b = skeleton(strategy=DefaultStrategyConfig(refine_every=70), opacity_reg=0.01)
    before = {k: v.clone() for k, v in b.params.items()}
    with pytest.raises(ValueError) as e:
        b.load_checkpoint(path)
    assert "strategy.refine_every" in str(e.value) and "opacity_reg" in str(e.value)
    assert "sh_degree" not in str(e.value)
    assert all(torch.equal(before[k], b.params[k]) for k in before) and b._param_gen == 0
    c = skeleton(sh_degree=2)
    with pytest.raises(ValueError, match="sh_degree.*strategy"):
        c.load_checkpoint(path)


def test_reference_files_take_the_evaluation_path(tmp_path):
    a = skeleton(seed=1)
    a.opt.step_count = 4
    a.opt.exp_avg[0] += 1.0
    ck = {"step": 4, "splats": {k: v.detach().clone() for k, v in a.params.items()}}
    half = N // 2
    p1, p2 = str(tmp_path / "ckpt_4_rank0.pt"), str(tmp_path / "ckpt_4_rank1.pt")
    torch.save({"step": 4, "splats": {k: v[:half] for k, v in ck["splats"].items()}}, p1)
    torch.save({"step": 4, "splats": {k: v[half:] for k, v in ck["splats"].items()}}, p2)
    b = skeleton(seed=2)
    b.opt.step_count = 9
    b.grad2d += 1.0
    with pytest.raises(ValueError, match="gsplat_hip"):
        b.load_checkpoint(p1)  # resume=True needs the block
    assert b.load_checkpoint([p1, p2], resume=False) == 4
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]), k
        assert all(not m.any() for m in b.moments()[k])
    assert b.opt.step_count == 0 and not b.grad2d.any() and b.grad2d.shape == (N,)
    # one file, fewer Gaussians than the trainer was built with
    assert b.load_checkpoint(p1, resume=False) == 4
    assert b.params["means"].shape == (half, 3) and b.count.shape == (half,)
    with pytest.raises(ValueError, match="shN"):
        b.load_splats({k: v for k, v in ck["splats"].items() if k != "shN"})


@pytest.mark.parametrize("kw", [dict(fused=False), dict(visible_adam=True)],
                         ids=["torch_adam", "selective_adam"])
def test_torch_optimizers_round_trip(tmp_path, kw):
    """The trainers whose Gaussians' Adam is a torch.optim optimizer keep the
    step count in its per-parameter state."""
    a = skeleton(seed=1, **kw)
    assert isinstance(a.opt, torch.optim.Optimizer)
    g = torch.Generator().manual_seed(3)
    for p in a.params.values():  # the state after five steps
        a.opt.state[p] = {"step": torch.tensor(5.0), "exp_avg": torch.randn(p.shape, generator=g),
                          "exp_avg_sq": torch.rand(p.shape, generator=g)}
    path = str(tmp_path / "c.pt")
    a.save_checkpoint(path, 4)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["gsplat_hip"]["adam_step"] == 5
    b = skeleton(seed=2, **kw)
    assert b.load_checkpoint(path) == 4
    for k, p in b.params.items():
        st = b.opt.state[p]
        assert float(st["step"]) == 5.0
        assert torch.equal(st["exp_avg"], a.moments()[k][0])
        assert torch.equal(st["exp_avg_sq"], a.moments()[k][1])
        assert torch.equal(p, a.params[k])
    assert [g_["params"][0] for g_ in b.opt.param_groups] == list(b.params.values())


# ---- files written before the side optimizers owned their state
# (tests/golden/make_golden_checkpoint.py: 8 Gaussians, 3 images of 16 x 16)
GOLDEN = ("app", "pose")


def golden_trainer(name, seed):
    from gsplat_hip.densify import DefaultStrategyConfig
    from gsplat_hip.train_step import Trainer
    kw = {"pose": dict(pose_opt=True, pose_noise=0.01, strategy=DefaultStrategyConfig()),
          "app": dict(app_opt=True)}[name]
    g = torch.Generator().manual_seed(1)
    return Trainer(torch.randn(8, 3, generator=g), torch.rand(8, 3, generator=g),
                   torch.eye(4)[None].repeat(N_IMG, 1, 1), torch.eye(3)[None].repeat(N_IMG, 1, 1),
                   16, 16, device="cpu", seed=seed, bilateral_grid=True,
                   bilateral_grid_shape=(2, 2, 2), **kw)


def golden_file(name):
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        f"checkpoint_{name}.pt")
    return path, torch.load(path, map_location="cpu", weights_only=True)


def assert_same(a, b, where="checkpoint"):
    """torch.equal on every tensor, == on everything else, the same keys."""
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert set(a) == set(b), (where, sorted(a), sorted(b))
        for k in a:
            assert_same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, list):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same(x, y, f"{where}[{i}]")
    elif torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    else:
        assert a == b, (where, a, b)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_constructor_draws_match_the_golden_files(name):
    """A fresh trainer with the file's seed holds what the constructor of the
    trainer that wrote the file produced."""
    _, ck = golden_file(name)
    fresh = ck["fresh"]
    tr = golden_trainer(name, fresh["seed"])
    assert_same({k: p.detach() for k, p in tr.params.items()}, fresh["params"], "params")
    if name == "pose":
        assert torch.equal(tr.pose.noise, fresh["pose_noise"])
        assert not tr.pose.embeds.any() and tr.pose.step_count == 0
    else:
        assert torch.equal(tr.app.embeds, fresh["app_embeds"])
        assert_same([t for t in tr.app.head], fresh["app_head"], "app_head")
    assert tr.bil.opt.step_count == 0


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_file_resumes_into_the_same_state(name):
    """load_checkpoint of a file of the earlier layout of the trainer's state,
    then checkpoint.state: the file's dictionary, tensor for tensor."""
    from gsplat_hip import checkpoint
    path, ck = golden_file(name)
    seed = ck.pop("fresh")["seed"]
    tr = golden_trainer(name, seed + 1)
    assert tr.load_checkpoint(path) == ck["step"]
    assert_same(checkpoint.state(tr, ck["step"]), ck)
    assert ck["gsplat_hip"]["side_steps"] == {"pose": {"bil": 11, "pose": 9},
                                              "app": {"bil": 11, "app": 7}}[name]


def test_golden_pose_file_on_the_evaluation_path():
    """resume=False: the pose table copied, its moments and step count zero;
    the grids, their moments and step count, and the noise table kept."""
    path, ck = golden_file("pose")
    tr = golden_trainer("pose", ck["fresh"]["seed"] + 1)
    tr.pose.step_count, tr.bil.opt.step_count = 4, 5
    for t in tr.pose.moments()["pose_embeds"] + tr.bil.moments()["bil_grids"]:
        t.fill_(0.5)
    with torch.no_grad():
        tr.bil.grids.mul_(2.0)
    grids, noise = tr.bil.grids.detach().clone(), tr.pose.noise.clone()
    assert tr.load_checkpoint(path, resume=False) == ck["step"]
    assert_same({k: p.detach() for k, p in tr.params.items()}, ck["splats"], "splats")
    assert torch.equal(tr.pose.embeds, ck["pose_adjust"]["embeds.weight"])
    assert tr.pose.step_count == 0 and tr.opt.step_count == 0
    assert all(not t.any() for t in tr.moments()["pose_embeds"])
    assert tr.bil.opt.step_count == 5 and torch.equal(tr.bil.grids, grids)
    assert all(bool((t == 0.5).all()) for t in tr.moments()["bil_grids"])
    assert torch.equal(tr.pose.noise, noise)
