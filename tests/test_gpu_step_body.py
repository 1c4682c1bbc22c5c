"""GPU: the one training-step body (Trainer._run_step) behind the eager and
the graph-replayed step.

* the captured step holds, node for node, what it held before the eager step
  and the captured step shared their body: the node census of every trainer
  configuration against tests/golden/step_census.json (recorded with the
  two-copy code; profiles/step_body/census.txt);
* an isect overflow with the side optimizers on (the bilateral grids', the
  pose table's, the appearance module's Adam): the voided steps are re-run,
  every step counter ends at the number of steps, and losses, side tables and
  their moments track an eager trainer's.

CONFIGS is shared with the measuring script of profiles/step_body (census and
eager / replayed parity of the code before and after)."""

import contextlib
import json
import os
import socket

import pytest
import torch

from test_gpu_trainer_pose import _trainer_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_census.json")

# Trainer keywords per configuration.  strategy="mcmc": MCMCStrategyConfig();
# depth_loss: the depth tables of depth_points() are added
CONFIGS = {
    "3dgs": {},
    "2dgs": dict(model="2dgs"),
    "2dgs_geometry": dict(model="2dgs", normal_loss=True, dist_loss=True, normal_start_iter=0,
                          dist_start_iter=0),
    "bilateral_grid": dict(bilateral_grid=True),
    "pose": dict(pose_opt=True, pose_noise=0.01),
    "depth_loss": dict(depth_loss=True),
    "app_opt": dict(app_opt=True),
    "app_bilagrid_depth": dict(app_opt=True, bilateral_grid=True, depth_loss=True),
    "pose_bilagrid_depth": dict(pose_opt=True, bilateral_grid=True, depth_loss=True),
    "mcmc": dict(strategy="mcmc"),
    "regularisers": dict(opacity_reg=0.01, scale_reg=0.01),
    "sharded_optimizer": dict(sharded_optimizer=True),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def depth_points(n_img, W, H):
    """Small depth tables made on the host: 150 + 37 i points for image i
    (image 2: none), positions inside the image, depths in [2, 6]."""
    out = []
    for i in range(n_img):
        g = torch.Generator().manual_seed(90 + i)
        m = 0 if i == 2 else 150 + 37 * i
        xy = torch.rand(m, 2, generator=g) * torch.tensor([W - 1.001, H - 1.001])
        out.append((xy, 2.0 + 4.0 * torch.rand(m, generator=g)))
    return out


@contextlib.contextmanager
def process_group(kw):
    """A one-rank RCCL group around a trainer with the sharded optimizer."""
    if not kw.get("sharded_optimizer"):
        yield
        return
    import gc
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        yield
    finally:
        gc.collect()  # graphs that captured RCCL collectives go before the group
        torch.cuda.synchronize()
        dist.destroy_process_group()


def make_trainer(kw, graph, **extra):
    """The 64 x 64, four-camera, ~2,000-Gaussian trainer of configuration `kw`."""
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    kw = dict(kw, **extra)
    if kw.get("strategy") == "mcmc":
        from gsplat_hip.mcmc import MCMCStrategyConfig
        kw["strategy"] = MCMCStrategyConfig()
    if kw.get("depth_loss"):
        kw["depth_points"] = depth_points(len(vm), W, H)
    return Trainer(means, rgbs, vm, K, W, H, device=DEV, graph=graph, max_steps=100, **kw)


def census_of(kw, steps=3):
    """The node census of configuration `kw`'s captured step after `steps` steps."""
    with process_group(kw):
        tr = make_trainer(kw, True)
        assert tr._graph is not None
        for it in range(steps):
            tr.step(it)
        tr.sync()
        assert tr.graph_fallback is None, tr.graph_fallback
        census = dict(tr._graph.census)
        tr.release_graph()
        del tr
    return census


@pytest.mark.parametrize("name", list(CONFIGS))
def test_census_matches_the_recorded_step(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = census_of(CONFIGS[name])
    print(f"{name}: census {got}, recorded {want}")
    assert got == want


def _side_state(tr):
    """The side tables and their moments, by name."""
    moms = tr.moments()
    out = {}
    if tr.bilateral_grid:
        out["bil_grids"] = tr.bil.grids.detach()
    if tr.pose_opt:
        out["pose_embeds"] = tr.pose.embeds
    if tr.app_opt:
        out["app_embeds"] = tr.app.embeds
        out["app_head"] = torch.cat([t.reshape(-1) for t in tr.app.head])
    for k in list(out):
        out[k + ".m"], out[k + ".v"] = moms[k][0].reshape(-1), moms[k][1].reshape(-1)
    return {k: v.detach().clone() for k, v in out.items()}


def _run(kw, graph, steps=6, **extra):
    tr = make_trainer(kw, graph, **extra)
    assert (tr._graph is not None) == graph
    losses = [tr.step(it) for it in range(steps)]
    tr.sync()
    assert tr.graph_fallback is None, tr.graph_fallback
    out = _side_state(tr)
    out["losses"] = torch.tensor([float(x.detach()) for x in losses])
    return out, tr


@pytest.mark.parametrize("name", ["pose_bilagrid_depth", "app_bilagrid"])
def test_recovery_with_side_optimizers(name):
    """isect_capacity=1000 is too small for the scene: the first steps are void
    (the sticky flag keeps every optimizer, the side ones too, from updating),
    the capacity grows, the step is re-captured and the void steps are re-run
    -- each optimizer's step counter taken back by the void steps and counted
    again by their redo.

    Tolerance, as the options' own graph-tracks-eager tests: 10 x the larger
    of the eager run-to-run spread and 1e-5 of the maximum, per quantity."""
    kw = dict(CONFIGS["pose_bilagrid_depth"]) if name == "pose_bilagrid_depth" else \
        dict(app_opt=True, bilateral_grid=True)
    steps = 6
    (a, tr_a), (a2, _), (b, tr) = _run(kw, False), _run(kw, False), \
        _run(kw, True, isect_capacity=1000)
    g = tr._graph
    print(f"{name}: recaptures {g.recaptures}, capacity {g.capacity}, max isects {g.max_isects}")
    assert tr.graph_fallback is None
    assert g.recaptures >= 2
    for t in (tr_a, tr):
        assert t.opt.step_count == steps
        assert t.bil.opt.step_count == steps
        if t.pose_opt:
            assert t.pose.step_count == steps
        if t.app_opt:
            assert t.app.step_count == steps
    assert set(a) == set(b) and len(a) >= 7
    for k in a:
        spread = float((a2[k] - a[k]).abs().max())
        top = float(a[k].abs().max())
        err = float((b[k] - a[k]).abs().max())
        bar = 10.0 * max(spread, 1e-5 * top)
        print(f"{k}: graph-vs-eager {err:.3e}, eager run-to-run {spread:.3e}, max {top:.3e}, "
              f"bar {bar:.3e}")
        assert top > 0.0 and err <= bar, (k, err, bar)
    tr.release_graph()
