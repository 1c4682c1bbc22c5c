"""Checkpoint files written by the trainer as it was BEFORE the pose,
appearance and grid optimizers owned their state (commit 67a481e, "SH colours:
float64-oracle test matrix"), for the cross-version test of
tests/test_checkpoint_host.py: the file layout and the constructors' draws must
not change with where the state lives.  Run once, on the CPU, in a checkout of
that commit (the attribute names below are that commit's Trainer's):

    python tests/golden/make_golden_checkpoint.py

The CPU skeleton trainer of tests/test_checkpoint_host.py with 8 Gaussians, 3
images of 16 x 16 and bilateral_grid_shape (2, 2, 2), in two configurations:

    checkpoint_pose.pt  pose_opt, pose_noise 0.01, bilateral_grid, DefaultStrategy
    checkpoint_app.pt   app_opt, bilateral_grid

Every side table, moment and step count is overwritten in place with seeded
random values and the trainer saved with checkpoint.save.  Each file also holds,
under "fresh", what the constructor produced before that: the seed, the
parameters, the pose-noise table and the appearance module's embeds and head.
Only CPU tensors, numbers, strings, lists and dicts (weights_only loads)."""

import os
import sys

import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(OUT, "..", "..", "gsplat-triton_amd"))

N, N_IMG, SIDE, SEED, STEP = 8, 3, 16, 5, 12


def configs():
    from gsplat_hip.densify import DefaultStrategyConfig
    return {"checkpoint_pose": dict(pose_opt=True, pose_noise=0.01, bilateral_grid=True,
                                    strategy=DefaultStrategyConfig()),
            "checkpoint_app": dict(app_opt=True, bilateral_grid=True)}


def skeleton(seed, **kw):
    from gsplat_hip.train_step import Trainer
    g = torch.Generator().manual_seed(1)
    return Trainer(torch.randn(N, 3, generator=g), torch.rand(N, 3, generator=g),
                   torch.eye(4)[None].repeat(N_IMG, 1, 1), torch.eye(3)[None].repeat(N_IMG, 1, 1),
                   SIDE, SIDE, device="cpu", seed=seed, bilateral_grid_shape=(2, 2, 2), **kw)


def main():
    from gsplat_hip import checkpoint
    for name, kw in configs().items():
        tr = skeleton(SEED, **kw)
        fresh = {"seed": SEED, "params": {k: p.detach().clone() for k, p in tr.params.items()}}
        if tr.pose_active:
            fresh["pose_noise"] = tr.pose_noise_table.clone()
        if tr.app_opt:
            fresh["app_embeds"] = tr.app_embeds.clone()
            fresh["app_head"] = [t.clone() for t in tr.app_head]
        g = torch.Generator().manual_seed(77)
        with torch.no_grad():
            tables = [tr.bil_grids]
            if tr.pose_active:
                tables += [tr.pose_embeds, tr.pose_noise_table]
            if tr.app_opt:
                tables += [tr.app_embeds, tr._app_flat]
            for t in tables:
                t.copy_(torch.randn(t.shape, generator=g))
            for m, v in tr.moments().values():
                m.copy_(torch.randn(m.shape, generator=g))
                v.copy_(torch.rand(v.shape, generator=g))
        tr.opt.step_count, tr.bil_opt.step_count = 13, 11
        if tr.pose_opt:
            tr.pose_step_count = 9
        if tr.app_opt:
            tr.app_step_count = 7
        path = os.path.join(OUT, name + ".pt")
        checkpoint.save(tr, path, STEP)
        ck = torch.load(path, map_location="cpu", weights_only=True)
        ck["fresh"] = fresh
        torch.save(ck, path)
        torch.load(path, map_location="cpu", weights_only=True)
        size = os.path.getsize(path)
        print(f"{name}: {size} bytes, side_steps {ck['gsplat_hip']['side_steps']}")
        assert size < 1_000_000, (name, size)


if __name__ == "__main__":
    main()
