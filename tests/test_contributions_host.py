"""CPU checks of the contribution-score surface: prune_splats, and every
refusal, which comes before any GPU work."""

import pytest
import torch

import gsplat_hip
from gsplat_hip._lib import GsplatHipError


def _splats(n=7):
    g = torch.Generator().manual_seed(0)
    return {"means": torch.randn(n, 3, generator=g), "quats": torch.randn(n, 4, generator=g),
            "scales": torch.randn(n, 3, generator=g), "opacities": torch.randn(n, generator=g),
            "sh0": torch.randn(n, 1, 3, generator=g), "shN": torch.randn(n, 15, 3, generator=g)}


@pytest.mark.parametrize("keep", [torch.tensor([True, False, True, True, False, False, True]),
                                  torch.tensor([6, 0, 3]), torch.tensor([2], dtype=torch.int32)])
def test_prune_splats_selects_rows_and_composes(keep):
    sp = _splats()
    out = gsplat_hip.prune_splats(sp, keep)
    idx = keep.nonzero().flatten() if keep.dtype == torch.bool else keep.long()
    assert set(out) == set(sp)
    for k in sp:
        assert torch.equal(out[k], sp[k][idx]) and out[k].data_ptr() != sp[k].data_ptr()
    merged = gsplat_hip.merge_splats([out, gsplat_hip.prune_splats(sp, torch.tensor([1]))])
    assert merged["shN"].shape == (len(idx) + 1, 15, 3)


@pytest.mark.parametrize("bad", [torch.ones(6, dtype=torch.bool), torch.tensor([7]),
                                 torch.tensor([0.5]), torch.tensor([[0, 1]])])
def test_prune_splats_refuses(bad):
    with pytest.raises(ValueError, match="prune_splats"):
        gsplat_hip.prune_splats(_splats(), bad)
    with pytest.raises(ValueError, match="different numbers of rows"):
        gsplat_hip.prune_splats(dict(_splats(), extra=torch.zeros(3)), torch.tensor([0]))


def test_exports_and_wrapper_refusals():
    for n in ("rasterize_to_contributions", "contribution_scores", "prune_splats"):
        assert n in gsplat_hip.__all__ and callable(getattr(gsplat_hip, n))
    C, N = 1, 5
    args = [torch.zeros(C, N, 2), torch.zeros(C, N, 3), torch.zeros(C, N), 16, 16]
    isects = [torch.zeros(C, 1, 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)]
    for ts in (8, 12, 4, 32):
        with pytest.raises(ValueError, match="tile_size must be 16"):
            gsplat_hip.rasterize_to_contributions(*args, ts, *isects)
    with pytest.raises(ValueError, match="fold needs dense"):
        gsplat_hip.rasterize_to_contributions(torch.zeros(N, 2), torch.zeros(N, 3),
                                              torch.zeros(N), 16, 16, 16, *isects, packed=True,
                                              fold=True)
    with pytest.raises(GsplatHipError, match="GPU only"):  # no CPU fallback
        gsplat_hip.rasterize_to_contributions(*args, 16, *isects)
    scene = [torch.zeros(N, 3), torch.zeros(N, 4), torch.zeros(N, 3), torch.zeros(N),
             torch.eye(4)[None], torch.eye(3)[None], 16, 16]
    with pytest.raises(ValueError, match="rasterize_mode"):
        gsplat_hip.contribution_scores(*scene, rasterize_mode="fast")
    with pytest.raises(ValueError, match="camera_batch"):
        gsplat_hip.contribution_scores(*scene, camera_batch=0)


@pytest.mark.parametrize("option", ["model='2dgs'", "app_opt", "gaussian_shard",
                                    "sharded_optimizer", "world_size"])
def test_trainer_contribution_scores_refuses(option):
    from gsplat_hip.train_step import Trainer
    tr = Trainer.__new__(Trainer)  # no tensors at all: the refusal comes before any work
    tr.gshard, tr.sharded, tr.world_size = False, False, 1
    attr, value = {"model='2dgs'": ("model", "2dgs"), "app_opt": ("app_opt", True),
                   "gaussian_shard": ("gshard", True), "sharded_optimizer": ("sharded", True),
                   "world_size": ("world_size", 2)}[option]
    setattr(tr, attr, value)
    with pytest.raises(NotImplementedError, match="contribution_scores.*" + option):
        tr.contribution_scores()
