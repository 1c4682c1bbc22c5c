"""Host: the layout of the captured step's input block (graph_step.BLOCK) --
no two fields overlap, and the offsets are the ones the kernels read."""

import numpy as np
import torch


def test_block_fields_do_not_overlap_and_keep_their_offsets():
    from gsplat_hip import graph_step as G
    G._check_block()
    size = {"float32": 4, "int64": 8}
    spans = sorted((off, off + n * size[dt], name) for name, off, dt, n in G.BLOCK)
    for (_, end, a), (start, _, b) in zip(spans, spans[1:]):
        assert end <= start, (a, b)
    assert spans[-1][1] <= G.SLOT == G.GraphStep.SLOT == 2048
    offsets = {name: off for name, off, _, _ in G.BLOCK}
    assert offsets == {"adam": 0, "app": 56 * 4, "bil": 60 * 4, "pose": 62 * 4, "cam": 256,
                       "mcmc_step": 264, "mcmc_scale": 272, "viewmats": 512, "Ks": 1024,
                       "c2w": 1536, "slot": G.SLOT - 8}
    counts = {name: n for name, _, _, n in G.BLOCK}
    # the largest launch plan of the Gaussians' Adam (six groups, a shard and a
    # remainder launch each: 24 floats) and the SH-Adam's three end below the
    # first option slot
    assert 4 * 6 + 3 <= counts["adam"] == 56 == min(offsets[k] for k in ("app", "bil", "pose")) // 4
    assert counts["viewmats"] == 16 * G.MAX_WORLD and counts["Ks"] == 9 * G.MAX_WORLD


def test_block_views_are_the_fields_of_one_buffer():
    """The device views (torch) and the host slots' views (numpy) come from the
    same table: a value written through one field is read at its byte offset."""
    from gsplat_hip import graph_step as G
    for lib, buf in ((torch, torch.zeros(G.SLOT, dtype=torch.uint8)),
                     (np, np.zeros(G.SLOT, dtype=np.uint8))):
        f = G.block_views(buf, lib)
        assert set(f) == {name for name, _, _, _ in G.BLOCK}
        f["bil"][0] = 1.5
        f["cam"][0] = 3
        f["slot"][0] = 7
        raw = np.asarray(buf)
        assert raw[240:244].view(np.float32)[0] == 1.5
        assert raw[256:264].view(np.int64)[0] == 3 and raw[G.SLOT - 8:].view(np.int64)[0] == 7
        assert f["viewmats"].shape[0] == 16 * G.MAX_WORLD and f["pose"].shape[0] == 2
