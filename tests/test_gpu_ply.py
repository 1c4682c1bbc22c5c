"""GPU: save_ply / load_ply through csrc/ply.hip (validity and counts, the
scan, the pack into rows, the unpack) against the reference's own files
(tests/golden/make_golden_ply.py) and against the numpy path.  Every
comparison is exact: the kernels move floats, and the one piece of arithmetic
(the colours' fp32 subtract and correctly rounded divide) must give the
reference's bytes."""

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

KEYS = ("means", "scales", "quats", "opacities", "sh0", "shN")


def on(device, g):
    s = {k: torch.from_numpy(g[k]).to(device) for k in KEYS}
    colors = torch.from_numpy(g["colors"]).to(device) if "colors" in g else None
    return s, colors


def written(tmp_path, name, splats, colors=None, **kw):
    import gsplat_hip
    path = str(tmp_path / name)
    n = gsplat_hip.save_ply(splats, path, colors, **kw)
    return open(path, "rb").read(), path, n


@pytest.mark.parametrize("name", ["ply_sh3", "ply_sh0", "ply_colors"])
@pytest.mark.parametrize("chunk", [None, 300])
def test_device_bytes_equal_the_reference(tmp_path, name, chunk):
    g = load_golden(name)
    s, colors = on("cuda", g)
    kw = {} if chunk is None else {"chunk_rows": chunk}
    data, _, _ = written(tmp_path, "dev.ply", s, colors, **kw)
    assert data == g["ply"].tobytes()


def seeded(N, K, seed=7):
    g = torch.Generator().manual_seed(seed)
    s = dict(means=torch.randn(N, 3, generator=g), scales=torch.randn(N, 3, generator=g),
             quats=torch.randn(N, 4, generator=g), opacities=torch.randn(N, generator=g),
             sh0=torch.randn(N, 1, 3, generator=g), shN=torch.randn(N, K - 1, 3, generator=g))
    colors = torch.rand(N, 3, generator=g)
    # dropped rows: singles in every field, a wave, the first and the last row
    s["means"][0, 0] = float("nan")
    s["scales"][70, 2] = float("inf")
    s["quats"][300, 3] = float("-inf")
    s["opacities"][1000] = float("nan")
    s["sh0"][2049, 0, 1] = float("inf")
    if K > 1:
        s["shN"][3000, K - 2, 2] = float("nan")
        s["shN"][1024:1088, 0, 0] = float("inf")
    s["means"][N - 1, 2] = float("nan")
    colors[513, 1] = float("nan")
    colors[4000, 0] = 3.0e38  # finite, but (c - 0.5) / C0 overflows: dropped
    return s, colors


# N = 4099: 17 workgroups, the last with 3 rows
@pytest.mark.parametrize("K", [25, 16, 4, 1])
@pytest.mark.parametrize("chunk", [None, 1000])
def test_device_equals_numpy_path(tmp_path, K, chunk):
    s, _ = seeded(4099, K)
    kw = {} if chunk is None else {"chunk_rows": chunk}
    cpu, _, n_cpu = written(tmp_path, "cpu.ply", s, **kw)
    dev, _, n_dev = written(tmp_path, "dev.ply", {k: v.cuda() for k, v in s.items()}, **kw)
    assert n_cpu == n_dev == 4099 - (7 + 64 if K > 1 else 6)
    assert dev == cpu


@pytest.mark.parametrize("chunk", [None, 1000])
def test_device_equals_numpy_path_with_colors(tmp_path, chunk):
    s, colors = seeded(4099, 16)
    kw = {} if chunk is None else {"chunk_rows": chunk}
    cpu, _, n_cpu = written(tmp_path, "cpu.ply", s, colors, **kw)
    dev, _, n_dev = written(tmp_path, "dev.ply", {k: v.cuda() for k, v in s.items()},
                            colors.cuda(), **kw)
    assert n_cpu == n_dev == 4099 - 7  # shN / sh0 are not part of a colour file
    assert dev == cpu


def test_empty_and_all_invalid(tmp_path):
    s, _ = seeded(4099, 16)
    s = {k: v[2100:2700].clone() for k, v in s.items()}
    empty, _, n0 = written(tmp_path, "e.ply", {k: v[:0].cuda() for k, v in s.items()})
    s["opacities"][:] = float("nan")
    bad, _, n1 = written(tmp_path, "b.ply", {k: v.cuda() for k, v in s.items()})
    assert n0 == n1 == 0 and empty == bad and empty.endswith(b"end_header\n")
    assert b"element vertex 0\n" in empty


@pytest.mark.parametrize("K", [25, 16, 1])
def test_load_on_the_device_round_trips(tmp_path, K):
    import gsplat_hip
    s, _ = seeded(4099, K)
    _, path, n = written(tmp_path, "rt.ply", {k: v.cuda() for k, v in s.items()})
    dev = gsplat_hip.load_ply(path, device="cuda")
    cpu = gsplat_hip.load_ply(path)
    keep = torch.ones(4099, dtype=torch.bool)
    for k in KEYS:
        keep &= torch.isfinite(s[k].reshape(4099, -1)).all(1)
    assert int(keep.sum()) == n
    for k in KEYS:
        assert dev[k].is_cuda and dev[k].shape == cpu[k].shape, k
        got = dev[k].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, cpu[k].numpy().view(np.uint32)), k
        assert np.array_equal(got, s[k][keep].numpy().view(np.uint32)), k
    # and what came back writes the same file again
    again, _, _ = written(tmp_path, "rt2.ply", dev)
    assert again == open(path, "rb").read()


def test_load_golden_on_the_device(tmp_path):
    import gsplat_hip
    g = load_golden("ply_sh3")
    path = tmp_path / "g.ply"
    path.write_bytes(g["ply"].tobytes())
    dev = gsplat_hip.load_ply(str(path), device="cuda")
    cpu = gsplat_hip.load_ply(str(path))
    for k in KEYS:
        assert np.array_equal(dev[k].cpu().numpy().view(np.uint32),
                              cpu[k].numpy().view(np.uint32)), k
