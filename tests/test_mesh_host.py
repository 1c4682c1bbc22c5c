"""CPU: mesh export without a GPU -- the marching-cubes case table the library
was compiled with (read through gsplat_hip_mc_table), the manifoldness of the
oracle's mesh on a random field, the conditions the GPU integrate test's scene
must meet, the argument checks and refusals, and the PLY writer."""

import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_cases as M
from conftest import ROOT
from test_checkpoint_host import skeleton


@pytest.fixture(scope="module")
def table():
    from gsplat_hip.mesh import mc_table
    t = mc_table()
    assert t.shape == (256, 16) and t.dtype == np.int8
    return t


def edge_corners(e):
    dx, dy, dz, ax = M.edge_owner(e)
    a = dx + 2 * dy + 4 * dz
    return a, a + (1 << ax)


def edge_faces(e):
    """The two cube faces (axis, side) that edge e lies in."""
    dx, dy, dz, ax = M.edge_owner(e)
    return {(d, (dx, dy, dz)[d]) for d in range(3) if d != ax}


def test_abi_and_exports():
    import gsplat_hip
    from gsplat_hip import _lib
    assert _lib.ABI_VERSION == 38
    for s in ("gsplat_hip_tsdf_integrate", "gsplat_hip_mc_count", "gsplat_hip_mc_emit",
              "gsplat_hip_mc_table"):
        assert s in _lib.EXPORTED
    for s in ("TSDFVolume", "save_mesh_ply"):
        assert s in gsplat_hip.__all__ and callable(getattr(gsplat_hip, s))


def test_table_properties(table):
    """All 256 cases: entries lie on sign-changing edges, every such edge is
    used, at most 5 triangles, the triangles' open half-edges close into loops
    lying in the cube's faces, and no fan diagonal joins two vertices of one
    cube face."""
    for cs in range(256):
        row = [int(e) for e in table[cs]]
        n = next((i for i, e in enumerate(row) if e < 0), 16)
        assert n % 3 == 0 and n <= 15 and all(e == -1 for e in row[n:]), (cs, row)
        used = row[:n]
        crossed = {e for e in range(12)
                   if ((cs >> edge_corners(e)[0]) & 1) != ((cs >> edge_corners(e)[1]) & 1)}
        assert set(used) == crossed, (cs, used, crossed)
        tris = [tuple(used[m:m + 3]) for m in range(0, n, 3)]
        assert all(len(set(t)) == 3 for t in tris)
        he = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
        assert len(set(he)) == len(he), cs  # no directed half-edge twice
        open_he = [(a, b) for a, b in he if (b, a) not in he]
        # the open half-edges are the loops' links: each lies in a cube face, and every
        # vertex has exactly one coming in and one going out (closed loops through all)
        assert all(edge_faces(a) & edge_faces(b) for a, b in open_he), cs
        assert sorted(a for a, _ in open_he) == sorted(crossed), cs
        assert sorted(b for _, b in open_he) == sorted(crossed), cs
        # a matched (interior) triangle edge is a fan diagonal
        for a, b in he:
            if (b, a) in he:
                assert not (edge_faces(a) & edge_faces(b)), (cs, a, b)


def test_header_equals_the_generator(tmp_path):
    header = os.path.join(ROOT, "gsplat-triton_amd", "csrc", "mc_table.h")
    out = str(tmp_path / "mc_table.h")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mc_table.py"), out],
                   check=True)
    assert open(out).read() == open(header).read()


def test_header_is_the_compiled_table(table):
    import re
    txt = open(os.path.join(ROOT, "gsplat-triton_amd", "csrc", "mc_table.h")).read()
    rows = re.findall(r"\{([^}]*)\}", txt)
    assert len(rows) == 256
    assert np.array_equal(np.array([[int(v) for v in r.split(",")] for r in rows]), table)


def test_oracle_mesh_is_manifold_on_a_random_field(table):
    """21^3 i.i.d. normal values: all 256 cases occur, every directed
    half-edge occurs once and has its opposite except in the outer faces."""
    tsdf, _, _ = M.random_field()
    V, F, _, owners, cases = M.extract_oracle(table, tsdf, np.ones_like(tsdf), (0, 0, 0), 1.0)
    assert len(set(cases.tolist())) == 256
    assert len(F) > 0 and set(F.ravel().tolist()) == set(range(len(V)))
    repeated, bad = M.half_edges(F, owners, (21, 21, 21))
    assert repeated == 0 and bad == 0, (repeated, bad)


def test_integrate_scene_conditions():
    """The scene of the GPU integrate test: at most 1 % of the (voxel, camera)
    pairs may flip in float32, at least 5 % update; one camera sees nothing;
    every kind of skipped pair occurs."""
    sc = M.IntegrateScene()
    for views in ([sc.first], [sc.first, sc.second]):
        st, updated, near = sc.oracle(views, np.float64)
        print(f"pairs {updated.size}: near {near.mean():.4%}, updated {updated.mean():.2%}, "
              f"per camera {updated.mean(1)}")
        assert near.mean() <= 0.01
        assert updated.mean() >= 0.05
    _, updated, _ = sc.oracle([sc.first], np.float64)
    assert updated[2].sum() == 0 and updated[0].sum() > 0 and updated[1].sum() > 0
    v = sc.first
    assert (v["depths"] == 0).any() and (v["depths"] > sc.depth_trunc).any()
    assert (v["alphas"] == np.float32(0.3)).any()
    x, y, z = M.grid_points(sc.origin, sc.h, sc.dims, np.float64)
    for c in range(3):
        V, K = v["viewmats"][c].astype(np.float64), v["Ks"][c].astype(np.float64)
        pc = V[:3, :3] @ np.stack([x, y, z]) + V[:3, 3:4]
        front = pc[2] > 0
        if c == 2:
            assert not front.any()  # every voxel behind the camera
            continue
        u = K[0, 0] * pc[0] / pc[2] + K[0, 2]
        w = K[1, 1] * pc[1] / pc[2] + K[1, 2]
        assert (front & ((u < 0) | (u >= sc.W) | (w < 0) | (w >= sc.H))).any()
    w = st["weight"].reshape(sc.dims[::-1])
    assert w.max() >= 3  # some voxels fused from several cameras


def test_volume_argument_checks_come_before_device_work():
    from gsplat_hip import TSDFVolume
    from gsplat_hip._lib import GsplatHipError
    for kw in (dict(origin=(0, 0)), dict(voxel_size=0.0), dict(voxel_size=-1.0),
               dict(dims=(4, 4)), dict(dims=(4, 0, 4)), dict(dims=(4, 2.5, 4)),
               dict(sdf_trunc=0.0), dict(dims=(1 << 13, 1 << 13, 1 << 13))):
        args = dict(origin=(0, 0, 0), voxel_size=0.1, dims=(4, 4, 4))
        args.update(kw)
        with pytest.raises(ValueError):
            TSDFVolume(**args)
    with pytest.raises(GsplatHipError, match="GPU only"):
        TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    vol = TSDFVolume((0, 0, 0), 0.1, (4, 5, 6))  # no state yet: nothing touched the device
    assert vol.sdf_trunc == pytest.approx(0.5) and vol._state is None and vol.has_colors
    C, H, W = 2, 6, 8
    good = dict(depths=torch.ones(C, H, W), viewmats=torch.eye(4).repeat(C, 1, 1),
                Ks=torch.eye(3).repeat(C, 1, 1), colors=torch.zeros(C, H, W, 3))
    bad = [dict(depths=torch.ones(C, H)), dict(depths=torch.ones(C, H, W, 2)),
           dict(depths=torch.ones(C, H, W, dtype=torch.float64)),
           dict(viewmats=torch.eye(4).repeat(C + 1, 1, 1)), dict(Ks=torch.eye(3)),
           dict(Ks=torch.eye(3).repeat(C, 1, 1).double()), dict(colors=None),
           dict(colors=torch.zeros(C, H, W)), dict(alphas=torch.ones(C, H, W + 1)),
           dict(alphas=torch.ones(C, H, W, dtype=torch.float16)), dict(depth_trunc=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            vol.integrate(**dict(good, **kw))
    with pytest.raises(ValueError):  # a volume without colours takes none
        TSDFVolume((0, 0, 0), 0.1, (4, 5, 6), colors=False).integrate(**good)
    with pytest.raises(GsplatHipError, match="GPU only"):
        vol.integrate(**good)
    with pytest.raises(GsplatHipError, match="GPU only"):
        vol.integrate(**dict(good, depths=torch.ones(C, H, W, 1), alphas=torch.ones(C, H, W, 1)))
    assert vol._state is None
    with pytest.raises(ValueError):
        vol.extract_mesh(min_weight=float("nan"))


COMPANIONS = ("gaussian_shard", "sharded_optimizer", "world_size")


def test_refusal_row():
    from gsplat_hip.train_step import _MANY, _REFUSALS, _refuse
    assert _REFUSALS["mesh"][1] == _MANY == COMPANIONS
    off = {c: False for c in COMPANIONS}
    _refuse("mesh", off)
    for c in COMPANIONS:
        with pytest.raises(NotImplementedError) as e:
            _refuse("mesh", dict(off, **{c: True}))
        assert "mesh" in str(e.value) and c in str(e.value)


@pytest.mark.parametrize("option", COMPANIONS)
def test_trainer_extract_mesh_refuses_multi_gpu(option):
    from gsplat_hip.train_step import Trainer
    tr = Trainer.__new__(Trainer)  # no tensors at all: the refusal comes before any work
    tr.gshard, tr.sharded, tr.world_size = False, False, 1
    if option == "world_size":
        tr.world_size = 2
    else:
        setattr(tr, {"gaussian_shard": "gshard", "sharded_optimizer": "sharded"}[option], True)
    with pytest.raises(NotImplementedError, match="mesh.*" + option):
        tr.extract_mesh()


def test_trainer_extract_mesh_checks():
    """On CPU skeletons: every check fires before any device work (a skeleton
    that got past them would raise GsplatHipError from the volume)."""
    from gsplat_hip import checkpoint as ck
    from gsplat_hip._lib import GsplatHipError
    with pytest.raises(NotImplementedError, match="app_opt.*colors=False"):
        skeleton(app_opt=True).extract_mesh(depth_mode="expected")
    tr = skeleton()
    fp = ck.fingerprint(tr)
    with pytest.raises(ValueError, match="expected depth only"):
        tr.extract_mesh()  # 3DGS, depth_mode="median"
    for kw in (dict(depth_mode="mean"), dict(camera_batch=0), dict(voxel_size=0.0),
               dict(sdf_trunc=-1.0), dict(resolution=10), dict(cameras=[0, 7]),
               dict(bounds=((0, 0, 0), (1, 1))), dict(bounds=((0, 0, 0), (1, -1, 1)))):
        with pytest.raises(ValueError):
            tr.extract_mesh(**dict(dict(depth_mode="expected"), **kw))
    with pytest.raises(ValueError, match="max_voxels"):
        tr.extract_mesh(depth_mode="expected", bounds=((0, 0, 0), (1, 1, 1)), voxel_size=0.01,
                        max_voxels=1000)
    with pytest.raises(ValueError, match="max_voxels"):
        tr.extract_mesh(depth_mode="expected", voxel_size=0.01, max_voxels=1000)
    with pytest.raises(GsplatHipError, match="GPU only"):
        tr.extract_mesh(depth_mode="expected", voxel_size=0.5)
    with pytest.raises(ValueError, match="expected|median"):
        skeleton(model="2dgs").extract_mesh(depth_mode="mode")
    assert ck.fingerprint(tr) == fp  # no constructor option, the fingerprint is unchanged


def parse_mesh_ply(path):
    """(vertices [V,3] f32, colors [V,3] u8 or None, faces [F,3] i32) of a
    binary little-endian PLY as save_mesh_ply writes it; checks every header
    line and that the file ends with the last face."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")[:-1]
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    assert lines[2].startswith("element vertex ")
    V = int(lines[2].split()[2])
    assert lines[3:6] == ["property float x", "property float y", "property float z"]
    col = lines[6:9] == ["property uchar red", "property uchar green", "property uchar blue"]
    rest = lines[9:] if col else lines[6:]
    assert rest[0].startswith("element face ")
    F = int(rest[0].split()[2])
    assert rest[1:] == ["property list uchar int vertex_indices", "end_header"]
    vsize = 15 if col else 12
    assert len(data) == end + vsize * V + 13 * F
    verts = np.zeros((V, 3), np.float32)
    cols = np.zeros((V, 3), np.uint8) if col else None
    for i in range(V):
        rec = data[end + vsize * i:end + vsize * (i + 1)]
        verts[i] = struct.unpack("<3f", rec[:12])
        if col:
            cols[i] = struct.unpack("<3B", rec[12:])
    faces = np.zeros((F, 3), np.int32)
    base = end + vsize * V
    for i in range(F):
        n, a, b, c = struct.unpack("<B3i", data[base + 13 * i:base + 13 * (i + 1)])
        assert n == 3
        faces[i] = (a, b, c)
    return verts, cols, faces


@pytest.mark.parametrize("with_colors", [True, False])
def test_save_mesh_ply_round_trip(tmp_path, with_colors):
    from gsplat_hip import save_mesh_ply
    rng = np.random.default_rng(3)
    V, F = 37, 23
    verts = rng.standard_normal((V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int64)
    cols = rng.random((V, 3)).astype(np.float32) * 1.4 - 0.2  # some outside [0, 1]
    cols[0] = (0.0, 1.0, 0.5)
    path = str(tmp_path / "m.ply")
    out = save_mesh_ply(path, torch.from_numpy(verts), torch.from_numpy(faces),
                        torch.from_numpy(cols) if with_colors else None, chunk_rows=10)
    assert out == (V, F)
    v, c, f = parse_mesh_ply(path)
    assert np.array_equal(v.view(np.uint32), verts.view(np.uint32))
    assert np.array_equal(f, faces)
    if with_colors:
        want = np.rint(np.clip(cols, 0, 1) * np.float32(255)).astype(np.uint8)
        assert np.array_equal(c, want) and tuple(c[0]) == (0, 255, 128)
    else:
        assert c is None
    # numpy arrays and int32 faces write the same bytes; an empty mesh is a header alone
    p2 = str(tmp_path / "m2.ply")
    save_mesh_ply(p2, verts, faces.astype(np.int32), cols if with_colors else None)
    assert open(p2, "rb").read() == open(path, "rb").read()
    p3 = str(tmp_path / "e.ply")
    assert save_mesh_ply(p3, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)) == (0, 0)
    v, c, f = parse_mesh_ply(p3)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    for bad in (dict(vertices=verts[:, :2]), dict(faces=faces.astype(np.float32)),
                dict(faces=faces + V), dict(colors=cols[:5]), dict(vertices=faces)):
        args = dict(vertices=verts, faces=faces, colors=None)
        args.update(bad)
        with pytest.raises(ValueError):
            save_mesh_ply(str(tmp_path / "bad.ply"), **args)
