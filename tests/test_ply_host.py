"""CPU: gsplat_hip.save_ply / load_ply on the numpy path against files the
reference's own save_ply wrote (tests/golden/make_golden_ply.py), byte for
byte, and the header parser's refusals."""

import inspect

import numpy as np
import pytest
import torch

from conftest import load_golden

KEYS = ("means", "scales", "quats", "opacities", "sh0", "shN")
C0 = np.float32(0.2820947917738781)


def splats_of(g):
    return {k: torch.from_numpy(g[k]) for k in KEYS}


def colors_of(g):
    return torch.from_numpy(g["colors"]) if "colors" in g else None


def written(tmp_path, splats, colors=None, **kw):
    import gsplat_hip
    path = str(tmp_path / "out.ply")
    gsplat_hip.save_ply(splats, path, colors, **kw)
    return open(path, "rb").read(), path


def header(n, n_rest):
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    names += [f"f_rest_{j}" for j in range(n_rest)]
    names += ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    return ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n"
            + "".join(f"property float {k}\n" for k in names) + "end_header\n").encode()


def layout_rows(s, colors=None):
    """The issue's row layout, built field by field (no filter)."""
    n = s["means"].shape[0]
    cols = [s["means"].numpy(), np.zeros((n, 3), np.float32)]
    if colors is not None:
        cols.append((colors.numpy() - np.float32(0.5)) / C0)
    else:
        cols.append(s["sh0"].numpy().transpose(0, 2, 1).reshape(n, -1))
        cols.append(s["shN"].numpy().transpose(0, 2, 1).reshape(n, -1))
    cols += [s["opacities"].numpy()[:, None], s["scales"].numpy(), s["quats"].numpy()]
    return np.concatenate(cols, 1).astype("<f4")


def kept_rows(g):
    bad = ~np.isfinite(g["means"]).all(1) | ~np.isfinite(g["shN"].reshape(len(g["means"]), -1)).all(1)
    return ~bad


@pytest.mark.parametrize("name", ["ply_sh3", "ply_sh0", "ply_colors"])
@pytest.mark.parametrize("chunk", [None, 300, 7])
def test_bytes_equal_the_reference(tmp_path, name, chunk):
    g = load_golden(name)
    kw = {} if chunk is None else {"chunk_rows": chunk}
    data, _ = written(tmp_path, splats_of(g), colors_of(g), **kw)
    assert data == g["ply"].tobytes()


def test_golden_sh3_is_the_layout():
    g = load_golden("ply_sh3")
    keep = kept_rows(g)
    assert keep.sum() == 740 and not keep[[0, 255, 256, 999]].any() and not keep[512:768].any()
    rows = layout_rows(splats_of(g))[keep]
    assert g["ply"].tobytes() == header(740, 45) + rows.tobytes()


@pytest.mark.parametrize("name", ["ply_sh3", "ply_sh0"])
def test_load_golden_gives_the_kept_rows(tmp_path, name):
    import gsplat_hip
    g = load_golden(name)
    path = tmp_path / "g.ply"
    path.write_bytes(g["ply"].tobytes())
    out = gsplat_hip.load_ply(str(path))
    keep = kept_rows(g)
    assert set(out) == set(KEYS)
    for k in KEYS:
        assert out[k].dtype == torch.float32 and out[k].is_contiguous()
        assert out[k].shape == g[k][keep].shape, k
        assert np.array_equal(out[k].numpy().view(np.uint32), g[k][keep].view(np.uint32)), k


def test_load_colors_file_has_no_shN(tmp_path):
    import gsplat_hip
    g = load_golden("ply_colors")
    path = tmp_path / "g.ply"
    path.write_bytes(g["ply"].tobytes())
    out = gsplat_hip.load_ply(str(path))
    assert out["shN"].shape == (300, 0, 3) and out["sh0"].shape == (300, 1, 3)
    want = (g["colors"] - np.float32(0.5)) / C0
    assert np.array_equal(out["sh0"].numpy()[:, 0, :], want)
    assert np.array_equal(out["means"].numpy(), g["means"])


def test_one_bad_opacity_drops_one_row(tmp_path):
    g = load_golden("ply_sh0")
    s = splats_of(g)
    s["opacities"] = s["opacities"].clone()
    s["opacities"][17] = float("nan")
    data, _ = written(tmp_path, s)
    keep = np.ones(300, bool)
    keep[17] = False
    assert data == header(299, 0) + layout_rows(s)[keep].tobytes()


def test_colors_stay_with_their_gaussians(tmp_path):
    g = load_golden("ply_colors")
    s, colors = splats_of(g), colors_of(g).clone()
    s["scales"] = s["scales"].clone()
    s["scales"][3, 1] = float("inf")
    colors[200, 2] = float("nan")  # a non-finite colour drops its row too
    s["shN"] = torch.full_like(s["shN"], float("nan"))  # not part of a colour file
    data, _ = written(tmp_path, s, colors, chunk_rows=128)
    keep = np.ones(300, bool)
    keep[[3, 200]] = False
    rows = layout_rows(s, colors)
    assert rows.shape[1] == 17
    assert data == header(298, 0) + rows[keep].tobytes()


@pytest.mark.parametrize("case", ["empty", "all_invalid"])
def test_header_only_files(tmp_path, case):
    import gsplat_hip
    g = load_golden("ply_sh3")
    s = splats_of(g)
    if case == "empty":
        s = {k: v[:0] for k, v in s.items()}
    else:
        s["quats"] = torch.full_like(s["quats"], float("nan"))
    data, path = written(tmp_path, s)
    assert data == header(0, 45)
    out = gsplat_hip.load_ply(path)
    assert out["means"].shape == (0, 3) and out["shN"].shape == (0, 15, 3)
    assert out["opacities"].shape == (0,) and out["sh0"].shape == (0, 1, 3)


def custom_file(path, props, rows, fmt="binary_little_endian 1.0", types=None):
    types = types or {}
    txt = "ply\nformat " + fmt + "\ncomment made by a test\n" + f"element vertex {len(rows)}\n"
    txt += "".join(f"property {types.get(p, 'float')} {p}\n" for p in props) + "end_header\n"
    path.write_bytes(txt.encode() + np.asarray(rows, "<f4").tobytes())


def test_permuted_and_extra_properties(tmp_path):
    import gsplat_hip
    g = load_golden("ply_sh3")
    keep = kept_rows(g)
    s = {k: torch.from_numpy(g[k][keep]) for k in KEYS}
    rows = layout_rows(s)
    names = header(0, 45).decode().split("\n")
    names = [ln.split()[2] for ln in names if ln.startswith("property")]
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(names))
    props = [names[i] for i in perm] + ["extra_a"]
    props.insert(5, "extra_b")
    data = rows[:, perm]
    data = np.concatenate([data, np.full((len(data), 1), 7.0, np.float32)], 1)
    data = np.insert(data, 5, -3.0, axis=1)
    path = tmp_path / "perm.ply"
    custom_file(path, props, data)
    out = gsplat_hip.load_ply(str(path))
    for k in KEYS:
        assert np.array_equal(out[k].numpy(), s[k].numpy()), k


def test_refused_headers(tmp_path):
    import gsplat_hip
    names = [ln.split()[2] for ln in header(0, 0).decode().split("\n") if ln.startswith("property")]
    rows = np.zeros((2, len(names)), np.float32)
    path = tmp_path / "bad.ply"
    custom_file(path, names, rows, fmt="ascii 1.0")
    with pytest.raises(ValueError, match="format ascii 1.0"):
        gsplat_hip.load_ply(str(path))
    custom_file(path, names, rows, types={"opacity": "double"})
    with pytest.raises(ValueError, match="property double opacity"):
        gsplat_hip.load_ply(str(path))
    bad = names[:9] + [f"f_rest_{j}" for j in range(10)] + names[9:]  # 10 is not 3 (K - 1)
    custom_file(path, bad, np.zeros((2, len(bad)), np.float32))
    with pytest.raises(ValueError, match="f_rest"):
        gsplat_hip.load_ply(str(path))
    bad = names[:9] + [f"f_rest_{j}" for j in range(6)] + names[9:]  # K = 3 is no square
    custom_file(path, bad, np.zeros((2, len(bad)), np.float32))
    with pytest.raises(ValueError, match="f_rest_5"):
        gsplat_hip.load_ply(str(path))
    custom_file(path, names[:-1], rows[:, :-1])
    with pytest.raises(ValueError, match="rot_3"):
        gsplat_hip.load_ply(str(path))


def test_signature_starts_like_the_reference():
    import gsplat_hip
    params = list(inspect.signature(gsplat_hip.save_ply).parameters.values())
    assert [p.name for p in params[:3]] == ["splats", "dir", "colors"]
    assert params[2].default is None
    assert str(inspect.signature(gsplat_hip.save_ply)).startswith("(splats, dir, colors=None")


def test_abi_exports_the_ply_entries():
    from gsplat_hip import _lib
    for k in ("workspace_bytes", "count", "pack", "unpack"):
        assert "gsplat_hip_ply_" + k in _lib.EXPORTED
    lib = _lib.load()
    assert lib.gsplat_hip_ply_workspace_bytes(1000) >= 1000 + 8 * 4
    assert lib.gsplat_hip_ply_workspace_bytes(0) == 0
