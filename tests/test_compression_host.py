"""CPU: the host side of the splat compression (gsplat_hip/compression.py) --
the PNG codec (Pillow and the stdlib fallback), the writer / reader of the
reference's on-disk format against the format's own error bars and the
reference's decode formula, the crop, the constant channel, the Morton order
against the numpy oracle, and the public surface.

Error bars (compression_oracle.half_step): an 8-bit parameter decodes within
(max - min) / (2 * 255) of its value per channel, the log-space means within
range / (2 * 65535), a centroid within (max - min) / (2 * 63); each plus a few
fp32 ulps (the decoded value is rounded to float32)."""

import json
import os

import numpy as np
import pytest
import torch

import compression_oracle as O
from conftest import GOLDEN

from gsplat_hip import compression as C


@pytest.fixture(params=["pillow", "stdlib"])
def codec(request, monkeypatch):
    if request.param == "pillow":
        pytest.importorskip("PIL")
    monkeypatch.setattr(C, "USE_PILLOW", request.param == "pillow")
    return request.param


# ------------------------------------------------------------------ PNG codec
@pytest.mark.parametrize("n", [1, 7, 64])
@pytest.mark.parametrize("chans", [None, 3, 4])
def test_png_round_trip(tmp_path, codec, n, chans):
    rng = np.random.default_rng(n * 10 + (chans or 0))
    img = rng.integers(0, 256, (n, n) if chans is None else (n, n, chans), dtype=np.uint8)
    path = str(tmp_path / "img.png")
    C.write_png(path, img)
    back = C.read_png(path)
    assert back.dtype == np.uint8 and back.shape == img.shape
    assert np.array_equal(back, img)


@pytest.mark.parametrize("n", [1, 7, 64])
@pytest.mark.parametrize("chans", [None, 3, 4])
def test_pillow_reads_the_fallbacks_files(tmp_path, n, chans):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(n * 10 + (chans or 0) + 1)
    img = rng.integers(0, 256, (n, n) if chans is None else (n, n, chans), dtype=np.uint8)
    path = str(tmp_path / "img.png")
    with open(path, "wb") as f:
        f.write(C.png_encode(img))
    with Image.open(path) as im:
        assert im.mode == {None: "L", 3: "RGB", 4: "RGBA"}[chans]
        assert np.array_equal(np.array(im), img)
    assert np.array_equal(C.png_decode(open(path, "rb").read()), img)


def test_fallback_writes_the_up_filter_and_refuses_what_it_cannot_read():
    import struct
    import zlib
    img = np.arange(5 * 6 * 3, dtype=np.uint8).reshape(5, 6, 3)
    data = C.png_encode(img)
    n = struct.unpack(">I", data[33:37])[0]
    assert data[37:41] == b"IDAT"
    raw = np.frombuffer(zlib.decompress(data[41:41 + n]), np.uint8).reshape(5, 1 + 18)
    assert (raw[:, 0] == 2).all()
    with pytest.raises(ValueError):
        C.png_encode(img.astype(np.uint16))
    with pytest.raises(ValueError):
        C.png_encode(img[:, :, :2])
    with pytest.raises(ValueError):
        C.png_decode(b"not a png at all")


# ----------------------------------------------------------------- host stage
def _arrays(n_side=8, K=5, seed=0, degree=3):
    rng = np.random.default_rng(seed)
    N = n_side * n_side
    f = np.float32
    quats = rng.normal(size=(N, 4))
    D = 3 * ((degree + 1) ** 2 - 1)
    cents = rng.normal(scale=0.2, size=(K, D)).astype(f)
    labels = rng.integers(0, K, N)
    labels[:K] = np.arange(K)
    arrays = {
        "means": O.log_transform(rng.normal(scale=3.0, size=(N, 3))).astype(f),
        "scales": rng.normal(-3.0, 1.0, (N, 3)).astype(f),
        "quats": (quats / np.linalg.norm(quats, axis=1, keepdims=True)).astype(f),
        "opacities": rng.normal(size=N).astype(f),
        "sh0": rng.normal(scale=0.5, size=(N, 1, 3)).astype(f),
        "shN": cents[labels].reshape(N, D // 3, 3),
        "features": rng.normal(size=(N, 32)).astype(f),
    }
    return arrays, cents, labels


def test_writer_files_meta_and_bars(tmp_path, codec):
    arrays, cents, labels = _arrays()
    d = str(tmp_path / "c")
    meta = C.write_arrays(d, arrays, (cents, labels))
    assert sorted(os.listdir(d)) == sorted(
        ["means_l.png", "means_u.png", "scales.png", "quats.png", "opacities.png", "sh0.png",
         "shN.npz", "features.npz", "meta.json"])
    assert json.load(open(os.path.join(d, "meta.json"))) == json.loads(json.dumps(meta))
    assert list(meta) == list(arrays)
    for k, a in arrays.items():
        assert meta[k]["shape"] == list(a.shape) and meta[k]["dtype"] == "float32"
    for k in ("means", "scales", "quats", "opacities", "sh0"):
        assert set(meta[k]) == {"shape", "dtype", "mins", "maxs"}
        C_ = arrays[k].reshape(64, -1).shape[1]
        assert len(meta[k]["mins"]) == C_ and len(meta[k]["maxs"]) == C_
        assert np.array_equal(np.asarray(meta[k]["mins"], np.float32),
                              arrays[k].reshape(64, -1).min(0))
    assert set(meta["shN"]) == {"shape", "dtype", "mins", "maxs", "quantization"}
    assert meta["shN"]["quantization"] == 6 and isinstance(meta["shN"]["mins"], float)
    assert set(meta["features"]) == {"shape", "dtype"}
    with np.load(os.path.join(d, "shN.npz")) as z:
        assert z["centroids"].dtype == np.uint8 and z["centroids"].shape == cents.shape
        assert z["centroids"].max() <= 63
        assert z["labels"].dtype == np.uint16 and np.array_equal(z["labels"], labels)
    assert C.read_png(os.path.join(d, "opacities.png")).shape == (8, 8)
    assert C.read_png(os.path.join(d, "quats.png")).shape == (8, 8, 4)

    out = C.read_arrays(d)
    assert list(out) == list(arrays)
    for k, a in arrays.items():
        assert out[k].shape == a.shape and out[k].dtype == np.float32, k
    for k, bits in (("means", 16), ("scales", 8), ("quats", 8), ("opacities", 8), ("sh0", 8)):
        bar = O.half_step(meta[k]["mins"], meta[k]["maxs"], bits)
        err = np.abs(out[k].astype(np.float64) - arrays[k]).reshape(64, -1)
        assert (err <= bar).all(), (k, err.max(0), bar)
    bar = O.half_step(meta["shN"]["mins"], meta["shN"]["maxs"], 6)
    err = np.abs(out["shN"].reshape(64, -1).astype(np.float64) - cents[labels])
    assert (err <= bar).all(), (err.max(), bar)
    # every row is its label's (dequantised) centroid: equal labels, equal rows
    rows = out["shN"].reshape(64, -1)
    for k in range(len(cents)):
        assert (rows[labels == k] == rows[labels == k][0]).all()
    assert np.array_equal(out["features"], arrays["features"])


def test_reference_decode_formula_gives_the_same_arrays(tmp_path, codec):
    """img / (2^b - 1) * (maxs - mins) + mins and centroids[labels], written
    out here on the raw files."""
    arrays, cents, labels = _arrays(seed=1)
    d = str(tmp_path / "c")
    C.write_arrays(d, arrays, (cents, labels))
    meta = json.load(open(os.path.join(d, "meta.json")))
    out = C.read_arrays(d)
    for k in ("scales", "quats", "opacities", "sh0"):
        img = C.read_png(os.path.join(d, k + ".png"))
        ref = img / (2 ** 8 - 1) * (np.array(meta[k]["maxs"]) - np.array(meta[k]["mins"])) \
            + np.array(meta[k]["mins"])
        assert np.array_equal(ref.reshape(meta[k]["shape"]).astype(np.float32), out[k]), k
        assert np.array_equal(img.reshape(64, -1),
                              O.quantize(arrays[k].reshape(64, -1), meta[k]["mins"],
                                         meta[k]["maxs"], 8)), k
    lo = C.read_png(os.path.join(d, "means_l.png"))
    hi = C.read_png(os.path.join(d, "means_u.png")).astype(np.uint16)
    img = (hi << 8) + lo
    m = meta["means"]
    ref = img / (2 ** 16 - 1) * (np.array(m["maxs"]) - np.array(m["mins"])) + np.array(m["mins"])
    assert np.array_equal(ref.reshape(m["shape"]).astype(np.float32), out["means"])
    z = np.load(os.path.join(d, "shN.npz"))
    s = meta["shN"]
    c = z["centroids"] / (2 ** s["quantization"] - 1) * (s["maxs"] - s["mins"]) + s["mins"]
    assert np.array_equal(c[z["labels"]].reshape(s["shape"]).astype(np.float32), out["shN"])


def test_decompress_inverts_the_log_transform(tmp_path):
    arrays, cents, labels = _arrays(seed=2)
    d = str(tmp_path / "c")
    meta = C.write_arrays(d, arrays, (cents, labels))
    out = C.PngCompression().decompress(d)
    assert all(isinstance(v, torch.Tensor) and v.dtype == torch.float32 for v in out.values())
    means = O.inverse_log_transform(arrays["means"])
    # d expm1(|y|) = exp(|y|) dy: the log-space bar times 1 + |x|
    bar = O.half_step(meta["means"]["mins"], meta["means"]["maxs"], 16) * (1 + np.abs(means)) \
        * (1 + 1e-3) + 8 * 2.0 ** -23 * np.abs(means)
    assert (np.abs(out["means"].numpy() - means) <= bar).all()


def test_constant_channel_and_empty_shN(tmp_path, codec):
    arrays, _, _ = _arrays(seed=3)
    arrays["scales"][:, 1] = -2.5
    arrays["opacities"][:] = 0.25
    arrays["shN"] = np.zeros((64, 0, 3), np.float32)
    d = str(tmp_path / "c")
    meta = C.write_arrays(d, arrays)
    assert set(meta["shN"]) == {"shape", "dtype"} and not os.path.exists(os.path.join(d, "shN.npz"))
    out = C.read_arrays(d)
    assert all(np.isfinite(v).all() for v in out.values())
    assert (out["scales"][:, 1] == np.float32(-2.5)).all()
    assert (out["opacities"] == np.float32(0.25)).all()
    assert (C.read_png(os.path.join(d, "opacities.png")) == 0).all()
    assert out["shN"].shape == (64, 0, 3)


def _splats(N, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"means": torch.randn(N, 3, generator=g) * 3, "scales": torch.randn(N, 3, generator=g),
            "quats": torch.randn(N, 4, generator=g), "opacities": torch.randn(N, generator=g),
            "sh0": torch.randn(N, 1, 3, generator=g), "shN": torch.randn(N, 15, 3, generator=g)}


def test_crop_keeps_the_highest_opacities_in_order():
    sp = _splats(70)
    out = C.PngCompression(use_sort=False, verbose=False).prepare(sp)
    gone = torch.argsort(sp["opacities"])[:6]
    keep = torch.ones(70, dtype=torch.bool)
    keep[gone] = False
    assert len(out["means"]) == 64
    for k in ("scales", "opacities", "sh0", "shN"):
        assert torch.equal(out[k], sp[k][keep]), k
    assert torch.equal(out["means"], torch.sign(sp["means"][keep])
                       * torch.log1p(sp["means"][keep].abs()))
    torch.testing.assert_close(out["quats"].norm(dim=-1), torch.ones(64))
    # sorted: the same Gaussians, permuted
    srt = C.PngCompression(use_sort=True, verbose=False).prepare(sp)
    assert torch.equal(torch.sort(srt["opacities"]).values, torch.sort(out["opacities"]).values)
    perm = C.morton_order(out["means"])
    assert torch.equal(srt["scales"], out["scales"][perm])


def test_callers_dict_is_unchanged():
    sp = _splats(70, seed=1)
    before = {k: v.clone() for k, v in sp.items()}
    ids = {k: id(v) for k, v in sp.items()}
    C.PngCompression(verbose=False).prepare(sp)
    assert list(sp) == list(before)
    for k in sp:
        assert id(sp[k]) == ids[k] and torch.equal(sp[k], before[k]), k


def test_compress_refuses_cpu_tensors(tmp_path):
    from gsplat_hip import _lib
    with pytest.raises(_lib.GsplatHipError):
        C.PngCompression(verbose=False).compress(str(tmp_path), _splats(16))
    with pytest.raises(_lib.GsplatHipError):
        C.kmeans_l1(torch.randn(10, 9))


# --------------------------------------------------------------------- Morton
def test_morton_ties_keep_index_order():
    base = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 0.2, 0.9], [0.2, 0.7, 0.1],
                     [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float32)
    pts = np.concatenate([base, base[::-1], base[[2, 2, 3]]])
    want = O.morton_order(pts)
    got = C.morton_order(torch.from_numpy(pts))
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    codes = O.morton_codes(pts)
    assert len(np.unique(codes)) < len(codes)  # the case has ties
    for a, b in zip(want[:-1], want[1:]):
        assert codes[a] < codes[b] or (codes[a] == codes[b] and a < b)
    # x is the lowest bit, z the highest of a triple
    assert list(O.morton_codes(base[[0, 4, 5, 6]]) >> 27) == [0, 1, 2, 4]


@pytest.fixture(scope="module")
def garden_log_means():
    from gsplat_hip.train_step import load_garden_scene
    means = load_garden_scene(os.path.join(GOLDEN, "garden_scene.npz"), scene_grid=1)[0]
    return C.log_transform(means[:10000].float())


def test_morton_matches_the_oracle_on_the_garden_scene(garden_log_means):
    got = C.morton_order(garden_log_means).numpy()
    assert np.array_equal(got, O.morton_order(garden_log_means.numpy()))


def test_sorted_means_grids_are_smaller(tmp_path, garden_log_means):
    """The two means PNGs of the Morton-sorted 100 x 100 grid against the
    unsorted ones: < 0.9 (measured with the numpy oracle and Pillow: 0.76; the
    margin is for another zlib -- the condition is only that sorting helps)."""
    x = garden_log_means.numpy()
    sizes = []
    for name, order in (("unsorted", np.arange(len(x))), ("sorted", O.morton_order(x))):
        d = str(tmp_path / name)
        C.write_arrays(d, {"means": x[order]})
        sizes.append(sum(os.path.getsize(os.path.join(d, f))
                         for f in ("means_l.png", "means_u.png")))
    print(f"means PNGs: unsorted {sizes[0]} B, sorted {sizes[1]} B, "
          f"ratio {sizes[1] / sizes[0]:.3f}")
    assert sizes[1] < 0.9 * sizes[0], sizes


# ------------------------------------------------------------- public surface
def test_public_surface():
    import dataclasses

    import gsplat_hip
    from gsplat_hip import _lib
    assert "PngCompression" in gsplat_hip.__all__
    assert gsplat_hip.PngCompression is C.PngCompression
    fields = {f.name: f.default for f in dataclasses.fields(C.PngCompression)}
    assert list(fields)[:2] == ["use_sort", "verbose"]
    assert fields["use_sort"] is True and fields["verbose"] is True
    assert all(f.default is not dataclasses.MISSING
               for f in dataclasses.fields(C.PngCompression))
    assert callable(C.PngCompression.compress) and callable(C.PngCompression.decompress)
    assert _lib.ABI_VERSION == 38
    for name in ("gsplat_hip_kmeans_l1_assign", "gsplat_hip_kmeans_update",
                 "gsplat_hip_kmeans_update_workspace_bytes"):
        assert name in _lib.EXPORTED
    from gsplat_hip.train_step import Trainer
    assert callable(Trainer.evaluate_compressed)
