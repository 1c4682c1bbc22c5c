"""Splat compression: gsplat/compression/png_compression.py's `PngCompression`
(`compression="png"` of examples/simple_trainer.py and its run_compression).

A trained scene leaves as a directory of PNG grids, one `shN.npz` and a
`meta.json`, in the reference's on-disk format file for file: its
`decompress` reads what `compress` writes here, and this `decompress` reads
what it writes.

* The parameters are quantised into `n x n` grids (`n = int(sqrt(N))`, the
  `N - n^2` lowest-opacity Gaussians are dropped): `means` -- after
  `sign(x) log1p(|x|)` -- to 16 bits split into `means_l.png` / `means_u.png`,
  `scales`, normalised `quats`, `opacities` and `sh0` to 8 bits, each over its
  per-channel min / max.
* The Gaussians are ordered so the grids are smooth and the PNG filters work
  (`morton_order`).  The reference sorts with PLAS, a randomised iterative
  grid sort from a package of its own; PLAS is NOT reproduced here.  In its
  place stands a deterministic 3-D Morton order of the log-transformed means,
  laid row-major into the grid.
* `shN` becomes up to 65,536 centroids (6 bits each) plus a 16-bit label per
  Gaussian: a k-means with a Manhattan-distance assignment and a mean update,
  both HIP kernels (csrc/compress.hip, `kmeans_l1`).  The reference hands this
  to torchpq's `KMeans(distance="manhattan")`; that library's iteration count,
  tolerance and initialisation are not reproduced: `max_iters=10`, `tol=1e-4`
  and the seeded `randperm` initialisation are this project's own defaults.

Three deliberate differences from the reference's `compress`: the caller's
dict is not modified (the reference overwrites `splats["means"]` /
`["quats"]`); a channel whose max equals its min quantises to zeros (the
reference divides by zero); an empty `shN` (degree 0) writes only its meta
entry.  Also, the Gaussians that survive the crop keep their order (the
reference leaves them in descending-opacity order); with `use_sort=False` the
files hold them in the caller's order.

PNG files go through Pillow when it imports (lazily, as the reference imports
its image library), else through a small `zlib` / `struct` codec for 8-bit
images of 1, 3 or 4 channels.
"""

import json
import os
import struct
import zlib
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._wrapper import _dev_check, _f32c, _ptr, _stream

MAX_CLUSTERS = 65536  # labels are stored as uint16
MAX_DIM = 72          # csrc/compress.hip's longest point row

# False forces the stdlib PNG codec even where Pillow imports
USE_PILLOW = True

_PNG_SIG = b"\x89PNG\r\n\x1a\n"
_COLOR_TYPE = {1: 0, 3: 2, 4: 6}  # channels -> PNG colour type (grey, RGB, RGBA)


# ------------------------------------------------------------------ PNG codec
def _pillow():
    if not USE_PILLOW:
        return None
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))


def png_encode(img: np.ndarray) -> bytes:
    """8-bit PNG of a uint8 [H,W], [H,W,1], [H,W,3] or [H,W,4] array with the
    "Up" filter on every row (the grids are smooth down a column too)."""
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError(f"png_encode: uint8 [H,W] or [H,W,C] expected, got {img.dtype} "
                         f"{img.shape}")
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    if ch not in _COLOR_TYPE or h < 1 or w < 1:
        raise ValueError(f"png_encode: 1, 3 or 4 channels and a non-empty image, got {img.shape}")
    rows = np.ascontiguousarray(img).reshape(h, w * ch)
    up = rows.copy()
    up[1:] -= rows[:-1]  # uint8 arithmetic wraps: the filter's modulo 256
    raw = np.concatenate([np.full((h, 1), 2, np.uint8), up], 1).tobytes()
    ihdr = struct.pack(">IIBBBBB", w, h, 8, _COLOR_TYPE[ch], 0, 0, 0)
    return (_PNG_SIG + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, 9))
            + _chunk(b"IEND", b""))


def png_decode(data: bytes) -> np.ndarray:
    """The inverse of png_encode: non-interlaced 8-bit grey / RGB / RGBA with
    the filters None, Sub and Up (what png_encode writes, and more is not
    claimed).  [H,W] for grey, else [H,W,C]."""
    if data[:8] != _PNG_SIG:
        raise ValueError("png_decode: not a PNG file")
    pos, idat, head = 8, [], None
    while pos + 8 <= len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        pos += 12 + n
    if head is None:
        raise ValueError("png_decode: no IHDR chunk")
    w, h, depth, ctype, _, _, interlace = head
    chans = {v: k for k, v in _COLOR_TYPE.items()}
    if depth != 8 or ctype not in chans or interlace != 0:
        raise ValueError(f"png_decode: only non-interlaced 8-bit grey / RGB / RGBA, got depth "
                         f"{depth}, colour type {ctype}, interlace {interlace}")
    ch = chans[ctype]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    if raw.size != h * (1 + w * ch):
        raise ValueError("png_decode: image data of the wrong length")
    raw = raw.reshape(h, 1 + w * ch)
    out = np.zeros((h, w * ch), np.uint8)
    prev = np.zeros(w * ch, np.uint8)
    for y in range(h):
        f, line = int(raw[y, 0]), raw[y, 1:]
        if f == 0:
            row = line
        elif f == 1:
            row = np.cumsum(line.reshape(w, ch), 0, dtype=np.uint8).reshape(-1)
        elif f == 2:
            row = line + prev
        else:
            raise ValueError(f"png_decode: filter type {f} is not supported")
        out[y] = prev = row
    return out.reshape(h, w) if ch == 1 else out.reshape(h, w, ch)


def write_png(path: str, img: np.ndarray) -> None:
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[:, :, 0]
    Image = _pillow()
    if Image is None:
        with open(path, "wb") as f:
            f.write(png_encode(img))
        return
    if img.dtype != np.uint8 or (img.ndim == 3 and img.shape[2] not in (3, 4)) or \
            img.ndim not in (2, 3):
        raise ValueError(f"write_png: uint8 image of 1, 3 or 4 channels expected, got "
                         f"{img.dtype} {img.shape}")
    Image.fromarray(np.ascontiguousarray(img)).save(path, format="PNG", compress_level=9)


def read_png(path: str) -> np.ndarray:
    Image = _pillow()
    if Image is None:
        with open(path, "rb") as f:
            return png_decode(f.read())
    with Image.open(path) as im:
        return np.array(im)


# -------------------------------------------------------- host stage (numpy)
def log_transform(x):
    """sign(x) log1p(|x|), numpy or torch (gsplat/utils.py log_transform)."""
    if isinstance(x, np.ndarray):
        return np.sign(x) * np.log1p(np.abs(x))
    return torch.sign(x) * torch.log1p(torch.abs(x))


def inverse_log_transform(y):
    if isinstance(y, np.ndarray):
        return np.sign(y) * np.expm1(np.abs(y))
    return torch.sign(y) * torch.expm1(torch.abs(y))


def _dtype_name(arr: np.ndarray) -> str:
    return str(arr.dtype)


def _quantize(values: np.ndarray, mins, maxs, bits: int) -> np.ndarray:
    """round((v - min) / (max - min) * (2^bits - 1)) in float64; 0 where
    max == min (the reference: 0 / 0)."""
    v = values.astype(np.float64)
    mins, maxs = np.asarray(mins, np.float64), np.asarray(maxs, np.float64)
    span = maxs - mins
    norm = (v - mins) / np.where(span > 0, span, 1.0)
    norm = np.where(span > 0, norm, 0.0)
    return np.round(norm * (2 ** bits - 1))


def _dequantize(q: np.ndarray, mins, maxs, bits: int) -> np.ndarray:
    """The reference's q / (2^bits - 1) * (maxs - mins) + mins, in float64."""
    mins, maxs = np.asarray(mins, np.float64), np.asarray(maxs, np.float64)
    return q / (2 ** bits - 1) * (maxs - mins) + mins


def _write_grid(compress_dir, name, arr, n, bits):
    meta = {"shape": list(arr.shape), "dtype": _dtype_name(arr)}
    if arr.size == 0:
        return meta
    grid = arr.reshape(n, n, -1)
    mins, maxs = grid.min((0, 1)), grid.max((0, 1))
    q = _quantize(grid, mins, maxs, bits)
    if bits == 8:
        write_png(os.path.join(compress_dir, f"{name}.png"), q.astype(np.uint8))
    else:
        q = q.astype(np.uint16)
        write_png(os.path.join(compress_dir, f"{name}_l.png"), (q & 0xFF).astype(np.uint8))
        write_png(os.path.join(compress_dir, f"{name}_u.png"), (q >> 8).astype(np.uint8))
    meta["mins"], meta["maxs"] = mins.tolist(), maxs.tolist()
    return meta


def _read_grid(compress_dir, name, meta, bits):
    dtype = np.dtype(meta["dtype"])
    if not np.all(meta["shape"]):
        return np.zeros(meta["shape"], dtype)
    if bits == 8:
        q = read_png(os.path.join(compress_dir, f"{name}.png")).astype(np.float64)
    else:
        lo = read_png(os.path.join(compress_dir, f"{name}_l.png")).astype(np.uint16)
        hi = read_png(os.path.join(compress_dir, f"{name}_u.png")).astype(np.uint16)
        q = ((hi << 8) + lo).astype(np.float64)
    n = q.shape[0]
    grid = _dequantize(q.reshape(n, n, -1), meta["mins"], meta["maxs"], bits)
    return grid.reshape(meta["shape"]).astype(dtype)


def _write_kmeans(compress_dir, name, arr, centroids, labels, quantization=6):
    meta = {"shape": list(arr.shape), "dtype": _dtype_name(arr)}
    if arr.size == 0:
        return meta
    if centroids is None or labels is None:
        raise ValueError(f"{name}: a non-empty array needs its (centroids, labels)")
    centroids = np.asarray(centroids)
    labels = np.asarray(labels)
    if labels.shape != (arr.shape[0],) or centroids.ndim != 2 or \
            centroids.shape[1] != arr.size // arr.shape[0]:
        raise ValueError(f"{name}: centroids {centroids.shape} / labels {labels.shape} do not "
                         f"fit {arr.shape}")
    if centroids.shape[0] > MAX_CLUSTERS or labels.min() < 0 or \
            labels.max() >= centroids.shape[0]:
        raise ValueError(f"{name}: labels outside the {centroids.shape[0]} centroids, or more "
                         f"than {MAX_CLUSTERS} of them")
    mins, maxs = centroids.min(), centroids.max()
    q = _quantize(centroids, mins, maxs, quantization).astype(np.uint8)
    np.savez_compressed(os.path.join(compress_dir, f"{name}.npz"), centroids=q,
                        labels=labels.astype(np.uint16))
    meta.update(mins=float(mins), maxs=float(maxs), quantization=quantization)
    return meta


def _read_kmeans(compress_dir, name, meta):
    dtype = np.dtype(meta["dtype"])
    if not np.all(meta["shape"]):
        return np.zeros(meta["shape"], dtype)
    with np.load(os.path.join(compress_dir, f"{name}.npz")) as z:
        q, labels = z["centroids"], z["labels"]
    centroids = _dequantize(q.astype(np.float64), meta["mins"], meta["maxs"],
                            meta["quantization"])
    return centroids[labels].reshape(meta["shape"]).astype(dtype)


def _write_npz(compress_dir, name, arr):
    np.savez_compressed(os.path.join(compress_dir, f"{name}.npz"), arr=arr)
    return {"shape": list(arr.shape), "dtype": _dtype_name(arr)}


def _read_npz(compress_dir, name, meta):
    with np.load(os.path.join(compress_dir, f"{name}.npz")) as z:
        arr = z["arr"]
    return arr.reshape(meta["shape"]).astype(np.dtype(meta["dtype"]))


_GRID_BITS = {"means": 16, "scales": 8, "quats": 8, "opacities": 8, "sh0": 8}


def write_arrays(compress_dir: str, arrays: Dict[str, np.ndarray], shn_clusters=None) -> dict:
    """The host stage of `compress`: numpy arrays of n^2 Gaussians, already
    transformed (log means, unit quats), cropped and ordered, to the files and
    `meta.json`.  `shn_clusters`: the (centroids [K,D], labels [N]) of
    `arrays["shN"]`.  Returns the meta dict."""
    os.makedirs(compress_dir, exist_ok=True)
    count = len(arrays["means"])
    n = int(count ** 0.5)
    if n * n != count:
        raise ValueError(f"write_arrays: {count} Gaussians are no square grid")
    meta = {}
    for name, arr in arrays.items():
        arr = np.asarray(arr)
        if len(arr) != count:
            raise ValueError(f"write_arrays: {name} has {len(arr)} rows, means {count}")
        if name in _GRID_BITS:
            meta[name] = _write_grid(compress_dir, name, arr, n, _GRID_BITS[name])
        elif name == "shN":
            cents, labels = shn_clusters if shn_clusters is not None else (None, None)
            meta[name] = _write_kmeans(compress_dir, name, arr, cents, labels)
        else:
            meta[name] = _write_npz(compress_dir, name, arr)
    with open(os.path.join(compress_dir, "meta.json"), "w") as f:
        json.dump(meta, f)
    return meta


def read_arrays(compress_dir: str) -> Dict[str, np.ndarray]:
    """The files of a compressed directory back to numpy arrays; `means` are
    still log-transformed."""
    with open(os.path.join(compress_dir, "meta.json"), "r") as f:
        meta = json.load(f)
    out = {}
    for name, m in meta.items():
        if name in _GRID_BITS:
            out[name] = _read_grid(compress_dir, name, m, _GRID_BITS[name])
        elif name == "shN":
            out[name] = _read_kmeans(compress_dir, name, m)
        else:
            out[name] = _read_npz(compress_dir, name, m)
    return out


def crop_indices(opacities, n_keep: int):
    """Indices, ascending, of the `n_keep` highest opacities (a tie at the cut
    keeps the lower index).  numpy or torch."""
    if isinstance(opacities, np.ndarray):
        order = np.argsort(-opacities.reshape(-1), kind="stable")
        return np.sort(order[:n_keep])
    order = torch.sort(opacities.reshape(-1), descending=True, stable=True).indices
    return torch.sort(order[:n_keep]).values


# ------------------------------------------------------------- Morton order
def morton_order(means_log: Tensor) -> Tensor:
    """The order that lays the Gaussians into the n x n grid, row-major: a
    stable argsort of the 30-bit Morton code of the log-transformed means
    [N,3], each axis quantised to 10 bits over its min-max as
    floor(t * 1023.999) (float64), x in the lowest bit.  Ties keep index order.

    It stands in for the reference's PLAS sort (gsplat/compression/sort.py),
    which is randomised, lives in a package of its own and is not reproduced;
    any order decodes the same, the order only decides how well the PNGs
    deflate."""
    x = means_log.detach().double()
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError(f"morton_order: means [N,3] expected, got {tuple(x.shape)}")
    if x.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=x.device)
    lo, hi = x.amin(0), x.amax(0)
    span = hi - lo
    t = (x - lo) / torch.where(span > 0, span, torch.ones_like(span))
    q = torch.floor(t * 1023.999).clamp_(0, 1023).to(torch.int64)
    code = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    for b in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> b) & 1) << (3 * b + axis)
    return torch.sort(code, stable=True).indices


# ------------------------------------------------------------------ k-means
def kmeans_assign(x: Tensor, centroids: Tensor, labels: Optional[Tensor] = None,
                  dist: Optional[Tensor] = None, n_changed: Optional[Tensor] = None) -> Tensor:
    """labels[i] = argmin_k sum_d |x[i,d] - centroids[k,d]| (int32 [N], lowest
    k on a tie), in place when `labels` is given; `dist` float32 [N] and
    `n_changed` int32 [1] (labels that differ from the incoming ones) are
    optional device outputs.  One HIP launch (two with n_changed)."""
    _dev_check(x, centroids, labels, dist, n_changed)
    N, D = x.shape
    K = centroids.shape[0]
    assert x.dtype == torch.float32 and x.is_contiguous(), "x: contiguous float32 [N,D]"
    assert centroids.dtype == torch.float32 and centroids.is_contiguous() and \
        centroids.shape == (K, D), "centroids: contiguous float32 [K,D]"
    if labels is None:
        labels = torch.full((N,), -1, dtype=torch.int32, device=x.device)
    assert labels.dtype == torch.int32 and labels.shape == (N,) and labels.is_contiguous()
    assert dist is None or (dist.dtype == torch.float32 and dist.shape == (N,)
                            and dist.is_contiguous())
    assert n_changed is None or (n_changed.dtype == torch.int32 and n_changed.numel() == 1)
    with torch.cuda.device(x.device):
        _lib.call("gsplat_hip_kmeans_l1_assign", N, K, D, _ptr(x), _ptr(centroids), _ptr(labels),
                  _ptr(dist), _ptr(n_changed), _stream())
    return labels


def kmeans_update(x: Tensor, labels: Tensor, centroids: Tensor, counts: Optional[Tensor] = None,
                  workspace: Optional[Tensor] = None) -> Tensor:
    """centroids[k] <- the mean of the rows of x labelled k, in place (a
    centroid without members keeps its value); returns the member counts
    int32 [K].  Bit-reproducible (no float atomics)."""
    _dev_check(x, labels, centroids, counts, workspace)
    N, D = x.shape
    K = centroids.shape[0]
    assert x.dtype == torch.float32 and x.is_contiguous(), "x: contiguous float32 [N,D]"
    assert centroids.dtype == torch.float32 and centroids.is_contiguous() and \
        centroids.shape == (K, D), "centroids: contiguous float32 [K,D]"
    assert labels.dtype == torch.int32 and labels.shape == (N,) and labels.is_contiguous()
    if counts is None:
        counts = torch.empty(K, dtype=torch.int32, device=x.device)
    assert counts.dtype == torch.int32 and counts.shape == (K,) and counts.is_contiguous()
    if workspace is None:
        workspace = kmeans_workspace(N, x.device)
    with torch.cuda.device(x.device):
        _lib.call("gsplat_hip_kmeans_update", N, K, D, _ptr(x), _ptr(labels), _ptr(centroids),
                  _ptr(counts), _ptr(workspace), _stream())
    return counts


def kmeans_workspace(N: int, device) -> Tensor:
    nbytes = int(_lib.query("gsplat_hip_kmeans_update_workspace_bytes", N))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def lloyd(x: Tensor, centroids: Tensor, max_iters: int, tol: float):
    """The loop of kmeans_l1 from given centroids (updated in place):
    (centroids, labels int32, iterations run).  An iteration is an assignment
    then an update; the host reads the changed-label counter once per
    iteration and stops when changed / N < tol."""
    N = x.shape[0]
    labels = torch.full((N,), -1, dtype=torch.int32, device=x.device)
    changed = torch.zeros(1, dtype=torch.int32, device=x.device)
    counts = torch.empty(centroids.shape[0], dtype=torch.int32, device=x.device)
    ws = kmeans_workspace(N, x.device)
    iters = 0
    for _ in range(int(max_iters)):
        kmeans_assign(x, centroids, labels, n_changed=changed)
        kmeans_update(x, labels, centroids, counts, ws)
        iters += 1
        if int(changed.item()) / N < tol:
            break
    return centroids, labels, iters


def kmeans_l1(x: Tensor, n_clusters: int = 65536, max_iters: int = 10, tol: float = 1e-4,
              seed: int = 0, init: Optional[Tensor] = None):
    """k-means of the rows of x [N,D] (device float32, D <= 72) with a
    Manhattan-distance assignment and a mean update: (centroids [K,D], labels
    int64 [N]), K = min(n_clusters, N).

    Initial centroids: the rows `torch.randperm(N, generator=Generator().
    manual_seed(seed))[:K]` of x, or `init` [K,D].  At most `max_iters`
    iterations (assign, update); stops early once fewer than `tol * N` labels
    changed.  The labels are those of the last assignment, i.e. against the
    centroids before the last update.  Deterministic: the same input and seed
    give the same bits.

    `max_iters` and `tol` are this project's own defaults.  The reference's
    clustering (torchpq `KMeans(n_clusters, distance="manhattan")`) brings its
    iteration count, tolerance and initialisation from that library, which are
    not reproduced here."""
    _dev_check(x, init)
    if x.ndim != 2 or x.shape[0] < 1 or not 1 <= x.shape[1] <= MAX_DIM:
        raise ValueError(f"kmeans_l1: x [N >= 1, 1 <= D <= {MAX_DIM}] expected, got "
                         f"{tuple(x.shape)}")
    if not 1 <= int(n_clusters) <= MAX_CLUSTERS:
        raise ValueError(f"kmeans_l1: n_clusters {n_clusters} outside [1, {MAX_CLUSTERS}] "
                         "(labels are stored as uint16)")
    x = _f32c(x.detach())
    N, D = x.shape
    K = min(int(n_clusters), N)
    if init is None:
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:K]
        centroids = x[perm.to(x.device)].contiguous()
    else:
        if tuple(init.shape) != (K, D):
            raise ValueError(f"kmeans_l1: init {tuple(init.shape)}, expected {(K, D)}")
        centroids = _f32c(init.detach()).clone()
    centroids, labels, _ = lloyd(x, centroids, max_iters, tol)
    return centroids, labels.to(torch.int64)


# ------------------------------------------------------------ PngCompression
@dataclass
class PngCompression:
    """gsplat.compression.PngCompression: quantised, sorted PNG grids and a
    k-means codebook for `shN` (the module docstring has the format and the
    differences).  `use_sort` / `verbose` are the reference's fields; the
    others are this project's: `n_clusters` (at most 65,536), `kmeans_iters`
    and `kmeans_tol` of `kmeans_l1`, and its `seed`.

    `compress` takes the pre-activation parameters `means`, `scales`, `quats`,
    `opacities`, `sh0`, `shN` on the GPU; any further key is stored with
    numpy's NPZ compression.  `decompress` returns CPU tensors, as the
    reference's."""

    use_sort: bool = True
    verbose: bool = True
    n_clusters: int = 65536
    kmeans_iters: int = 10
    kmeans_tol: float = 1e-4
    seed: int = 0

    def prepare(self, splats: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """The splats as the files hold them, in a new dict: log-transformed
        means, unit quats, cropped to n^2 and ordered.  Plain torch on the
        tensors' device."""
        splats = {k: v.detach() for k, v in splats.items()}  # the caller's dict stays
        splats["means"] = log_transform(splats["means"])
        splats["quats"] = torch.nn.functional.normalize(splats["quats"], dim=-1)
        n_gs = len(splats["means"])
        n = int(n_gs ** 0.5)
        order = None
        if n * n != n_gs:
            order = crop_indices(splats["opacities"], n * n)
            if self.verbose:
                print(f"PngCompression: {n_gs} Gaussians fill a {n} x {n} grid; the "
                      f"{n_gs - n * n} of lowest opacity are dropped")
        if self.use_sort:
            kept = splats["means"] if order is None else splats["means"][order]
            perm = morton_order(kept)
            order = perm if order is None else order[perm]
        if order is not None:
            splats = {k: v[order] for k, v in splats.items()}
        return splats

    def compress(self, compress_dir: str, splats: Dict[str, Tensor]) -> None:
        _dev_check(*splats.values())
        splats = self.prepare(splats)
        clusters = None
        shn = splats.get("shN")
        if shn is not None and shn.numel() > 0:
            cents, labels = kmeans_l1(shn.reshape(shn.shape[0], -1), self.n_clusters,
                                      self.kmeans_iters, self.kmeans_tol, self.seed)
            clusters = (cents.cpu().numpy(), labels.cpu().numpy())
        write_arrays(compress_dir, {k: v.cpu().numpy() for k, v in splats.items()}, clusters)

    def decompress(self, compress_dir: str) -> Dict[str, Tensor]:
        splats = {k: torch.from_numpy(v) for k, v in read_arrays(compress_dir).items()}
        splats["means"] = inverse_log_transform(splats["means"])
        return splats
