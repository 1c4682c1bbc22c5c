"""Splats to and from PLY files in the INRIA layout, the format the
reference's `save_ply` writes (gsplat/utils.py:10-98) and every 3DGS viewer
and editor reads.

    save_ply(splats, dir, colors=None)   the reference's names and order
    load_ply(path, device=None)          the same dict back

A vertex is one row of little-endian float32,

    x y z | nx ny nz (zeros) | f_dc_0..2 | f_rest_0..3(K-1)-1 | opacity |
    scale_0..2 | rot_0..3

the SH coefficients channel-major (`sh0.transpose(0, 2, 1)`,
`shN.transpose(0, 2, 1)`, flattened); with `colors` there is no f_rest and
f_dc_j = (colors[:, j] - 0.5) / 0.2820947917738781 in float32.  Rows with a
NaN or Inf in any value of the file row are dropped, the rest keep their order.

Tensors on the GPU are packed by csrc/ply.hip (validity and per-workgroup
counts, the exclusive scan, the pack into rows) in chunks of `chunk_rows`
source rows through one device staging buffer and one pinned host buffer;
tensors on the CPU take a vectorised numpy path that writes the same bytes.
There is no torch fallback of the device path.

Two deliberate differences from the reference's save_ply:
  * it tests `opacities` with `.any(axis=0)`, so one non-finite opacity empties
    the whole file; here the test is per row;
  * it filters the parameter rows but indexes `colors` unfiltered, so after the
    first dropped row the colours belong to the wrong Gaussians; here `colors`
    is filtered with the rows (and a non-finite colour drops its row).  With
    `colors`, sh0 / shN are not part of the file and are not read.
"""

import math
import os

import numpy as np
import torch

from . import _lib

C0 = 0.2820947917738781  # SH band 0
_FIXED = ("x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2")
_TAIL = ("opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")
_FLOAT = ("float", "float32")


def _header(n, n_rest):
    """The reference's header (utils.py:49-77) for n vertices."""
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    names += [f"f_rest_{j}" for j in range(n_rest)]
    names += list(_TAIL)
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    lines += [f"property float {k}" for k in names]
    lines.append("end_header")
    return ("\n".join(lines) + "\n").encode()


def _fields(splats, colors):
    """The tensors of `splats` (anything with .items()) checked and detached:
    (dict, N, K - 1)."""
    d = {k: (v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(v))
         for k, v in splats.items()}
    need = ["means", "scales", "quats", "opacities"] + ([] if colors is not None
                                                        else ["sh0", "shN"])
    for k in need:
        if k not in d:
            raise KeyError(f"save_ply: splats has no {k!r}")
    N = d["means"].shape[0]
    shapes = {"means": (N, 3), "scales": (N, 3), "quats": (N, 4), "opacities": (N,)}
    K1 = 0
    if colors is None:
        shN = d["shN"]
        if shN.dim() != 3 or shN.shape[0] != N or shN.shape[2] != 3:
            raise ValueError(f"save_ply: shN must be [N, K-1, 3], got {tuple(shN.shape)}")
        K1 = int(shN.shape[1])
        shapes.update(sh0=(N, 1, 3), shN=(N, K1, 3))
    else:
        colors = colors.detach() if isinstance(colors, torch.Tensor) else torch.as_tensor(colors)
        d["colors"] = colors
        shapes["colors"] = (N, 3)
    out = {}
    for k, shp in shapes.items():
        if tuple(d[k].shape) != shp:
            raise ValueError(f"save_ply: {k} must be {list(shp)}, got {list(d[k].shape)}")
        out[k] = d[k]
    return out, N, K1


def _rows_numpy(f, a, b):
    """The file rows [b - a, F] of source rows a..b, before the filter."""
    n = b - a
    cols = [f["means"][a:b], np.zeros((n, 3), np.float32)]
    if "colors" in f:
        # the constant rounded to fp32, an fp32 subtract, an fp32 divide
        cols.append((f["colors"][a:b] - np.float32(0.5)) / np.float32(C0))
    else:
        cols.append(f["sh0"][a:b].transpose(0, 2, 1).reshape(n, -1))
        cols.append(f["shN"][a:b].transpose(0, 2, 1).reshape(n, -1))
    cols += [f["opacities"][a:b, None], f["scales"][a:b], f["quats"][a:b]]
    return np.concatenate(cols, axis=1).astype("<f4", copy=False)


def _save_numpy(f, N, K1, path, chunk_rows):
    f = {k: np.ascontiguousarray(v.cpu().numpy(), dtype=np.float32) for k, v in f.items()}
    spans = [(a, min(a + chunk_rows, N)) for a in range(0, N, chunk_rows)]
    with np.errstate(over="ignore", invalid="ignore"):
        # the count first (the header names it), then the rows chunk by chunk
        n_valid = sum(int(np.isfinite(_rows_numpy(f, a, b)).all(axis=1).sum()) for a, b in spans)
        with open(path, "wb") as fh:
            fh.write(_header(n_valid, 3 * K1))
            for a, b in spans:
                rows = _rows_numpy(f, a, b)
                fh.write(rows[np.isfinite(rows).all(axis=1)].tobytes())
    return n_valid


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _save_device(f, N, K1, path, chunk_rows):
    from ._wrapper import _stream
    dev = f["means"].device
    f = {k: v.to(dev, torch.float32).contiguous() for k, v in f.items()}
    F = 17 + 3 * K1
    spans = [(a, min(a + chunk_rows, N)) for a in range(0, N, chunk_rows)]
    names = ("means", "scales", "quats", "opacities", "sh0", "shN", "colors")

    def args(a, b):
        return [b - a, K1] + [_ptr(f[k][a:b]) if k in f else 0 for k in names]

    with torch.cuda.device(dev):
        # a workspace per chunk (a byte per row and 8 per 256 rows): the counts
        # of every chunk first, one host read, then the header
        ws_bytes = [int(_lib.query("gsplat_hip_ply_workspace_bytes", b - a)) for a, b in spans]
        ws_off = np.concatenate([[0], np.cumsum(ws_bytes)]).astype(np.int64)
        ws = torch.empty(int(ws_off[-1]) + 16, dtype=torch.uint8, device=dev)
        base = ws.data_ptr() + (-ws.data_ptr()) % 16
        counts = torch.zeros(max(len(spans), 1), dtype=torch.int64, device=dev)
        for i, (a, b) in enumerate(spans):
            _lib.call("gsplat_hip_ply_count", *args(a, b), base + int(ws_off[i]),
                      counts.data_ptr() + 8 * i, _stream())
        n_chunk = [int(c) for c in counts.cpu()[:len(spans)]]
        rows_max = max(n_chunk, default=0)
        if rows_max:  # the two buffers of the whole call
            stage = torch.empty(rows_max * F, dtype=torch.float32, device=dev)
            pinned = torch.empty(rows_max * F, dtype=torch.float32, pin_memory=True)
            host = pinned.numpy()
        with open(path, "wb") as fh:
            fh.write(_header(sum(n_chunk), 3 * K1))
            for i, (a, b) in enumerate(spans):
                nv = n_chunk[i]
                if nv == 0:
                    continue
                _lib.call("gsplat_hip_ply_pack", *args(a, b), base + int(ws_off[i]),
                          stage.data_ptr(), _stream())
                pinned[:nv * F].copy_(stage[:nv * F], non_blocking=True)
                torch.cuda.current_stream().synchronize()
                fh.write(host[:nv * F].data)
    return sum(n_chunk)


def save_ply(splats, dir, colors=None, chunk_rows=1 << 20):
    """Write the Gaussians `splats` to the PLY file `dir` (the reference's
    parameter name for the path); returns the number of vertices written.

    splats: a dict (or anything with .items()) of the pre-activation
        parameters means [N,3], scales [N,3], quats [N,4], opacities [N],
        sh0 [N,1,3], shN [N,K-1,3] (K-1 = 0 allowed)
    colors: [N,3] in [0, 1]: written as f_dc instead of sh0 / shN (no f_rest)
    chunk_rows: source rows per pass of the device path's staging buffers (and
        of the numpy path's temporaries)

    Where `means` is on the GPU every tensor goes through the HIP kernels,
    otherwise through numpy; the bytes are the same."""
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError(f"save_ply: chunk_rows must be >= 1, got {chunk_rows}")
    f, N, K1 = _fields(splats, colors)
    if K1 > 24:
        raise ValueError(f"save_ply: shN holds {K1} coefficients, at most 24 (degree 4)")
    if f["means"].is_cuda:
        return _save_device(f, N, K1, dir, chunk_rows)
    if any(v.is_cuda for v in f.values()):
        raise ValueError("save_ply: means is on the CPU, another tensor on the GPU")
    return _save_numpy(f, N, K1, dir, chunk_rows)


def _parse_header(fh, path):
    """(vertex count, property names in file order, data offset)."""
    def bad(line, why):
        raise ValueError(f"load_ply: {path}: {why}: {line!r}")

    lines = []
    while True:
        raw = fh.readline()
        if not raw:
            raise ValueError(f"load_ply: {path}: no end_header line")
        line = raw.decode("ascii", errors="replace").rstrip("\r\n")
        lines.append(line)
        if line.strip() == "end_header":
            break
        if len(lines) > 4096:
            raise ValueError(f"load_ply: {path}: no end_header within 4096 lines")
    if lines[0].strip() != "ply":
        bad(lines[0], "not a PLY file")
    n, props, fmt = None, [], False
    for line in lines[1:-1]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            if tok[1:] != ["binary_little_endian", "1.0"]:
                bad(line, "only binary_little_endian 1.0 is read")
            fmt = True
        elif tok[0] == "element":
            if len(tok) != 3 or tok[1] != "vertex" or n is not None or not tok[2].isdigit():
                bad(line, "one `element vertex <count>` is read")
            n = int(tok[2])
        elif tok[0] == "property":
            if n is None:
                bad(line, "a property before `element vertex`")
            if len(tok) != 3 or tok[1] not in _FLOAT:
                bad(line, "only float properties are read")
            if tok[2] in props:
                bad(line, "a property named twice")
            props.append(tok[2])
        else:
            bad(line, "unknown header line")
    if not fmt:
        bad(lines[1] if len(lines) > 1 else "", "no format line")
    if n is None:
        bad(lines[-1], "no `element vertex` line")
    return n, props, fh.tell()


def _columns(props, path):
    """(K - 1, the column of each named property in the kernels' order:
    x y z, f_dc_0..2, f_rest_0.., opacity, scale_0..2, rot_0..3)."""
    rest = [p for p in props if p.startswith("f_rest_")]
    R = len(rest)
    K = R // 3 + 1
    if R % 3 or math.isqrt(K) ** 2 != K or K > 25:
        raise ValueError(f"load_ply: {path}: {R} f_rest properties, not 3 (K - 1) with K a "
                         f"square <= 25: {'property float ' + rest[-1]!r}")
    want = list(_FIXED) + [f"f_rest_{j}" for j in range(R)] + list(_TAIL)
    for k in want:
        if k not in props:
            raise ValueError(f"load_ply: {path}: no line 'property float {k}'")
    return K - 1, [props.index(k) for k in want]


def load_ply(path, device=None):
    """The dict `save_ply` takes, from a `binary_little_endian 1.0` PLY of
    float properties addressed by name (any order; others, such as nx ny nz,
    are ignored): means [N,3], scales [N,3], quats [N,4], opacities [N],
    sh0 [N,1,3], shN [N,K-1,3] with K from the number of f_rest_*.  Files of the
    INRIA trainer load through the same path.  `device`: None or "cpu" for CPU
    tensors (numpy), a GPU for the HIP unpack kernel.  Anything else in the
    header raises ValueError naming the line."""
    with open(path, "rb") as fh:
        n, props, off = _parse_header(fh, path)
        K1, cols = _columns(props, path)
        F = len(props)
        size = os.path.getsize(path) - off
        if size < 4 * F * n:
            raise ValueError(f"load_ply: {path}: {size} data bytes, 'element vertex {n}' of {F} "
                             f"floats needs {4 * F * n}")
        dev = torch.device("cpu" if device is None else device)
        if dev.type == "cpu":
            rows = np.fromfile(fh, dtype="<f4", count=n * F).reshape(n, F)
            return _unpack_numpy(rows, n, K1, cols)
        return _unpack_device(fh, n, K1, F, cols, dev)


def _unpack_numpy(rows, n, K1, cols):
    c = np.asarray(cols)
    g = lambda a, b: np.ascontiguousarray(rows[:, c[a:b]], dtype=np.float32)  # noqa: E731
    R = 3 * K1
    out = {"means": g(0, 3), "scales": g(7 + R, 10 + R), "quats": g(10 + R, 14 + R),
           "opacities": g(6 + R, 7 + R).reshape(n),
           "sh0": g(3, 6).reshape(n, 3, 1).transpose(0, 2, 1),
           "shN": g(6, 6 + R).reshape(n, 3, K1).transpose(0, 2, 1)}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


def _unpack_device(fh, n, K1, F, cols, dev, chunk_rows=1 << 20):
    from ._wrapper import _stream
    assert all(0 <= c < F for c in cols)
    with torch.cuda.device(dev):
        shapes = {"means": (n, 3), "scales": (n, 3), "quats": (n, 4), "opacities": (n,),
                  "sh0": (n, 1, 3), "shN": (n, K1, 3)}
        out = {k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items()}
        if n == 0:
            return out
        cols_dev = torch.tensor(cols, dtype=torch.int32, device=dev)
        m = min(chunk_rows, n)
        stage = torch.empty(m * F, dtype=torch.float32, device=dev)
        pinned = torch.empty(m * F, dtype=torch.float32, pin_memory=True)
        host = pinned.numpy()
        for a in range(0, n, m):
            b = min(a + m, n)
            got = fh.readinto(memoryview(host[:(b - a) * F]).cast("B"))
            if got != 4 * (b - a) * F:
                raise ValueError(f"load_ply: short read at vertex {a}")
            stage[:(b - a) * F].copy_(pinned[:(b - a) * F], non_blocking=True)
            _lib.call("gsplat_hip_ply_unpack", b - a, K1, F, stage.data_ptr(),
                      cols_dev.data_ptr(),
                      *[_ptr(out[k][a:b]) for k in ("means", "scales", "quats", "opacities",
                                                    "sh0")],
                      _ptr(out["shN"][a:b]) if K1 else 0, _stream())
            torch.cuda.current_stream().synchronize()  # the buffers are reused
    return out
