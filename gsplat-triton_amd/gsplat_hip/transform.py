"""Similarity transforms of splat scenes (csrc/transform.hip): move a trained
scene, or segments of it, by x' = A x + t with A = s R, s > 0 and R a proper
rotation.  The reference has no counterpart.

For the pre-activation parameter dict used everywhere in this package:

    means'  = A means + t
    quats'  = q_R (x) quats      (wxyz; the raw parameter, its norm is kept)
    scales' = scales + log s     (all three columns, 2DGS dicts included)
    shN'    : per degree l = 1..L and colour channel, the 2l+1 coefficients are
              multiplied by M_l(R), where  sum_k a'_k Y_k(d) = sum_k a_k Y_k(R^T d)
              for every unit d, Y the basis of csrc/sh_basis.h.  The `dirs` of
              `spherical_harmonics` are means - campos in the world frame, so
              the moved scene seen from the moved camera shows the same colour.
    sh0, opacities and every other key pass through as the same tensor objects.

M_l(R) = Y_l(P_l)^-1 Y_l(P_l R) for a fixed direction set P_l (rows); R is the
polar factor of A / s, so a matrix that is a rotation only to rounding gives
orthogonal blocks.  On the GPU a prepare kernel writes one float32 record per
segment (computed in float64) and a streaming kernel applies it; CPU tensors
(`load_ply(device=None)`, `PngCompression.decompress`) take a torch path here,
float64 throughout and rounded to float32 once.  GPU and CPU tensors mixed in
one dict raise GsplatHipError.

There is no autograd: this is an editing and export operation.  Out of scope:
rotating Adam moments or moving a live trainer in place (second moments do not
rotate), non-uniform scale or shear, cropping (a boolean index), and moving an
extracted mesh (`colmap.transform_points` on its vertices).
"""

import functools
import math

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._wrapper import _ptr, _stream

HEADER_FLOATS = 20            # A[9], t[3], q_R[4], log s, s, 2 unused
BLOCK_FLOATS = (0, 9, 34, 83, 164)
SIMILARITY_TOL = 1e-4         # max|A^T A / s^2 - I|
STATUS_REFLECTION = 1
STATUS_NOT_SIMILARITY = 2
_DEG_OF_WIDTH = {0: 0, 3: 1, 8: 2, 15: 3, 24: 4}
_GEOM_KEYS = ("means", "quats", "scales")


def record_floats(sh_degree: int) -> int:
    return HEADER_FLOATS + BLOCK_FLOATS[sh_degree]


# ------------------------------------------------------------ float64 algebra
def sh_basis64(dirs: Tensor, sh_degree: int) -> Tensor:
    """The basis of csrc/sh_basis.h at unit `dirs` [..., 3] in the dtype of
    `dirs` (float64 here): [..., (sh_degree + 1)^2]."""
    x, y, z = dirs.unbind(-1)
    B = [torch.full_like(x, 0.28209479177387814)]
    if sh_degree >= 1:
        C1 = 0.4886025119029199
        B += [-C1 * y, C1 * z, -C1 * x]
    if sh_degree >= 2:
        zz = z * z
        g2, h2 = 2 * x * y, x * x - y * y
        C22 = 0.5462742152960396
        c21 = -1.0925484305920792 * z
        B += [C22 * g2, c21 * y, 0.9461746957575601 * zz - 0.3153915652525201, c21 * x, C22 * h2]
    if sh_degree >= 3:
        g3, h3 = x * g2 + y * h2, x * h2 - y * g2
        C33, C32 = -0.5900435899266435, 1.445305721320277
        c31 = -2.285228997322329 * zz + 0.4570457994644658
        B += [C33 * g3, C32 * g2 * z, c31 * y, z * (1.865881662950577 * zz - 1.119528997770346),
              c31 * x, C32 * h2 * z, C33 * h3]
    if sh_degree >= 4:
        g4, h4 = x * g3 + y * h3, x * h3 - y * g3
        C44, C43 = 0.6258357354491761, -1.7701307697799304
        c41 = z * (-4.683325804901024 * zz + 2.0071396306718676)
        c42 = 3.31161143515146 * zz - 0.47308734787878
        B += [C44 * g4, C43 * g3 * z, c42 * g2, c41 * y,
              zz * (3.7024941420321507 * zz - 3.1735664074561294) + 0.31735664074561293,
              c41 * x, c42 * h2, C43 * h3 * z, C44 * h4]
    return torch.stack(B, -1)


@functools.lru_cache(maxsize=None)
def _host_fit(l: int):
    """(P [64,3], pinv(Y_l(P)) [2l+1, 64]) for a 64-point Fibonacci lattice."""
    i = torch.arange(64, dtype=torch.float64) + 0.5
    z = 1 - 2 * i / 64
    phi = i * (math.pi * (3 - math.sqrt(5)))
    r = (1 - z * z).sqrt()
    P = torch.stack([r * phi.cos(), r * phi.sin(), z], -1)
    Y = sh_basis64(P, l)[:, l * l:]
    return P, torch.linalg.pinv(Y)


def _host_blocks(R: Tensor, sh_degree: int):
    """M_l(R) for rotations R [S,3,3] float64: a list of [S, 2l+1, 2l+1]."""
    out = []
    for l in range(1, sh_degree + 1):
        P, pinv = _host_fit(l)
        Yr = sh_basis64(P @ R, l)[..., l * l:]   # rows p^T R = (R^T p)^T
        out.append(pinv @ Yr)
    return out


def _rotmat_to_quat(R: Tensor) -> Tensor:
    """Unit wxyz quaternion of rotations [S,3,3] (Shepperd: the largest of
    the four squared components picks the formula)."""
    m = R
    tr = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    a, b, c = m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1]
    d, e, f = m[:, 0, 1] + m[:, 1, 0], m[:, 0, 2] + m[:, 2, 0], m[:, 1, 2] + m[:, 2, 1]
    cand = torch.stack([
        torch.stack([1 + tr, a, b, c], -1),
        torch.stack([a, 1 + 2 * m[:, 0, 0] - tr, d, e], -1),
        torch.stack([b, d, 1 + 2 * m[:, 1, 1] - tr, f], -1),
        torch.stack([c, e, f, 1 + 2 * m[:, 2, 2] - tr], -1)], 1)
    k = torch.stack([tr, m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]], -1).argmax(-1)
    q = cand[torch.arange(len(m)), k]
    return q / q.norm(dim=-1, keepdim=True)


def _quat_mul(a: Tensor, b: Tensor) -> Tensor:
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz,
                        aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw], -1)


def _decompose(T: Tensor):
    """Float64 [S,4,4] on the CPU -> dict(A, t, s, R, status, dev, det)."""
    A, t = T[:, :3, :3], T[:, :3, 3]
    det = torch.linalg.det(A)
    pos = det > 0
    s = torch.where(pos, det.abs().pow(1.0 / 3.0), torch.ones_like(det))
    Q = A / s[:, None, None]
    dev = (Q.transpose(1, 2) @ Q - torch.eye(3, dtype=T.dtype)).abs().amax((1, 2))
    status = (~pos).int() * STATUS_REFLECTION
    status = status | (~(dev <= SIMILARITY_TOL)).int() * STATUS_NOT_SIMILARITY
    Qs = torch.where((status == 0)[:, None, None], Q, torch.eye(3, dtype=T.dtype).expand_as(Q))
    U, _, Vh = torch.linalg.svd(Qs)
    return dict(A=A, t=t, s=s, R=U @ Vh, status=status, dev=dev, det=det)


def _status_message(what, i, det, dev):
    if not det > 0:
        return (f"{what}: segment {i}: det A = {det:.6g} <= 0 (a reflection or a singular "
                "matrix is no similarity)")
    return (f"{what}: segment {i}: max|A^T A / s^2 - I| = {dev:.3g} > {SIMILARITY_TOL:g} "
            "(non-uniform scale or shear)")


def _raise_first_bad(what, status, T_of):
    """`status`: CPU int tensor [S]; T_of(i): that segment's float64 [4,4]."""
    bad = torch.nonzero(status)
    if bad.numel():
        i = int(bad[0])
        d = _decompose(T_of(i)[None].double().cpu())
        raise ValueError(_status_message(what, i, float(d["det"][0]), float(d["dev"][0])))


# ----------------------------------------------------------------- arguments
def _as_transforms(transforms, what, last=4):
    """-> (float64 tensor [S, last, last] on its own device, came_from_host)."""
    if isinstance(transforms, np.ndarray):
        transforms = torch.from_numpy(np.ascontiguousarray(transforms))
    if not isinstance(transforms, Tensor):
        transforms = torch.as_tensor(transforms)
    if transforms.requires_grad:
        raise NotImplementedError(f"{what}: transforms require grad; there is no autograd "
                                  "through a scene transform")
    if transforms.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: transforms must be float32 or float64, got {transforms.dtype}")
    if transforms.dim() == 2:
        transforms = transforms[None]
    if transforms.dim() != 3 or tuple(transforms.shape[1:]) != (last, last) or len(transforms) < 1:
        raise ValueError(f"{what}: transforms must be [{last},{last}] or [S,{last},{last}] with "
                         f"S >= 1, got {list(transforms.shape)}")
    return transforms.detach().double().contiguous(), not transforms.is_cuda


def _check_ids(segment_ids, N, device, what):
    if segment_ids is None:
        return None
    if not isinstance(segment_ids, Tensor) or segment_ids.dtype != torch.int64:
        raise ValueError(f"{what}: segment_ids must be an int64 tensor, got "
                         f"{getattr(segment_ids, 'dtype', type(segment_ids))}")
    if tuple(segment_ids.shape) != (N,):
        raise ValueError(f"{what}: segment_ids must be [{N}], got {list(segment_ids.shape)}")
    if segment_ids.device != device:
        raise _lib.GsplatHipError(f"{what}: segment_ids is on {segment_ids.device}, the "
                                  f"Gaussians on {device}")
    return segment_ids.contiguous()


def _sh_degree_of(shN, N, what):
    if shN is None:
        return 0
    if shN.dim() != 3 or shN.shape[0] != N or shN.shape[2] != 3:
        raise ValueError(f"{what}: shN must be [{N}, K-1, 3], got {list(shN.shape)}")
    if shN.shape[1] not in _DEG_OF_WIDTH:
        raise ValueError(f"{what}: shN holds {shN.shape[1]} coefficients, which is no degree "
                         f"(K-1 is one of {sorted(_DEG_OF_WIDTH)})")
    return _DEG_OF_WIDTH[shN.shape[1]]


def _same_device(tensors, what):
    devs = {str(t.device) for t in tensors if t is not None}
    if len(devs) > 1:
        raise _lib.GsplatHipError(f"{what}: tensors on different devices: {sorted(devs)}")


def _f32_in(t, name, inplace, what):
    t = t.detach()
    if inplace:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"{what}: inplace needs a contiguous, 16-byte aligned float32 "
                             f"`{name}`")
        return t
    t = t.float().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


# ------------------------------------------------------------------ GPU path
def _prepare_device(T: Tensor, sh_degree: int):
    """T: float64 [S,4,4] on the GPU -> (records float32 [S, RF], flags int32
    [2 + S]: the int64 out-of-range counter, then the status per segment)."""
    S = len(T)
    rec = torch.empty(S, record_floats(sh_degree), dtype=torch.float32, device=T.device)
    flags = torch.empty(2 + S, dtype=torch.int32, device=T.device)
    with torch.cuda.device(T.device):
        _lib.call("gsplat_hip_splat_xform_prepare", S, sh_degree, _ptr(T), _ptr(rec),
                  flags.data_ptr() + 8, _stream())
    return rec, flags


def _apply_device(N, sh_degree, S, rec, flags, ids, src, dst):
    """src, dst: (means, quats, scales, shN), geometry None for the SH part
    alone."""
    with torch.cuda.device(rec.device):
        if src[0] is None:
            _lib.call("gsplat_hip_splat_xform_rotate_sh", N, sh_degree, S, _ptr(rec),
                      flags.data_ptr() + 8, _ptr(ids), _ptr(src[3]), _ptr(dst[3]),
                      flags.data_ptr(), _stream())
        else:
            _lib.call("gsplat_hip_splat_xform_apply", N, sh_degree, S, _ptr(rec),
                      flags.data_ptr() + 8, _ptr(ids), *[_ptr(t) for t in src],
                      *[_ptr(t) for t in dst], flags.data_ptr(), _stream())


def _validate_device(what, flags, T, ids):
    host = flags.cpu()                       # the one host read
    _raise_first_bad(what, host[2:], lambda i: T[i])
    oob = int(host[:2].view(torch.int64)[0])
    if oob:
        raise ValueError(f"{what}: {oob} of {len(ids)} segment_ids lie outside [0, {len(T)})")


# ------------------------------------------------------------------ CPU path
def _host_segments(what, T, ids, N, validate):
    """-> (decomposition, seg int64 [N] clamped, keep bool [N] or None)."""
    d = _decompose(T)
    if validate:
        _raise_first_bad(what, d["status"], lambda i: T[i])
    S = len(T)
    if ids is None:
        seg = torch.zeros(N, dtype=torch.int64)
        inside = torch.ones(N, dtype=torch.bool)
    else:
        inside = (ids >= 0) & (ids < S)
        if validate and not bool(inside.all()):
            raise ValueError(f"{what}: {int((~inside).sum())} of {N} segment_ids lie outside "
                             f"[0, {S})")
        seg = torch.where(inside, ids, torch.zeros_like(ids))
    move = inside & (d["status"][seg] == 0)
    return d, seg, move


def _host_rotate_sh(shN, R, seg, move, sh_degree):
    out = shN.double().clone()
    at = 0
    for l, M in enumerate(_host_blocks(R, sh_degree), start=1):
        n = 2 * l + 1
        out[:, at:at + n] = torch.einsum("nij,njc->nic", M[seg], out[:, at:at + n])
        at += n
    return torch.where(move[:, None, None], out, shN.double()).float()


# -------------------------------------------------------------- public entry
def sh_rotation_matrices(rotations, sh_degree: int):
    """The real Wigner blocks M_l(R), l = 1..sh_degree, of rotations [3,3] or
    [S,3,3] in this package's SH basis: a list of [S, 2l+1, 2l+1] tensors with
    shN'[l] = M_l shN[l] per colour channel.  CPU input: computed in float64,
    returned in the input's dtype.  GPU input: the prepare kernel's float32
    records.  Raises ValueError for a matrix that is no proper rotation."""
    what = "sh_rotation_matrices"
    sh_degree = int(sh_degree)
    if not 0 <= sh_degree <= 4:
        raise ValueError(f"{what}: sh_degree {sh_degree} outside [0, 4]")
    R, on_host = _as_transforms(rotations, what, last=3)
    dtype = rotations.dtype if isinstance(rotations, Tensor) else torch.float64
    S = len(R)
    T = torch.zeros(S, 4, 4, dtype=torch.float64, device=R.device)
    T[:, :3, :3] = R
    T[:, 3, 3] = 1
    if on_host:
        d = _decompose(T)
        _raise_first_bad(what, d["status"], lambda i: T[i])
        return [M.to(dtype) for M in _host_blocks(d["R"], sh_degree)]
    rec, flags = _prepare_device(T, sh_degree)
    _raise_first_bad(what, flags[2:].cpu(), lambda i: T[i])
    out, at = [], HEADER_FLOATS
    for l in range(1, sh_degree + 1):
        n = 2 * l + 1
        out.append(rec[:, at:at + n * n].reshape(S, n, n).clone())
        at += n * n
    return out


def rotate_sh(shN: Tensor, rotations, segment_ids=None, out=None):
    """The SH part alone: `shN` [N, K-1, 3] rotated by `rotations` ([3,3] or
    [S,3,3], row i of `segment_ids` int64 [N] picking the rotation; without
    ids there is one).  Returns float32 [N, K-1, 3], written into `out` when
    given (`out` may be `shN` itself)."""
    what = "rotate_sh"
    if not isinstance(shN, Tensor) or shN.dim() != 3:
        raise ValueError(f"{what}: shN must be a [N, K-1, 3] tensor")
    N = shN.shape[0]
    deg = _sh_degree_of(shN, N, what)
    R, on_host = _as_transforms(rotations, what, last=3)
    ids = _check_ids(segment_ids, N, shN.device, what)
    S = len(R)
    if ids is None and S != 1:
        raise ValueError(f"{what}: {S} rotations need segment_ids")
    if out is not None:
        if (out.shape != shN.shape or out.dtype != torch.float32 or not out.is_contiguous()
                or out.data_ptr() % 16):
            raise ValueError(f"{what}: out must be a contiguous, 16-byte aligned float32 "
                             f"{list(shN.shape)}")
        _same_device((shN, out), what)
    T = torch.zeros(S, 4, 4, dtype=torch.float64, device=R.device)
    T[:, :3, :3] = R
    T[:, 3, 3] = 1
    if on_host:
        _raise_first_bad(what, _decompose(T)["status"], lambda i: T[i])
    if not shN.is_cuda:
        d, seg, move = _host_segments(what, T.cpu(), ids, N, True)
        res = _host_rotate_sh(shN.detach(), d["R"], seg, move, deg)
        if out is None:
            return res
        out.copy_(res)
        return out
    src = _f32_in(shN, "shN", False, what)
    dst = torch.empty_like(src) if out is None else out
    if deg == 0 or N == 0:
        return dst
    T = T.to(shN.device)
    rec, flags = _prepare_device(T, deg)
    _apply_device(N, deg, S, rec, flags, ids, (None, None, None, src), (None, None, None, dst))
    _validate_device(what, flags, T, ids)
    return dst


def transform_splats(splats, transforms, segment_ids=None, inplace=False, validate=True):
    """Move the Gaussians `splats` (a dict of the pre-activation parameters:
    means [N,3], quats [N,4] wxyz, scales [N,3] log-scales, optionally shN
    [N,K-1,3]; every other key passes through) by the similarity `transforms`.

    transforms: [4,4] or [S,4,4], a numpy array or a tensor on either device,
        float32 or float64: x' = A x + t with A = T[:3,:3], t = T[:3,3] (the
        fourth row is not read).  A must be s R with s > 0 and R a rotation:
        det A <= 0, or max|A^T A / s^2 - I| > 1e-4, is refused.
    segment_ids: int64 [N], row i moves by transforms[segment_ids[i]]; needed
        when S > 1.
    inplace: write into the given tensors (contiguous float32) instead of new
        ones.
    validate: True makes one host read after the launch and raises ValueError
        naming the first refused segment, or the number of ids outside [0, S).
        False reads nothing back; rows of a refused segment and rows with an id
        out of range come back unchanged.

    Returns a dict with the same keys; float32 for the four moved tensors.
    `transform_splats(splats, np.linalg.inv(parser.transform))` takes a scene
    trained on `colmap.Parser(normalize=True)` back to COLMAP's frame."""
    what = "transform_splats"
    for k in _GEOM_KEYS:
        if k not in splats:
            raise ValueError(f"{what}: splats has no `{k}`")
    means, quats, scales = (splats[k] for k in _GEOM_KEYS)
    shN = splats.get("shN")
    N = means.shape[0]
    if tuple(means.shape) != (N, 3) or tuple(quats.shape) != (N, 4) \
            or tuple(scales.shape) != (N, 3):
        raise ValueError(f"{what}: means {list(means.shape)}, quats {list(quats.shape)} and "
                         f"scales {list(scales.shape)} must be [N,3], [N,4] and [N,3]")
    deg = _sh_degree_of(shN, N, what)
    T, on_host = _as_transforms(transforms, what)
    _same_device((means, quats, scales, shN), what)
    ids = _check_ids(segment_ids, N, means.device, what)
    S = len(T)
    if ids is None and S != 1:
        raise ValueError(f"{what}: {S} transforms need segment_ids")
    if on_host and validate:
        _raise_first_bad(what, _decompose(T)["status"], lambda i: T[i])
    names = _GEOM_KEYS + (("shN",) if shN is not None else ())
    src = {k: _f32_in(splats[k], k, inplace, what) for k in names}
    out = dict(splats)

    if not means.is_cuda:
        d, seg, move = _host_segments(what, T.cpu(), ids, N, validate)
        m, q, sc = (src[k].double() for k in _GEOM_KEYS)
        A, t = d["A"][seg], d["t"][seg]
        qR = _rotmat_to_quat(d["R"])[seg]
        res = {"means": (A @ m[:, :, None])[:, :, 0] + t,
               "quats": _quat_mul(qR, q),
               "scales": sc + d["s"].log()[seg][:, None]}
        res = {k: torch.where(move[:, None], v, src[k].double()).float()
               for k, v in res.items()}
        if shN is not None:
            res["shN"] = _host_rotate_sh(src["shN"], d["R"], seg, move, deg)
        for k in names:
            if inplace:
                src[k].copy_(res[k])      # out[k] stays the caller's tensor
            else:
                out[k] = res[k]
        return out

    dst = src if inplace else {k: torch.empty_like(v) for k, v in src.items()}
    if not inplace:
        out.update(dst)
    if N == 0:
        return out
    T = T.to(means.device)
    rec, flags = _prepare_device(T, deg)
    _apply_device(N, deg, S, rec, flags, ids,
                  tuple(src.get(k) for k in _GEOM_KEYS + ("shN",)),
                  tuple(dst.get(k) for k in _GEOM_KEYS + ("shN",)))
    if validate:
        _validate_device(what, flags, T, ids)
    return out


def merge_splats(list_of_dicts):
    """Concatenate splat dicts along N.  `shN` is zero-padded to the highest
    degree present; the key sets must agree and every tensor must be on one
    device."""
    what = "merge_splats"
    dicts = list(list_of_dicts)
    if not dicts:
        raise ValueError(f"{what}: nothing to merge")
    keys = set(dicts[0])
    for i, d in enumerate(dicts):
        if set(d) != keys:
            raise ValueError(f"{what}: dict {i} has keys {sorted(d)}, dict 0 has {sorted(keys)}")
    devs = {str(v.device) for d in dicts for v in d.values()}
    if len(devs) > 1:
        raise ValueError(f"{what}: tensors on different devices: {sorted(devs)}")
    out = {}
    for k in dicts[0]:
        parts = [d[k] for d in dicts]
        if k == "shN":
            for i, p in enumerate(parts):
                _sh_degree_of(p, p.shape[0], f"{what}: dict {i}")
            width = max(p.shape[1] for p in parts)
            parts = [torch.cat([p, p.new_zeros(p.shape[0], width - p.shape[1], 3)], 1)
                     if p.shape[1] < width else p for p in parts]
        elif len({tuple(p.shape[1:]) for p in parts}) > 1:
            raise ValueError(f"{what}: `{k}` has shapes {[list(p.shape) for p in parts]}")
        out[k] = torch.cat(parts, 0)
    return out
