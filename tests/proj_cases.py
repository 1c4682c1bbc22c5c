"""Float64 oracle and seeded cases for the quat / scale EWA projection kernels
(csrc/projection.hip, csrc/proj_math.h).  Host only: torch on the CPU, no GPU
import.

The oracle is written from the definitions, not from the kernels' listing:

    q  = quat / |quat| (wxyz),  R_q its rotation,  Sigma = (R_q S)(R_q S)^T
    mc = R m + t,  Sigma_c = R Sigma R^T    (R, t: the view matrix's 12
                                             entries as given, R any matrix)
    J  = [[fx/z, 0, -fx tx/z], [0, fy/z, -fy ty/z]],  (tx, ty) = (x/z, y/z)
         clamped to the image plus a 15 % margin
    cov2d = J Sigma_c J^T,  blurred = cov2d + eps2d I,  conic = blurred^-1
    comp  = sqrt(max(det cov2d / det blurred, 0))
    radius = ceil(3 sqrt(b + sqrt(max(0.01, b^2 - det)))),  b = tr blurred / 2
    valid: near < z < far, det > 0, radius > radius_clip and the four strict
           frustum tests on means2d +- radius; invalid entries are zeros

Gradients are float64 autograd of sum(cotangent x output) over the pairs with
radii > 0.  Two conventions of the kernels differ from plain autograd; each
is expressed in one place: `means2d_clamped_gradient` and `CompSqrt`.
Everything else is plain autograd.  `oracle_adam` feeds the gradients of the
trainer's parameters [means, log_scales, quats, logits] to torch.optim.Adam's
update.

Cases are named; the seed comes from the name (zlib.crc32).  They hold
float32 arrays, which the oracle promotes to the dtype it runs in.  Every
case is homogeneous in depth and in scale (within about a factor 2 each, for
the Gaussians meant to be valid): the error measure is max error / max
|oracle| per output per case.

Gates.  Every discrete decision (the two depth tests, det > 0, the ceil of
the radius, radius > radius_clip, the four frustum tests, the four clamp
tests) is a gate.  The generator redraws any Gaussian one of whose (camera,
Gaussian) pairs has a float64 gate quantity within GATE_MARGIN of its
threshold where that gate decides the result (`undecided`): depths relative
to the plane, det relative to the product of the blurred diagonal, 3 sqrt(v1)
and the frustum quantities in pixels, the clamp quantities in units of x/z.
GATE_MARGIN = 1e-5 is the smallest power of ten at which the float32 run of
oracle/gsplat_oracle.py's proj_fwd (and the float32 run of this oracle)
reproduces every radius of the float64 oracle on every case; at 1e-6 the
frustum case below, which sits at twice the margin, is decided differently
(tests/test_proj_cases_host.py checks the zero-mismatch condition).  The
largest share of redrawn pairs is 0 % at this margin (0.4 % at 1e-4; cap:
5 %, asserted in the host test).  The at-the-gate cases (`gate_*`) are built
apart from that rule so that float32 and float64 agree by construction:
identity rotation and zero translation (mc == m exactly); in the frustum case
z = 4, so that f x / z + c rounds at most twice (one ulp of 72 is 7.6e-6,
under the 2e-5 the case keeps from the edge).

tests/golden/make_golden_proj_matrix.py measures per case and output the
float32 error of two float32 evaluations against the float64 oracle (`bar`);
the tests bound errors by max(FACTOR x bar, FLOOR).
"""

import functools
import math
import zlib
from types import SimpleNamespace

import numpy as np
import torch

FACTOR = 4.0
FLOOR = 1e-6
GATE_MARGIN = 1e-5
REDRAW_CAP = 0.05
W_IMG, H_IMG = 64, 48
INTRINSICS = dict(fx=58.0, fy=66.0, cx=30.5, cy=25.25)
EPS2D = 0.3
MARGIN = 0.15
# the trainer's geometry learning rates [means, log_scales, quats, logits]
ADAM = dict(lrs=(1.6e-4, 5e-3, 1e-3, 5e-2), betas=(0.9, 0.999), eps=1e-15, step=3)
GROUPS = ("means", "log_scales", "quats", "logits")
FWD_OUT = ("means2d", "depths", "conics", "comps")
BWD_OUT = ("v_means", "v_quats", "v_scales", "v_viewmats")


def _t(a, dtype, grad=False):
    return torch.from_numpy(np.array(a)).to(dtype).requires_grad_(grad)


def _np(t):
    return t.detach().numpy()


# ==================================================================== oracle
class CompSqrt(torch.autograd.Function):
    """Compensation epsilon: y = sqrt(x) whose backward is 0.5 g / (y + 1e-6),
    the kernels' `Da = 0.5 vcp / (cp + 1e-6)` (proj_math.h, conic_blur_vjp)."""

    @staticmethod
    def forward(ctx, x):
        y = x.sqrt()
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return 0.5 * g / (y + 1e-6)


def means2d_clamped_gradient(m2, J, mc):
    """Clamped means2d gradient: the value stays the unclamped f x/z + c, the
    gradient wrt the camera-space mean is J^T v with the clamped J (proj_math.h
    persp_vjp<true>: `vmc[2] = Jxz vm2x + Jyz vm2y`)."""
    return m2.detach() + (J.detach() @ (mc - mc.detach())[..., None])[..., 0]


def quat_to_rotmat(q):
    w, x, y, z = (q / q.pow(2).sum(-1, keepdim=True).sqrt()).unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
                       -1).reshape(*q.shape[:-1], 3, 3)


def clamp_limits(case, dtype=torch.float64):
    """(lox, hix, loy, hiy) of x/z and y/z."""
    k = case.K
    W, H = float(case.W), float(case.H)
    mx, my = MARGIN * W / k["fx"], MARGIN * H / k["fy"]
    return (-mx - k["cx"] / k["fx"], mx + (W - k["cx"]) / k["fx"],
            -my - k["cy"] / k["fy"], my + (H - k["cy"]) / k["fy"])


def project_pairs(case, m, q, s, V):
    """The projection of P (camera, Gaussian) pairs: means m [P,3], quats q
    [P,4], scales s [P,3], view matrices V [P,4,4] (rows 0..2 are read)."""
    k = case.K
    Rq = quat_to_rotmat(q)
    M = Rq * s[..., None, :]
    sigma = M @ M.transpose(-1, -2)
    R, t = V[..., :3, :3], V[..., :3, 3]
    mc = (R @ m[..., None])[..., 0] + t
    sigma_c = R @ sigma @ R.transpose(-1, -2)
    x, y, z = mc.unbind(-1)
    lox, hix, loy, hiy = clamp_limits(case)
    tx_raw, ty_raw = x / z, y / z
    tx, ty = tx_raw.clamp(lox, hix), ty_raw.clamp(loy, hiy)
    zero = torch.zeros_like(z)
    J = torch.stack([k["fx"] / z, zero, -k["fx"] * tx / z,
                     zero, k["fy"] / z, -k["fy"] * ty / z], -1).reshape(*z.shape, 2, 3)
    m2 = torch.stack([k["fx"] * tx_raw + k["cx"], k["fy"] * ty_raw + k["cy"]], -1)
    m2 = means2d_clamped_gradient(m2, J, mc)
    cov = J @ sigma_c @ J.transpose(-1, -2)
    det0 = cov[..., 0, 0] * cov[..., 1, 1] - cov[..., 0, 1] * cov[..., 1, 0]
    bxx, byy, bxy = cov[..., 0, 0] + case.eps2d, cov[..., 1, 1] + case.eps2d, cov[..., 0, 1]
    det = bxx * byy - bxy * cov[..., 1, 0]
    conics = torch.stack([byy / det, -bxy / det, bxx / det], -1)
    comps = CompSqrt.apply(torch.clamp_min(det0 / det, 0.0))
    b = 0.5 * (bxx + byy)
    disc = b * b - det
    ext = 3.0 * torch.sqrt(b + torch.sqrt(torch.clamp_min(disc, 0.01)))
    return SimpleNamespace(means2d=m2, depths=z, conics=conics, comps=comps, ext=ext,
                           radius=torch.ceil(ext), det=det, det_rel=det / (bxx * byy), disc=disc,
                           tx=tx_raw, ty=ty_raw)


def gates(case, dtype=torch.float64):
    """Per (camera, Gaussian) pair [C, N], without gradients: the projection,
    `cull` (name -> failed that test) and `clamp` (name -> clamped there)."""
    C, N = case.C, case.N
    with torch.no_grad(), np.errstate(all="ignore"):
        m, q, s = (_t(a, dtype)[None].expand(C, N, -1) for a in (case.means, case.quats, case.scales))
        V = _t(case.viewmats, dtype)[:, None].expand(C, N, 4, 4)
        p = project_pairs(case, m, q, s, V)
    z, r, m2 = p.depths, p.radius, p.means2d
    W, H = float(case.W), float(case.H)
    p.cull = {"near": ~(z > case.near), "far": ~(z < case.far), "det": ~(p.det > 0),
              "clip": ~(r > case.radius_clip), "left": ~(m2[..., 0] + r > 0),
              "right": ~(m2[..., 0] - r < W), "top": ~(m2[..., 1] + r > 0),
              "bottom": ~(m2[..., 1] - r < H)}
    lox, hix, loy, hiy = clamp_limits(case)
    p.clamp = {"x-": p.tx < lox, "x+": p.tx > hix, "y-": p.ty < loy, "y+": p.ty > hiy}
    p.valid = ~torch.stack(list(p.cull.values())).any(0)
    # gate quantities: distance to the threshold, in the units of the docstring
    p.dist = {"near": (z / case.near - 1).abs(), "far": (z / case.far - 1).abs(),
              "det": p.det_rel.abs(), "ceil": (p.ext - p.ext.round()).abs(),
              "clip": torch.ones_like(r),  # integers both: decided once the ceil is
              "left": (m2[..., 0] + r).abs(), "right": (m2[..., 0] - r - W).abs(),
              "top": (m2[..., 1] + r).abs(), "bottom": (m2[..., 1] - r - H).abs(),
              "x-": (p.tx - lox).abs(), "x+": (p.tx - hix).abs(),
              "y-": (p.ty - loy).abs(), "y+": (p.ty - hiy).abs()}
    return p


def undecided(p, margin=None):
    """[C, N] bool: the pair's result could flip within `margin`.  A depth test
    that fails by the margin decides alone; otherwise the ceil must be clear,
    then a radius or frustum test that fails by the margin decides; otherwise
    every test and every clamp test must be clear."""
    margin = GATE_MARGIN if margin is None else margin

    def clear(k):
        d = p.dist[k]
        return ~(d < margin) & ~torch.isnan(d)

    culled_by_depth = (p.cull["near"] & clear("near")) | (p.cull["far"] & clear("far"))
    later = ("det", "clip", "left", "right", "top", "bottom")
    culled_later = torch.zeros_like(culled_by_depth)
    all_clear = clear("near") & clear("far") & clear("ceil")
    for k in later:
        culled_later |= p.cull[k] & clear(k)
        all_clear &= clear(k)
    for k in p.clamp:
        all_clear &= clear(k)
    safe = culled_by_depth | (clear("near") & clear("far") & clear("ceil") & culled_later) | all_clear
    return ~safe


def oracle_fwd(case, dtype=torch.float64):
    """radii i32 [C,N]; means2d, depths, conics, comps with invalid entries
    zero (depths: every pair, they are written before culling)."""
    p = gates(case, dtype)
    v = p.valid
    z32 = lambda a: _np(torch.where(v.reshape(v.shape + (1,) * (a.dim() - 2)), a,
                                    torch.zeros_like(a)))  # noqa: E731
    return {"radii": _np(torch.where(v, p.radius, torch.zeros_like(p.radius))).astype(np.int32),
            "means2d": z32(p.means2d), "depths": _np(p.depths), "conics": z32(p.conics),
            "comps": z32(p.comps)}


def oracle_bwd(case, dtype=torch.float64, comps=False, depths=True, valid=None):
    """Gradients of sum(cotangent x output) over the valid pairs (`valid`
    [C,N]: other than this dtype's own): dense v_means / v_quats / v_scales
    [N, .] and v_viewmats [C,4,4], and the per-pair rows pp_* [nnz, .] in
    (camera, Gaussian) order."""
    if valid is None:
        valid = _np(gates(case, dtype).valid)
    ci, ni = (torch.from_numpy(a) for a in np.nonzero(valid))
    N, C = case.N, case.C
    m = _t(case.means, dtype)[ni].requires_grad_(True)
    q = _t(case.quats, dtype)[ni].requires_grad_(True)
    s = _t(case.scales, dtype)[ni].requires_grad_(True)
    V = _t(case.viewmats, dtype)[ci].requires_grad_(True)
    out = {}
    if len(ci):
        p = project_pairs(case, m, q, s, V)
        cot = lambda a: _t(a, dtype)[ci, ni]  # noqa: E731
        loss = (p.means2d * cot(case.v_means2d)).sum() + (p.conics * cot(case.v_conics)).sum()
        if depths:
            loss = loss + (p.depths * cot(case.v_depths)).sum()
        if comps:
            loss = loss + (p.comps * cot(case.v_comps)).sum()
        gm, gq, gs, gV = torch.autograd.grad(loss, (m, q, s, V))
    else:
        gm, gq, gs, gV = (torch.zeros_like(a) for a in (m, q, s, V))
    for k, g, rows in (("v_means", gm, N), ("v_quats", gq, N), ("v_scales", gs, N),
                       ("v_viewmats", gV, C)):
        idx = ci if k == "v_viewmats" else ni
        out[k] = _np(torch.zeros((rows,) + g.shape[1:], dtype=dtype).index_add_(0, idx, g))
        out["pp_" + k] = _np(g)
    return out


def adam_step(p, g, m, v, lr, step, betas, eps):
    """torch.optim.Adam (no weight decay, no amsgrad), 1-based step."""
    b1, b2 = betas
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def adam_gradients(case, dtype=torch.float64, dirs=True, opac=True, valid=None):
    """d/d[means, log_scales, quats, logits] of  sum cotangents . projection(
    means, quats, exp(log_scales)) + v_dirs . means + v_opac . sigmoid(logits)
    (camera 0 of a one-camera case; compensations off)."""
    assert case.C == 1
    if valid is None:
        valid = _np(gates(case, dtype).valid)
    ni = torch.from_numpy(np.nonzero(valid[0])[0])
    means = _t(case.means, dtype, True)
    ls = _t(case.log_scales, dtype, True)
    quats = _t(case.quats, dtype, True)
    logits = _t(case.logits, dtype, True)
    loss = means.sum() * 0 + ls.sum() * 0 + quats.sum() * 0 + logits.sum() * 0
    if len(ni):
        V = _t(case.viewmats, dtype)[0].expand(len(ni), 4, 4)
        p = project_pairs(case, means[ni], quats[ni], torch.exp(ls)[ni], V)
        cot = lambda a: _t(a, dtype)[0, ni]  # noqa: E731
        loss = loss + (p.means2d * cot(case.v_means2d)).sum() + (p.conics * cot(case.v_conics)).sum() \
            + (p.depths * cot(case.v_depths)).sum()
    if dirs:
        loss = loss + (means * _t(case.v_dirs, dtype)).sum()
    if opac:
        loss = loss + (torch.sigmoid(logits) * _t(case.v_opac, dtype)).sum()
    return [g.detach() for g in torch.autograd.grad(loss, (means, ls, quats, logits))]


def oracle_adam(case, dtype=torch.float64, dirs=True, opac=True, betas=None, valid=None):
    """g_<group>: the gradients; m1_<group>: exp_avg after step 1 from zero
    moments; p_ / m_ / v_<group>: one update at ADAM["step"] from the case's
    seeded moments.  `betas`: other than ADAM's."""
    betas = ADAM["betas"] if betas is None else betas
    g = adam_gradients(case, dtype, dirs, opac, valid)
    params = [_t(getattr(case, k), dtype) for k in GROUPS]
    out = {}
    for i, k in enumerate(GROUPS):
        zero = torch.zeros_like(params[i])
        _, m1, _ = adam_step(params[i], g[i], zero, zero, ADAM["lrs"][i], 1, betas, ADAM["eps"])
        p, m, v = adam_step(params[i], g[i], _t(case.m_init[i], dtype), _t(case.v_init[i], dtype),
                            ADAM["lrs"][i], ADAM["step"], betas, ADAM["eps"])
        out.update({"g_" + k: _np(g[i]), "m1_" + k: _np(m1), "p_" + k: _np(p), "m_" + k: _np(m),
                    "v_" + k: _np(v)})
    return out


ADAM_OUT = tuple(f"{a}_{k}" for a in ("g", "m1", "p", "m", "v") for k in GROUPS)
BWD_VARIANTS = [(False, True), (False, False), (True, True), (True, False)]  # (comps, depths)
ADAM_VARIANTS = [(True, True), (False, True), (True, False), (False, False)]  # (dirs, opac)


def bwd_key(comps, depths):
    return "bwd" + ("_comp" if comps else "") + ("" if depths else "_nodepth")


def adam_key(dirs, opac):
    return "adam" + ("" if dirs else "_nodirs") + ("" if opac else "_noopac")


def freeze(out):
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fwd64(name):
    """The float64 forward of a case, computed once and shared read-only."""
    return freeze(oracle_fwd(build(name)))


@functools.lru_cache(maxsize=None)
def bwd64(name, comps=False, depths=True):
    return freeze(oracle_bwd(build(name), comps=comps, depths=depths))


@functools.lru_cache(maxsize=None)
def adam64(name, dirs=True, opac=True, f32_betas=False):
    betas = tuple(float(np.float32(b)) for b in ADAM["betas"]) if f32_betas else None
    return freeze(oracle_adam(build(name), dirs=dirs, opac=opac, betas=betas))


# ===================================================================== cases
# name -> (population, N, C, options)
SPECS = {
    "z03_n257_c1": ("plain", 257, 1, dict(z=0.3)),
    "z3_n1_c1": ("plain", 1, 1, dict(z=3.0)),
    "z3_n255_c1": ("plain", 255, 1, dict(z=3.0)),
    "z3_n600_c3": ("plain", 600, 3, dict(z=3.0)),
    "z30_n257_c3": ("plain", 257, 3, dict(z=30.0)),
    "skew_n257_c1": ("plain", 257, 1, dict(z=3.0, skew=True)),
    "skew_n600_c3": ("plain", 600, 3, dict(z=3.0, skew=True)),
    "qnorm_n255_c1": ("plain", 255, 1, dict(z=3.0, qnorm=True)),
    "qnorm_n257_c3": ("plain", 257, 3, dict(z=3.0, qnorm=True)),
    "iso_n257_c1": ("iso", 257, 1, dict(z=3.0)),
    "iso_n255_c3": ("iso", 255, 3, dict(z=3.0)),
    "needle_n257_c1": ("needle", 257, 1, dict(z=3.0)),
    "disc_n257_c1": ("disc", 257, 1, dict(z=3.0)),
    "edgeon_n255_c1": ("edgeon", 255, 1, dict(z=3.0)),
    "aniso_n600_c3": ("aniso", 600, 3, dict(z=3.0)),
    "clamp_n257_c1": ("clamp", 257, 1, dict(z=3.0)),
    "clamp_n600_c3": ("clamp", 600, 3, dict(z=3.0)),
    "clamp_skew_n255_c1": ("clamp", 255, 1, dict(z=3.0, skew=True)),
    "cull_near_n255_c1": ("cull", 255, 1, dict(z=3.0, by="near")),
    "cull_far_n257_c1": ("cull", 257, 1, dict(z=3.0, by="far", far=6.0)),
    "cull_left_n255_c1": ("cull", 255, 1, dict(z=3.0, by="left")),
    "cull_right_n257_c1": ("cull", 257, 1, dict(z=3.0, by="right")),
    "cull_top_n255_c1": ("cull", 255, 1, dict(z=3.0, by="top")),
    "cull_bottom_n257_c1": ("cull", 257, 1, dict(z=3.0, by="bottom")),
    "cull_clip3_n255_c1": ("cull", 255, 1, dict(z=3.0, by="clip", radius_clip=3.0)),
    "cull_clip0_n255_c1": ("cull", 255, 1, dict(z=3.0, by="clip", radius_clip=0.0)),
    "allculled_n257_c3": ("allculled", 257, 3, dict(z=3.0)),
    "allculled_n1_c1": ("allculled", 1, 1, dict(z=3.0)),
    "deadwave_n600_c1": ("deadwave", 600, 1, dict(z=3.0)),
    "deadwave_n257_c3": ("deadwave", 257, 3, dict(z=3.0)),
    "tail_n255_c3": ("tail", 255, 3, dict(z=3.0)),
    "tail_n257_c1": ("tail", 257, 1, dict(z=3.0)),
    "gate_near": ("gate_near", 2, 1, dict(z=0.3)),
    "gate_clip": ("gate_clip", 2, 1, dict(z=3.0, radius_clip=3.0)),
    "gate_frustum": ("gate_frustum", 8, 1, dict(z=4.0)),
}
ALL_NAMES = list(SPECS)
GATE_NAMES = [n for n in ALL_NAMES if n.startswith("gate_")]
SEEDED_NAMES = [n for n in ALL_NAMES if n not in GATE_NAMES]
ADAM_NAMES = [n for n in ALL_NAMES if SPECS[n][2] == 1]
CLAMP_KINDS = ("x+", "x-", "y+", "y-", "x+y+", "x+y-", "x-y+", "x-y-")
CULL_TESTS = ("near", "far", "det", "clip", "left", "right", "top", "bottom")


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _loguniform(g, lo, hi, *shape):
    return torch.exp(_rand(g, *shape) * (math.log(hi) - math.log(lo)) + math.log(lo))


def _unit_quats(g, n):
    q = _randn(g, n, 4)
    return q / q.norm(dim=-1, keepdim=True)


def _quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _quat_z_to(nrm):
    """Unit quaternions [n,4] whose rotation takes the z axis to nrm [n,3]."""
    zax = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand_as(nrm)
    q = torch.cat([1.0 + (zax * nrm).sum(-1, keepdim=True), torch.cross(zax, nrm, dim=-1)], -1)
    return q / q.norm(dim=-1, keepdim=True)


def _viewmats(g, C, z, skew):
    """Camera 0: a random rotation rounded to float32 and |t| of about the
    depth; the others a few degrees and a few per cent of the depth from it.
    skew: 0.9 I + 0.1 R, near the identity and not orthonormal."""
    vm = torch.eye(4, dtype=torch.float64).repeat(C, 1, 1)
    R0 = quat_to_rotmat(_unit_quats(g, 1))[0]
    if skew:
        R0 = 0.9 * torch.eye(3, dtype=torch.float64) + 0.1 * R0
    t0 = _randn(g, 3) * 0.3 * z
    for c in range(C):
        d = torch.cat([torch.ones(1, dtype=torch.float64), _randn(g, 3) * (0.03 if c else 0.0)])
        Rd = quat_to_rotmat(d[None])[0]
        vm[c, :3, :3] = Rd @ R0
        vm[c, :3, 3] = Rd @ t0 + (_randn(g, 3) * 0.03 * z if c else 0.0)
    return vm.float().numpy()


def _draw(c, g, n):
    """n Gaussians of the case's population, placed in camera 0's frame:
    (camera-space means [n,3], unit quats [n,4] in the world frame, scales
    [n,3], kind [n]).  Pixel sizes are at the band's depth z."""
    k, z0, pop = c.K, c.opt["z"], c.pop
    f = 0.5 * (k["fx"] + k["fy"])
    z = z0 * (0.8 + 0.7 * _rand(g, n))
    u = _rand(g, n) * c.W  # target pixel
    v = _rand(g, n) * c.H
    quats = _unit_quats(g, n)
    sig = 1.6 + 1.4 * _rand(g, n, 1)  # pixels
    ratio = 0.8 + 0.2 * _rand(g, n, 3)
    kind = torch.zeros(n, dtype=torch.int64)
    if pop == "iso":
        sig, ratio = 0.4 + 0.4 * _rand(g, n, 1), 0.98 + 0.04 * _rand(g, n, 3)  # round within 2 %
        u = k["cx"] + (_rand(g, n) - 0.5) * 0.3 * k["fx"]
        v = k["cy"] + (_rand(g, n) - 0.5) * 0.3 * k["fy"]
    elif pop in ("needle", "disc", "edgeon", "aniso"):
        kind = torch.randint(0, 3, (n,), generator=g) if pop == "aniso" else \
            torch.full((n,), ("needle", "disc", "edgeon").index(pop))
        sig = 4.0 + 4.0 * _rand(g, n, 1)
        thin = 1.0 / _loguniform(g, 10.0, 1e3, n)
        ratio = torch.stack([0.85 + 0.15 * _rand(g, n), torch.where(kind == 0, thin, 0.7 + 0.3 * _rand(g, n)),
                             thin], -1)
    elif pop == "clamp":
        kind = torch.randint(0, len(CLAMP_KINDS) + 2, (n,), generator=g)  # the last two: unclamped
        sig = 5.5 + 2.5 * _rand(g, n, 1)
        over = 1.0 + 5.0 * _rand(g, n)
        for i, name in enumerate(CLAMP_KINDS):
            sel = kind == i
            if "x+" in name:
                u = torch.where(sel, c.W * (1 + MARGIN) + over, u)
            if "x-" in name:
                u = torch.where(sel, -c.W * MARGIN - over, u)
            if "y+" in name:
                v = torch.where(sel, c.H * (1 + MARGIN) + over, v)
            if "y-" in name:
                v = torch.where(sel, -c.H * MARGIN - over, v)
    elif pop == "cull":
        by = c.opt["by"]
        kind = (_rand(g, n) < 0.5).long()  # 1: meant to be culled
        off = 1.0 + 4.0 * _rand(g, n)
        rad = 3.0 * sig[:, 0] + 1.0
        if by == "near":
            z = torch.where(kind == 1, -z, z)  # behind the camera
        elif by == "far":
            z = torch.where(kind == 1, c.far * (1.25 + 0.25 * _rand(g, n)), z)
        elif by == "left":
            u = torch.where(kind == 1, -rad - off, u)
        elif by == "right":
            u = torch.where(kind == 1, c.W + rad + off, u)
        elif by == "top":
            v = torch.where(kind == 1, -rad - off, v)
        elif by == "bottom":
            v = torch.where(kind == 1, c.H + rad + off, v)
        elif by == "clip":
            sig = torch.where(kind[:, None] == 1, 0.2 + 0.4 * _rand(g, n, 1), sig)
    elif pop == "allculled":
        z = -z
    if pop in ("deadwave", "tail"):
        kind = (_rand(g, n) < (0.0 if pop == "deadwave" else 0.3)).long()
        z = torch.where(kind == 1, -z, z)
    mc = torch.stack([(u - k["cx"]) / k["fx"] * z, (v - k["cy"]) / k["fy"] * z, z], -1)
    scales = sig * ratio * (z0 / f)
    if pop in ("edgeon", "aniso"):
        # discs seen nearly edge-on: the normal 1e-3 .. 1e-1 rad from
        # perpendicular to the ray, in camera 0's frame
        ray = mc / mc.norm(dim=-1, keepdim=True)
        a = _randn(g, n, 3)
        perp = a - (a * ray).sum(-1, keepdim=True) * ray
        perp = perp / perp.norm(dim=-1, keepdim=True)
        th = _loguniform(g, 1e-3, 1e-1, n)[:, None]
        nrm_cam = torch.cos(th) * perp + torch.sin(th) * ray
        R0 = _t(c.viewmats, torch.float64)[0, :3, :3]
        nrm = nrm_cam @ torch.linalg.inv(R0).T
        nrm = nrm / nrm.norm(dim=-1, keepdim=True)
        spin = torch.zeros(n, 4, dtype=torch.float64)
        ang = _rand(g, n) * math.pi
        spin[:, 0], spin[:, 3] = torch.cos(ang), torch.sin(ang)
        edge = _quat_mul(_quat_z_to(nrm), spin)
        quats = torch.where((kind == 2)[:, None], edge, quats)
    return mc, quats, scales, kind


def _accept(c, p, kind):
    """[n] bool: the drawn Gaussians are what the population says."""
    valid, n = p.valid, kind.shape[0]
    ok = torch.ones(n, dtype=torch.bool)
    ncull = torch.stack([p.cull[k] for k in CULL_TESTS]).sum(0)  # [C, n]
    if c.pop in ("plain", "iso", "needle", "disc", "edgeon", "aniso"):
        ok = valid.all(0)
        if c.pop == "iso":
            ok &= (p.disc < 0.01).all(0)
    elif c.pop == "clamp":
        ok = valid[0].clone()
        cl = p.clamp
        for i, name in enumerate(CLAMP_KINDS):
            want = torch.ones(n, dtype=torch.bool)
            for key in ("x+", "x-", "y+", "y-"):
                want &= cl[key][0] == (key in name)
            ok &= (kind != i) | want
        anyc = torch.stack(list(cl.values())).any(0)[0]
        ok &= (kind < len(CLAMP_KINDS)) | ~anyc
    elif c.pop == "cull":
        by = c.opt["by"]
        alone = (p.cull[by] & (ncull == 1)).all(0)
        if by == "clip" and c.radius_clip == 0.0:
            alone = valid.all(0)  # nothing has radius <= 0: the same Gaussians stay
        ok = torch.where(kind == 1, alone, valid.all(0))
    elif c.pop == "allculled":
        ok = (~valid).all(0)
    elif c.pop in ("deadwave", "tail"):
        ok = torch.where(kind == 1, (~valid).all(0), valid.all(0))
    return ok


def _build_seeded(c, g):
    N, C = c.N, c.C
    c.viewmats = _viewmats(g, C, c.opt["z"], c.opt.get("skew", False))
    V0 = _t(c.viewmats, torch.float64)[0]
    R0inv = torch.linalg.inv(V0[:3, :3])
    means = torch.zeros(N, 3, dtype=torch.float64)
    quats = torch.zeros(N, 4, dtype=torch.float64)
    scales = torch.ones(N, 3, dtype=torch.float64)
    kinds = torch.zeros(N, dtype=torch.int64)
    todo = torch.ones(N, dtype=torch.bool)
    forced = {}
    if c.pop == "deadwave":
        forced = {i: 1 for i in range(64, 128)}
    if c.pop == "tail":
        forced = {N - 1: 0}
    redrawn = 0
    for _ in range(400):
        n = int(todo.sum())
        if n == 0:
            break
        mc, q, s, kind = _draw(c, g, n)
        idx = torch.nonzero(todo)[:, 0]
        for j, i in enumerate(idx.tolist()):
            if i in forced and int(kind[j]) != forced[i]:
                kind[j] = forced[i]
                mc[j] = mc[j] * (-1.0 if (mc[j, 2] < 0) != (forced[i] == 1) else 1.0)
        if c.opt.get("qnorm"):
            q = q * _loguniform(g, 1e-3, 1e3, n)[:, None]
        means[todo] = (mc - V0[:3, 3]) @ R0inv.T
        quats[todo], scales[todo], kinds[todo] = q, s, kind
        c.means, c.quats = means.float().numpy(), quats.float().numpy()
        c.log_scales = torch.log(scales).float().numpy()
        c.scales = torch.exp(_t(c.log_scales, torch.float64)).float().numpy()
        p = gates(c)
        near_gate = undecided(p).any(0)
        bad = ~_accept(c, p, kinds) & todo
        gate_only = near_gate & ~bad & todo
        redrawn += int(gate_only.sum())
        todo = bad | (near_gate & todo)
        # a Gaussian accepted earlier stays: its arrays did not change
    assert not todo.any(), (c.name, int(todo.sum()))
    c.kind = kinds.numpy()
    c.redrawn = redrawn * C / float(C * N)
    return c


def _identity_camera(c):
    c.viewmats = np.eye(4, dtype=np.float32)[None].copy()


def _iso_sigma(ext):
    """Pixel sigma of an isotropic footprint with 3 sqrt(v1) == ext at the
    image centre (b^2 - det under the floor: v1 = sigma^2 + eps2d + 0.1)."""
    return math.sqrt((ext / 3.0) ** 2 - EPS2D - 0.1)


def _build_gate(c):
    k, z0 = c.K, c.opt["z"]
    _identity_camera(c)
    f = 0.5 * (k["fx"] + k["fy"])
    N = c.N
    means = np.zeros((N, 3), np.float64)
    sig = np.full(N, 1.2 if c.pop == "gate_frustum" else 2.0)
    if c.pop == "gate_near":
        # z == near_plane exactly (mc = 1 m + 0: exact in any precision)
        z = np.float32(c.near)
        means[:, 2] = [z, np.nextafter(z, np.float32(1))]
    elif c.pop == "gate_clip":
        means[:, 2] = z0
        sig[:] = [_iso_sigma(2.5), _iso_sigma(3.5)]  # radii 3 (culled at clip 3) and 4
    else:
        means[:, 2] = z0
    c.quats = np.tile(np.array([[1.0, 0, 0, 0]], np.float32), (N, 1))
    # 3 % off round: exactly isotropic Gaussians have no quaternion gradient to compare
    scale = sig[:, None] * (means[:, 2:3] / f) * np.array([[1.0, 0.97, 1.03]])
    c.log_scales = np.log(scale).astype(np.float32)
    c.scales = np.exp(c.log_scales.astype(np.float64)).astype(np.float32)
    c.means = means.astype(np.float32)
    if c.pop == "gate_frustum":
        # rows 0..3 culled, 4..7 kept: means2d +- radius lies 2 GATE_MARGIN
        # beyond / inside the left, right, top, bottom edge.  The radius
        # depends (weakly) on the position: fixed point of a few rounds.
        d = 2 * GATE_MARGIN
        sides = [(0, 0.0, -1), (0, float(c.W), 1), (1, 0.0, -1), (1, float(c.H), 1)] * 2
        radius = np.full(N, 7.0)
        for _ in range(6):
            for i, (axis, edge, sgn) in enumerate(sides):
                px = edge + sgn * (radius[i] + (d if i < 4 else -d))
                fk, ck = (k["fx"], k["cx"]) if axis == 0 else (k["fy"], k["cy"])
                means[i, axis] = (px - ck) / fk * z0
            c.means = means.astype(np.float32)
            radius = _np(gates(c).radius)[0]
    c.kind = np.zeros(N, np.int64)
    c.redrawn = 0.0
    return c


def _cotangents(c, g):
    N, C = c.N, c.C
    c.v_means2d = torch.randn(C, N, 2, generator=g).numpy()
    c.v_depths = torch.randn(C, N, generator=g).numpy()
    c.v_conics = torch.randn(C, N, 3, generator=g).numpy()
    c.v_comps = torch.randn(C, N, generator=g).numpy()
    # the geometry Adam's other inputs; the SH and rasterizer backwards give
    # zero rows for the Gaussians camera 0 culls
    vis = torch.from_numpy(_np(gates(c).valid)[0].astype(np.float32))
    c.logits = torch.randn(N, generator=g).numpy()
    c.opac = torch.sigmoid(_t(c.logits, torch.float64)).float().numpy()
    c.v_dirs = (torch.randn(N, 3, generator=g) * vis[:, None]).numpy()
    c.v_opac = (torch.randn(N, generator=g) * vis).numpy()
    shapes = ((N, 3), (N, 3), (N, 4), (N,))
    # moments of the size of the case's own gradients and their squares, with
    # exp_avg_sq at least a quarter of its largest: the step |m^| / sqrt(v^)
    # stays of order 1, as with moments Adam itself produced.  (A tiny
    # exp_avg_sq beside a large exp_avg makes a step of many lr, which only
    # magnifies the rounding of beta2 to a C float in 1 - beta2^t, 6.4e-6 of
    # the step: diagnosed in tests/test_gpu_sh_matrix.py.)
    gr = [float(np.abs(_np(x)).max()) or 1.0 for x in adam_gradients(c)] if C == 1 else [1.0] * 4
    c.m_init = [(torch.randn(*s, generator=g) * 0.1 * a).numpy() for s, a in zip(shapes, gr)]
    c.v_init = [((0.25 + 0.75 * torch.rand(*s, generator=g)) * 0.01 * a * a).numpy() for s, a in zip(shapes, gr)]


@functools.lru_cache(maxsize=None)
def build(name):
    """The case of that name (float32 numpy arrays, read-only)."""
    pop, N, C, opt = SPECS[name]
    c = SimpleNamespace(name=name, pop=pop, N=N, C=C, opt=opt, W=W_IMG, H=H_IMG, K=INTRINSICS,
                        eps2d=EPS2D, radius_clip=float(opt.get("radius_clip", 0.0)),
                        near=float(np.float32(0.1 * opt["z"])), far=float(opt.get("far", 1e10)))
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    c = _build_gate(c) if pop.startswith("gate_") else _build_seeded(c, g)
    _cotangents(c, g)
    c.Ks = np.tile(np.array([[c.K["fx"], 0, c.K["cx"]], [0, c.K["fy"], c.K["cy"]], [0, 0, 1]],
                            np.float32), (C, 1, 1))
    for v in list(vars(c).values()):
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return c


# -------------------------------------------- the repository's numpy oracle
def numpy_fwd(case, dtype=np.float32):
    """oracle/gsplat_oracle.py's proj_fwd in `dtype`, compensations on."""
    from oracle import gsplat_oracle as O
    with O.precision(dtype):
        r, m2, d, cn, cp = O.proj_fwd(case.means, case.quats, case.scales, case.viewmats, case.Ks,
                                      case.W, case.H, case.eps2d, case.near, case.far,
                                      case.radius_clip, calc_comp=True)
    return {"radii": r, "means2d": m2, "depths": d, "conics": cn, "comps": cp}


def numpy_bwd(case, fwd, dtype=np.float32, comps=False, depths=True):
    """Its proj_bwd in `dtype`, from that run's own forward."""
    from oracle import gsplat_oracle as O
    vd = case.v_depths if depths else np.zeros_like(case.v_depths)
    with O.precision(dtype):
        out = O.proj_bwd(case.means, case.quats, case.scales, case.viewmats, case.Ks, case.W,
                         case.H, case.eps2d, fwd["radii"], fwd["conics"],
                         fwd["comps"] if comps else None, case.v_means2d, vd, case.v_conics,
                         case.v_comps if comps else None)
    return dict(zip(BWD_OUT, out))


# ================================================================ comparison
def rel_err(ours, ref):
    ref = np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    return float(np.abs(np.asarray(ours, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def load_bars(path):
    """{"<case>:<variant>:<output>": bar} from proj_matrix.npz."""
    z = np.load(path)
    return dict(zip((str(k) for k in z["bar_names"]), (float(v) for v in z["bar_values"])))


def bound(bar):
    return max(FACTOR * bar, FLOOR)
