"""Float64 oracle and seeded cases for the spherical-harmonics colour kernels
(csrc/sh.hip, csrc/sh_basis.h).  Host only: torch on the CPU, no GPU import.

The oracle is written from the definition of the real spherical harmonics,
not from the kernels' polynomial listing:

    Y_l^m(x, y, z) = (-1)^|m| N_l^|m| Pbar_l^|m|(z) T_m(x, y)
    N_l^m   = sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!), times sqrt 2 for m != 0
    Pbar_l^m = P_l^m(z) / (1-z^2)^(m/2)   (no Condon-Shortley phase), by
               Pbar_m^m = (2m-1)!!,  Pbar_{m+1}^m = (2m+1) z Pbar_m^m,
               (l-m) Pbar_l^m = (2l-1) z Pbar_{l-1}^m - (l+m-1) Pbar_{l-2}^m
    T_m     = Re (x+iy)^m for m >= 0, Im (x+iy)^|m| for m < 0

ordered l ascending, m = -l .. l: polynomials in (x, y, z), differentiable at
the poles.  Around the basis: the L2 normalisation of the direction (no
epsilon), masks, the fused colour path of rasterization() (direction = mean -
camera centre, the centre -R^T t from the float32 view-matrix entries, then
clamp_min(sh + 0.5, 0) and 0.5 for rows with radii <= 0), the sum over
cameras, and torch.optim.Adam's update.  Autograd gives the gradients.

Cases are built from a seed derived from their name and hold float32 arrays;
the oracle reads those float32 values promoted to the dtype it runs in
(float64 for the truth, float32 to show what plain float32 arithmetic gives).
tests/golden/make_golden_sh_matrix.py measures, per case and output, the
float32 error of the reference's torch implementation against its float64 run
(`bar`); the tests bound errors by max(FACTOR x bar, FLOOR), relative to the
largest |float64 value| of the output.
"""

import functools
import math
import zlib
from types import SimpleNamespace

import numpy as np
import torch

FACTOR = 4.0
FLOOR = 1e-6
GATE_MARGIN = 1e-3
# the trainer's SH learning rates (sh0, shN) and Adam settings
ADAM = dict(lr0=2.5e-3, lr_rest=1.25e-4, betas=(0.9, 0.999), eps=1e-15, steps=3)


# ===================================================================== basis
def basis(d, deg):
    """Real SH basis of the unit directions d [..., 3] -> [..., (deg+1)^2]."""
    x, y, z = d.unbind(-1)
    one = torch.ones_like(z)
    re, im = [one], [torch.zeros_like(z)]
    for _ in range(deg):
        r, i = re[-1], im[-1]
        re.append(r * x - i * y)
        im.append(r * y + i * x)
    P = {}
    for m in range(deg + 1):
        dfact = 1.0
        for j in range(2 * m - 1, 0, -2):
            dfact *= j
        P[m, m] = dfact * one
        if m + 1 <= deg:
            P[m + 1, m] = (2 * m + 1) * z * P[m, m]
        for l in range(m + 2, deg + 1):
            P[l, m] = ((2 * l - 1) * z * P[l - 1, m] - (l + m - 1) * P[l - 2, m]) / (l - m)
    out = []
    for l in range(deg + 1):
        for m in range(-l, l + 1):
            am = abs(m)
            norm = math.sqrt((2 * l + 1) / (4 * math.pi)
                             * math.factorial(l - am) / math.factorial(l + am))
            if m:
                norm *= math.sqrt(2.0)
            out.append(((-1) ** am * norm) * P[l, am] * (re[am] if m >= 0 else im[am]))
    return torch.stack(out, -1)


B0 = math.sqrt(1.0 / (4 * math.pi))


def sh_eval(deg, dirs, coeffs):
    """Colours [..., 3] of directions [..., 3] (any length but 0) and
    coefficients [..., K, 3]; those above the active degree are not read."""
    d = dirs / dirs.pow(2).sum(-1, keepdim=True).sqrt()
    nb = (deg + 1) ** 2
    return (basis(d, deg)[..., None] * coeffs[..., :nb, :]).sum(-2)


def _t(a, dtype, grad=False):
    return torch.from_numpy(np.array(a)).to(dtype).requires_grad_(grad)


def _np(t):
    return t.detach().numpy()


def _grad(loss, ins):
    gs = torch.autograd.grad(loss, ins, allow_unused=True)
    return [torch.zeros_like(i) if g is None else g for g, i in zip(gs, ins)]


# ==================================================================== oracle
def oracle_nf(case, dtype=torch.float64):
    """spherical_harmonics(): colours, v_coeffs (summed over the cameras the
    coefficient rows are broadcast to) and v_dirs, each row of v_dirs
    multiplied by its direction's length (lengths span six decades)."""
    dirs = _t(case.dirs, dtype, True)
    coeffs = _t(case.coeffs, dtype, True)
    col = sh_eval(case.deg, dirs, coeffs.expand(*dirs.shape[:-1], -1, -1))
    if case.masks is not None:
        col = col * _t(case.masks, dtype)[..., None]
    v_coeffs, v_dirs = _grad((col * _t(case.v_colors, dtype)).sum(), (coeffs, dirs))
    norm = _t(case.dirs, torch.float64).pow(2).sum(-1, keepdim=True).sqrt().to(dtype)
    return {"colors": _np(col), "v_coeffs": _np(v_coeffs), "v_dirs": _np(v_dirs * norm)}


def camera_centres(viewmats, dtype=torch.float64):
    """-R^T t [C, 3] from the float32 view-matrix entries."""
    vm = _t(viewmats, dtype)
    return -(vm[:, :3, :3].transpose(1, 2) @ vm[:, :3, 3:4])[..., 0]


def _fused_colors(case, means, coeffs, dtype):
    """clamp_min(sh + 0.5, 0) [C, N, 3] (0.5 where radii <= 0) and sh + 0.5."""
    dirs = means[None] - camera_centres(case.viewmats, dtype)[:, None]
    C, N = case.radii.shape
    sh = sh_eval(case.deg, dirs, coeffs.expand(C, N, -1, -1))
    on = _t(case.radii > 0, dtype)[..., None]
    pre = sh * on + 0.5
    return torch.clamp_min(pre, 0.0), pre


def oracle_fz(case, dtype=torch.float64):
    """sh_colors(): colours [C,N,3], v_coeffs in the coefficients' shape
    (shared [N,K,3]: summed over cameras) and v_means [N,3] summed."""
    means = _t(case.means, dtype, True)
    coeffs = _t(case.coeffs, dtype, True)
    col, pre = _fused_colors(case, means, coeffs, dtype)
    v_coeffs, v_means = _grad((col * _t(case.v_colors, dtype)).sum(), (coeffs, means))
    return {"colors": _np(col), "v_coeffs": _np(v_coeffs), "v_means": _np(v_means),
            "gate": _np(pre)}


def adam_step(p, g, m, v, lr, step, betas, eps):
    """torch.optim.Adam (no weight decay, no amsgrad), 1-based step; lr may be
    an array broadcast over p.  Returns the new (p, m, v)."""
    b1, b2 = betas
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def oracle_adam(case, dtype=torch.float64, steps=None, first_step=1, betas=None):
    """`steps` Adam steps on the coefficients [N,16,3] (row 0 of each with
    lr0, the rest with lr_rest) from the fused colour backward with the same
    cotangents every step.  v_coeffs is the first step's gradient, m1 the
    first moment after it; m / v / p the state after the last step, v_means
    the last step's means gradient.  `betas`: other than ADAM's."""
    steps = ADAM["steps"] if steps is None else steps
    betas = ADAM["betas"] if betas is None else betas
    p = _t(case.coeffs, dtype)
    m, v = _t(case.m_init, dtype), _t(case.v_init, dtype)
    lr = torch.full((16, 1), ADAM["lr_rest"], dtype=dtype)
    lr[0] = ADAM["lr0"]
    out, gates = {}, []
    for s in range(first_step, first_step + steps):
        means = _t(case.means, dtype, True)
        pc = p.clone().requires_grad_(True)
        col, pre = _fused_colors(case, means, pc, dtype)
        g, v_means = _grad((col * _t(case.v_colors, dtype)).sum(), (pc, means))
        gates.append(_np(pre))
        p, m, v = adam_step(p, g, m, v, lr, s, betas, ADAM["eps"])
        if s == first_step:
            out["v_coeffs"], out["m1"] = _np(g), _np(m)
    out.update(m=_np(m), v=_np(v), p=_np(p), v_means=_np(v_means), gate=np.stack(gates))
    return out


def oracle(case, dtype=torch.float64):
    return {"nf": oracle_nf, "fz": oracle_fz, "adam": oracle_adam}[case.kind](case, dtype)


OUTPUTS = {"nf": ("colors", "v_coeffs", "v_dirs"), "fz": ("colors", "v_coeffs", "v_means"),
           "adam": ("v_coeffs", "m", "v", "p", "v_means")}


@functools.lru_cache(maxsize=None)
def oracle64(name):
    """The float64 oracle of a case, computed once and shared read-only."""
    out = oracle(build(name))
    for a in out.values():
        a.setflags(write=False)
    return out


# ===================================================================== cases
def fixed_dirs():
    """+-x, +-y, +-z, six face diagonals, the body diagonal: [13, 3] float64."""
    s2, s3 = math.sqrt(0.5), math.sqrt(1.0 / 3.0)
    return np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                     [s2, s2, 0], [s2, -s2, 0], [s2, 0, s2], [s2, 0, -s2], [0, s2, s2],
                     [0, s2, -s2], [s3, s3, s3]], np.float64)


NFIX = 13
NF_SHAPES = [(1, 1, "on"), (65, 1, "on"), (321, 1, "on"), (321, 1, "rand"), (321, 1, "dead"),
             (321, 3, "rand")]
FZ_SHAPES = [(1, 1, "on", False), (65, 3, "on", False), (321, 1, "rand", False),
             (321, 1, "dead", False), (321, 3, "rand", False), (321, 3, "dead", False),
             (65, 3, "on", True), (321, 3, "rand", True), (321, 3, "dead", True)]
ADAM_SHAPES = [s[:3] for s in FZ_SHAPES if not s[3]]


def nf_k_above(deg):
    """K > (deg+1)^2 for spherical_harmonics (none at degree 4: K <= 25)."""
    return {0: 16, 1: 16, 2: 25, 3: 25}.get(deg)


def fz_k_above(deg):
    """16, the trainer's layout, where it is above (deg+1)^2; 25 at degree 3."""
    return {0: 16, 1: 16, 2: 16, 3: 25}.get(deg)


def _names():
    nf, fz, adam = [], [], []
    for deg in range(5):
        for K in ((deg + 1) ** 2, nf_k_above(deg)):
            if K is not None:
                nf += [f"nf_d{deg}_k{K}_n{N}_c{C}_{mk}" for N, C, mk in NF_SHAPES]
        for K in ((deg + 1) ** 2, fz_k_above(deg)):
            if K is not None:
                fz += [f"fz_d{deg}_k{K}_n{N}_c{C}_{mk}_{'pc' if pc else 'sh'}"
                       for N, C, mk, pc in FZ_SHAPES]
        if deg <= 3:
            adam += [f"adam_d{deg}_k16_n{N}_c{C}_{mk}" for N, C, mk in ADAM_SHAPES]
    return nf, fz, adam


NF_NAMES, FZ_NAMES, ADAM_NAMES = _names()
ALL_NAMES = NF_NAMES + FZ_NAMES + ADAM_NAMES
SAMPLE = "nf_d4_k25_n65_c1_on"  # the case whose reference float64 outputs are stored


def _parse(name):
    f = name.split("_")
    return SimpleNamespace(name=name, kind=f[0], deg=int(f[1][1:]), K=int(f[2][1:]),
                           N=int(f[3][1:]), C=int(f[4][1:]), mask=f[5],
                           percam=len(f) > 6 and f[6] == "pc")


def _unit(g, *shape):
    v = torch.randn(*shape, 3, generator=g, dtype=torch.float64)
    return v / v.norm(dim=-1, keepdim=True)


def _loguniform(g, lo, hi, *shape):
    u = torch.rand(*shape, generator=g, dtype=torch.float64)
    return torch.exp(u * (math.log(hi) - math.log(lo)) + math.log(lo))


def _on_rows(g, C, N, kind):
    """[C, N] bool: all on / 30 % off at random / rows 64..127 off in every
    camera (a dead wave between live ones).  The fixed block stays on."""
    on = torch.ones(C, N, dtype=torch.bool)
    if kind == "rand":
        on = torch.rand(C, N, generator=g) >= 0.3
        on[:, :NFIX] = True
    elif kind == "dead":
        on[:, 64:128] = False
    else:
        assert kind == "on", kind
    return on


def _coeffs(g, *lead_k):
    c = torch.randn(*lead_k, 3, generator=g) * 0.2
    c[..., 0, :] *= 2.5  # randn * 0.5 for the DC term
    return c


def _build_nf(c, g):
    N, C = c.N, c.C
    lead = (N,) if C == 1 else (C, N)
    dirs = _unit(g, *lead) * _loguniform(g, 1e-3, 1e3, *lead)[..., None]
    nfix = min(NFIX, N)
    dirs.view(-1, 3)[:nfix] = torch.from_numpy(fixed_dirs()[:nfix])
    c.dirs = dirs.float().numpy()
    c.coeffs = _coeffs(g, N, c.K).numpy()  # C > 1: broadcast over the cameras
    on = _on_rows(g, C, N, c.mask).view(lead)
    c.masks = None if c.mask == "on" else on.numpy()
    c.v_colors = torch.randn(*lead, 3, generator=g).numpy()
    return c


def _unit4(g, C):
    q = torch.randn(C, 4, generator=g, dtype=torch.float64)
    return q / q.norm(dim=-1, keepdim=True)


def _viewmats(g, C):
    """Rotations of random unit quaternions rounded to float32, |t| about 3."""
    q = _unit4(g, C).float().double()
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
                    -1).reshape(C, 3, 3)
    t = _unit(g, C) * (3.0 * (0.8 + 0.4 * torch.rand(C, 1, generator=g, dtype=torch.float64)))
    vm = torch.eye(4, dtype=torch.float64).repeat(C, 1, 1)
    vm[:, :3, :3] = R
    vm[:, :3, 3] = t
    return vm.float().numpy()


def fused_distance_ratio(case):
    """|mean - centre_c| / |t_c| [C, N] in float64."""
    ctr = camera_centres(case.viewmats)
    d = _t(case.means, torch.float64)[None] - ctr[:, None]
    return (d.norm(dim=-1) / ctr.norm(dim=-1)[:, None]).numpy()


def _build_fused(c, g):
    """Inputs of sh_colors() (kind fz) and of the fused Adam (kind adam)."""
    N, C = c.N, c.C
    c.viewmats = _viewmats(g, C)
    ctr = camera_centres(c.viewmats)
    tn = ctr.norm(dim=-1)

    def ok(m):  # float32 means within [0.25, 4] |t| of every camera
        r = (m.float().double()[None] - ctr[:, None]).norm(dim=-1) / tn[:, None]
        return ((r >= 0.25) & (r <= 4.0)).all(0)

    means = torch.zeros(N, 3, dtype=torch.float64)
    todo = torch.ones(N, dtype=torch.bool)
    for _ in range(200):
        n = int(todo.sum())
        if n == 0:
            break
        means[todo] = ctr[0] + _unit(g, n) * (tn[0] * _loguniform(g, 0.25, 4.0, n))[:, None]
        todo = ~ok(means)
    assert not todo.any(), c.name
    c.nfix = 0
    if c.kind == "fz":  # the fixed block, seen from camera 0
        c.nfix = min(NFIX, N)
        for scale in (1.0, 2.0, 0.5, 3.0, 1.5):
            blk = ctr[0] + torch.from_numpy(fixed_dirs()[:c.nfix]) * (tn[0] * scale)
            if ok(blk).all():
                break
        else:
            raise AssertionError(f"{c.name}: no place for the fixed directions")
        means[:c.nfix] = blk
    c.means = means.float().numpy()
    on = _on_rows(g, C, N, c.mask)
    c.radii = torch.where(on, torch.randint(1, 20, (C, N), generator=g),
                          torch.zeros(C, N, dtype=torch.int64)).to(torch.int32).numpy()
    c.v_colors = torch.randn(C, N, 3, generator=g).numpy()
    lead = (C, N) if c.percam else (N,)
    coeffs = _coeffs(g, *lead, c.K)
    c.m_init = np.zeros((N, c.K, 3), np.float32)
    c.v_init = np.zeros((N, c.K, 3), np.float32)

    def gate(cf):
        """sh + 0.5 of the visible rows [..., C, N, 3]; inf elsewhere."""
        c.coeffs = cf.numpy()
        pre = torch.from_numpy(oracle(c)["gate"])
        return torch.where(on[..., None], pre, torch.full_like(pre, float("inf")))

    # about half the visible rows get a closed channel: one DC shift for all
    pre = gate(coeffs)[0] if c.kind == "adam" else gate(coeffs)
    vis = pre[on]
    shift = 0.0
    if vis.shape[0] >= 8:
        shift = float(np.float32(-vis.min(-1).values.median().item() / B0))
        coeffs[..., 0, :] += shift
    # no channel within the margin of the gate (adam: at any step)
    for _ in range(200):
        pre = gate(coeffs)
        near = (pre.abs() < GATE_MARGIN).reshape(-1, C, N, 3).any(-1).any(0).any(0)  # [N]
        if not near.any():
            break
        fresh = _coeffs(g, *lead, c.K)
        fresh[..., 0, :] += shift
        coeffs[..., near, :, :] = fresh[..., near, :, :]
    else:
        raise AssertionError(f"{c.name}: rows left within the gate margin")
    c.coeffs = coeffs.numpy()
    return c


@functools.lru_cache(maxsize=None)
def build(name):
    """The case of that name (float32 / int32 / bool numpy arrays, read-only)."""
    c = _parse(name)
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    c = _build_nf(c, g) if c.kind == "nf" else _build_fused(c, g)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def gate_stats(case):
    """(smallest |sh + 0.5| over the visible rows' channels, share of visible
    rows with a closed channel), from the float64 oracle (adam: all steps)."""
    pre = oracle64(case.name)["gate"].reshape(-1, case.C, case.N, 3)
    on = case.radii > 0
    vis = pre[:, on]  # [steps, rows, 3]
    return float(np.abs(vis).min()), float((vis[0] < 0).any(-1).mean())


# ================================================================ comparison
def rel_err(ours, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(ours, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def load_bars(path):
    """{"<case>:<output>": bar} from sh_matrix.npz."""
    z = np.load(path)
    return dict(zip((str(k) for k in z["bar_names"]), (float(v) for v in z["bar_values"])))


def bound(bar):
    return max(FACTOR * bar, FLOOR)
