"""Float64 oracle and seeded cases for the similarity transform of splat scenes
(gsplat_hip/transform.py, csrc/transform.hip).  Host only: numpy, no GPU
import.

The oracle is written from the definitions, not from the kernels' method:

    x' = A x + t,  A = s R:  s = det(A)^(1/3),  R = the orthogonal polar factor
        of A / s (numpy's SVD: U V^T)
    means'  = A means + t
    quats'  = q_R (x) quats  (wxyz, Hamilton product; q_R from R by the trace
              formula, or from the largest diagonal entry when the trace is
              not positive)
    scales' = scales + log s
    shN'    : per degree l the 2l+1 coefficients of each channel times M_l(R),
              M_l = the least-squares solution of  Y_l(D) M = Y_l(D R)  over
              N_DIRS seeded random unit directions D (rows), which is the
              defining identity  sum_k a'_k Y_k(d) = sum_k a_k Y_k(R^T d)
              imposed at those directions.  Y: `basis`, a restatement of the
              constants of csrc/sh_basis.h.

`oracle(case, dtype)` runs everything in `dtype`: float64 is the reference;
the float32 run's error against it, max err / max |oracle| per output, is the
`bar` that tests/golden/make_golden_transform.py stores.  Tests bound errors
by max(FACTOR x bar, FLOOR).

Quaternions are compared through their norm and the rotation matrix of the
normalised quaternion (`quat_views`): q and -q are the same rotation, and a
q_R near w = 0 may take either sign.

Cases are named; the seed comes from the name (zlib.crc32).  They hold float32
arrays, which the oracle promotes.
"""

import zlib
from types import SimpleNamespace

import numpy as np

FACTOR = 4.0
FLOOR = 1e-6
N_DIRS = 400
OUTPUTS = ("means", "scales", "shN", "quat_norm", "quat_rot")


def seed_of(name):
    return zlib.crc32(name.encode())


# ==================================================================== oracle
def basis(d, L):
    """Y_k(d), k < (L+1)^2, at unit directions d [n,3], in d's dtype."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    T = d.dtype.type
    B = [np.full_like(x, T(0.28209479177387814))]
    if L >= 1:
        B += [T(-0.4886025119029199) * y, T(0.4886025119029199) * z, T(-0.4886025119029199) * x]
    if L >= 2:
        B += [T(1.0925484305920792) * x * y, T(-1.0925484305920792) * y * z,
              T(0.9461746957575601) * z * z - T(0.3153915652525201),
              T(-1.0925484305920792) * x * z, T(0.5462742152960396) * (x * x - y * y)]
    if L >= 3:
        B += [T(-0.5900435899266435) * y * (T(3) * x * x - y * y),
              T(2.890611442640554) * x * y * z,
              T(0.4570457994644658) * y * (T(1) - T(5) * z * z),
              T(0.3731763325901154) * z * (T(5) * z * z - T(3)),
              T(0.4570457994644658) * x * (T(1) - T(5) * z * z),
              T(1.445305721320277) * z * (x * x - y * y),
              T(-0.5900435899266435) * x * (x * x - T(3) * y * y)]
    if L >= 4:
        x2, y2, z2 = x * x, y * y, z * z
        B += [T(2.5033429417967046) * x * y * (x2 - y2),
              T(-1.7701307697799304) * y * z * (T(3) * x2 - y2),
              T(0.9461746957575601) * x * y * (T(7) * z2 - T(1)),
              T(-0.6690465435572892) * y * z * (T(7) * z2 - T(3)),
              T(0.10578554691520431) * (T(35) * z2 * z2 - T(30) * z2 + T(3)),
              T(-0.6690465435572892) * x * z * (T(7) * z2 - T(3)),
              T(0.47308734787878004) * (x2 - y2) * (T(7) * z2 - T(1)),
              T(-1.7701307697799304) * x * z * (x2 - T(3) * y2),
              T(0.6258357354491761) * (x2 * (x2 - T(3) * y2) - y2 * (T(3) * x2 - y2))]
    return np.stack(B, -1)


def unit_dirs(n, seed, dtype=np.float64):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(dtype)


def sh_blocks(R, L):
    """[M_1 .. M_L] of one rotation R [3,3], in R's dtype."""
    D = unit_dirs(N_DIRS, 12345, R.dtype)
    out = []
    for l in range(1, L + 1):
        Y = basis(D, l)[:, l * l:]
        Yr = basis(D @ R, l)[:, l * l:]          # rows (R^T d)^T
        out.append(np.linalg.lstsq(Y, Yr, rcond=None)[0].astype(R.dtype))
    return out


def decompose(T):
    """One [4,4] -> (A, t, s, R) in T's dtype."""
    A, t = T[:3, :3], T[:3, 3]
    s = np.linalg.det(A) ** T.dtype.type(1.0 / 3.0)
    U, _, Vt = np.linalg.svd(A / s)
    return A, t, s, (U @ Vt).astype(T.dtype)


def rotmat_to_quat(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        w = np.sqrt(1 + tr) / 2
        q = [w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w),
             (R[1, 0] - R[0, 1]) / (4 * w)]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        v = np.sqrt(1 + R[i, i] - R[j, j] - R[k, k]) / 2
        q = [0, 0, 0, 0]
        q[0] = (R[k, j] - R[j, k]) / (4 * v)
        q[1 + i] = v
        q[1 + j] = (R[j, i] + R[i, j]) / (4 * v)
        q[1 + k] = (R[k, i] + R[i, k]) / (4 * v)
    return np.array(q, R.dtype)


def quat_mul(a, b):
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw], -1)


def quat_to_rotmat(q):
    """Rotation matrices of unit quaternions [...,4] wxyz."""
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
                    -1).reshape(q.shape[:-1] + (3, 3))


def quat_views(q):
    """(norm [N], rotation matrix of q / |q| [N,3,3]) in float64."""
    q = np.asarray(q, np.float64)
    n = np.linalg.norm(q, axis=-1)
    return n, quat_to_rotmat(q / n[:, None])


def oracle(case, dtype=np.float64):
    """-> dict(means, quats, scales, shN) in `dtype`."""
    c = SimpleNamespace(**{k: (v.astype(dtype) if v.dtype == np.float32 else v)
                           for k, v in vars(case).items() if isinstance(v, np.ndarray)})
    out = {k: getattr(c, k).copy() for k in ("means", "quats", "scales", "shN")}
    ids = case.ids if case.ids is not None else np.zeros(case.N, np.int64)
    for s_i in range(len(c.transforms)):
        rows = np.nonzero(ids == s_i)[0]
        if rows.size == 0:
            continue
        A, t, s, R = decompose(c.transforms[s_i])
        out["means"][rows] = c.means[rows] @ A.T + t
        out["quats"][rows] = quat_mul(rotmat_to_quat(R)[None], c.quats[rows])
        out["scales"][rows] = c.scales[rows] + np.log(s)
        at = 0
        for l, M in enumerate(sh_blocks(R, case.deg), start=1):
            n = 2 * l + 1
            out["shN"][rows, at:at + n] = np.einsum("ij,njc->nic", M, c.shN[rows, at:at + n])
            at += n
    return out


def views(res):
    """The compared outputs of a result dict (any float type) in float64."""
    qn, qr = quat_views(res["quats"])
    return {"means": np.asarray(res["means"], np.float64),
            "scales": np.asarray(res["scales"], np.float64),
            "shN": np.asarray(res["shN"], np.float64), "quat_norm": qn, "quat_rot": qr}


def rel_err(got, want):
    """max err / max |oracle| (0 for an empty array)."""
    if want.size == 0:
        return 0.0
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def bound(bar):
    return max(FACTOR * float(bar), FLOOR)


# ===================================================================== cases
def rotation(kind, rng):
    """A float64 rotation matrix of the named kind."""
    if kind == "identity":
        return np.eye(3)
    if kind == "generic":
        q = rng.normal(size=4)
    elif kind in ("axis_x", "axis_y", "axis_z"):
        a = rng.uniform(0.3, 2.5)
        q = np.zeros(4)
        q[0], q["xyz".index(kind[-1]) + 1] = np.cos(a / 2), np.sin(a / 2)
    elif kind == "pi":                      # by pi about a random axis: w = 0
        q = np.concatenate([[0.0], rng.normal(size=3)])
    else:
        raise ValueError(kind)
    return quat_to_rotmat(q / np.linalg.norm(q))


#        name                N    deg S    ids        rotations             scale  tmax
SPECS = [
    ("n1_d3_generic",        1,    3, 1,   None,      ("generic",),         1.0,   1.0),
    ("n63_d1_axis",          63,   1, 1,   None,      ("axis_z",),          0.01,  10.0),
    ("n64_d2_pi",            64,   2, 1,   None,      ("pi",),              37.0,  1e3),
    ("n65_d4_generic",       65,   4, 1,   None,      ("generic",),         0.01,  1e3),
    ("n257_d0_generic",      257,  0, 1,   None,      ("generic",),         37.0,  100.0),
    ("n257_d4_s3",           257,  4, 3,   "unsorted", ("generic", "pi", "axis_x"), 1.0, 10.0),
    ("n1000_d3_identity",    1000, 3, 1,   None,      ("identity",),        1.0,   0.0),
    ("n1000_d3_s300",        1000, 3, 300, "random",  None,                 None,  1e3),
    ("n1000_d2_axis_y",      1000, 2, 1,   None,      ("axis_y",),          37.0,  1.0),
]
NAMES = [s[0] for s in SPECS]
_KINDS = ("generic", "axis_x", "axis_y", "axis_z", "pi", "identity")
_SCALES = (0.01, 1.0, 37.0)


def make_case(name):
    _, N, deg, S, idk, kinds, scale, tmax = SPECS[NAMES.index(name)]
    rng = np.random.default_rng(seed_of(name))
    T = np.zeros((S, 4, 4))
    for s_i in range(S):
        kind = kinds[s_i] if kinds is not None else _KINDS[s_i % len(_KINDS)]
        sc = scale if scale is not None else _SCALES[s_i % 3]
        T[s_i, :3, :3] = sc * rotation(kind, rng)
        T[s_i, :3, 3] = rng.uniform(-1, 1, 3) * tmax
        T[s_i, 3, 3] = 1
    if idk is None:
        ids = None
    elif idk == "unsorted":                 # segment 1 stays empty
        ids = rng.choice(np.array([0, 2], np.int64), size=N)
    else:
        ids = rng.integers(0, S, size=N, dtype=np.int64)
    K1 = (deg + 1) ** 2 - 1
    return SimpleNamespace(
        name=name, N=N, deg=deg, S=S, ids=ids,
        transforms=T.astype(np.float32),
        means=(rng.normal(size=(N, 3)) * 3).astype(np.float32),
        quats=(rng.normal(size=(N, 4)) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32),
        scales=rng.uniform(-6, 0, (N, 3)).astype(np.float32),
        shN=(rng.normal(size=(N, K1, 3)) * 0.3).astype(np.float32))


def splats_of(case, torch, device=None):
    """The case as a torch splat dict (plus sh0 and opacities, which pass
    through), and (transforms, segment_ids) tensors."""
    rng = np.random.default_rng(seed_of(case.name) + 1)
    d = {"means": case.means, "quats": case.quats, "scales": case.scales,
         "opacities": rng.normal(size=case.N).astype(np.float32),
         "sh0": rng.uniform(-1, 1, (case.N, 1, 3)).astype(np.float32), "shN": case.shN}
    d = {k: torch.from_numpy(v.copy()).to(device or "cpu") for k, v in d.items()}
    T = torch.from_numpy(case.transforms.copy()).to(device or "cpu")
    ids = None if case.ids is None else torch.from_numpy(case.ids.copy()).to(device or "cpu")
    return d, T, ids


# ============================================================== render check
def similarity(scale, kind, tmax, seed):
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    T[:3, :3] = scale * rotation(kind, rng)
    T[:3, 3] = rng.uniform(-1, 1, 3) * tmax
    return T


def move_camera(viewmat, T):
    """World-to-camera matrix of the camera moved with the scene: c' = s R c +
    t, R_c' = R R_c.  Camera-space coordinates scale by s."""
    A, t = T[:3, :3], T[:3, 3]
    s = np.linalg.det(A) ** (1.0 / 3.0)
    R = A / s
    c2w = np.linalg.inv(viewmat)
    out = np.eye(4)
    out[:3, :3] = R @ c2w[:3, :3]
    out[:3, 3] = A @ c2w[:3, 3] + t
    return np.linalg.inv(out), s


def render_scene(seed=3, stride=56, deg=3, W=64, H=64):
    """The garden crop's every `stride`-th point (~2,000 Gaussians), camera 0
    at W x H, random rotations, log-scales, opacities and shN.  Seed 3: the
    float32 run of the oracle's render has no alpha-threshold flip against the
    float64 run, before or after the move (make_golden_transform.py asserts
    it; seeds 0, 1 and 6 have some)."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = np.load(os.path.join(root, "tests", "golden", "garden_scene.npz"))
    means = d["means3d"].astype(np.float32)[::stride]
    rgb = d["colors"].astype(np.float32)[::stride] / 255.0
    K = d["Ks"][0].astype(np.float64).copy()
    K[0] *= W / int(d["width"])
    K[1] *= H / int(d["height"])
    N = len(means)
    rng = np.random.default_rng(seed)
    K1 = (deg + 1) ** 2 - 1
    splats = {"means": means,
              "quats": rng.normal(size=(N, 4)).astype(np.float32),
              "scales": np.log(rng.uniform(0.02, 0.12, (N, 3))).astype(np.float32),
              "opacities": rng.normal(size=N).astype(np.float32),
              "sh0": ((rgb - 0.5) / 0.28209479177387814)[:, None, :].astype(np.float32),
              "shN": (rng.normal(size=(N, K1, 3)) * 0.25).astype(np.float32)}
    return splats, d["viewmats"][0].astype(np.float64), K, W, H


def render(splats, viewmat, K, W, H, deg, near, far, dtype):
    """The numpy oracle's render of a pre-activation splat dict in `dtype`:
    [H,W,3].  The tile lists are sorted by the depth in `dtype`."""
    from oracle import gsplat_oracle as O
    ts = 16
    tw, th = -(-W // ts), -(-H // ts)
    with O.precision(dtype):
        f = lambda a: np.asarray(a, dtype)  # noqa: E731
        means, quats = f(splats["means"]), f(splats["quats"])
        scales = np.exp(f(splats["scales"]))
        opac = 1 / (1 + np.exp(-f(splats["opacities"])))
        vm, Kc = f(viewmat)[None], f(K)[None]
        radii, m2, depths, conics, _ = O.proj_fwd(means, quats, scales, vm, Kc, W, H,
                                                  near=near, far=far)
        campos = np.linalg.inv(f(viewmat))[:3, 3]
        dirs = means - campos[None]
        dirs = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
        coeffs = np.concatenate([f(splats["sh0"]), f(splats["shN"])], 1)
        colors = np.maximum(O.sh_fwd(deg, dirs, coeffs) + dtype(0.5), 0)
        _, ids, fids = O.isect_tiles(m2, radii, np.zeros_like(depths), ts, tw, th, sort=False)
        tile = ids >> 32
        order = np.lexsort((depths.reshape(-1)[fids], tile))
        ids, fids = tile[order] << 32, fids[order]
        off = O.isect_offset_encode(ids, 1, tw, th)
        img, _, _ = O.raster_fwd(m2, conics, colors[None], opac[None], None, W, H, ts, off, fids)
    return np.asarray(img[0], np.float64)
