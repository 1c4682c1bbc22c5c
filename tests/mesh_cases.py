"""Scenes and a numpy oracle for the mesh-export tests (test_mesh_host.py,
test_gpu_mesh.py).  The oracle restates gsplat_hip.mesh's integrate rule and
the extraction's ordering contract; it runs in the dtype it is given (float64
as the reference, float32 for the rounding bar) and takes the marching-cubes
case table as an argument.

The kernels' inputs are float32 numbers (origin, voxel size, truncations,
matrices, images): the oracle evaluates the rule on those same numbers, so a
parameter such as 0.1 is rounded to float32 first in either dtype.
"""

import itertools

import numpy as np

NEAR_PIX = 1e-4  # a pair this close (in pixels) to a pixel boundary or image edge, or
NEAR_CUT = 1e-4  # this close (times sdf_trunc) to the -sdf_trunc cut, may flip in float32


def f32(x):
    return np.asarray(x, dtype=np.float32)


# ---------------------------------------------------------------- cameras --
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """World-to-camera [4, 4] (float64) of a camera at `eye` looking at
    `target`: +z forward, +x right, +y down."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    V = np.eye(4)
    V[:3, :3] = R
    V[:3, 3] = -R @ eye
    return V


def intrinsics(f, W, H):
    return np.array([[f, 0.0, 0.5 * W], [0.0, f, 0.5 * H], [0.0, 0.0, 1.0]])


def analytic_depth(viewmat, K, W, H, center, radius, plane_n, plane_b):
    """z-depth at the pixel centres of the nearer of a sphere and the plane
    plane_n . x = plane_b, 0 where the ray hits neither.  [H, W] float64."""
    R, t = viewmat[:3, :3], viewmat[:3, 3]
    o = -R.T @ t
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d_cam = np.stack([(px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1], np.ones_like(px)], -1)
    d = d_cam @ R  # R^T d_cam per pixel; the ray parameter is the z-depth
    oc = o - np.asarray(center, dtype=np.float64)
    a = (d * d).sum(-1)
    b = 2.0 * (d @ oc)
    c = oc @ oc - radius * radius
    disc = b * b - 4.0 * a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        s_sph = np.where(disc > 0.0, (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a), np.inf)
        s_sph = np.where(s_sph > 0.0, s_sph, np.inf)
        n = np.asarray(plane_n, dtype=np.float64)
        den = d @ n
        s_pl = np.where(np.abs(den) > 1e-12, (plane_b - n @ o) / den, np.inf)
        s_pl = np.where(s_pl > 0.0, s_pl, np.inf)
    s = np.minimum(s_sph, s_pl)
    return np.where(np.isfinite(s), s, 0.0)


# ------------------------------------------------------- integrate oracle --
def grid_points(origin, h, dims, dtype):
    """x, y, z of every grid point, flattened in [nz, ny, nx] order."""
    nx, ny, nz = dims
    o, h = f32(origin).astype(dtype), dtype(np.float32(h))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (o[0] + h * i.ravel().astype(dtype), o[1] + h * j.ravel().astype(dtype),
            o[2] + h * k.ravel().astype(dtype))


def integrate_oracle(state, origin, h, dims, depths, viewmats, Ks, colors=None, alphas=None,
                     sdf_trunc=None, depth_trunc=np.inf, alpha_min=0.5, dtype=np.float64):
    """Fuses the C views into `state` = dict(tsdf, weight[, color]) of flat
    arrays of `dtype` ([n] and [3, n]), in place, and returns per (camera,
    voxel) the flags `updated` and `near` (the pair may flip in float32)."""
    dtype = np.dtype(dtype).type
    x, y, z = grid_points(origin, h, dims, dtype)
    trunc = dtype(np.float32(sdf_trunc))
    dtr = dtype(np.float32(depth_trunc))
    amin = dtype(np.float32(alpha_min))
    C, H, W = depths.shape[:3]
    depths = f32(depths).reshape(C, H * W).astype(dtype)
    if alphas is not None:
        alphas = f32(alphas).reshape(C, H * W).astype(dtype)
    if colors is not None:
        colors = f32(colors).reshape(C, H * W, 3).astype(dtype)
    tsdf, w = state["tsdf"], state["weight"]
    n = tsdf.shape[0]
    updated = np.zeros((C, n), dtype=bool)
    near = np.zeros((C, n), dtype=bool)
    one = dtype(1.0)
    for c in range(C):
        V, K = f32(viewmats[c]).astype(dtype), f32(Ks[c]).astype(dtype)
        pc = [V[r, 0] * x + V[r, 1] * y + V[r, 2] * z + V[r, 3] for r in range(3)]
        ok = pc[2] > 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u = K[0, 0] * pc[0] / pc[2] + K[0, 2]
            v = K[1, 1] * pc[1] / pc[2] + K[1, 2]
        ok &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
        with np.errstate(invalid="ignore"):
            around = (pc[2] > 0) & (u > -1) & (u < W + 1) & (v > -1) & (v < H + 1)
            near[c] = around & ((np.abs(u - np.rint(u)) < NEAR_PIX)
                                | (np.abs(v - np.rint(v)) < NEAR_PIX))
        pix = np.zeros(n, dtype=np.int64)
        pix[ok] = np.floor(v[ok]).astype(np.int64) * W + np.floor(u[ok]).astype(np.int64)
        d = depths[c][pix]
        ok &= (d > 0) & (d <= dtr)
        if alphas is not None:
            ok &= alphas[c][pix] >= amin
        sdf = d - pc[2]
        near[c] |= ok & (np.abs(sdf + trunc) < NEAR_CUT * trunc)
        ok &= ~(sdf < -trunc)
        s = np.minimum(one, sdf / trunc)
        w1 = w + one
        tsdf[ok] = ((tsdf * w + s) / w1)[ok]
        if colors is not None:
            for ch in range(3):
                plane = state["color"][ch]
                plane[ok] = ((plane * w + colors[c][pix, ch]) / w1)[ok]
        w[ok] = w1[ok]
        updated[c] = ok
    return updated, near


def empty_state(dims, colors, dtype):
    n = dims[0] * dims[1] * dims[2]
    st = {"tsdf": np.zeros(n, dtype), "weight": np.zeros(n, dtype)}
    if colors:
        st["color"] = np.zeros((3, n), dtype)
    return st


# --------------------------------------------------------- integrate scene --
class IntegrateScene:
    """25 x 19 x 17 grid points (no multiple of 4 or 64 along x, several
    workgroups), h = 0.1, sdf_trunc = 4 h, a sphere over a floor plane, and
    48 x 40 look-at cameras with the analytic z-depth at the pixel centres.
    Pixels that hit nothing have depth 0; the far floor lies beyond
    depth_trunc; a patch of each image has alpha below alpha_min; the narrow
    field of view leaves voxels outside the image; the third camera looks away
    from the volume (every voxel behind it: it sees nothing).  `second`: three
    more cameras for an integrate on top of the first."""

    dims = (25, 19, 17)
    h = 0.1
    origin = (-1.2, -0.9, -0.8)
    sdf_trunc = 0.4
    depth_trunc = 3.75
    alpha_min = 0.5
    W, H = 48, 40
    center, radius = (0.05, -0.02, 0.03), 0.7
    plane_n, plane_b = (0.0, 0.0, 1.0), -0.72  # the floor z = -0.72

    EYES = [((2.31, 1.43, 1.07), 62.0), ((-1.87, 2.21, 0.93), 55.0), ((0.4, -3.3, 0.6), 50.0)]
    EYES2 = [((1.13, -2.57, 1.21), 58.0), ((-2.63, -0.97, 1.33), 52.0), ((0.37, 0.91, 2.93), 60.0)]

    def __init__(self, seed=0):
        rng = np.random.default_rng(seed)
        self.first = self._views(self.EYES, rng, away=2)
        self.second = self._views(self.EYES2, rng, away=None)

    def _views(self, eyes, rng, away):
        vms, Ks, depths, alphas = [], [], [], []
        for n, (eye, f) in enumerate(eyes):
            eye = np.asarray(eye)
            target = np.asarray(self.center) + (0.03 * n, -0.02 * n, 0.01)
            if n == away:  # looks away from the volume
                target = 2.0 * eye - target
            V, K = look_at(eye, target), intrinsics(f, self.W, self.H)
            # the images are rendered with the float32 matrices the kernel gets
            V32, K32 = f32(V).astype(np.float64), f32(K).astype(np.float64)
            d = analytic_depth(V32, K32, self.W, self.H, self.center, self.radius, self.plane_n,
                               self.plane_b)
            a = np.where(d > 0.0, 1.0, 0.0)
            a[5 + 3 * n:12 + 3 * n, 20:31] = 0.3  # below alpha_min
            vms.append(V)
            Ks.append(K)
            depths.append(d)
            alphas.append(a)
        C = len(eyes)
        return dict(viewmats=f32(np.stack(vms)), Ks=f32(np.stack(Ks)), depths=f32(np.stack(depths)),
                    alphas=f32(np.stack(alphas)),
                    colors=f32(rng.random((C, self.H, self.W, 3))))

    def oracle(self, views, dtype, state=None, colors=True):
        """(state, updated, near) after fusing `views` (a list of view dicts,
        in order) into `state` (default: an empty volume)."""
        st = empty_state(self.dims, colors, dtype) if state is None else state
        ups, nears = [], []
        for v in views:
            u, n = integrate_oracle(st, self.origin, self.h, self.dims, v["depths"],
                                    v["viewmats"], v["Ks"], v["colors"] if colors else None,
                                    v["alphas"], self.sdf_trunc, self.depth_trunc,
                                    self.alpha_min, dtype)
            ups.append(u)
            nears.append(n)
        return st, np.concatenate(ups), np.concatenate(nears)


# ------------------------------------------------------- extraction oracle --
def edge_owner(e):
    """(dx, dy, dz, axis) of table edge e = 4 axis + r: the edge runs along
    `axis` from the corner whose other two coordinates are (r & 1, r >> 1)."""
    axis, r = e >> 2, e & 3
    others = [a for a in range(3) if a != axis]
    p = [0, 0, 0]
    p[others[0]], p[others[1]] = r & 1, r >> 1
    return p[0], p[1], p[2], axis


def extract_oracle(table, tsdf, weight, origin, h, color=None, min_weight=0.0):
    """The indexed mesh of the extraction contract in float64: (vertices
    [V, 3], faces [F, 3] int64, colors [V, 3] or None, owners [V, 4] = the
    (i, j, k, axis) of each vertex's grid edge, cases [n_cells_valid])."""
    nz, ny, nx = tsdf.shape
    dims = (nx, ny, nz)
    tsdf = np.asarray(tsdf, dtype=np.float64)
    inside = tsdf < 0
    w_ok = np.asarray(weight) > np.float32(min_weight)
    cellv = np.zeros((nz, ny, nx), dtype=bool)
    if min(dims) > 1:
        cv = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
        for dz, dy, dx in itertools.product((0, 1), repeat=3):
            cv &= w_ok[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1]
        cellv[:nz - 1, :ny - 1, :nx - 1] = cv
    o = f32(origin).astype(np.float64)
    h = float(np.float32(h))
    vid = -np.ones((nz, ny, nx, 3), dtype=np.int64)
    verts, cols, owners = [], [], []
    for k, j, i in itertools.product(range(nz), range(ny), range(nx)):
        p = (i, j, k)
        for ax in range(3):
            q = list(p)
            q[ax] += 1
            if q[ax] >= dims[ax] or inside[k, j, i] == inside[q[2], q[1], q[0]]:
                continue
            u, v = [a for a in range(3) if a != ax]
            used = False
            for b, c in itertools.product((0, 1), repeat=2):
                cell = list(p)
                cell[u] -= b
                cell[v] -= c
                if cell[u] >= 0 and cell[v] >= 0 and cellv[cell[2], cell[1], cell[0]]:
                    used = True
            if not used:
                continue
            va, vb = tsdf[k, j, i], tsdf[q[2], q[1], q[0]]
            t = va / (va - vb)
            pa, pb = o + h * np.array(p, dtype=np.float64), o + h * np.array(q, dtype=np.float64)
            vid[k, j, i, ax] = len(verts)
            verts.append(pa + t * (pb - pa))
            owners.append((i, j, k, ax))
            if color is not None:
                ca = np.asarray(color[:, k, j, i], dtype=np.float64)
                cb = np.asarray(color[:, q[2], q[1], q[0]], dtype=np.float64)
                cols.append(ca + t * (cb - ca))
    faces, cases = [], []
    for k, j, i in itertools.product(range(nz - 1), range(ny - 1), range(nx - 1)):
        if not cellv[k, j, i]:
            continue
        cs = 0
        for c in range(8):
            if inside[k + (c >> 2), j + ((c >> 1) & 1), i + (c & 1)]:
                cs |= 1 << c
        cases.append(cs)
        row = [int(e) for e in table[cs] if e >= 0]
        for m in range(0, len(row), 3):
            tri = []
            for e in row[m:m + 3]:
                dx, dy, dz, ax = edge_owner(e)
                n = vid[k + dz, j + dy, i + dx, ax]
                assert n >= 0, (i, j, k, cs, e)
                tri.append(n)
            faces.append(tri)
    V = np.array(verts, dtype=np.float64).reshape(-1, 3)
    F = np.array(faces, dtype=np.int64).reshape(-1, 3)
    Cc = np.array(cols, dtype=np.float64).reshape(-1, 3) if color is not None else None
    return V, F, Cc, np.array(owners, dtype=np.int64).reshape(-1, 4), np.array(cases)


def half_edges(faces, owners, dims):
    """(directed half-edges that occur more than once, unmatched half-edges
    that do not lie in an outer face of the grid)."""
    faces = np.asarray(faces, dtype=np.int64)
    he = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    assert (he[:, 0] != he[:, 1]).all()
    nv = int(faces.max()) + 1 if faces.size else 1
    key = he[:, 0] * nv + he[:, 1]
    uniq, counts = np.unique(key, return_counts=True)
    repeated = int((counts > 1).sum())
    have = set(uniq.tolist())
    bad = 0
    for a, b in he[~np.isin(he[:, 1] * nv + he[:, 0], uniq)]:
        assert (b * nv + a) not in have
        if not _share_outer_face(owners[a], owners[b], dims):
            bad += 1
    return repeated, bad


def _share_outer_face(oa, ob, dims):
    """Both vertices (grid edges (i, j, k, axis)) lie in one outer face."""
    for d in range(3):
        for side in (0, dims[d] - 1):
            if all(o[3] != d and o[d] == side for o in (oa, ob)):
                return True
    return False


def random_field(n=21, seed=0):
    """The i.i.d. normal field of the table's manifoldness check: [n, n, n]
    float32 from default_rng(seed), then colours [3, n, n, n] and weights with
    about 10 % zeros from the same generator."""
    rng = np.random.default_rng(seed)
    tsdf = f32(rng.standard_normal((n, n, n)))
    color = f32(rng.random((3, n, n, n)))
    weight = f32(np.where(rng.random((n, n, n)) < 0.1, 0.0, rng.integers(1, 5, (n, n, n))))
    return tsdf, color, weight


def sphere_field(n=33, h=0.05, r_cells=10, trunc_cells=5):
    """The exact SDF of a sphere of radius r_cells * h about the volume's
    centre, clamped to +-trunc_cells * h, over sdf_trunc: (tsdf [n, n, n]
    float32, origin, h, radius, centre)."""
    origin = np.full(3, -0.5 * (n - 1) * h)
    ax = origin[0] + h * np.arange(n)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    r = r_cells * h
    sdf = np.sqrt(x * x + y * y + z * z) - r
    trunc = trunc_cells * h
    return f32(np.clip(sdf, -trunc, trunc) / trunc), origin, h, r, np.zeros(3)
