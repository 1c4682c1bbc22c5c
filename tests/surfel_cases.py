"""Float64 oracle and seeded cases for the 2DGS rasterizer (csrc/surfel.hip,
csrc/surfel_cull.h).  Host only: torch on the CPU, no GPU import.

The oracle is written from the definitions, not from the kernels' listing.
Per pixel centre p = (x + 0.5, y + 0.5) and per record of the pixel's tile, in
the tile's isect order, with ray transform rows u, v, w:

    hu = p_x w - u,  hv = p_y w - v,  r = hu x hv,  s = r_xy / r_z   (r_z != 0)
    g3 = |s|^2,  g2 = 2 |mean2d - p|^2,  sigma = min(g3, g2) / 2
    alpha = min(0.999, opacity exp(-sigma));  alpha < float32(1/255): no hit
    nT = T (1 - alpha);  nT <= 1e-4: the pixel is finished, the record unused
    w = alpha T:  colour += w c,  normal += w n,
                  distortion += 2 w (d A - B)   (A = 1 - T, B = sum of earlier
                  w d, d the record's last colour channel)
    median = d and median id = the isect while T > 0.5;  last id = the isect
    T = nT

colours = colour + T background, alphas = 1 - T.  A masked tile is the
background colour with everything else empty.  The walk runs every tile in
lockstep (padded to the longest), sequential over a tile's isects and
vectorised over pixels; thresholds are the float32 constants of the reference.

Gradients are float64 autograd of sum(cotangent x output).  v_means2d_abs is
the sum over pixels of |gradient| wrt a per-pixel copy of the mean kept in the
graph; v_densify is (v_rt[0,2], v_rt[1,2]) rt[2,2]; v_backgrounds comes from
the same graph.  Two conventions differ from plain autograd, each expressed
in one place: `padded_background_gradient` (a padded channel count drops the
depth channel's background) and `zero_depth_background`: the reference's
backward reads the distortion's depth sum back from render_colors, exact only
with a zero depth background, which is what rasterization_2dgs passes; the
cases hold it to 0.
Where g3 == g2 or opacity vis == 0.999 exactly the gradient follows g3 and
the unclamped branch (`<=`), as the reference.

The 33-channel evaluation of a (case, tile size) is computed once
(`graph64`, lru_cache); a render of D channels is channels 0..D-2 and the
last one (`channels`), since a channel's image depends on no other channel
but the depth, which stays last.

Cases are named; the seed comes from the name (zlib.crc32).  They hold
float32 arrays.  sparse / dense / thin follow tests/test_surfel_oracle.py's
surfel_scene (3-D surfels through oracle/surfel_oracle.py's projection);
cull, edge and gate_alpha are described at their builders.

Gates.  Every discrete decision per live (pixel, record) pair is a gate:
r_z != 0, alpha against 1/255, opacity vis against 0.999, nT against 1e-4,
T against 0.5 and g3 against g2 (contributing, unclamped pairs: it picks the
gradient's branch).  The generator redraws any surfel with a pair whose
float64 quantity lies within GATE_MARGIN (relative) of its threshold, at any
tile size the case is used with (T against 0.5 is charged to the record that
produced that T).  At GATE_MARGIN = 1e-5 oracle/surfel_oracle.py and this
oracle in float32 reproduce every last id, median id and contributor set of
the float64 oracle on every case (tests/test_surfel_cases_host.py asserts the
zero-mismatch condition).  They also do at 1e-6 and with no redraw at all
(the closest pair of the undrawn scenes lies 2.8e-6 from T = 0.5), so that
condition does not bound the margin from below here; 1e-5 is the smallest
power of ten that also exceeds the float32 runs' own error of T at its gate
(twice their alphas error: 8.4e-6 on every case but the needles).  The
largest share of redrawn surfels is 1.67 % (cull; sparse 0.33 %, two cameras
0.67 %, dense 0.33 %, thin 0; cap: 5 %, asserted in the host test).
gate_alpha and gate_thalf are built apart from that rule: a pixel centre
exactly on the mean with s = 0, so sigma is exactly 0 and alpha == opacity in
any precision.

tests/golden/make_golden_surfel_matrix.py measures per case, tile size and
output the float32 error of two float32 evaluations against the float64
oracle (`bar`); the tests bound errors by max(FACTOR x bar, FLOOR).
"""

import functools
import math
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from proj_cases import FACTOR, FLOOR, REDRAW_CAP, bound, rel_err  # noqa: F401

GATE_MARGIN = 1e-5
DMAX = 33
ALPHA_MIN = float(np.float32(1.0 / 255.0))
ALPHA_MAX = float(np.float32(0.999))
T_MIN = float(np.float32(1e-4))
FWD_OUT = ("colors", "alphas", "normals", "distort", "median")
BWD_OUT = ("v_means2d", "v_ray_transforms", "v_colors", "v_opacities", "v_normals", "v_densify")
GATES = ("rz", "alpha", "clamp", "tmin", "thalf", "g3g2")
KEEP_BRANCHES = ("op", "disk", "box", "sign", "quad_keep", "quad_drop")
# the hand-built cases' camera: a power-of-two focal length, principal point
FX, CX, CY = 32.0, 20.0, 18.0

# name -> (population, N, W, H, C, tile sizes)
SPECS = {
    "sparse": ("plain", 300, 70, 52, 1, (16, 4, 8, 12, 32)),
    "sparse_c2": ("plain", 300, 70, 52, 2, (16,)),
    "dense": ("plain", 1500, 40, 36, 1, (16,)),
    "thin": ("thin", 300, 70, 52, 1, (16, 8)),
    "cull": ("cull", 240, 70, 52, 1, (16, 8)),
    "edge": ("edge", 0, 40, 36, 1, (16, 8)),
    "gate_alpha": ("gate_alpha", 3, 40, 36, 1, (16, 8)),
    "gate_thalf": ("gate_thalf", 4, 40, 36, 1, (16, 8)),
}
ALL_NAMES = list(SPECS)
GATE_NAMES = [n for n in ALL_NAMES if n.startswith("gate_")]


def zero_depth_background(bg):
    """The depth background convention: the reference's backward takes the
    distortion's depth sum from render_colors[..., -1], which equals the sum
    of w d only when the depth channel's background is 0 (rasterization_2dgs
    appends exactly that).  Every case's background goes through here."""
    bg = np.array(bg, np.float32)
    bg[..., -1] = 0.0
    return bg


def padded_background_gradient(v_backgrounds):
    """A channel count that is not compiled is padded as the reference pads
    it: the colours before the depth, the backgrounds at the end.  The depth
    channel's background is thereby dropped -- not rendered (the cases' is 0
    anyway) and without a gradient."""
    v = np.array(v_backgrounds)
    v[..., -1] = 0.0
    return v


def channels(D):
    """The channels of the 33-channel evaluation that a D-channel render is."""
    return list(range(D - 1)) + [DMAX - 1]


# ==================================================================== tiles
@functools.lru_cache(maxsize=None)
def tiles(name, ts):
    """Isects of a case at a tile size: off i32 [C,th,tw], fids i32 [n]."""
    geo = _tiles_of(build(name), ts)
    for a in (geo.off, geo.fids, geo.tpg):
        a.setflags(write=False)
    return geo


def _pixels(c, geo):
    """Pixel centres of every tile, padded: px, py f64 [Tn,P], inside bool,
    and the (camera, y, x) index of every lane."""
    ts, tw, th = geo.ts, geo.tw, geo.th
    t = np.arange(c.C * th * tw)
    cam, rem = np.divmod(t, th * tw)
    ty, tx = np.divmod(rem, tw)
    ly, lx = (a.reshape(-1) for a in np.meshgrid(np.arange(ts), np.arange(ts), indexing="ij"))
    yi, xi = ty[:, None] * ts + ly[None], tx[:, None] * ts + lx[None]
    inside = (yi < c.H) & (xi < c.W)
    return cam[:, None] + 0 * yi, yi, xi, inside


# =================================================================== oracle
def _walk(c, geo, dtype, grad, trace=None):
    """The lockstep walk.  Returns leaves, per-pixel results [Tn,P,...] and
    the per-step (surfel ids, per-pixel mean copies)."""
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    G = c.C * c.N
    leaves = SimpleNamespace(
        m2=tt(c.m2).to(dtype).reshape(G, 2).requires_grad_(grad),
        rt=tt(c.rt).to(dtype).reshape(G, 9).requires_grad_(grad),
        colors=tt(c.colors).to(dtype).reshape(G, DMAX).requires_grad_(grad),
        opac=tt(c.opac).to(dtype).reshape(G).requires_grad_(grad),
        nr=tt(c.nr).to(dtype).reshape(G, 3).requires_grad_(grad))
    cam, yi, xi, inside_np = _pixels(c, geo)
    inside = tt(inside_np)
    px = (tt(xi).to(dtype) + 0.5)
    py = (tt(yi).to(dtype) + 0.5)
    pix = torch.stack([px, py], -1)
    Tn, P = px.shape
    L = int(geo.cnt.max()) if len(geo.cnt) else 0
    J = geo.starts[:, None] + np.arange(max(L, 1))[None]
    valid_np = np.arange(max(L, 1))[None] < geo.cnt[:, None]
    fpad = np.concatenate([geo.fids.astype(np.int64), np.zeros(1, np.int64)])
    Gt = tt(np.where(valid_np, fpad[np.minimum(J, len(geo.fids))], 0))
    Jt, valid = tt(J.astype(np.int64)), tt(valid_np)
    zero = torch.zeros((), dtype=dtype)
    T = torch.ones(Tn, P, dtype=dtype)
    done = torch.zeros(Tn, P, dtype=torch.bool)
    col = torch.zeros(Tn, P, DMAX, dtype=dtype)
    nrm = torch.zeros(Tn, P, 3, dtype=dtype)
    dist, avd, med = (torch.zeros(Tn, P, dtype=dtype) for _ in range(3))
    cur = torch.zeros(Tn, P, dtype=torch.int64)
    mid = torch.zeros(Tn, P, dtype=torch.int64)
    ncon = torch.zeros(Tn, P, dtype=torch.int64)  # contributor set: count and
    jsum = torch.zeros(Tn, P, dtype=torch.int64)  # sum of squared isect indices
    fst = torch.zeros(Tn, P, dtype=torch.int64)  # the first contributor's isect
    bsum = torch.zeros(Tn, P, dtype=torch.int64)  # which pairs took the g3 branch / the clamp
    steps = []
    for k in range(L):
        g, v = Gt[:, k], valid[:, k]
        m = leaves.rt[g]
        mp = leaves.m2[g][:, None, :].expand(Tn, P, 2)
        if grad:
            steps.append((g, mp))
        hu = px[..., None] * m[:, None, 6:9] - m[:, None, 0:3]
        hv = py[..., None] * m[:, None, 6:9] - m[:, None, 3:6]
        r = torch.cross(hu, hv, dim=-1)
        rz = r[..., 2]
        rz_ok = rz != 0
        s = r[..., :2] / torch.where(rz_ok, rz, torch.ones_like(rz))[..., None]
        g3 = (s * s).sum(-1)
        d = mp - pix
        g2 = 2.0 * (d * d).sum(-1)
        use3 = g3 <= g2
        # the branch not taken gets no gradient (and no 0 x inf through s)
        g3t = (torch.where(use3[..., None], s, zero) ** 2).sum(-1)
        sigma = 0.5 * torch.where(use3, g3t, g2)
        a0 = leaves.opac[g][:, None] * torch.exp(-sigma)
        clamped = a0 > ALPHA_MAX
        alpha = torch.where(clamped, torch.full_like(a0, ALPHA_MAX), a0)
        live = inside & ~done & v[:, None]
        ok = live & rz_ok & ~(alpha < ALPHA_MIN)
        nT = T * (1.0 - alpha)
        stop = ok & (nT <= T_MIN)
        act = ok & ~stop
        w = torch.where(act, alpha * T, zero)
        cg = leaves.colors[g]
        depth = cg[:, None, DMAX - 1]
        if trace is not None:
            _trace(trace, g, live, rz_ok, ok, act, stop, clamped, use3, hu, hv, rz, alpha, a0, nT,
                   T, g3, g2)
        col = col + w[..., None] * cg[:, None, :]
        nrm = nrm + w[..., None] * leaves.nr[g][:, None, :]
        dist = dist + 2.0 * (w * depth * (1.0 - T) - w * avd)
        avd = avd + w * depth
        upd = act & (T > 0.5)
        med = torch.where(upd, depth.expand(Tn, P), med)
        jk = Jt[:, k][:, None].expand(Tn, P)
        mid = torch.where(upd, jk, mid)
        cur = torch.where(act, jk, cur)
        fst = torch.where(act & (ncon == 0), jk, fst)
        ncon = ncon + act.long()
        bsum = bsum + (act & use3).long() * (jk + 1) + (act & clamped).long() * (jk + 1) * 1000003
        jsum = jsum + act.long() * jk * jk
        T = torch.where(act, nT, T)
        done = done | stop
    idx = tuple(tt(a[inside_np]) for a in (cam, yi, xi))

    def image(x):
        tail = tuple(x.shape[2:])
        return torch.zeros((c.C, c.H, c.W) + tail, dtype=x.dtype).index_put(idx, x[inside])

    out = SimpleNamespace(col=image(col), T=image(T)[..., None], normals=image(nrm),
                          distort=image(dist)[..., None], median=image(med)[..., None],
                          last_ids=image(cur), median_ids=image(mid), ncon=image(ncon),
                          jsum=image(jsum), first_ids=image(fst), bsum=image(bsum),
                          done=image(done))
    return leaves, out, steps


def _trace(tr, g, live, rz_ok, ok, act, stop, clamped, use3, hu, hv, rz, alpha, a0, nT, T, g3, g2):
    """Smallest relative distance to each gate per surfel, and the populations."""
    big = torch.full_like(T, 1e30)

    def put(name, where, dist):
        dmin = torch.where(where, dist, big).amin(1)
        tr["dist"][name].scatter_reduce_(0, g, dmin, "amin")

    mag = (hu[..., 0] * hv[..., 1]).abs() + (hu[..., 1] * hv[..., 0]).abs()
    put("rz", live & rz_ok, rz.abs() / mag.clamp_min(1e-300))
    put("alpha", live & rz_ok, (alpha / ALPHA_MIN - 1).abs())
    put("clamp", ok, (a0 / ALPHA_MAX - 1).abs())
    put("tmin", ok, (nT / T_MIN - 1).abs())
    # T against 0.5 decides at the next record: charged to the one that made it
    put("thalf", act, (nT / 0.5 - 1).abs())
    top = torch.maximum(g3, g2)
    put("g3g2", act & ~clamped & (top > 0), (g3 - g2).abs() / top.clamp_min(1e-300))
    tr["pairs"] += int(live.sum())
    tr["rz0"] += int((live & ~rz_ok).sum())
    tr["clamped"] += int((act & clamped).sum())
    tr["by_g3"] += int((act & use3).sum())
    tr["by_g2"] += int((act & ~use3).sum())
    tr["contrib"] += int(act.sum())
    tr["hits"][g[act.any(1)]] = True


@functools.lru_cache(maxsize=None)
def gates(name, ts):
    """Float64 gate distances [G] per gate and the populations of a case at a
    tile size (no gradients)."""
    c = build(name)
    return _gates(c, tiles(name, ts))


def _gates(c, geo):
    G = c.C * c.N
    tr = {"dist": {k: torch.full((G,), 1e30, dtype=torch.float64) for k in GATES}, "pairs": 0,
          "rz0": 0, "clamped": 0, "by_g3": 0, "by_g2": 0, "contrib": 0,
          "hits": torch.zeros(G, dtype=torch.bool)}
    with torch.no_grad():
        _, out, _ = _walk(c, geo, torch.float64, False, trace=tr)
    tr["terminated"] = int(out.done.sum())
    tr["pixels"] = c.C * c.H * c.W
    tr["isects"] = int(len(geo.fids))
    tr["longest"] = int(geo.cnt.max())
    tr["min"] = {k: float(v.min()) for k, v in tr["dist"].items()}
    return tr


def undecided(tr, margin=None):
    """[G] bool: the surfel has a pair within `margin` of a gate."""
    margin = GATE_MARGIN if margin is None else margin
    return torch.stack([tr["dist"][k] < margin for k in GATES]).any(0)


class Graph:
    """The 33-channel evaluation of a (case, tile size) with its autograd
    graph (float64: computed once and shared, `graph64`)."""

    def __init__(self, name, ts, dtype=torch.float64, grad=True):
        self.c, self.geo, self.dtype = build(name), tiles(name, ts), dtype
        ctx = torch.enable_grad() if grad else torch.no_grad()
        with ctx:
            self.leaves, self.out, self.steps = _walk(self.c, self.geo, dtype, grad)
        c, geo = self.c, self.geo
        yy, xx = np.meshgrid(np.arange(c.H) // ts, np.arange(c.W) // ts, indexing="ij")
        self._tile_of = (yy, xx)

    def _mask_px(self, masks):
        if masks is None:
            return None
        yy, xx = self._tile_of
        return torch.from_numpy(np.asarray(masks, bool)[:, yy, xx])  # [C,H,W]

    def _compose(self, D, bg, masks):
        o, ch = self.out, channels(D)
        alphas = 1.0 - o.T
        colors = o.col[..., ch]
        bgt = None
        if bg is not None:
            bgt = torch.from_numpy(np.ascontiguousarray(bg)).to(self.dtype).requires_grad_(
                torch.is_grad_enabled())
            colors = colors + o.T * bgt[:, None, None, :]
        res = dict(colors=colors, alphas=alphas, normals=o.normals, distort=o.distort,
                   median=o.median)
        ids = dict(last_ids=o.last_ids, median_ids=o.median_ids, ncon=o.ncon, jsum=o.jsum,
                   first_ids=o.first_ids, bsum=o.bsum)
        mp = self._mask_px(masks)
        if mp is not None:
            for k in res:
                empty = torch.zeros_like(res[k])
                if k == "colors" and bgt is not None:
                    empty = empty + bgt[:, None, None, :]
                res[k] = torch.where(mp[..., None], res[k], empty)
            ids = {k: torch.where(mp, v, torch.zeros_like(v)) for k, v in ids.items()}
        return res, ids, bgt

    def forward(self, D=DMAX, bg=None, masks=None):
        """numpy images (colors [C,H,W,D], alphas, normals, distort, median)
        and last_ids / median_ids / ncon / jsum."""
        with torch.no_grad():
            res, ids, _ = self._compose(D, bg, masks)
        out = {k: v.detach().numpy() for k, v in res.items()}
        out.update({k: v.numpy().astype(np.int64) for k, v in ids.items()})
        return out

    def backward(self, D=DMAX, bg=None, masks=None, lean=False, v_alpha=True):
        """Gradients of sum(cotangent x output) with the case's cotangents
        (lean: colours and alphas only; v_alpha False: none on the alphas).
        v_* numpy arrays shaped as the
        inputs, v_means2d_abs, v_densify and v_backgrounds (or None)."""
        c, lv, ch = self.c, self.leaves, channels(D)
        G = c.C * c.N
        with torch.enable_grad():
            res, _, bgt = self._compose(D, bg, masks)
            cot = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dtype)  # noqa: E731
            loss = (res["colors"] * cot(c.v_colors[..., ch])).sum()
            if v_alpha:
                loss = loss + (res["alphas"] * cot(c.v_alphas)).sum()
            if not lean:
                loss = loss + (res["normals"] * cot(c.v_normals)).sum() + \
                    (res["distort"] * cot(c.v_distort)).sum() + \
                    (res["median"] * cot(c.v_median)).sum()
            wrt = [lv.m2, lv.rt, lv.colors, lv.opac, lv.nr] + ([bgt] if bgt is not None else [])
            nl = len(wrt)
            gr = torch.autograd.grad(loss, wrt + [mp for _, mp in self.steps], retain_graph=True,
                                     allow_unused=True)
        gr = [torch.zeros_like(t) if g is None else g for g, t in
              zip(gr, wrt + [mp for _, mp in self.steps])]
        vab = torch.zeros(G, 2, dtype=self.dtype)
        for (g, _), gm in zip(self.steps, gr[nl:]):
            vab.index_add_(0, g, gm.abs().sum(1))
        vrt = gr[1]
        rt = lv.rt.detach()
        vden = torch.stack([vrt[:, 2] * rt[:, 8], vrt[:, 5] * rt[:, 8]], -1)
        sh = (c.C, c.N)
        return {"v_means2d": gr[0].reshape(sh + (2,)).numpy(),
                "v_ray_transforms": vrt.reshape(sh + (3, 3)).numpy(),
                "v_colors": gr[2][:, ch].reshape(sh + (D,)).numpy(),
                "v_opacities": gr[3].reshape(sh).numpy(),
                "v_normals": gr[4].reshape(sh + (3,)).numpy(),
                "v_densify": vden.reshape(sh + (2,)).numpy(),
                "v_means2d_abs": vab.reshape(sh + (2,)).numpy(),
                "v_backgrounds": None if bgt is None else gr[5].numpy()}


@functools.lru_cache(maxsize=None)
def graph64(name, ts):
    return Graph(name, ts)


def freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _mkey(masks):
    """Tile masks as a hashable cache key (None stays None)."""
    if masks is None:
        return None
    m = np.asarray(masks, bool)
    return m.shape, m.tobytes()


def _masks(key):
    return None if key is None else np.frombuffer(key[1], bool).reshape(key[0])


@functools.lru_cache(maxsize=None)
def _fwd64(name, ts, D, bg, mkey):
    c = build(name)
    return freeze(graph64(name, ts).forward(D, c.bg[:, channels(D)] if bg else None, _masks(mkey)))


@functools.lru_cache(maxsize=None)
def _bwd64(name, ts, D, bg, mkey, lean, v_alpha):
    c = build(name)
    return freeze(graph64(name, ts).backward(D, c.bg[:, channels(D)] if bg else None,
                                             _masks(mkey), lean, v_alpha))


def fwd64(name, ts, D=DMAX, bg=False, masks=None):
    """The float64 forward, computed once and shared read-only (bg: with the
    case's background)."""
    return _fwd64(name, ts, D, bg, _mkey(masks))


def bwd64(name, ts, D=DMAX, bg=False, masks=None, lean=False, v_alpha=True):
    return _bwd64(name, ts, D, bg, _mkey(masks), lean, v_alpha)


def tile_masks(name, ts):
    """The case's seeded tile masks at a tile size (about 60 % rendered)."""
    geo = tiles(name, ts)
    rng = np.random.default_rng(zlib.crc32(f"{name}:masks:{ts}".encode()))
    m = rng.random(geo.off.shape) > 0.4
    assert m.any() and not m.all()
    return m


# ------------------------------------------- the repository's numpy oracle
def numpy_fwd(name, ts, D=DMAX, bg=False, masks=None, contrib=True):
    """oracle/surfel_oracle.py's raster2dgs_fwd in its native float32."""
    from oracle import surfel_oracle as S
    c, geo, ch = build(name), tiles(name, ts), channels(D)
    con = {} if contrib else None
    oc, oa, on, od, om, ol, omi = S.raster2dgs_fwd(
        c.m2, c.rt, c.colors[..., ch], c.opac, c.nr, c.bg[:, ch] if bg else None, masks, c.W, c.H,
        ts, geo.off, geo.fids, contrib=con)
    out = dict(colors=oc, alphas=oa, normals=on, distort=od, median=om,
               last_ids=ol.astype(np.int64), median_ids=omi.astype(np.int64))
    if contrib:
        out.update(ncon=con["ncon"], jsum=con["jsum"])
    return out


def numpy_bwd(name, ts, fwd, D=DMAX, bg=False, masks=None, lean=False):
    """Its raster2dgs_bwd, from that run's own forward."""
    from oracle import surfel_oracle as S
    c, geo, ch = build(name), tiles(name, ts), channels(D)
    z = np.zeros_like
    vs = [c.v_colors[..., ch], c.v_alphas] + \
        [z(a) if lean else a for a in (c.v_normals, c.v_distort, c.v_median)]
    vm, vrt, vcl, vop, vnr, vden, vbg, vab = S.raster2dgs_bwd(
        c.m2, c.rt, c.colors[..., ch], c.opac, c.nr, c.bg[:, ch] if bg else None, masks, c.W, c.H,
        ts, geo.off, geo.fids, fwd["colors"], fwd["alphas"], fwd["last_ids"].astype(np.int32),
        fwd["median_ids"].astype(np.int32), *vs, absgrad=True)
    return {"v_means2d": vm, "v_ray_transforms": vrt, "v_colors": vcl, "v_opacities": vop,
            "v_normals": vnr, "v_densify": vden, "v_means2d_abs": vab, "v_backgrounds": vbg}


def torch32(name, ts):
    """This oracle in float32 (with its graph)."""
    return Graph(name, ts, torch.float32)


# ======================================================== surfel_keep in f64
def strips(c, ts):
    """Pixel-centre rectangles [S,4] (x0, x1, y0, y1) of the kernels' strips
    and the tile of each: 16x8 bands at tile size 16, a wave's rows otherwise."""
    tw, th = math.ceil(c.W / ts), math.ceil(c.H / ts)
    rows = [(8 * w, 8 * w + 7) for w in range(2)] if ts == 16 else \
        [((64 * w) // ts, min(ts - 1, (64 * w + 63) // ts)) for w in range((ts * ts + 63) // 64)]
    out = []
    for t in range(th * tw):
        ty, tx = divmod(t, tw)
        for r0, r1 in rows:
            out.append((t, tx * ts + 0.5, tx * ts + ts - 0.5, ty * ts + r0 + 0.5, ty * ts + r1 + 0.5))
    return np.array(out, np.float64)


def keep64(m, xy, op, rect):
    """A float64 restatement of surfel_keep without its rounding margins
    (0.05 on ln(255 op), 1 px on the box): (keep, branch) for one record and
    one strip; branch names: KEEP_BRANCHES."""
    x0, x1, y0, y1 = rect
    if not op >= ALPHA_MIN:
        return False, "op"
    lnv = math.log(255.0 * op)
    ddx, ddy = max(x0 - xy[0], xy[0] - x1, 0.0), max(y0 - xy[1], xy[1] - y1, 0.0)
    if ddx * ddx + ddy * ddy <= lnv:
        return True, "disk"
    r2 = 2.0 * lnv
    u, v, w = m[0:3], m[3:6], m[6:9]
    c22 = r2 * (w[0] ** 2 + w[1] ** 2) - w[2] ** 2
    if c22 < 0:
        c00 = r2 * (u[0] ** 2 + u[1] ** 2) - u[2] ** 2
        c11 = r2 * (v[0] ** 2 + v[1] ** 2) - v[2] ** 2
        c02 = r2 * (u[0] * w[0] + u[1] * w[1]) - u[2] * w[2]
        c12 = r2 * (v[0] * w[0] + v[1] * w[1]) - v[2] * w[2]
        cx, cy = c02 / c22, c12 / c22
        hx = math.sqrt(max(cx * cx - c00 / c22, 0.0))
        hy = math.sqrt(max(cy * cy - c11 / c22, 0.0))
        if cx + hx < x0 or cx - hx > x1 or cy + hy < y0 or cy - hy > y1:
            return False, "box"
    a0, a1, a2 = np.cross(v, w), np.cross(w, u), np.cross(u, v)
    pts = []
    for X, Y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1)):
        pts.append(X * a0 + Y * a1 + a2)
    zs = [p[2] for p in pts]
    if not (min(zs) > 0 or max(zs) < 0):
        return True, "sign"
    sx = [p[0] / p[2] for p in pts]
    sy = [p[1] / p[2] for p in pts]
    best, pos, neg = 1e300, True, True
    for i in range(4):
        j = (i + 1) & 3
        ex, ey = sx[j] - sx[i], sy[j] - sy[i]
        cr = ey * sx[i] - ex * sy[i]
        pos, neg = pos and cr >= 0, neg and cr <= 0
        Lq = ex * ex + ey * ey
        t = min(max(-(sx[i] * ex + sy[i] * ey) / Lq, 0.0), 1.0) if Lq > 0 else 0.0
        dx, dy = sx[i] + t * ex, sy[i] + t * ey
        best = min(best, dx * dx + dy * dy)
    keep = pos or neg or best <= r2
    return keep, "quad_keep" if keep else "quad_drop"


@functools.lru_cache(maxsize=None)
def keep_population(name, ts):
    """Surfels per surfel_keep branch over the (strip, record) pairs of the
    case's isects: {branch: number of surfels with a pair deciding there}."""
    c, geo = build(name), tiles(name, ts)
    st = strips(c, ts)
    m = c.rt.reshape(-1, 9).astype(np.float64)
    xy = c.m2.reshape(-1, 2).astype(np.float64)
    op = c.opac.reshape(-1).astype(np.float64)
    ntile = geo.tw * geo.th
    seen = {b: set() for b in KEEP_BRANCHES}
    for t in range(c.C * ntile):
        rects = st[st[:, 0] == t % ntile][:, 1:]
        for j in range(geo.starts[t], geo.starts[t] + geo.cnt[t]):
            g = int(geo.fids[j])
            for rect in rects:
                seen[keep64(m[g], xy[g], op[g], rect)[1]].add(g)
    return {b: len(s) for b, s in seen.items()}


# ===================================================================== cases
def _project(c, means, quats, scales, K, vm):
    from oracle import surfel_oracle as S
    with np.errstate(all="ignore"):
        radii, m2, depths, rt, nr = S.proj2dgs_fwd(means, quats, scales, vm, K, c.W, c.H)
    return radii, np.nan_to_num(m2), depths, np.nan_to_num(rt), np.nan_to_num(nr)


def _draw(c, rng, n):
    """n surfels of the case's population: means, quats, scales, opacities."""
    means = (rng.standard_normal((n, 3)) * [0.5, 0.5, 0.3] + [0, 0, 3]).astype(np.float32)
    quats = rng.standard_normal((n, 4)).astype(np.float32)
    scales = (rng.random((n, 3)) * 0.25 + 0.05).astype(np.float32)
    opac = (rng.random(n) * 0.9 + 0.05).astype(np.float32)
    kind = np.zeros(n, np.int64)
    if c.pop == "thin":  # needles, one axis 100x shorter, many seen edge-on
        scales[:, 0] = rng.uniform(0.2, 0.8, n)
        scales[:, 1] = rng.uniform(0.001, 0.008, n)
    if c.pop == "cull":
        kind = rng.integers(0, 6, n)
        # 0: planes through (nearly) the camera centre: large surfels whose
        #    normal is perpendicular to the viewing ray within 0.02 .. 0.2 rad,
        #    so part of the disk lies behind the camera (c22 >= 0)
        # 1: the same, smaller: the horizon line (c_z = 0) crosses strips
        for kd, (lo, hi) in ((0, (2.0, 4.0)), (1, (0.3, 0.8))):
            sel = np.nonzero(kind == kd)[0]
            ray = means[sel] / np.linalg.norm(means[sel], axis=-1, keepdims=True)
            a = rng.standard_normal((len(sel), 3))
            perp = a - (a * ray).sum(-1, keepdims=True) * ray
            perp /= np.linalg.norm(perp, axis=-1, keepdims=True)
            th = rng.uniform(0.02, 0.2, (len(sel), 1))
            nrm = np.cos(th) * perp + np.sin(th) * ray
            zax = np.array([0.0, 0.0, 1.0])
            q = np.concatenate([1.0 + (nrm * zax).sum(-1, keepdims=True), np.cross(zax + 0 * nrm, nrm)], -1)
            quats[sel] = q.astype(np.float32)
            scales[sel, :2] = rng.uniform(lo, hi, (len(sel), 2))
        # 2: large surfels centred outside the image
        sel = kind == 2
        side = rng.integers(0, 4, n)
        off = rng.uniform(1.3, 2.2, n) * np.where(side % 2 == 0, 1.0, -1.0)
        means[sel, 0] = np.where(side < 2, off * 3 * 35 / 60, means[:, 0])[sel]
        means[sel, 1] = np.where(side >= 2, off * 3 * 26 / 60, means[:, 1])[sel]
        means[sel, 2] = 3.0
        scales[sel, :2] = rng.uniform(0.5, 1.2, (int(sel.sum()), 2))
        # 3: opacities a little above 1/255: the disk is tiny
        sel = kind == 3
        opac[sel] = (ALPHA_MIN * rng.uniform(1.02, 1.6, n)[sel]).astype(np.float32)
        # 4: tiny surfels: a strip is reached only through the 2-D filter g2
        sel = kind == 4
        scales[sel, :2] = rng.uniform(0.001, 0.004, (int(sel.sum()), 2))
        opac[sel] = rng.uniform(0.6, 0.95, int(sel.sum()))
        # 5: plain
    return means, quats, scales, opac, kind


def _finish_3d(c, means, quats, scales, opac):
    from oracle import surfel_oracle as S
    c.means, c.quats, c.scales = means, quats, scales
    radii, c.m2, c.depths, c.rt, c.nr = _project(c, means, quats, scales, c.K, c.vm)
    if c.pop == "cull":
        # every surfel in every tile: the culling test, not the isect, decides;
        # the projection zeroes what it culls (a plane through the camera has
        # no bounded image), so the ray transforms come from the definition
        # K [R_q s_u | R_q s_v | mean] (identity view) and the 2-D mean is the
        # pinhole image of the 3-D one
        radii = np.full_like(radii, 128)
        Rq = S.quat_to_R(quats).astype(np.float64)
        K = c.K[0].astype(np.float64)
        cols = np.stack([Rq[:, :, 0] * scales[:, 0:1], Rq[:, :, 1] * scales[:, 1:2],
                         means.astype(np.float64)], -1)  # [N,3,3]
        c.rt = (K[None] @ cols).astype(np.float32)[None]
        c.m2 = (c.rt[..., :2, 2] / c.rt[..., 2:3, 2]).astype(np.float32)
        nz = Rq[:, :, 2]
        sgn = np.where(-(nz * means).sum(-1) > 0, 1.0, -1.0)
        c.nr = (nz * sgn[:, None]).astype(np.float32)[None]
        c.depths = means[None, :, 2].astype(np.float32)
    c.radii = radii
    c.opac = np.tile(opac[None], (c.C, 1)).astype(np.float32)
    c.colors = np.ascontiguousarray(c.col3[:, :c.N]).copy()
    c.colors[..., -1] = c.depths


def _build_seeded(c, rng):
    N, C = c.N, c.C
    c.vm = np.tile(np.eye(4, dtype=np.float32), (C, 1, 1))
    c.vm[:, 0, 3] = np.arange(C) * 0.1
    c.K = np.tile(np.array([[60.0, 0, c.W / 2], [0, 60.0, c.H / 2], [0, 0, 1]], np.float32), (C, 1, 1))
    c.col3 = rng.random((C, N, DMAX)).astype(np.float32)
    means, quats, scales, opac, kind = _draw(c, rng, N)
    redrawn = np.zeros(N, bool)
    for _ in range(40):
        _finish_3d(c, means, quats, scales, opac)
        bad = np.zeros(N, bool)
        for ts in c.ts_list:
            geo = _tiles_of(c, ts)
            bad |= undecided(_gates(c, geo)).numpy().reshape(C, N).any(0)
        if not bad.any():
            break
        redrawn |= bad
        nm, nq, ns, no, nk = _draw(c, rng, int(bad.sum()))
        keepk = kind[bad]
        if c.pop == "cull":  # a redrawn surfel keeps its population: redraw until it does
            for i in range(len(nk)):
                while nk[i] != keepk[i]:
                    a = _draw(c, rng, 1)
                    nm[i], nq[i], ns[i], no[i], nk[i] = (x[0] for x in a)
        means[bad], quats[bad], scales[bad], opac[bad] = nm, nq, ns, no
    else:
        raise AssertionError((c.name, int(bad.sum())))
    c.kind = kind
    c.redrawn = float(redrawn.mean())


def _tiles_of(c, ts):
    from oracle import gsplat_oracle as O
    tw, th = math.ceil(c.W / ts), math.ceil(c.H / ts)
    tpg, ids, fids = O.isect_tiles(c.m2, c.radii, c.depths, ts, tw, th)
    off = O.isect_offset_encode(ids, c.C, tw, th).astype(np.int32)
    flat = off.reshape(-1).astype(np.int64)
    return SimpleNamespace(off=off, fids=np.array(fids, np.int32), tw=tw, th=th, ts=ts,
                           starts=flat, cnt=np.append(flat[1:], len(fids)) - flat,
                           tpg=np.array(tpg, np.int32))


def _flat(x, y, z, su, sv):
    """Ray transform of a surfel facing an identity camera at (x, y, z) with
    half axes su, sv along x, y: K [t_u | t_v | mean] with cx, cy below."""
    return [FX * su, 0.0, FX * x + CX * z, 0.0, FX * sv, FX * y + CY * z, 0.0, 0.0, z]


def _hand(c, recs):
    """recs: (px, py, z, su, sv, opacity) with (px, py) the mean in pixels, or
    a dict(rt=, m2=, z=, op=) given directly."""
    rt, m2, z, op = [], [], [], []
    for r in recs:
        if isinstance(r, dict):
            rt.append(r["rt"]), m2.append(r["m2"]), z.append(r["z"]), op.append(r["op"])
            continue
        pxm, pym, zz, su, sv, o = r
        rt.append(_flat((pxm - CX) * zz / FX, (pym - CY) * zz / FX, zz, su, sv))
        m2.append([pxm, pym]), z.append(zz), op.append(o)
    n = len(recs)
    c.N = n
    c.rt = np.array(rt, np.float32).reshape(1, n, 3, 3)
    c.m2 = np.array(m2, np.float32).reshape(1, n, 2)
    c.depths = np.array(z, np.float32).reshape(1, n)
    c.opac = np.array(op, np.float32).reshape(1, n)
    c.nr = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (1, n, 1))
    c.radii = np.full((1, n), 128, np.int32)  # every record in every tile


def _build_edge(c, rng):
    """The value edges, one population per image region (40 x 36):
      clamp   opacity 1 (> 0.999) at the centre: alpha clamped over a disk;
              two small ones in front and two large ones behind everything,
              the second of which ends the pixels the first has clamped
      rz0     a record given directly whose r_z = v_1 - p_y is exactly 0 on the
              row p_y = 9.5 (rows u = (1, 3, 0.25), v = (0, 9.5, 0.5), w = (0, 1, 0):
              small dyadic numbers, exact in any operation order)
      zero    opacity exactly 0;  below: the float32 under 1/255
      tied    three overlapping surfels at the same depth
      first   an opaque surfel in front of faint ones: the median stays at the
              pixel's first contributor;  last: faint ones only: T > 0.5
              throughout, the median is the last contributor
    """
    below = float(np.nextafter(np.float32(ALPHA_MIN), np.float32(0)))
    recs = [
        (6.5, 5.5, 2.0, 0.30, 0.22, 1.0), (8.5, 6.5, 2.25, 0.25, 0.25, 0.9995),
        dict(rt=[1.0, 3.0, 0.25, 0.0, 9.5, 0.5, 0.0, 1.0, 0.0], m2=[30.5, 9.5], z=2.5, op=0.7),
        (20.5, 6.5, 2.75, 0.3, 0.3, 0.0), (22.5, 7.5, 3.0, 0.3, 0.3, below),
        (8.3, 24.2, 3.25, 0.35, 0.2, 0.31), (10.1, 25.4, 3.25, 0.2, 0.35, 0.43),
        (9.2, 23.1, 3.25, 0.3, 0.3, 0.27),
        (22.4, 24.3, 3.5, 0.35, 0.35, 0.83), (23.2, 25.1, 3.75, 0.4, 0.3, 0.21),
        (21.7, 23.6, 4.0, 0.3, 0.4, 0.33),
        (33.3, 26.2, 4.25, 0.3, 0.3, 0.11), (34.1, 27.3, 4.5, 0.35, 0.3, 0.13),
        (32.6, 25.4, 4.75, 0.3, 0.35, 0.09), (33.8, 26.9, 5.0, 0.32, 0.32, 0.12),
        (12.3, 14.2, 6.0, 4.0, 4.5, 1.0), (27.6, 21.7, 6.5, 4.5, 4.0, 0.99999),
    ]
    _hand(c, recs)
    c.kind = np.array([0, 0, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 5, 0, 0])
    c.col3 = rng.random((1, c.N, DMAX)).astype(np.float32)
    c.colors = c.col3.copy()
    c.colors[..., -1] = c.depths
    c.redrawn = 0.0


def _build_gate_alpha(c, rng):
    """Three surfels whose mean is a pixel centre (s = 0 there: sigma = 0 and
    alpha == opacity exactly), half a pixel wide so that no other pixel comes
    near the gate (sigma >= 1 one pixel away): opacity float32(1/255) (equal:
    contributes), the float32 below (dropped) and the float32 above."""
    eq = np.float32(ALPHA_MIN)
    ops = [eq, np.nextafter(eq, np.float32(0)), np.nextafter(eq, np.float32(1))]
    su = 0.25 * 2.0 / FX  # a quarter pixel at z = 2
    _hand(c, [(8.5 + 10 * i, 9.5 + 8 * i, 2.0, su, su, float(o)) for i, o in enumerate(ops)])
    c.kind = np.arange(3)
    c.col3 = (0.5 + 0.5 * rng.random((1, c.N, DMAX))).astype(np.float32)
    c.colors = c.col3.copy()
    c.colors[..., -1] = c.depths
    c.redrawn = 0.0
    c.centres = [(9 + 8 * i, 8 + 10 * i) for i in range(3)]  # (y, x)


def _build_gate_thalf(c, rng):
    """Two pixels whose first contributor has alpha == 0.5 exactly (its mean
    is the pixel centre, s = 0, opacity 0.5), so the second one meets T == 0.5:
    `T > 0.5` fails at equality and the median stays at the first."""
    su = 0.5 * 2.0 / FX  # half a pixel at z = 2
    _hand(c, [(12.5, 10.5, 2.0, su, su, 0.5), (12.5, 10.5, 3.0, 0.3, 0.3, 0.3),
              (27.5, 21.5, 2.5, su, su, 0.5), (28.1, 21.2, 3.5, 0.25, 0.35, 0.6)])
    c.kind = np.arange(4) % 2
    c.col3 = (0.5 + 0.5 * rng.random((1, c.N, DMAX))).astype(np.float32)
    c.colors = c.col3.copy()
    c.colors[..., -1] = c.depths
    c.redrawn = 0.0
    c.centres = [(10, 12), (21, 27)]  # (y, x)


def _cotangents(c, rng):
    shp = (c.C, c.H, c.W)
    c.v_colors = rng.standard_normal(shp + (DMAX,)).astype(np.float32)
    c.v_alphas = rng.standard_normal(shp + (1,)).astype(np.float32)
    c.v_normals = rng.standard_normal(shp + (3,)).astype(np.float32)
    c.v_distort = rng.standard_normal(shp + (1,)).astype(np.float32)
    c.v_median = rng.standard_normal(shp + (1,)).astype(np.float32)
    c.bg = zero_depth_background(rng.random((c.C, DMAX)))


@functools.lru_cache(maxsize=None)
def build(name):
    """The case of that name (float32 numpy arrays, read-only)."""
    pop, N, W, H, C, ts_list = SPECS[name]
    c = SimpleNamespace(name=name, pop=pop, N=N, W=W, H=H, C=C, ts_list=ts_list)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if pop == "edge":
        _build_edge(c, rng)
    elif pop == "gate_alpha":
        _build_gate_alpha(c, rng)
    elif pop == "gate_thalf":
        _build_gate_thalf(c, rng)
    else:
        _build_seeded(c, rng)
    _cotangents(c, rng)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def load_bars(path):
    """{"<case>:<tile size>:<variant>:<output>": bar} from surfel_matrix.npz."""
    z = np.load(path)
    return dict(zip((str(k) for k in z["bar_names"]), (float(v) for v in z["bar_values"])))


def clear_caches():
    """Drop every cached case, isect, graph and result."""
    for f in (build, tiles, gates, graph64, _fwd64, _bwd64, keep_population):
        f.cache_clear()
