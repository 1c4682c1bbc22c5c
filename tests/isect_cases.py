"""Cases and expected values of the tile intersection's exact-oracle matrix
(tests/test_gpu_isect_matrix.py; csrc/isect.hip, isect_st.h, lsd_sort.h).
Host only: numpy and the numpy oracle, no GPU import.

A case is (means2d, radii, depths, ts, tw, th) built from a seed, optionally
packed (camera_ids / gaussian_ids).  Every random case has depth ties (a
tenth of the Gaussians sit in clusters of four that share one depth and,
within a few pixels, one centre, so the ties meet in a tile), +0.0 and -0.0,
about 1 % negative depths, radius-0 Gaussians and means up to 40 px outside
the image.

Expected values: oracle.gsplat_oracle.isect_tiles / isect_offset_encode /
tile_rect, plus two definitions that live here:

  packed   the oracle unsorted on the input viewed as [1, nnz], the camera id
           OR-ed in above the tile bits (a negative depth's sign extension
           already fills them), stable argsort on the low 32 + tile_bits +
           cam_bits bits;
  ranks    order = stable argsort of the unsigned 32-bit depth patterns of
           the Gaussians with a tile, in flattened index order (negative
           depths last); vis_rank[order[s]] = s; rank_ids[p] =
           vis_rank[flatten_ids[p]].

Offsets: the ids of negative-depth isects are sign-extended, so they carry no
tile; the kernels count them past every real tile.  The expected offsets are
therefore the oracle's isect_offset_encode of the sorted non-negative ids
(the negative ones sort last).

The constants that decide which kernel a Gaussian, a supertile or a grid
takes are read out of the headers: a changed constant moves the statistics
that tests/test_isect_cases_host.py asserts, never silently un-tests a path.
"""

import functools
import os
import re
from types import SimpleNamespace

import numpy as np

from oracle import gsplat_oracle as O

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gsplat-triton_amd", "csrc")


def _src(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _const(src, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


@functools.lru_cache(None)
def constants():
    """The path constants of isect_st.h, isect.hip and lsd_sort.h."""
    st, isect, lsd = _src("isect_st.h"), _src("isect.hip"), _src("lsd_sort.h")
    k = {n: _const(st, n) for n in ("S", "kSeg", "kMaxKeys", "kLanePairs", "kHugePairs")}
    k.update({n: _const(isect, n) for n in ("kLaneTiles", "kGridTiles", "kSmallCap", "kLargeCap")})
    assert re.search(r"constexpr int kMaxTiles = kMaxKeys \* S \* S;", st)
    k["kMaxTiles"] = k["kMaxKeys"] * k["S"] * k["S"]
    # the supertile expansion runs for nst <= kMaxKeys supertile keys
    assert re.search(r"return on && g\.nst <= st::kMaxKeys;", isect)
    m = re.search(r"pick_ipt\(int64_t n\) \{ return n <= \(\(int64_t\)1 << (\d+)\) \? (\d+) : (\d+); \}",
                  lsd)
    nt = _const(lsd, "NT")
    k["lsd_small_n"] = 1 << int(m.group(1))      # up to here: the small LSD tiles
    k["lsd_tile_small"] = nt * int(m.group(2))
    k["lsd_tile"] = nt * int(m.group(3))         # items per LSD tile of larger inputs
    k["tile_scan_round"] = int(re.search(r"constexpr int R = (\d+), PT = R / 1024;", st).group(1))
    return SimpleNamespace(**k)


def n_keys(C, tw, th):
    """Supertile keys of a grid: C * supertiles + the negative-depth one."""
    S = constants().S
    return C * ((tw + S - 1) // S) * ((th + S - 1) // S) + 1


def ranked(C, tw, th):
    """gsplat_hip_isect_ranked recomputed: (tiles fit, keys fit)."""
    k = constants()
    return C * tw * th <= k.kMaxTiles, n_keys(C, tw, th) <= k.kMaxKeys


# ------------------------------------------------------------------- cases
TIE_POOL = (0.0, 0.5, 2.5, 7.0)

#  name: (seed, C, N, ts, tw, th, radii, negative fraction)
RANDOM = {
    "st_small": (11, 2, 1500, 16, 21, 14, (0, 1, 2, 5, 17, 90, 300), 0.01),
    "st_huge": (12, 1, 600, 16, 63, 50, (0, 2, 9, 40, 400, 2000), 0.01),
    "st_keys_2047": (13, 1, 800, 16, 124, 264, (0, 3, 20, 100), 0.01),
    "st_keys_max": (14, 1, 800, 16, 92, 356, (0, 3, 20, 100), 0.01),
    "legacy_keys_2049": (15, 1, 800, 16, 128, 256, (0, 3, 20, 100), 0.01),
    "legacy_t4": (16, 1, 1500, 4, 200, 170, (0, 1, 3, 9, 30, 200, 200), 0.01),
    "legacy_c8": (17, 8, 400, 16, 80, 60, (0, 2, 9, 40, 150, 700), 0.01),
    # one tile holds at most N isects: a third of the depths negative, and
    # the means at most 4 px outside, so that both kinds are there in numbers
    "one_tile": (18, 1, 300, 16, 1, 1, (0, 1, 5), 0.3),
    "pow2_last_tile": (19, 4, 700, 16, 8, 8, (0, 3, 9, 30, 70), 0.01),
}
PILES = (300, 5000, 20000)
PACKED_OF = {"packed_st_small": "st_small", "packed_legacy_c8": "legacy_c8"}
DEGENERATE = ("empty", "none_visible", "single")
ALL = tuple(RANDOM) + tuple(f"st_pile[{p}]" for p in PILES) + tuple(PACKED_OF) + DEGENERATE


def _case(name, means2d, radii, depths, ts, tw, th, camera_ids=None, gaussian_ids=None, C=None):
    packed = camera_ids is not None
    return SimpleNamespace(
        name=name, means2d=np.ascontiguousarray(means2d, np.float32),
        radii=np.ascontiguousarray(radii, np.int32), depths=np.ascontiguousarray(depths, np.float32),
        ts=ts, tw=tw, th=th, packed=packed, camera_ids=camera_ids, gaussian_ids=gaussian_ids,
        C=C if packed else radii.shape[0], N=0 if packed else radii.shape[1])


def _ties_and_signs(rng, m2, r, d, W, H, radii_pos, neg, n_clusters=None):
    """In place: clusters of four with one depth and one centre (a tenth of
    the Gaussians unless n_clusters says otherwise), -0.0, and the negative
    depths."""
    C, N = r.shape
    for c in range(C):
        idx = rng.permutation(N)[: 4 * (n_clusters or N // 40)].reshape(-1, 4)
        centre = np.stack([rng.uniform(2, W - 2, len(idx)), rng.uniform(2, H - 2, len(idx))], -1)
        m2[c, idx] = centre[:, None] + rng.uniform(-1.5, 1.5, idx.shape + (2,))
        r[c, idx] = rng.choice(radii_pos, idx.shape)
        dc = np.where(rng.random(len(idx)) < 0.5, rng.choice(TIE_POOL, len(idx)), d[c, idx[:, 0]])
        d[c, idx] = dc[:, None]
    flip = rng.random((C, N)) < neg
    d[flip] = -d[flip]  # (a tied +0.0 becomes -0.0)
    if N >= 8:
        d[:, N - 2:] = -0.0
        d[:, N - 4:N - 2] = 0.0


def _random_case(name):
    seed, C, N, ts, tw, th, radii, neg = RANDOM[name]
    rng = np.random.default_rng(seed)
    W, H = tw * ts, th * ts
    out = 4 if name == "one_tile" else 40
    m2 = np.stack([rng.uniform(-out, W + out, (C, N)), rng.uniform(-out, H + out, (C, N))], -1)
    r = rng.choice(radii, (C, N))
    d = rng.uniform(0.05, 50, (C, N)).astype(np.float32)
    # (one_tile: a third of the depths change sign, which parts many clusters;
    # half of its Gaussians are clustered)
    _ties_and_signs(rng, m2, r, d, W, H, [x for x in radii if x > 0], neg,
                    N // 8 if name == "one_tile" else None)
    return _case(name, m2, r, d, ts, tw, th)


def _pile_case(n_pile):
    """test_isect_tile_first_long_runs' scene: n_pile Gaussians per camera on
    one tile, a third of them at one depth."""
    rng = np.random.default_rng(100 + n_pile)
    C, ts, tw, th = 2, 16, 6, 5
    N = n_pile + 2000
    W, H = tw * ts, th * ts
    m2 = np.stack([rng.uniform(-40, W + 40, (C, N)), rng.uniform(-40, H + 40, (C, N))], -1)
    r = (rng.random((C, N)) * 6).astype(np.int32)
    d = (rng.random((C, N)) * 10).astype(np.float32)
    _ties_and_signs(rng, m2, r, d, W, H, [1, 2, 3, 4, 5], 0.0)
    m2[:, :n_pile] = 40.0
    r[:, :n_pile] = 3
    d[:, :n_pile] = (rng.random((C, n_pile)) * 10).astype(np.float32)
    d[:, : n_pile // 3] = 2.5
    # 1 % negative depths; the small scene needs 6 % for a hundred such isects
    flip = rng.random((C, N)) < (0.06 if n_pile < 1000 else 0.01)
    d[flip] = -d[flip]
    return _case(f"st_pile[{n_pile}]", m2, r, d, ts, tw, th)


def _packed_case(name):
    """The rows with radius > 0 plus every 7th radius-0 row."""
    b = build_case(PACKED_OF[name])
    flat_r = b.radii.reshape(-1)
    zero = np.flatnonzero(flat_r == 0)[::7]
    rows = np.sort(np.concatenate([np.flatnonzero(flat_r > 0), zero]))
    return _case(name, b.means2d.reshape(-1, 2)[rows], flat_r[rows], b.depths.reshape(-1)[rows],
                 b.ts, b.tw, b.th, camera_ids=(rows // b.N).astype(np.int64),
                 gaussian_ids=(rows % b.N).astype(np.int64), C=b.C)


@functools.lru_cache(None)
def build_case(name):
    if name in RANDOM:
        return _random_case(name)
    if name.startswith("st_pile["):
        return _pile_case(int(name[8:-1]))
    if name in PACKED_OF:
        return _packed_case(name)
    if name == "empty":
        return _case(name, np.zeros((1, 0, 2)), np.zeros((1, 0)), np.zeros((1, 0)), 16, 4, 3)
    if name == "none_visible":
        return _case(name, np.full((2, 5, 2), 20.0), np.zeros((2, 5)), np.ones((2, 5)), 16, 4, 3)
    if name == "single":  # one Gaussian on one tile
        return _case(name, np.full((1, 1, 2), 24.0), np.full((1, 1), 3), np.ones((1, 1)), 16, 4, 3)
    raise KeyError(name)


# ---------------------------------------------------------- expected values
def _rows(case):
    """The case as the oracle's [C', N'] input ([1, nnz] when packed)."""
    if case.packed:
        return case.means2d[None], case.radii[None], case.depths[None]
    return case.means2d, case.radii, case.depths


def expected_offsets(sorted_ids, C, tw, th):
    ids = np.asarray(sorted_ids, np.int64)
    neg = ids < 0
    assert not neg[: ids.size - int(neg.sum())].any(), "negative-depth isects sort last"
    return O.isect_offset_encode(ids[~neg], C, tw, th)


def rank_expectation(tpg, depths, flatten_ids):
    """(vis_rank [G] with -1 where a Gaussian has no tile, rank_ids [n])."""
    vis = np.flatnonzero(np.asarray(tpg).reshape(-1) > 0)
    bits = np.ascontiguousarray(depths, np.float32).reshape(-1).view(np.uint32)[vis]
    order = vis[np.argsort(bits, kind="stable")]
    vis_rank = np.full(np.asarray(tpg).size, -1, np.int32)
    vis_rank[order] = np.arange(order.size, dtype=np.int32)
    return vis_rank, vis_rank[np.asarray(flatten_ids, np.int64)]


@functools.lru_cache(None)
def expected(name):
    """Everything the kernels must return for a case, computed once."""
    case = build_case(name)
    m2, r, d = _rows(case)
    C, tw, th = case.C, case.tw, case.th
    tpg, ids_u, fids_u = O.isect_tiles(m2, r, d, case.ts, tw, th, sort=False)
    tb, cb = O.tile_bits(tw * th), O.tile_bits(C)
    if case.packed:
        ids_u = ids_u | (case.camera_ids[fids_u] << (32 + tb))
        tpg = tpg.reshape(-1)
    n = int(ids_u.size)
    nbits = 32 + tb + cb
    key = ids_u & ((1 << nbits) - 1)
    order = np.argsort(key, kind="stable")
    ids, fids = ids_u[order], fids_u[order]
    if not case.packed:  # the oracle's own sort agrees with the definition above
        _, oids, ofids = O.isect_tiles(m2, r, d, case.ts, tw, th, sort=True)
        assert np.array_equal(ids, oids) and np.array_equal(fids, ofids)
    vis_rank, rank_ids = rank_expectation(tpg, d, fids)
    return SimpleNamespace(
        tpg=tpg, ids_unsorted=ids_u, fids_unsorted=fids_u, ids=ids, fids=fids, key=key[order],
        n=n, n_vis=int((tpg > 0).sum()), offsets=expected_offsets(ids, C, tw, th),
        vis_rank=vis_rank, visible=vis_rank >= 0, rank_ids=rank_ids)


# --------------------------------------------------------------- statistics
@functools.lru_cache(None)
def stats(name):
    """Which kernels' work a case holds, from tile_rect."""
    case, e, k = build_case(name), expected(name), constants()
    m2, r, d = _rows(case)
    S = k.S
    x0, x1, y0, y1 = (a.reshape(-1) for a in O.tile_rect(m2, r, case.ts, case.tw, case.th))
    tpg = e.tpg.reshape(-1).astype(np.int64)
    on = tpg > 0
    neg = d.reshape(-1).view(np.int32) < 0
    pairs = np.where(neg, 1, ((x1 - 1) // S - x0 // S + 1) * ((y1 - 1) // S - y0 // S + 1))
    pairs = np.where(on, pairs, 0)
    cam = case.camera_ids if case.packed else np.arange(tpg.size) // max(case.N, 1)
    stw, sth = (case.tw + S - 1) // S, (case.th + S - 1) // S
    per_st = np.zeros(n_keys(case.C, case.tw, case.th), np.int64)
    per_st[-1] = int((on & neg).sum())
    for g in np.flatnonzero(on & ~neg):
        sx = np.arange(x0[g] // S, (x1[g] - 1) // S + 1)
        sy = np.arange(y0[g] // S, (y1[g] - 1) // S + 1)
        np.add.at(per_st, (cam[g] * stw * sth + sy[:, None] * stw + sx[None]).reshape(-1), 1)
    real = e.ids[e.ids >= 0] >> 32
    runs = np.bincount(real) if real.size else np.zeros(1, np.int64)
    # pairs of Gaussians with one id (camera, tile and depth bits equal)
    same = np.flatnonzero(e.ids[1:] == e.ids[:-1])
    tied = np.unique(e.fids[same].astype(np.int64) * (tpg.size + 1) + e.fids[same + 1]).size
    # Gaussians of the grid-wide class that follow one another in depth order
    # (vis_rank of the visible, argsorted: the visible Gaussians in depth order)
    big =(tpg[e.visible] > k.kGridTiles)[np.argsort(e.vis_rank[e.visible], kind="stable")]
    return SimpleNamespace(
        tpg=tpg, pairs=pairs, per_supertile=per_st, longest_run=int(runs.max()),
        last_tile_run=int(runs[-1]) if real.size else 0,
        n_negative=int((e.ids < 0).sum()), tied_pairs=int(tied),
        adjacent_grid_wide=int((big[1:] & big[:-1]).sum()),
        st_lane=int(((pairs > 0) & (pairs <= k.kLanePairs)).sum()),
        st_wave=int(((pairs > k.kLanePairs) & (pairs <= k.kHugePairs)).sum()),
        st_huge=int((pairs > k.kHugePairs).sum()),
        lane=int(((tpg > 0) & (tpg <= k.kLaneTiles)).sum()),
        wave=int(((tpg > k.kLaneTiles) & (tpg <= k.kGridTiles)).sum()),
        grid=int((tpg > k.kGridTiles).sum()))


# ------------------------------------------------------------ surfel scene
SURFEL = SimpleNamespace(N=3000, W=1000, H=800, ts=16, tw=63, th=50, n_needles=50)


@functools.lru_cache(None)
def surfel_scene():
    """About 3000 surfels at 1000 x 800: small discs, 3 % large ones, and 50
    needles (one axis a few depths long, the other 1e-3) through the view
    volume: their rectangle is the whole image, their image a thin line."""
    rng = np.random.default_rng(31)
    s = SURFEL
    means = (rng.standard_normal((s.N, 3)) * [1.2, 0.8, 0.4] + [0, 0, 3]).astype(np.float32)
    quats = rng.standard_normal((s.N, 4)).astype(np.float32)
    scales = (rng.random((s.N, 3)) * 0.05 + 0.005).astype(np.float32)
    big = rng.random(s.N) < 0.03
    scales[big, :2] *= 20.0
    scales[: s.n_needles, 0] = rng.uniform(6.0, 12.0, s.n_needles)
    scales[: s.n_needles, 1] = rng.uniform(0.0005, 0.002, s.n_needles)
    opac = rng.random(s.N).astype(np.float32)
    vm = np.eye(4, dtype=np.float32)[None]
    K = np.array([[900.0, 0, s.W / 2], [0, 900.0, s.H / 2], [0, 0, 1]], np.float32)[None]
    return SimpleNamespace(means=means, quats=quats, scales=scales, opacities=opac, viewmats=vm,
                           Ks=K)


def surfel_pairs(means2d, radii):
    """Supertile pairs per surfel of a projected scene (no negative depths:
    the projection drops them)."""
    s, S = SURFEL, constants().S
    x0, x1, y0, y1 = (a.reshape(-1) for a in O.tile_rect(means2d, radii, s.ts, s.tw, s.th))
    tiles = np.where(np.asarray(radii).reshape(-1) > 0, (x1 - x0) * (y1 - y0), 0)
    pairs = ((x1 - 1) // S - x0 // S + 1) * ((y1 - 1) // S - y0 // S + 1)
    return np.where(tiles > 0, pairs, 0), tiles
