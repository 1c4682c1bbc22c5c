"""GPU: every emission path of the tile intersection (csrc/isect.hip,
isect_st.h, lsd_sort.h) against the numpy oracle, everything exact.

Cases, expected values and the definitions of the packed order and of the
depth ranks: tests/isect_cases.py; tests/test_isect_cases_host.py shows on the
CPU that every case reaches the kernels it is here for (supertile expansion
with one and many segments, exactly kMaxKeys keys and one more, the
depth-first emission's lane / wave / grid-wide classes, > 2^20 isects, eight
cameras, one tile, an all-ones last tile key, packed input).

  a  synchronous matrix: every case x ISECT_SORT; ids, flatten ids, tile
     counts, the offsets written with the isects, isect_offset_encode, and
     the unsorted emission
  b  depth ranks (rank_ids / vis_rank) where the supertile expansion runs,
     none handed out where it does not
  c  capacity mode (finish_capped, the captured step's sync-free isect):
     capacities at, just above and far above the count; overflow (count - 1
     and 0) with the sticky status; ids=False and ids=False, ranks=False
  d  tile culling of large surfels: structure only (subsequence per tile)
  e  GSPLAT_HIP_ISECT_ST=0 in a child process: the depth-first emission and
     its key_bits == 0 finalize kernel on small grids
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import isect_cases as IC
from isect_cases import build_case, expected

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("tile_first", "depth_first", "full")
CAP_CASES = ("st_small", "st_huge", "st_pile[5000]", "st_keys_max", "legacy_keys_2049",
             "legacy_c8", "one_tile", "pow2_last_tile", "packed_st_small", "packed_legacy_c8",
             "none_visible", "empty")
OVERFLOW_CASES = tuple(n for n in CAP_CASES if n not in ("none_visible", "empty"))  # n > 0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401  (fails loudly if the .so is missing)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N_(t):
    return t.cpu().numpy()


def _guard(fn, *a, **kw):
    """A HIP error (a fault on the card) ends the session: no further kernel
    is launched on a card that has faulted."""
    try:
        out = fn(*a, **kw)
        torch.cuda.synchronize()
        return out
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"GPU fault, stopping: {e}", returncode=3)
        raise


def _begin(case, sync=True):
    from gsplat_hip import _wrapper
    kw = {}
    if case.packed:
        kw = dict(packed=True, n_cameras=case.C, camera_ids=T(case.camera_ids),
                  gaussian_ids=T(case.gaussian_ids))
    return _wrapper.isect_tiles_begin(T(case.means2d), T(case.radii), T(case.depths), case.ts,
                                      case.tw, case.th, sync=sync, **kw)


def _eq(got, want, what):
    got = N_(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
        raise AssertionError(f"{what}: first difference at {i} of {want.size}: "
                             f"{got.reshape(-1)[i]} != {want.reshape(-1)[i]}")


def _check_ranks(p, e, n):
    rank_ids, vis_rank = p.ranks
    _eq(rank_ids[:n], e.rank_ids, "rank_ids")
    _eq(N_(vis_rank)[e.visible], e.vis_rank[e.visible], "vis_rank")


# ------------------------------------------------------ a: synchronous matrix
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", IC.ALL)
def test_sync_matrix(name, mode, monkeypatch):
    import gsplat_hip
    from gsplat_hip import _wrapper
    monkeypatch.setattr(_wrapper, "ISECT_SORT", mode)
    case, e = build_case(name), expected(name)
    p = _begin(case)
    tpg, ids, fids = _guard(p.finish, sort=True)
    _eq(tpg, e.tpg, "tiles_per_gauss")
    _eq(ids, e.ids, "isect_ids")
    _eq(fids, e.fids, "flatten_ids")
    if mode == "depth_first":
        assert p.offsets is not None
    if p.offsets is not None:
        _eq(p.offsets, e.offsets, "offsets written with the isects")
    _eq(_guard(gsplat_hip.isect_offset_encode, ids, case.C, case.tw, case.th), e.offsets,
        "isect_offset_encode")
    tpg_u, ids_u, fids_u = _guard(_begin(case).finish, sort=False)
    _eq(tpg_u, e.tpg, "tiles_per_gauss (unsorted)")
    _eq(ids_u, e.ids_unsorted, "isect_ids (unsorted)")
    _eq(fids_u, e.fids_unsorted, "flatten_ids (unsorted)")


# ------------------------------------------------------------------ b: ranks
@pytest.mark.parametrize("name", IC.ALL)
def test_ranks(name, monkeypatch):
    from gsplat_hip import _lib, _wrapper
    monkeypatch.setattr(_wrapper, "ISECT_SORT", "depth_first")
    case, e = build_case(name), expected(name)
    p = _begin(case)
    supertiles = bool(_lib.query("gsplat_hip_isect_ranked", case.C, case.tw, case.th))
    assert supertiles == all(IC.ranked(case.C, case.tw, case.th))
    assert p.will_rank() == (supertiles and not case.packed)
    tpg, ids, fids = _guard(p.finish, sort=True)
    _eq(ids, e.ids, "isect_ids")
    if not p.will_rank() or case.radii.size == 0:
        # no unwritten buffers are handed out
        assert p.ranks is None
        return
    _check_ranks(p, e, e.n)
    q = _begin(case)
    _, ids2, fids2 = _guard(q.finish, sort=True, ranks=False)
    assert q.ranks is None
    _eq(ids2, e.ids, "isect_ids (ranks=False)")
    _eq(fids2, e.fids, "flatten_ids (ranks=False)")
    _eq(q.offsets, e.offsets, "offsets (ranks=False)")


# --------------------------------------------------------- c: capacity matrix
def _capped(case, cap, status=None, **kw):
    p = _begin(case, sync=False)
    tpg, ids, fids, counts = _guard(p.finish_capped, cap, status=status, **kw)
    return p, tpg, ids, fids, N_(counts).tolist()


@pytest.mark.parametrize("name", CAP_CASES)
def test_capacity_fits(name):
    case, e = build_case(name), expected(name)
    n = e.n
    for cap in (n, n + 1, 4 * n + 5000):
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        p, tpg, ids, fids, counts = _capped(case, cap, status)
        assert counts == [n, e.n_vis, 0, n], (cap, counts)
        assert int(status[0]) == 0
        assert ids.numel() == cap and fids.numel() == cap
        _eq(tpg, e.tpg, f"tiles_per_gauss cap={cap}")
        _eq(ids[:n], e.ids, f"isect_ids cap={cap}")
        _eq(fids[:n], e.fids, f"flatten_ids cap={cap}")
        _eq(p.offsets, e.offsets, f"offsets cap={cap}")
        if p.will_rank(capped=True) and case.radii.size:
            _check_ranks(p, e, n)
        else:
            assert p.ranks is None


@pytest.mark.parametrize("name", OVERFLOW_CASES)
def test_capacity_overflow(name):
    case, e = build_case(name), expected(name)
    n = e.n
    assert n > 0
    for cap in (n - 1, 0):
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        p, tpg, ids, fids, counts = _capped(case, cap, status)
        assert counts == [0, e.n_vis, 1, n], (cap, counts)
        assert int(status[0]) & 1
        _eq(tpg, e.tpg, f"tiles_per_gauss cap={cap}")
        assert not N_(p.offsets).any(), f"offsets after an overflow, cap={cap}"
        if p.will_rank(capped=True):
            # the ranks are written even when the call is void (rect_kernel)
            _eq(N_(p.ranks[1])[e.visible], e.vis_rank[e.visible], f"vis_rank cap={cap}")
        # sticky: a later call that fits leaves the bit set, and is itself whole
        p, _, ids, fids, counts = _capped(case, n, status)
        assert counts == [n, e.n_vis, 0, n] and int(status[0]) & 1
        _eq(ids[:n], e.ids, "isect_ids after an overflow")
        _eq(fids[:n], e.fids, "flatten_ids after an overflow")
        _eq(p.offsets, e.offsets, "offsets after an overflow")


@pytest.mark.parametrize("name", OVERFLOW_CASES)
def test_capacity_without_ids(name):
    case, e = build_case(name), expected(name)
    n, cap = e.n, e.n + 1
    will_rank = _begin(case, sync=False).will_rank(capped=True)
    assert will_rank == (all(IC.ranked(case.C, case.tw, case.th)) and not case.packed)
    # ids=False: the rank ids and the offsets only, where there are ranks
    p, _, ids, fids, counts = _capped(case, cap, ids=False)
    assert counts == [n, e.n_vis, 0, n]
    if will_rank:
        assert ids is None and fids is None
        _check_ranks(p, e, n)
    else:
        assert p.ranks is None
        _eq(ids[:n], e.ids, "isect_ids (ids=False, no ranks)")
        _eq(fids[:n], e.fids, "flatten_ids (ids=False, no ranks)")
    _eq(p.offsets, e.offsets, "offsets (ids=False)")
    # ids=False, ranks=False: the flatten ids and the offsets only, where the
    # supertile expansion runs; both id arrays where it does not
    p, _, ids, fids, counts = _capped(case, cap, ids=False, ranks=False)
    assert counts == [n, e.n_vis, 0, n] and p.ranks is None
    if will_rank:
        assert ids is None
    else:
        _eq(ids[:n], e.ids, "isect_ids (ids=False, ranks=False)")
    _eq(fids[:n], e.fids, "flatten_ids (ids=False, ranks=False)")
    _eq(p.offsets, e.offsets, "offsets (ids=False, ranks=False)")


# ------------------------------------------------- d: surfel culling, structure
def test_surfel_cull_structure():
    import gsplat_hip
    from gsplat_hip import _wrapper
    K, s, sc = IC.constants(), IC.SURFEL, IC.surfel_scene()
    radii, m2, depths, rt, _ = _guard(
        gsplat_hip.fully_fused_projection_2dgs, T(sc.means), T(sc.quats), T(sc.scales),
        T(sc.viewmats), T(sc.Ks), s.W, s.H)
    opac = T(sc.opacities)[None]
    pairs, tiles = IC.surfel_pairs(N_(m2), N_(radii))
    assert (pairs > K.kHugePairs).sum() >= 30 and (tiles == s.tw * s.th).sum() >= 30
    cap = int(tiles.sum()) + 1000
    out = []
    for cull in (None, (rt, opac)):
        p = _wrapper.isect_tiles_begin(m2, radii, depths, s.ts, s.tw, s.th, sync=False)
        _, ids, fids, counts = _guard(p.finish_capped, cap, ids=False, ranks=False,
                                      surfel_cull=cull)
        assert ids is None
        counts = N_(counts).tolist()
        off = N_(p.offsets).reshape(-1).astype(np.int64)
        assert counts[2] == 0 and counts[3] == int(tiles.sum()) and counts[0] <= counts[3]
        assert (np.diff(off) >= 0).all() and off[0] == 0 and off[-1] <= counts[0]
        f = N_(fids)[: counts[0]].astype(np.int64)
        # tile of every isect, from the offsets (the end of the last tile's run = counts[0])
        tile = np.searchsorted(off, np.arange(counts[0]), side="right") - 1
        out.append((counts, f, tile))
    (c0, f0, t0), (c1, f1, t1) = out
    assert c0[0] == c0[3], "the unculled call writes every isect of the rectangles"
    assert c1[0] < c0[0], "no isect culled"
    print(f"isects written {c1[0]} of {c0[0]}")
    # per tile an order-preserving subsequence: a (tile, surfel) occurs once,
    # so the culled isects' positions in the unculled list must increase
    G = tiles.size
    k0, k1 = t0 * G + f0, t1 * G + f1
    assert np.unique(k0).size == k0.size and np.unique(k1).size == k1.size
    order = np.argsort(k0, kind="stable")
    at = np.searchsorted(k0[order], k1)
    assert (at < k0.size).all() and np.array_equal(k0[order][np.minimum(at, k0.size - 1)], k1), \
        "a culled call's isect is not among the unculled ones"
    assert (np.diff(order[at]) > 0).all(), "order changed within a tile"
    # small surfels keep every isect
    small = (pairs > 0) & (pairs <= K.kLanePairs)
    n0, n1 = np.bincount(f0, minlength=G), np.bincount(f1, minlength=G)
    assert small.sum() >= 1000 and np.array_equal(n0[small], n1[small])
    assert np.array_equal(n0, tiles) and (n1 <= n0).all()


# ----------------------------------------------------- e: the documented switch
def test_supertiles_switched_off_in_a_child():
    """GSPLAT_HIP_ISECT_ST=0 is read once per process: a fresh child runs the
    small cases of the synchronous matrix on the depth-first emission (and the
    finalize kernel of a grid without key bits)."""
    env = dict(os.environ, GSPLAT_HIP_ISECT_ST="0")
    r = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", os.path.abspath(__file__), "-k",
         "sync_matrix and (st_small or one_tile or pow2_last_tile)"],
        env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]
