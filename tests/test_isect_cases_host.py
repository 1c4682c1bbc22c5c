"""CPU: the cases of the tile intersection's GPU matrix (tests/isect_cases.py)
reach the kernels their rows name, by the constants read out of the headers,
and the expected values are consistent with themselves.

A case that no longer crosses a constant -- because the constant moved or
isect_cases.py was edited -- fails here, instead of leaving a path of
csrc/isect.hip / isect_st.h / lsd_sort.h without a test."""

import numpy as np
import pytest

import isect_cases as IC
from isect_cases import build_case, constants, expected, stats

K = constants()
RANDOM_AND_PILES = [n for n in IC.ALL if n not in IC.DEGENERATE]


def _ranked(case):
    tiles_fit, keys_fit = IC.ranked(case.C, case.tw, case.th)
    return tiles_fit and keys_fit


def test_constants_are_read():
    assert K.S == 4 and K.kMaxTiles == K.kMaxKeys * 16
    assert K.kLanePairs < K.kHugePairs and K.kLaneTiles < K.kGridTiles
    assert K.kSmallCap < K.kLargeCap and K.lsd_tile > K.lsd_tile_small > 0


# ------------------------------------------------ the oracle against itself
@pytest.mark.parametrize("name", IC.ALL)
def test_expected_values_are_consistent(name):
    case, e = build_case(name), expected(name)
    assert e.n == int(e.tpg.sum()) == e.ids.size == e.fids.size
    assert (np.diff(e.key) >= 0).all(), "sorted ids decrease on the masked key"
    # the same multiset as the unsorted emission
    assert np.array_equal(np.sort(e.ids), np.sort(e.ids_unsorted))
    # offsets = searchsorted of the (camera, tile) keys; negative ids past every tile
    T = case.C * case.tw * case.th
    tb = IC.O.tile_bits(case.tw * case.th)
    hi = e.ids >> 32
    tkey = np.where(e.ids < 0, T, (hi >> tb) * (case.tw * case.th) + (hi & ((1 << tb) - 1)))
    assert (np.diff(tkey) >= 0).all() and (tkey[e.ids >= 0] < T).all()
    assert np.array_equal(e.offsets.reshape(-1), np.searchsorted(tkey, np.arange(T), "left"))
    # ranks: a permutation of the visible, depth patterns non-decreasing along it
    vr = e.vis_rank[e.visible]
    assert np.array_equal(np.sort(vr), np.arange(e.n_vis))
    bits = build_case(name).depths.reshape(-1).view(np.uint32)[e.visible][np.argsort(vr)]
    assert (np.diff(bits.astype(np.int64)) >= 0).all()
    assert e.rank_ids.size == e.n and (e.rank_ids >= 0).all()


def test_degenerate_sizes():
    assert expected("empty").n == 0 and build_case("empty").radii.shape == (1, 0)
    assert expected("none_visible").n == 0 and expected("none_visible").n_vis == 0
    assert build_case("none_visible").radii.shape == (2, 5)
    assert expected("single").n == 1 and expected("single").n_vis == 1


# -------------------------------------------------- what every case carries
@pytest.mark.parametrize("name", RANDOM_AND_PILES)
def test_case_ingredients(name):
    case, e, s = build_case(name), expected(name), stats(name)
    d, r = case.depths.reshape(-1), case.radii.reshape(-1)
    bits = d.view(np.uint32)
    assert (bits == 0).any() and (bits == 0x80000000).any(), "+0.0 and -0.0"
    assert (r == 0).any() and (r > 0).any()
    W, H = case.tw * case.ts, case.th * case.ts
    m = case.means2d.reshape(-1, 2)
    assert ((m < 0).any(-1) | (m[:, 0] > W) | (m[:, 1] > H)).sum() >= 10
    assert m.min() >= -40 and m[:, 0].max() <= W + 40 and m[:, 1].max() <= H + 40
    # a tenth of the Gaussians in clusters of four with one depth: three of
    # four are duplicates (7.5 %), fewer where a sign flip parts a cluster
    assert np.unique(d).size <= d.size - d.size // 20, "about a tenth of the depths tied"
    assert s.tied_pairs >= 50, s.tied_pairs
    # negative depths: at least 100 isects; the single tile of one_tile holds
    # at most N = 300 isects in all, 20 negative ones there
    assert s.n_negative >= (20 if name == "one_tile" else 100), s.n_negative
    assert (e.ids >= 0).sum() >= 20


# --------------------------------------------------------- the rows' claims
def test_st_small():
    case, s = build_case("st_small"), stats("st_small")
    assert _ranked(case) and case.tw % K.S and case.th % K.S
    assert s.st_lane >= 20 and s.st_wave >= 20, (s.st_lane, s.st_wave)


def test_st_huge():
    case, s = build_case("st_huge"), stats("st_huge")
    assert _ranked(case) and IC.n_keys(case.C, case.tw, case.th) == 209
    assert s.st_huge >= 20 and s.st_wave >= 20 and s.st_lane >= 20, (s.st_huge, s.st_wave)


@pytest.mark.parametrize("n_pile", IC.PILES)
def test_st_pile(n_pile):
    name = f"st_pile[{n_pile}]"
    case, s = build_case(name), stats(name)
    assert _ranked(case)
    # the run lengths lie on both sides of the tile-first path's two limits
    if n_pile == IC.PILES[0]:
        assert s.longest_run <= K.kSmallCap
    elif n_pile == IC.PILES[1]:
        assert K.kSmallCap < s.longest_run <= K.kLargeCap
        assert s.per_supertile.max() > 4 * K.kSeg      # five segments in one supertile
    else:
        assert s.longest_run > K.kLargeCap
        assert s.per_supertile.max() > 19 * K.kSeg
    e = expected(name)
    run = np.flatnonzero((e.ids >= 0) & ((e.ids >> 32) == np.bincount(e.ids[e.ids >= 0] >> 32).argmax()))
    assert (np.diff(e.ids[run]) == 0).sum() >= n_pile // 4, "ties inside the run"


@pytest.mark.parametrize("name,keys", [("st_keys_2047", K.kMaxKeys - 1), ("st_keys_max", K.kMaxKeys)])
def test_st_keys(name, keys):
    case = build_case(name)
    assert IC.ranked(case.C, case.tw, case.th) == (True, True)
    assert IC.n_keys(case.C, case.tw, case.th) == keys
    T = case.C * case.tw * case.th
    assert K.tile_scan_round * 3 < T + 1 <= K.kMaxTiles, "four rounds of the tile scan"
    # isects in the scan's last round and in the last supertile row and column
    e = expected(name)
    assert (e.offsets.reshape(-1)[K.tile_scan_round * 3:] < e.offsets.max()).any()
    assert (np.diff(e.offsets.reshape(-1)[K.tile_scan_round * 3:]) > 0).any()
    assert stats(name).per_supertile[-2] + stats(name).per_supertile[-3] > 0 or \
        stats(name).per_supertile[-40:-1].sum() > 0


def test_legacy_keys_2049():
    case = build_case("legacy_keys_2049")
    # the first grid that is not ranked: the tiles still fit, the keys do not
    assert IC.ranked(case.C, case.tw, case.th) == (True, False)
    assert IC.n_keys(case.C, case.tw, case.th) == K.kMaxKeys + 1
    assert case.C * case.tw * case.th == K.kMaxTiles
    s = stats("legacy_keys_2049")
    assert s.lane >= 20 and s.wave >= 20, (s.lane, s.wave)


def test_legacy_t4():
    case, e, s = build_case("legacy_t4"), expected("legacy_t4"), stats("legacy_t4")
    assert IC.ranked(case.C, case.tw, case.th)[0] is False
    assert s.lane >= 20 and s.wave >= 20 and s.grid >= 20, (s.lane, s.wave, s.grid)
    assert e.n > 2 ** 20 and e.n > K.lsd_small_n, "the large LSD tiles"
    assert e.n > 2 * K.lsd_tile
    assert s.n_negative >= 10000


def test_legacy_c8():
    case, s = build_case("legacy_c8"), stats("legacy_c8")
    assert IC.ranked(case.C, case.tw, case.th)[0] is False
    assert IC.O.tile_bits(case.C) == 3
    assert s.grid >= 20 and s.wave >= 20 and s.lane >= 20, (s.grid, s.wave, s.lane)
    assert s.adjacent_grid_wide >= 20, "grid-wide Gaussians adjacent in depth order"
    # ... at several cameras
    e = expected("legacy_c8")
    cams = np.unique(np.flatnonzero(s.tpg > K.kGridTiles) // case.N)
    assert cams.size >= 4 and e.n < 2 ** 30


def test_one_tile_and_pow2():
    one = build_case("one_tile")
    assert IC.O.tile_bits(one.tw * one.th) == 0 and IC.O.tile_bits(one.C) == 0 and _ranked(one)
    p = build_case("pow2_last_tile")
    bits = IC.O.tile_bits(p.tw * p.th) + IC.O.tile_bits(p.C)
    last = p.C * p.tw * p.th - 1
    assert last == (1 << bits) - 1, "the last (camera, tile) key is all ones"
    e = expected("pow2_last_tile")
    real_last = ((e.ids >= 0) & ((e.ids >> 32) == last)).sum()
    assert real_last >= 3 and stats("pow2_last_tile").n_negative >= 100
    # ... and the negative ones follow that tile's
    assert (e.ids[-stats("pow2_last_tile").n_negative:] < 0).all()


@pytest.mark.parametrize("name", list(IC.PACKED_OF))
def test_packed(name):
    case, base = build_case(name), build_case(IC.PACKED_OF[name])
    e, eb = expected(name), expected(IC.PACKED_OF[name])
    assert case.packed and (case.radii == 0).sum() >= 20 and (case.radii > 0).sum() >= 100
    # the same isects as the unpacked scene, Gaussian for Gaussian
    rows = case.camera_ids * base.N + case.gaussian_ids
    assert np.array_equal(e.ids, eb.ids) and np.array_equal(rows[e.fids], eb.fids)
    assert e.n_vis == eb.n_vis


def test_surfel_scene():
    """The 2DGS scene of the culling test, by the numpy projection oracle."""
    from oracle import surfel_oracle as SO
    sc, s = IC.surfel_scene(), IC.SURFEL
    radii, m2, _, _, _ = SO.proj2dgs_fwd(sc.means, sc.quats, sc.scales, sc.viewmats, sc.Ks, s.W, s.H)
    pairs, tiles = IC.surfel_pairs(m2, radii)
    assert (s.tw, s.th) == (-(-s.W // s.ts), -(-s.H // s.ts))
    whole = tiles[: s.n_needles] == s.tw * s.th
    assert whole.sum() >= 30, whole.sum()
    assert (pairs > K.kHugePairs).sum() >= 30
    assert ((pairs > K.kLanePairs) & (pairs <= K.kHugePairs)).sum() >= 20
    assert ((pairs > 0) & (pairs <= K.kLanePairs)).sum() >= 1000
