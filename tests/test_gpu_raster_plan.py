"""GPU: the exact output of the 16x16 forward's planning kernels.

gsplat_hip_rasterize_prepare is driven with synthetic isect offsets (no scene,
no render) and the areas it writes into the forward's state are compared, entry
for entry, with numpy models written from the documented contracts:

* the per-tile dispatch order (tile_order_kernel, GSPLAT_HIP_DBG bit 4);
* the XCD-grouped order (tile_order_grouped_kernel, the default);
* the split plan (fwd_plan_kernel: whole tiles' order, the split tiles'
  chunks, their cleared counters and hand-off flags);
* the sizes of the forward state and of the backward workspace (the layout
  documented in rasterize16_plan.hip at chunk_slot_bytes, order_bytes and
  SplitLayout).

The tile counts are drawn from both sides of every bucket edge (512, 1024,
2048) and of the split threshold used here (1000).  The grids are the
smallest that reach every loop of the kernels: one tile; odd sides (edge
groups with missing tiles); more than 1024 tiles (two tiles per lane); more
than 1024 groups (two groups per lane) over two cameras.
"""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

L, SL = 256, 1024  # the library's defaults: backward chunk, split chunk (isects)
D = 3
SPLIT = 1000  # split threshold of the plan tests: a tile with more isects splits
SENTINEL = -7
SEED = 11
COUNTS = np.array([0, 1, 63, 511, 512, 1023, 1024, 2047, 2048, 5000])
GRIDS = [(1, 1, 1), (1, 5, 3), (1, 40, 30), (2, 50, 42)]  # (C, tw, th)
PX = 256  # pixels of a tile


def _align256(x):
    return (x + 255) // 256 * 256


@functools.lru_cache(maxsize=None)
def _counts(grid):
    """Isect count per tile, (C, th, tw) row-major.  The seven counts from 511
    up are drawn with probability min(0.08, 40 / n_tiles) each (an expected
    total near 0.5 M isects on the large grids), the three light ones share
    the rest."""
    C, tw, th = grid
    nt = C * tw * th
    q = min(0.08, 40.0 / nt)
    p = np.array([(1 - 7 * q) / 3] * 3 + [q] * 7)
    cnt = COUNTS[np.random.RandomState(SEED + nt).choice(len(COUNTS), size=nt, p=p)]
    cnt = cnt.astype(np.int64)
    cnt.setflags(write=False)
    return cnt


def _bucket(n):
    return np.where(n >= 2048, 0, np.where(n >= 1024, 1, np.where(n >= 512, 2, 3)))


def _lane_order(ids, bucket):
    """ids sorted by (bucket, id % 1024, id // 1024): heaviest bucket first,
    inside a bucket the order of the 1024 lanes that hold ids l, l + 1024, ..."""
    ids = np.asarray(ids, dtype=np.int64)
    return ids[np.lexsort((ids // 1024, ids % 1024, bucket))]


def _slot_bytes(d, n):
    return (n // L + 1) * PX * (1 + d) * 4 if n > 0 else 0


def _order_bytes(nt, n):
    return _align256(4 * (2 * nt + 64)) if n > 0 and 0 < nt <= 16384 else 0


def _split_layout(d, nt, n):
    """Byte offsets of the split area's parts, from its start."""
    nc, m = n // L + 1, nt + n // SL + 1
    lay = {"hdr": 0, "fitems": 256}
    lay["prod"] = lay["fitems"] + _align256(8 * m)
    lay["pflag"] = lay["prod"] + _align256(4 * nc * PX)
    lay["ctr"] = lay["pflag"] + _align256(16 * nc)
    lay["cout"] = lay["ctr"] + _align256(4 * m)
    lay["bytes"] = lay["cout"] + _align256(4 * m * PX * (2 + d))
    return lay


def _state_bytes(d, nt, n, split_on):
    b = _slot_bytes(d, n) + _order_bytes(nt, n)
    if split_on and _order_bytes(nt, n) > 0:
        b += _split_layout(d, nt, n)["bytes"]
    return b


def _prepare(grid, flags, split):
    """The state gsplat_hip_rasterize_prepare leaves (int32 words, pre-filled
    with the sentinel), the tile counts, the offsets and the isect count."""
    from gsplat_hip import _lib
    from gsplat_hip._wrapper import _ptr, _stream
    C, tw, th = grid
    cnt = _counts(grid)
    offs_np = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    n = int(cnt.sum())
    assert n < 1_000_000
    offs = torch.from_numpy(offs_np.astype(np.int32)).to(DEV)
    old = _lib.query("gsplat_hip_debug_set_fwd_split", split)
    old_flags = _lib.query("gsplat_hip_debug_set_flags", flags)
    try:
        sb = int(_lib.query("gsplat_hip_rasterize_fwd_state_bytes", C, D, 16, tw, th, n))
        assert sb == _state_bytes(D, cnt.size, n, split != 0)
        state = torch.full((max(sb // 4, 1),), SENTINEL, dtype=torch.int32, device=DEV)
        _lib.call("gsplat_hip_rasterize_prepare", C, D, 16, tw, th, _ptr(offs), n, None,
                  _ptr(state), sb, _stream())
        torch.cuda.synchronize()
    finally:
        _lib.query("gsplat_hip_debug_set_fwd_split", old)
        _lib.query("gsplat_hip_debug_set_flags", old_flags)
    return state.cpu().numpy(), cnt, offs_np, n


def test_counts_cover_every_bucket_and_split():
    """The draw the other tests rely on (numpy only)."""
    for grid in GRIDS[1:]:
        cnt = _counts(grid)
        assert cnt.sum() < 1_000_000, grid
        assert set(_bucket(cnt)) == {0, 1, 2, 3}, grid
        assert (cnt > SPLIT).sum() >= 4, grid
        # a split tile of one chunk, and of several
        assert ((cnt > SPLIT) & (cnt <= SL)).any() and (cnt > SL).any(), grid
    assert _counts(GRIDS[0]).sum() > 0


@pytest.mark.parametrize("grid", GRIDS)
def test_per_tile_order_exact(grid):
    """tile_order_kernel: the first n_tiles entries of the order area are the
    tiles sorted by (bucket, t % 1024, t // 1024); nothing else is written."""
    state, cnt, _, n = _prepare(grid, flags=16, split=0)
    nt = cnt.size
    order = state[_slot_bytes(D, n) // 4:]
    assert order.size == _order_bytes(nt, n) // 4
    want = _lane_order(np.arange(nt), _bucket(cnt))
    assert np.array_equal(order[:nt], want)
    assert np.all(order[nt:] == SENTINEL)
    assert np.all(state[:_slot_bytes(D, n) // 4] == SENTINEL)


def _grouped_model(grid, cnt):
    C, tw, th = grid
    gw, gh = (tw + 1) // 2, (th + 1) // 2
    ng = C * gw * gh
    tiles = np.full((ng, 4), -1, dtype=np.int64)  # [group][k = 2 dy + dx]
    g = np.arange(ng)
    c, r = g // (gw * gh), g % (gw * gh)
    gy, gx = r // gw, r % gw
    for k in range(4):
        ty, tx = 2 * gy + k // 2, 2 * gx + k % 2
        ok = (tx < tw) & (ty < th)
        tiles[ok, k] = ((c * th + ty) * tw + tx)[ok]
    heaviest = np.where(tiles >= 0, cnt[np.maximum(tiles, 0)], 0).max(axis=1)
    ranked = _lane_order(g, _bucket(heaviest))  # ranked[q] = the q-th group
    q_end = (ng + 7) // 8 * 8
    want = np.full(32 * ((ng + 7) // 8), SENTINEL, dtype=np.int64)
    for k in range(4):
        q = np.arange(q_end)
        want[32 * (q >> 3) + (q & 7) + 8 * k] = -1
        q = np.arange(ng)
        want[32 * (q >> 3) + (q & 7) + 8 * k] = tiles[ranked, k]
    return want


@pytest.mark.parametrize("grid", GRIDS)
def test_grouped_order_exact(grid):
    """tile_order_grouped_kernel: every one of the 32 ceil(groups / 8) slots."""
    state, cnt, _, n = _prepare(grid, flags=0, split=0)
    order = state[_slot_bytes(D, n) // 4:]
    want = _grouped_model(grid, cnt)
    assert not np.any(want == SENTINEL)  # the model defines every slot
    assert want.size <= order.size
    assert np.array_equal(order[:want.size], want)
    assert np.all(order[want.size:] == SENTINEL)


@pytest.mark.parametrize("grid", GRIDS)
def test_split_plan_exact(grid):
    """fwd_plan_kernel at a threshold of 1000 isects."""
    state, cnt, offs, n = _prepare(grid, flags=0, split=SPLIT)
    nt = cnt.size
    o0 = _slot_bytes(D, n) // 4
    s0 = o0 + _order_bytes(nt, n) // 4
    lay = _split_layout(D, nt, n)
    assert state.size == s0 + lay["bytes"] // 4
    order, area = state[o0:s0], state[s0:]
    part = lambda name: area[lay[name] // 4:]
    hdr, fitems, pflag, ctr = part("hdr"), part("fitems"), part("pflag"), part("ctr")

    tiles = np.arange(nt)
    whole, split = tiles[cnt <= SPLIT], tiles[cnt > SPLIT]
    assert hdr[0] == whole.size
    assert np.array_equal(order[:whole.size], _lane_order(whole, _bucket(cnt[whole])))

    split = _lane_order(split, np.zeros(split.size, dtype=np.int64))
    nch = (cnt[split] + SL - 1) // SL
    assert hdr[1] == nch.sum()
    want = np.array([(t, k) for t, m in zip(split, nch) for k in range(m)],
                    dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(fitems[:2 * len(want)].reshape(-1, 2), want)
    first = np.cumsum(nch) - nch  # index of each split tile's chunk 0
    assert np.all(ctr[first] == 0)
    for t, m in zip(split, nch):
        for k in range(m - 1):
            s = (offs[t] + (k + 1) * SL) // L
            assert np.all(pflag[4 * s:4 * s + 4] == 0), (t, k)


@pytest.mark.parametrize("d", [1, 3, 4, 32])
@pytest.mark.parametrize("split", [0, SPLIT])
def test_state_and_workspace_sizes(d, split):
    """The two size queries against the documented layout (no GPU work)."""
    from gsplat_hip import _lib
    cases = [(g, int(_counts(g).sum())) for g in GRIDS]
    cases += [((1, 16385, 1), 400_000), ((1, 40, 30), 0)]  # no order area; no isects
    G = 12345
    old = _lib.query("gsplat_hip_debug_set_fwd_split", split)
    try:
        for (C, tw, th), n in cases:
            nt = C * tw * th
            got = int(_lib.query("gsplat_hip_rasterize_fwd_state_bytes", C, d, 16, tw, th, n))
            assert got == _state_bytes(d, nt, n, split != 0), ((C, tw, th), n)
            if nt == 16385:
                assert got == _slot_bytes(d, n)
            for absgrad in (0, 1):
                f = d + 6 + 2 * absgrad
                packed = _align256(4 * ((f + 15) // 16 * 16) * G)
                items = (nt + n // L + 1 + 31) // 32 * 32  # whole rounds of 8 XCDs x 4 items
                got = int(_lib.query("gsplat_hip_rasterize_bwd_workspace_bytes", G, d, 16,
                                     absgrad, C, tw, th, n))
                assert got == packed + 256 + 8 * items, ((C, tw, th), n, absgrad)
    finally:
        _lib.query("gsplat_hip_debug_set_fwd_split", old)
