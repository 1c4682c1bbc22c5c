"""Host checks of the 2DGS rasterizer's test matrix (tests/surfel_cases.py): no
GPU.  The float64 torch oracle against the repository's numpy oracle (ids and
contributor sets exactly, images and gradients within the stored bars),
against stored finite differences of its own forward and against the
independent torch restatement of tests/test_surfel_oracle.py; the cases'
populations, the gate condition, the at-the-gate case and the bars."""

import os

import numpy as np
import pytest
import torch

import surfel_cases as SC
from conftest import GOLDEN
from test_surfel_oracle import torch_raster2dgs

NPZ = os.path.join(GOLDEN, "surfel_matrix.npz")
BARS = SC.load_bars(NPZ)
CASE_TS = [(n, ts) for n in SC.ALL_NAMES for ts in SC.SPECS[n][5]]
IDS = ("last_ids", "median_ids", "ncon", "jsum")


def _arrays(c):
    return {k: v for k, v in vars(c).items() if isinstance(v, np.ndarray)}


def test_cases_are_deterministic():
    names = ["sparse_c2", "cull", "edge", "gate_alpha"]
    first = {n: _arrays(SC.build(n)) for n in names}
    SC.clear_caches()
    for n in names:
        again = _arrays(SC.build(n))
        assert first[n].keys() == again.keys()
        for k in again:
            assert np.array_equal(first[n][k], again[k]), (n, k)


def test_shapes_are_the_issue_s():
    assert SC.SPECS["sparse"][1:5] == (300, 70, 52, 1) and SC.SPECS["sparse_c2"][4] == 2
    assert set(SC.SPECS["sparse"][5]) == {4, 8, 12, 16, 32}
    assert SC.SPECS["dense"][1:4] == (1500, 40, 36)
    for n in SC.ALL_NAMES:
        c = SC.build(n)
        assert c.W % 16 and c.H % 16  # partial tiles at the right and bottom edge
        assert not c.bg[:, -1].any()  # zero_depth_background


@pytest.mark.parametrize("name,ts", CASE_TS)
def test_population_is_what_its_name_says(name, ts):
    c, tr = SC.build(name), SC.gates(name, ts)
    pop = c.pop
    assert tr["contrib"] > 0 and tr["by_g3"] > 0
    if name.startswith("sparse"):
        assert 150 <= tr["longest"] <= 300 and tr["by_g2"] > 500  # several 64-record batches
        assert 0 < tr["terminated"] < 0.1 * tr["pixels"]
    if name == "dense":
        # several 64-record batches per tile and most pixels ending at T <= 1e-4
        assert tr["longest"] >= 1000 and tr["terminated"] >= 0.75 * tr["pixels"]
    if pop == "thin":
        s = c.scales.astype(np.float64)
        assert (s[:, 0] / s[:, 1]).min() >= 25 and np.median(s[:, 0] / s[:, 1]) >= 100
        assert tr["by_g2"] > tr["by_g3"] > 1000  # needles: the 2-D filter decides most pairs
    if pop == "cull":
        kp = SC.keep_population(name, ts)
        for b in ("disk", "box", "sign", "quad_keep", "quad_drop"):
            assert kp[b] >= 30, (b, kp)
        m = c.rt.reshape(-1, 9).astype(np.float64)
        r2 = 2 * np.log(255.0 * c.opac.reshape(-1).astype(np.float64))
        c22 = r2 * (m[:, 6] ** 2 + m[:, 7] ** 2) - m[:, 8] ** 2
        assert (c22[c.kind == 0] >= 0).sum() >= 15  # unbounded conics
        x, y = c.m2[0, c.kind == 2, 0], c.m2[0, c.kind == 2, 1]
        assert ((x < 0) | (x > c.W) | (y < 0) | (y > c.H)).all() and len(x) >= 20
        op3 = c.opac[0, c.kind == 3]
        assert len(op3) >= 20 and (op3 > SC.ALPHA_MIN).all() \
            and (op3 < 1.7 * SC.ALPHA_MIN).all()
        hits = tr["hits"].numpy()
        for kd in range(6):  # every population reaches pixels
            assert hits[c.kind == kd].sum() >= 5, kd
    if pop == "edge":
        assert tr["clamped"] >= 4 and tr["rz0"] == 40 and tr["terminated"] >= 4
        assert (c.opac[0] == 0).sum() == 1
        assert (c.opac[0] == np.nextafter(np.float32(SC.ALPHA_MIN), np.float32(0))).sum() == 1
        assert (np.unique(c.depths[0], return_counts=True)[1] == 3).any()  # tied depths
        f = SC.fwd64(name, ts)
        first = (f["median_ids"] == f["first_ids"]) & (f["ncon"] > 1)
        last = (f["median_ids"] == f["last_ids"]) & (f["ncon"] > 1)
        assert first.sum() >= 10 and last.sum() >= 10  # the median at the first / last contributor
    if pop == "gate_thalf":
        assert tr["min"]["thalf"] == 0.0  # T == 0.5 exactly
    if pop == "gate_alpha":
        assert tr["contrib"] == 2  # the centre pixels of the equal and the above surfel, nothing else


@pytest.mark.parametrize("name,ts", CASE_TS)
def test_gate_condition_and_float32_decisions(name, ts):
    """No pair of a seeded case within GATE_MARGIN of a gate, at most 5 %
    redrawn, and both float32 evaluations reproduce every id and every
    contributor set of the float64 oracle (zero mismatches)."""
    c = SC.build(name)
    if c.pop in ("plain", "thin", "cull"):
        assert not SC.undecided(SC.gates(name, ts)).any()
        assert c.redrawn <= SC.REDRAW_CAP
    f64 = SC.fwd64(name, ts)
    n32 = SC.numpy_fwd(name, ts)
    t32 = SC.torch32(name, ts).forward()
    for k in IDS:
        assert np.array_equal(n32[k], f64[k]), (k, int((n32[k] != f64[k]).sum()))
        assert np.array_equal(t32[k], f64[k]), (k, int((t32[k] != f64[k]).sum()))


def test_at_the_gate_case_decides_as_designed():
    """alpha == opacity exactly at the three centre pixels: float32(1/255)
    contributes, the float32 below is dropped, the one above contributes, in
    the float64 oracle and in both float32 evaluations, forward and backward."""
    name = "gate_alpha"
    c = SC.build(name)
    eq = np.float32(SC.ALPHA_MIN)
    assert c.opac[0].tolist() == [eq, np.nextafter(eq, np.float32(0)), np.nextafter(eq, np.float32(1))]
    for ts in c.ts_list:
        runs = {"f64": SC.fwd64(name, ts), "n32": SC.numpy_fwd(name, ts),
                "t32": SC.torch32(name, ts).forward()}
        for lab, f in runs.items():
            got = [int(f["ncon"][0, y, x]) for y, x in c.centres]
            assert got == [1, 0, 1] and f["ncon"].sum() == 2, (lab, got)
            for (y, x), op, n in zip(c.centres, c.opac[0], got):
                assert abs(float(f["alphas"][0, y, x, 0]) - n * float(op)) <= 1e-9, lab
        b64 = SC.bwd64(name, ts)
        n32b = SC.numpy_bwd(name, ts, runs["n32"])
        t32b = SC.torch32(name, ts).backward()
        for lab, b in (("f64", b64), ("n32", n32b), ("t32", t32b)):
            vo = b["v_opacities"][0]
            assert vo[0] != 0 and vo[1] == 0 and vo[2] != 0, (lab, vo)


def test_median_gate_case_decides_as_designed():
    """T == 0.5 exactly at the second contributor of the two centre pixels:
    the median stays at the first, in float64 and in both float32 runs."""
    name = "gate_thalf"
    c = SC.build(name)
    for ts in c.ts_list:
        for lab, f in (("f64", SC.fwd64(name, ts)), ("n32", SC.numpy_fwd(name, ts)),
                       ("t32", SC.torch32(name, ts).forward())):
            for y, x in c.centres:
                assert f["ncon"][0, y, x] == 2 and f["alphas"][0, y, x, 0] > 0.5, lab
                if "first_ids" in f:  # the numpy oracle returns none
                    assert f["median_ids"][0, y, x] == f["first_ids"][0, y, x], lab
                assert f["median_ids"][0, y, x] != f["last_ids"][0, y, x], lab
                assert f["median"][0, y, x, 0] in (2.0, 2.5), lab


@pytest.mark.parametrize("name,ts", CASE_TS)
def test_numpy_float32_is_inside_the_bounds(name, ts):
    """oracle/surfel_oracle.py, forward and hand-derived backward, within
    max(FACTOR x bar, FLOOR) of the float64 oracle."""
    f64, n32 = SC.fwd64(name, ts, bg=True), SC.numpy_fwd(name, ts, bg=True)
    for k in SC.FWD_OUT:
        assert SC.rel_err(n32[k], f64[k]) <= SC.bound(BARS[f"{name}:{ts}:fwd:{k}"]), k
    for key, lean in (("bwd", False), ("lean", True)):
        b64 = SC.bwd64(name, ts, bg=True, lean=lean)
        nb = SC.numpy_bwd(name, ts, n32, bg=True, lean=lean)
        for k in b64:
            assert SC.rel_err(nb[k], b64[k]) <= SC.bound(BARS[f"{name}:{ts}:{key}:{k}"]), (key, k)


@pytest.mark.parametrize("name,ts,D", [("sparse", 16, 4), ("sparse", 8, 1), ("thin", 16, 9),
                                       ("edge", 16, 3)])
def test_fewer_channels_and_masks_are_the_numpy_oracle_s(name, ts, D):
    """A D-channel render taken from the 33-channel evaluation, with and
    without tile masks and backgrounds, against the numpy oracle run at D."""
    for bg, masks in ((False, None), (True, SC.tile_masks(name, ts))):
        f64 = SC.fwd64(name, ts, D, bg, masks)
        n32 = SC.numpy_fwd(name, ts, D, bg, masks, contrib=False)
        assert f64["colors"].shape[-1] == D
        for k in ("last_ids", "median_ids"):
            assert np.array_equal(n32[k], f64[k]), k
        for k in SC.FWD_OUT:
            assert SC.rel_err(n32[k], f64[k]) <= SC.bound(BARS[f"{name}:{ts}:fwd:{k}"]), k
        b64 = SC.bwd64(name, ts, D, bg, masks)
        nb = SC.numpy_bwd(name, ts, n32, D, bg, masks)
        for k in b64:
            if b64[k] is not None:
                assert SC.rel_err(nb[k], b64[k]) <= SC.bound(BARS[f"{name}:{ts}:bwd:{k}"]), k
        if masks is not None:
            off = ~np.repeat(np.repeat(masks, ts, 1), ts, 2)[:, :f64["alphas"].shape[1],
                                                            :f64["alphas"].shape[2]]
            c = SC.build(name)
            assert np.array_equal(f64["colors"][off],
                                  np.broadcast_to(c.bg[0, SC.channels(D)].astype(np.float64),
                                                  f64["colors"][off].shape))
            for k in ("alphas", "normals", "distort", "median", "last_ids", "median_ids"):
                assert not f64[k][off].any(), k


@pytest.mark.parametrize("name,ts", [("edge", 16), ("gate_alpha", 8), ("sparse", 16)])
def test_oracle_equals_the_torch_restatement_in_float64(name, ts):
    """tests/test_surfel_oracle.py's torch_raster2dgs (per tile, written from
    the reference's forward kernel) fed float64 tensors."""
    c, geo, f64 = SC.build(name), SC.tiles(name, ts), SC.fwd64(name, ts, bg=True)
    t = lambda a: torch.from_numpy(np.array(a)).double()  # noqa: E731
    torch.set_default_dtype(torch.float64)  # its state and images, for this call
    try:
        tt = torch_raster2dgs(t(c.m2), t(c.rt), t(c.colors), t(c.opac), t(c.nr), t(c.bg), c.W, c.H,
                              ts, geo.off, geo.fids)
    finally:
        torch.set_default_dtype(torch.float32)
    # the restatement clamps at the double 0.999, the oracle at float32(0.999),
    # 1.3e-8 above: clamped pairs (edge) differ by that much
    tol = 1e-7 if SC.gates(name, ts)["clamped"] else 1e-12
    for k, o in (("c", "colors"), ("a", "alphas"), ("n", "normals"), ("d", "distort"), ("m", "median")):
        assert SC.rel_err(tt[k].numpy(), f64[o]) <= tol, (o, SC.rel_err(tt[k].numpy(), f64[o]))


def test_oracle_gradient_matches_the_stored_finite_differences():
    """Central differences in float64 of sum(cotangent x output) (tests/golden/
    make_golden_surfel_matrix.py): every entry of a few surfels' inputs."""
    z = np.load(NPZ)
    names = [str(n) for n in z["fd_names"]]
    assert len(names) == 2
    keys = {"m2": "v_means2d", "rt": "v_ray_transforms", "opac": "v_opacities", "nr": "v_normals",
            "colors": "v_colors"}
    for name in names:
        c = SC.build(name)
        G = c.C * c.N
        b64 = SC.bwd64(name, 16, bg=True)
        rows = z[f"fd_{name}_rows"]
        for which, key in keys.items():
            ours = b64[key].reshape(G, -1)[rows]
            if which == "colors":
                ours = ours[:, [0, 5, SC.DMAX - 1]]
            fd = z[f"fd_{name}_{which}"]
            ok = np.isfinite(fd)  # NaN: no step left every decision fixed
            assert ok.mean() >= 0.9, (name, which, ok.mean())
            err = np.abs(ours - fd)[ok].max() / np.abs(b64[key]).max()
            assert np.abs(fd[ok]).max() > 0 and err <= 1e-6, (name, which, err)


def test_absgrad_and_densify_follow_their_definitions():
    b = SC.bwd64("sparse", 16, bg=True)
    c = SC.build("sparse")
    assert (b["v_means2d_abs"] >= np.abs(b["v_means2d"]) - 1e-12).all()
    assert (b["v_means2d_abs"] > np.abs(b["v_means2d"]) * 1.001).any()  # signs do cancel
    rt, vrt = c.rt.astype(np.float64), b["v_ray_transforms"]
    assert np.array_equal(b["v_densify"][..., 0], vrt[..., 0, 2] * rt[..., 2, 2])
    assert np.array_equal(b["v_densify"][..., 1], vrt[..., 1, 2] * rt[..., 2, 2])
    f = SC.fwd64("sparse", 16, bg=True)
    want = (c.v_colors.astype(np.float64) * (1.0 - f["alphas"])).sum((1, 2))
    assert SC.rel_err(b["v_backgrounds"], want) <= 1e-12  # as in the wrapper


def test_every_bar_is_stored():
    want = set()
    for name, ts in CASE_TS:
        want |= {f"{name}:{ts}:fwd:{k}" for k in SC.FWD_OUT}
        for key in ("bwd", "lean"):
            want |= {f"{name}:{ts}:{key}:{k}" for k in SC.BWD_OUT + ("v_means2d_abs", "v_backgrounds")}
    assert want == set(BARS)
    assert os.path.getsize(NPZ) < 100_000
