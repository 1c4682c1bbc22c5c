"""Host checks of the projection test matrix's oracle and cases
(tests/proj_cases.py): no GPU.  The float64 torch oracle against the
repository's numpy oracle in float64 (two independently written oracles),
against the stored float64 results of the reference, and against finite
differences of its own forward; the cases' populations, gates and bars."""

import os

import numpy as np
import pytest
import torch

import proj_cases as PC
from conftest import GOLDEN

NPZ = os.path.join(GOLDEN, "proj_matrix.npz")
BARS = PC.load_bars(NPZ)


def _arrays(c):
    out = {}
    for k, v in vars(c).items():
        for i, a in enumerate(v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                out[f"{k}{i}"] = a
    return out


def test_cases_are_deterministic():
    first = {n: _arrays(PC.build(n)) for n in PC.ALL_NAMES}
    PC.build.cache_clear()
    try:
        for n in PC.ALL_NAMES:
            again = _arrays(PC.build(n))
            assert first[n].keys() == again.keys()
            for k in again:
                assert np.array_equal(first[n][k], again[k]), (n, k)
    finally:
        for f in (PC.fwd64, PC.bwd64, PC.adam64):
            f.cache_clear()


def test_shapes_cover_the_block_edges():
    assert {PC.SPECS[n][1] for n in PC.SEEDED_NAMES} == {1, 255, 257, 600}
    assert {PC.SPECS[n][2] for n in PC.ALL_NAMES} == {1, 3}
    pops = {PC.SPECS[n][0] for n in PC.ALL_NAMES}
    assert pops >= {"plain", "iso", "needle", "disc", "edgeon", "aniso", "clamp", "cull",
                    "allculled", "deadwave", "tail"}
    for n in PC.ALL_NAMES:
        c = PC.build(n)
        assert c.K["fx"] != c.K["fy"] and c.K["cx"] != c.W / 2 and c.K["cy"] != c.H / 2
        assert (c.W, c.H) == (64, 48)


@pytest.mark.parametrize("name", PC.SEEDED_NAMES)
def test_population_is_what_its_name_says(name):
    c = PC.build(name)
    p = PC.gates(c)
    valid = p.valid.numpy()
    pop, N, C, opt = PC.SPECS[name]
    z = p.depths.numpy()
    s = c.scales.astype(np.float64)
    live = valid.any(0)
    if pop in ("plain", "iso", "needle", "disc", "edgeon", "aniso"):
        assert valid.all()
    if live.any():  # homogeneous in depth and (largest) scale, within about a factor 2
        assert z[valid].max() / z[valid].min() <= 2.5, (z[valid].min(), z[valid].max())
        big = s[live].max(-1)
        # (the radius-clip cases need Gaussians of two sizes: the small ones of
        # cull_clip3 are culled, the same ones of cull_clip0, its control, are not)
        assert opt.get("by") == "clip" or big.max() / big.min() <= 2.5, (big.min(), big.max())
        assert 0.5 <= np.median(z[valid]) / opt["z"] <= 2.0  # the band it is named after
    if opt.get("skew"):
        R = c.viewmats[0, :3, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() > 0.05
    if opt.get("qnorm"):
        n = np.linalg.norm(c.quats.astype(np.float64), axis=-1)
        assert n.min() < 1e-2 and n.max() > 1e2 and n.min() >= 1e-3 * 0.99 and n.max() <= 1e3 * 1.01
    if pop == "iso":
        assert (p.disc.numpy()[valid] < 0.01).all()  # under the floor
    if pop in ("needle", "disc", "edgeon", "aniso"):
        ratio = s.max(-1) / s.min(-1)
        assert ratio.max() > 300 and ratio.max() <= 1e3 / 0.69 and ratio.min() >= 8
    if pop in ("edgeon", "aniso"):
        assert PC.fwd64(name)["comps"][valid].min() < 0.05  # det0 -> 0, comp -> 0
    if pop == "clamp":
        cl = {k: v.numpy() & valid for k, v in p.clamp.items()}
        for kind in PC.CLAMP_KINDS:  # valid clamped pairs of each kind
            want = np.ones_like(valid)
            for key in ("x+", "x-", "y+", "y-"):
                want &= cl[key] == (key in kind)
            assert (want & valid).sum() >= 3, (kind, int((want & valid).sum()))
        anyc = np.any(list(cl.values()), axis=0)
        assert (valid & ~anyc).sum() >= 3  # and unclamped ones beside them
    if pop == "cull":
        by = opt["by"]
        fails = np.stack([p.cull[k].numpy() for k in PC.CULL_TESTS])
        culled = ~valid
        if by == "clip" and c.radius_clip == 0.0:
            assert not culled.any() and (PC.fwd64(name)["radii"] <= 3).sum() > 50
        else:
            assert 50 <= culled.sum() <= N - 50
            assert (fails[:, culled].sum(0) == 1).all()  # by that test alone
            assert fails[PC.CULL_TESTS.index(by)][culled].all()
    if pop == "allculled":
        assert not valid.any()
    if pop == "deadwave":
        assert not valid[:, 64:128].any()
        assert valid[:, :64].all() and valid[:, 128:].all()
    if pop == "tail":
        assert valid[:, N - 1].all() and N in (255, 257) and (~valid).sum() > 20


def test_every_cull_test_and_side_is_covered():
    seen = {PC.SPECS[n][3]["by"] for n in PC.ALL_NAMES if PC.SPECS[n][0] == "cull"}
    assert seen == {"near", "far", "left", "right", "top", "bottom", "clip"}
    assert {PC.build(n).radius_clip for n in PC.ALL_NAMES if "clip" in n} == {0.0, 3.0}


@pytest.mark.parametrize("name", PC.ALL_NAMES)
def test_gate_condition_and_float32_decisions(name):
    """No pair of a seeded case within GATE_MARGIN of a deciding gate, at most
    5 % redrawn, and both float32 evaluations decide as float64 does."""
    c = PC.build(name)
    if name in PC.SEEDED_NAMES:
        assert not PC.undecided(PC.gates(c)).any()
        assert c.redrawn <= PC.REDRAW_CAP
    want = PC.fwd64(name)["radii"]
    assert np.array_equal(PC.numpy_fwd(c)["radii"], want)
    assert np.array_equal(PC.oracle_fwd(c, torch.float32)["radii"], want)


def test_at_the_gate_cases_decide_as_designed():
    r = PC.fwd64("gate_near")["radii"][0]
    c = PC.build("gate_near")
    assert c.means[0, 2] == np.float32(c.near) and c.means[1, 2] == np.nextafter(np.float32(c.near), np.float32(1))
    assert r[0] == 0 and r[1] > 0
    # radius clip 3: radius 3 is culled, radius 4 kept; both clear of the ceil
    c = PC.build("gate_clip")
    p = PC.gates(c)
    assert c.radius_clip == 3.0 and p.radius[0].tolist() == [3.0, 4.0]
    assert PC.fwd64("gate_clip")["radii"][0].tolist() == [0, 4]
    assert (p.dist["ceil"] > 0.3).all()
    # frustum: rows 0..3 culled by the left, right, top, bottom test alone,
    # 2 GATE_MARGIN beyond the edge; rows 4..7 kept, 2 GATE_MARGIN inside
    c = PC.build("gate_frustum")
    p = PC.gates(c)
    assert PC.fwd64("gate_frustum")["radii"][0].tolist()[:4] == [0] * 4 and p.valid[0, 4:].all()
    d = 2 * PC.GATE_MARGIN
    for i, k in enumerate(("left", "right", "top", "bottom")):
        for row in (i, i + 4):
            assert abs(float(p.dist[k][0, row]) - d) < 0.5 * PC.GATE_MARGIN, (k, row)
        assert [kk for kk in PC.CULL_TESTS if p.cull[kk][0, i]] == [k]
    assert (p.dist["ceil"] > 0.05).all() and not PC.undecided(p).any()
    assert not torch.stack(list(p.clamp.values())).any()


@pytest.mark.parametrize("name", PC.ALL_NAMES)
def test_torch_and_numpy_oracles_agree_in_float64(name):
    """Every output and gradient of every variant, clamped and compensation
    cases included, to 1e-9 of the largest value."""
    c = PC.build(name)
    f64, n64 = PC.fwd64(name), PC.numpy_fwd(c, np.float64)
    assert np.array_equal(n64["radii"], f64["radii"])
    for k in PC.FWD_OUT:
        assert PC.rel_err(n64[k], f64[k]) <= 1e-9, (k, PC.rel_err(n64[k], f64[k]))
    for comps, depths in PC.BWD_VARIANTS:
        b64 = PC.bwd64(name, comps, depths)
        nb = PC.numpy_bwd(c, n64, np.float64, comps, depths)
        for k in PC.BWD_OUT:
            assert PC.rel_err(nb[k], b64[k]) <= 1e-9, (comps, depths, k, PC.rel_err(nb[k], b64[k]))
        # the per-pair rows sum to the dense gradients
        ci, ni = np.nonzero(f64["radii"] > 0)
        dense = np.zeros_like(b64["v_means"])
        np.add.at(dense, ni, b64["pp_v_means"])
        assert PC.rel_err(dense, b64["v_means"]) <= 1e-12


def test_oracle_equals_the_stored_reference_results():
    z = np.load(NPZ)
    names = [str(n) for n in z["ref_names"]]
    assert len(names) == 2
    for name in names:
        ours = {**PC.fwd64(name), **PC.bwd64(name)}
        assert np.array_equal(ours["radii"], z[f"ref_{name}_radii"]) and (ours["radii"] > 0).any()
        for k in ("means2d", "depths", "conics") + PC.BWD_OUT:
            assert PC.rel_err(ours[k], z[f"ref_{name}_{k}"]) <= 1e-10, (name, k)


@pytest.mark.parametrize("name", PC.ALL_NAMES)
def test_numpy_float32_is_inside_the_bounds(name):
    c = PC.build(name)
    f64, n32 = PC.fwd64(name), PC.numpy_fwd(c)
    for k in PC.FWD_OUT:
        assert PC.rel_err(n32[k], f64[k]) <= PC.bound(BARS[f"{name}:fwd:{k}"]), k
    for comps, depths in PC.BWD_VARIANTS:
        b64, nb = PC.bwd64(name, comps, depths), PC.numpy_bwd(c, n32, np.float32, comps, depths)
        for k in PC.BWD_OUT:
            assert PC.rel_err(nb[k], b64[k]) <= PC.bound(BARS[f"{name}:{PC.bwd_key(comps, depths)}:{k}"]), k


def test_every_bar_is_stored():
    want = set()
    for name in PC.ALL_NAMES:
        want |= {f"{name}:fwd:{k}" for k in PC.FWD_OUT}
        for v in PC.BWD_VARIANTS:
            want |= {f"{name}:{PC.bwd_key(*v)}:{p}{k}" for k in PC.BWD_OUT for p in ("", "pp_")}
        if name in PC.ADAM_NAMES:
            for v in PC.ADAM_VARIANTS:
                want |= {f"{name}:{PC.adam_key(*v)}:{k}" for k in PC.ADAM_OUT}
    assert want == set(BARS)
    assert os.path.getsize(NPZ) < 1_000_000


def test_adam_oracle_is_torch_optim_adam():
    """One update at step 3 from the seeded moments: torch.optim.Adam with that
    state, in float64."""
    name = "z3_n255_c1"
    c, ref = PC.build(name), PC.adam64(name)
    for i, k in enumerate(PC.GROUPS):
        p = torch.from_numpy(np.array(getattr(c, k))).double().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=PC.ADAM["lrs"][i], betas=PC.ADAM["betas"], eps=PC.ADAM["eps"])
        opt.state[p] = {"step": torch.tensor(float(PC.ADAM["step"] - 1)),
                        "exp_avg": torch.from_numpy(np.array(c.m_init[i])).double(),
                        "exp_avg_sq": torch.from_numpy(np.array(c.v_init[i])).double()}
        p.grad = torch.from_numpy(np.array(ref["g_" + k]))
        opt.step()
        assert PC.rel_err(p.detach().numpy(), ref["p_" + k]) <= 1e-14
        assert PC.rel_err(opt.state[p]["exp_avg"].numpy(), ref["m_" + k]) <= 1e-14
        assert PC.rel_err(opt.state[p]["exp_avg_sq"].numpy(), ref["v_" + k]) <= 1e-14
        assert PC.rel_err(ref["m1_" + k], 0.1 * ref["g_" + k]) <= 1e-15
    culled = ~(PC.fwd64(name)["radii"][0] > 0)
    assert not culled.any() or all(not ref["g_" + k][culled].any() for k in PC.GROUPS)


def _loss(c, means, quats, scales, vms, ci, ni):
    """sum(cotangent x output) over the pairs (ci, ni), compensations off."""
    t = lambda a: torch.from_numpy(np.array(a)).double()  # noqa: E731
    with torch.no_grad():
        p = PC.project_pairs(c, t(means)[ni], t(quats)[ni], t(scales)[ni], t(vms)[ci])
        return float((p.means2d * t(c.v_means2d)[ci, ni]).sum() + (p.depths * t(c.v_depths)[ci, ni]).sum()
                     + (p.conics * t(c.v_conics)[ci, ni]).sum())


def _finite_difference(c, ci, ni, which, rows):
    base = {"means": c.means, "quats": c.quats, "scales": c.scales, "vms": c.viewmats}
    base = {k: v.astype(np.float64) for k, v in base.items()}
    fd = np.zeros_like(base[which])
    for row in rows:
        for j in np.ndindex(base[which].shape[1:]):
            if which == "vms" and j[0] == 3:
                continue
            h = 1e-6 * max(abs(base[which][(row,) + j]), np.abs(base[which][row]).max())
            vals = []
            for sgn in (1, -1):
                x = {k: v.copy() for k, v in base.items()}
                x[which][(row,) + j] += sgn * h
                vals.append(_loss(c, x["means"], x["quats"], x["scales"], x["vms"], ci, ni))
            fd[(row,) + j] = (vals[0] - vals[1]) / (2 * h)
    return fd


def test_oracle_gradient_matches_finite_differences_away_from_the_clamp():
    """Central differences of the oracle's own float64 forward (the pairs'
    validity held fixed).  Pairs away from the clamp: 1e-6 relative.  On a
    clamped pair the means2d convention is deliberately not the derivative:
    there the two differ."""
    name = "clamp_n257_c1"
    c = PC.build(name)
    p = PC.gates(c)
    clamped = torch.stack(list(p.clamp.values())).any(0).numpy()[0]
    valid = p.valid.numpy()[0]
    b64 = PC.bwd64(name)
    free = np.nonzero(valid & ~clamped)[0][:12]
    assert len(free) == 12
    pairs = lambda rows: (torch.zeros(len(rows), dtype=torch.int64), torch.from_numpy(rows))  # noqa: E731
    ci, ni = pairs(free)
    for which, key in (("means", "v_means"), ("quats", "v_quats"), ("scales", "v_scales")):
        fd = _finite_difference(c, ci, ni, which, free)
        err = PC.rel_err(fd[free], b64[key][free])
        assert err <= 1e-6, (which, err)
    fd = _finite_difference(c, ci, ni, "vms", [0])
    want = np.zeros((4, 4))
    where = {int(n): i for i, n in enumerate(np.nonzero(valid)[0])}
    for n in free:
        want += b64["pp_v_viewmats"][where[int(n)]]
    assert PC.rel_err(fd[0], want) <= 1e-6
    # a pair clamped in x: the oracle's v_means is not the finite difference
    row = np.nonzero(valid & (p.clamp["x+"].numpy()[0] | p.clamp["x-"].numpy()[0]))[0][:1]
    ci, ni = pairs(row)
    fd = _finite_difference(c, ci, ni, "means", row)
    assert PC.rel_err(fd[row], b64["v_means"][row]) > 1e-3
