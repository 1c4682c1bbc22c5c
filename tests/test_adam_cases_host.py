"""Host: the Adam matrix's oracle against torch.optim.Adam in float64, and its
rounding bounds against a float32 restatement of adam_update
(tests/adam_cases.py)."""

import numpy as np
import pytest
import torch

import adam_cases as AC


@pytest.mark.parametrize("eps", [1e-15, 1e-8])
def test_oracle_is_torch_adam_in_float64(eps):
    """Five chained oracle steps against torch.optim.Adam on float64 tensors
    (betas, lr and eps the float32 values), to 1e-13 relative."""
    r = np.random.default_rng(7)
    n, lr = 4099, AC.LRS[1]
    p = r.standard_normal(n).astype(np.float32)
    q = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    opt = torch.optim.Adam([q], lr=AC.f32(lr), betas=tuple(AC.f32(b) for b in AC.BETAS),
                           eps=AC.f32(eps))
    m, v = np.zeros(n), np.zeros(n)
    p = p.astype(np.float64)
    for t in range(1, 6):
        g = r.standard_normal(n).astype(np.float32)
        q.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        o = AC.oracle_step(p, m, v, g, None, 0, lr, AC.BETAS, eps, t)
        p, m, v = o.p, o.m, o.v
        st = opt.state[q]
        for got, want in ((p, q.detach().numpy()), (m, st["exp_avg"].numpy()),
                          (v, st["exp_avg_sq"].numpy())):
            assert np.abs(got - want).max() <= 1e-13 * max(np.abs(want).max(), 1.0)
    assert int(st["step"]) == 5


def test_modes_are_the_definitions():
    g, a = np.array([0.5, -2.0, 3.0]), np.array([0.25, 0.5, 1.0])
    assert np.array_equal(AC.xform(0, g, a), g)
    assert np.array_equal(AC.xform(1, g, a), g + a)
    assert np.array_equal(AC.xform(2, g, a), g * a)
    assert np.array_equal(AC.xform(3, g, a), g * (1 - a) * a)
    assert AC.xform(3, g, a)[2] == 0.0


def test_factors_match_the_package():
    """adam_factors restates the library's host arithmetic; the oracle's
    float64 factors round to the same float32 numbers."""
    from gsplat_hip.losses import adam_factors
    for t in (1, 2, 1000, 30000, 30002):
        got = adam_factors(AC.LRS, AC.BETAS, t)
        assert got == [AC.factors32(lr, AC.BETAS, t) for lr in AC.LRS]
    ss, ib = AC.factors64(1e-3, AC.BETAS, 1)
    # (the float32 betas: 0.9f is 2.4e-8 above 0.9, 3e-7 of 1 - beta1)
    assert abs(ss / (1e-3 / (1 - 0.9)) - 1) < 1e-6 and abs(ib * np.sqrt(1e-3) - 1) < 1e-4


def test_case_table_covers_the_issue():
    sizes = {g.numel for n in AC.NAMES for g in AC.case(n).groups}
    assert {1, 3, 4, 5, 7, 8, 1001 * 3, 1001 * 4, 1001 * 45} <= sizes
    assert max(len(AC.case(n).groups) for n in AC.NAMES) == AC.MAX_GROUPS
    assert {g.lr for g in AC.case("lrs").groups} == set(AC.LRS) and len(AC.LRS) == 6
    for n in ("mags_eps1e-15", "mags_eps1e-8"):
        assert tuple(g.mag for g in AC.case(n).groups) == AC.MAGS
    assert AC.case("mags_eps1e-15").eps == 1e-15 and AC.case("mags_eps1e-8").eps == 1e-8
    assert sorted(g.mode for g in AC.case("modes").groups) == [0, 1, 2, 3]
    assert any(g.grad == "none" for g in AC.case("no_grad").groups)
    (_, aux), = [x for x, g in zip(AC.grads("modes", 0, 0), AC.case("modes").groups)
                 if g.mode == 3]
    assert tuple(aux[:3]) == (0.0, 0.5, 1.0)
    g0 = AC.grads("then_zero", 0, 2)[0][0]
    g1 = AC.grads("then_zero", 1, 0)[0][0]
    assert np.abs(g0).min() > 0 and not g1.any()
    # the second trip of the grid-stride loop, and its sample
    assert AC.BIG > 16384 * 256 * 4
    idx = AC.big_sample()
    assert idx[0] == 0 and idx[-1] == AC.BIG - 1 and 1_000_000 <= idx.size < 1_010_000
    assert (idx >= 16384 * 256 * 4).sum() > 4096
    # the gradient underflows against eps = 1e-15 in float32, not in the oracle
    g = AC.grads("mags_eps1e-15", 0, 0)[0][0]
    assert (np.float32(1e-3) * g * g == 0).all() and (g.astype(np.float64) ** 2 > 0).all()


def _chain(name):
    """Yields (group, t, state before, (g, aux), float32 restatement's new state)
    over the case's runs, the restatement's state feeding the next step."""
    c = AC.case(name)
    state = [tuple(a.copy() for a in s) for s in AC.initial(name)]
    for run, t0 in enumerate(c.starts):
        for s in range(AC.RUN):
            t = t0 + s
            ga = AC.grads(name, run, s)
            for i, gr in enumerate(c.groups):
                ss, ib = AC.factors32(gr.lr, c.betas, t)
                new = AC.step32(*state[i], ga[i][0], ga[i][1], gr.mode, ss, ib, c.betas, c.eps)
                yield i, gr, t, state[i], ga[i], new
                state[i] = new


@pytest.mark.parametrize("name", AC.NAMES)
def test_float32_restatement_meets_the_bounds(name):
    """A correct float32 adam_update is inside the bounds on every case, every
    step; and the bounds are tight enough to see a 1e-5 relative error."""
    c = AC.case(name)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, gr, t, (p, m, v), (g, aux), (p1, m1, v1) in _chain(name):
        o = AC.oracle_step(p, m, v, g, aux, gr.mode, gr.lr, c.betas, c.eps, t)
        for k, got, want, bd in (("p", p1, o.p, o.bp), ("m", m1, o.m, o.bm), ("v", v1, o.v, o.bv)):
            assert np.isfinite(want).all() and np.isfinite(bd).all() and (bd > 0).all()
            j, r = AC.worst(got, want, bd)
            worst[k] = max(worst[k], r)
            assert r <= 1.0, (name, i, t, k, j, float(got[j]), float(want[j]), float(bd[j]))
        # teeth: the bounds are a few ulps -- far below 1e-5 of the quantities
        assert (o.bm <= 4.04 * AC.U * np.maximum.reduce([np.abs(o.m), np.abs(m),
                np.abs(AC.xform(gr.mode, np.zeros_like(p, np.float64) if g is None
                                else g.astype(np.float64),
                                None if aux is None else aux.astype(np.float64)))]) + AC.T).all()
        assert (o.bv <= 9.1 * AC.U * o.v + 3 * AC.T).all()
    assert all(0.0 < r <= 1.0 for r in worst.values()), worst


def test_a_wrong_update_is_outside_the_bounds():
    """ib dropped, and 1 - beta1 in place of 1 - beta2: both leave the bounds
    on the plain-gradient case at t = 1000 (what the GPU matrix must catch)."""
    name = "lrs"
    c = AC.case(name)
    (p, m, v), gr = AC.initial(name)[0], c.groups[0]
    g = AC.grads(name, 1, 0)[0][0]
    t = 1000
    o = AC.oracle_step(p, m, v, g, None, 0, gr.lr, c.betas, c.eps, t)
    ss, ib = AC.factors32(gr.lr, c.betas, t)
    p_bad, _, _ = AC.step32(p, m, v, g, None, 0, ss, 1.0, c.betas, c.eps)
    assert AC.worst(p_bad, o.p, o.bp)[1] > 10.0
    _, _, v_bad = AC.step32(p, m, v, g, None, 0, ss, ib, (c.betas[0], c.betas[0]), c.eps)
    assert AC.worst(v_bad, o.v, o.bv)[1] > 10.0
