"""GPU: the multi-tensor Adam (csrc/adam.hip, adam_update in csrc/common.h)
against the float64 oracle of tests/adam_cases.py, one step at a time: after
every step (p, m, v) are compared with the oracle's step from the state the
kernel had before it, inside the rounding bounds derived in that module; the
kernel's state then feeds the next step.  Through adam_groups (the host and
the device-factor form) and FusedAdam.

Measured on an MI355X (profiles/loss_matrix/parity.txt): see MEASURED below."""

import zlib

import numpy as np
import pytest
import torch

import adam_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda"

MEASURED = """Worst error / bound over a case's steps (t = 1.., 1000.., 30000..), p / m / v:
sizes8 0.980 / 0.971 / 0.344, shN 0.988 / 0.982 / 0.465, lrs 0.984 / 0.979 / 0.373,
no_grad 0.979 / 0.963 / 0.337, then_zero 0.978 / 0.975 / 0.329, mags_eps1e-15
0.985 / 0.979 / 0.422, mags_eps1e-8 0.986 / 0.971 / 0.343, modes 0.979 / 0.974 /
0.429, modes_small 0.887 / 0.764 / 0.268; the device-factor form and FusedAdam
give the same figures as adam_groups on their cases (the same bits).  17 M
elements: 0.989 / 0.987 / 0.688.  p and m sit just under 1 because the bounds'
leading term is the final rounding itself (half an ulp of the result).  The
file runs in 1.7 s."""


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def _to(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _via_groups(c, state, gd, t):
    from gsplat_hip.losses import adam_groups
    modes = [g.mode for g in c.groups]
    adam_groups([s[0] for s in state], [g for g, _ in gd], [s[1] for s in state],
                [s[2] for s in state], [g.lr for g in c.groups], c.betas, c.eps, t,
                aux=[a for _, a in gd], modes=modes)


def _via_dev(c, state, gd, t, skip=0):
    from gsplat_hip.losses import adam_factors, adam_groups
    hyper = torch.tensor([x for pair in adam_factors([g.lr for g in c.groups], c.betas, t)
                          for x in pair], dtype=torch.float32, device=DEV)
    flag = torch.tensor([skip], dtype=torch.int32, device=DEV)
    adam_groups([s[0] for s in state], [g for g, _ in gd], [s[1] for s in state],
                [s[2] for s in state], None, c.betas, c.eps, 0, aux=[a for _, a in gd],
                modes=[g.mode for g in c.groups], hyper=hyper, skip=flag)


def _compare(label, c, i, t, before, ga, after, worst):
    gr = c.groups[i]
    o = AC.oracle_step(*before, ga[0], ga[1], gr.mode, gr.lr, c.betas, c.eps, t)
    bad = []
    for k, got, want, bd in (("p", after[0], o.p, o.bp), ("m", after[1], o.m, o.bm),
                             ("v", after[2], o.v, o.bv)):
        j, r = AC.worst(got, want, bd)
        worst[k] = max(worst[k], r)
        if not r <= 1.0:
            bad.append((k, j, float(got[j]), float(want[j]), float(bd[j]), r))
    assert not bad, (label, i, t, bad)
    # the update is not vacuous: something moved, by about what the oracle says
    if ga[0] is not None and gr.numel >= 3:
        assert np.abs(o.upd).max() > 0.0


def _drive(name, launch):
    c = AC.case(name)
    state = [[_to(a) for a in s] for s in AC.initial(name)]
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for run, t0 in enumerate(c.starts):
        for s in range(AC.RUN):
            t = t0 + s
            ga = AC.grads(name, run, s)
            before = [[a.cpu().numpy() for a in st] for st in state]
            launch(c, state, [(_to(g), _to(a)) for g, a in ga], t)
            for i in range(len(c.groups)):
                _compare(name, c, i, t, before[i], ga[i],
                         [a.cpu().numpy() for a in state[i]], worst)
    print(f"{name} [{launch.__name__}]: worst error / bound p {worst['p']:.3f} "
          f"m {worst['m']:.3f} v {worst['v']:.3f} over {len(c.starts) * AC.RUN} steps")
    assert all(r > 0.0 for r in worst.values())
    return state


@pytest.mark.parametrize("name", AC.NAMES)
def test_each_step_meets_the_oracle(name):
    _drive(name, _via_groups)


@pytest.mark.parametrize("name", ["lrs", "modes", "mags_eps1e-15", "sizes8"])
def test_device_factor_form_meets_the_same_bounds(name):
    """hyper from adam_factors: an error in those factors is an error here."""
    state = _drive(name, _via_dev)
    c = AC.case(name)
    keep = [[a.clone() for a in st] for st in state]
    _via_dev(c, state, [(_to(g), _to(a)) for g, a in AC.grads(name, 0, 0)], 7, skip=1)
    for st, kp in zip(state, keep):
        assert all(torch.equal(a, b) for a, b in zip(st, kp))


@pytest.mark.parametrize("name", ["sizes8", "no_grad", "then_zero"])
def test_fused_adam_class_meets_the_oracle(name):
    """FusedAdam.step with step_count set to the run's start."""
    from gsplat_hip.losses import FusedAdam
    c = AC.case(name)
    assert all(g.mode == 0 for g in c.groups)
    init = AC.initial(name)
    params = [_to(s[0]).requires_grad_(True) for s in init]
    opt = FusedAdam(params, [g.lr for g in c.groups], betas=c.betas, eps=c.eps)
    for i, s in enumerate(init):
        opt.exp_avg[i].copy_(_to(s[1]))
        opt.exp_avg_sq[i].copy_(_to(s[2]))

    def launch(c_, state, gd, t):
        opt.step_count = t - 1
        for p, (g, _) in zip(params, gd):
            p.grad = g
        opt.step()
        assert opt.step_count == t
        for i, st in enumerate(state):  # _drive reads the state from these
            st[0], st[1], st[2] = params[i].detach(), opt.exp_avg[i], opt.exp_avg_sq[i]

    launch.__name__ = "FusedAdam"
    _drive(name, launch)


def test_a_ninth_group_is_refused():
    from gsplat_hip._lib import GsplatHipError
    from gsplat_hip.losses import adam_groups
    n = AC.MAX_GROUPS + 1
    ts = [[torch.ones(4, device=DEV) for _ in range(n)] for _ in range(4)]
    with pytest.raises(GsplatHipError, match="groups"):
        adam_groups(ts[0], ts[1], ts[2], ts[3], [1e-3] * n, AC.BETAS, 1e-15, 1)
    for t in ts[0] + ts[2] + ts[3]:
        assert torch.equal(t, torch.ones(4, device=DEV))
    adam_groups(ts[0][:8], ts[1][:8], ts[2][:8], ts[3][:8], [1e-3] * 8, AC.BETAS, 1e-15, 1)
    assert all(float(t[0]) != 1.0 for t in ts[0][:8]) and float(ts[0][8][0]) == 1.0


def test_seventeen_million_elements_take_the_second_trip():
    """One group past the grid's 16,777,216 elements per pass: the oracle on
    every 17th element and both ends, and every element's first moment
    against the float32 lerp (nothing skipped, nothing stepped twice)."""
    from gsplat_hip.losses import adam_groups
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(b"seventeen"))
    p = torch.randn(AC.BIG, device=DEV, generator=g)
    m = 0.3 * torch.randn(AC.BIG, device=DEV, generator=g)
    v = torch.rand(AC.BIG, device=DEV, generator=g)
    gr = torch.randn(AC.BIG, device=DEV, generator=g)
    idx = torch.from_numpy(AC.big_sample()).to(DEV)
    before = [a[idx].cpu().numpy() for a in (p, m, v)]
    lerp = torch.lerp(m, gr, 1.0 - AC.f32(AC.BETAS[0]))
    lr, t = AC.LRS[5], 1
    adam_groups([p], [gr], [m], [v], [lr], AC.BETAS, 1e-15, t)
    o = AC.oracle_step(*before, gr[idx].cpu().numpy(), None, 0, lr, AC.BETAS, 1e-15, t)
    for k, got, want, bd in (("p", p, o.p, o.bp), ("m", m, o.m, o.bm), ("v", v, o.v, o.bv)):
        j, r = AC.worst(got[idx].cpu().numpy(), want, bd)
        print(f"17M {k}: worst error / bound {r:.3f} at sample {j}")
        assert r <= 1.0, (k, j, r)
    # float32 lerp against the kernel's fma form: two roundings apart at most
    tol = 4 * AC.U * torch.maximum(m.abs(), torch.maximum(gr.abs(), lerp.abs())) + 1e-37
    assert bool(((m - lerp).abs() <= tol).all())
