"""Host: the loss matrix's oracle against closed forms, its case table against
the kernel list of ssim.hip, and its bars (tests/loss_cases.py)."""

import math
from collections import Counter

import pytest
import torch

import loss_cases as LC
import masked_loss_oracle as O


@pytest.mark.parametrize("a,b", [(0.3, 0.8), (0.0, 0.5), (0.01, 0.012), (-0.4, 2.2), (0.7, 0.7)])
def test_constant_images_have_the_closed_form_ssim(a, b):
    """Two constant images: every variance vanishes, SSIM = (2ab + C1) / (a^2 + b^2 + C1)."""
    x = torch.full((2, 17, 23, 3), a, dtype=torch.float64)
    y = torch.full((2, 17, 23, 3), b, dtype=torch.float64)
    C1 = 0.01 ** 2
    S, L1 = O.ssim_and_l1(x, y)
    assert abs(float(S) - (2 * a * b + C1) / (a * a + b * b + C1)) <= 1e-12
    assert abs(float(L1) - abs(a - b)) <= 1e-12


def test_identical_images_have_ssim_one():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 33, 21, 3, generator=g, dtype=torch.float64) * 3 - 0.5
    S, L1 = O.ssim_and_l1(x, x.clone())
    assert abs(float(S) - 1.0) <= 1e-12 and float(L1) == 0.0


@pytest.mark.parametrize("name", ["sl1_uniform_b1_11x75_c3", "masked_uniform_b1_33x65_c3_disc_bkgd",
                                  "fused_wide_b1_33x65_c1_idx0_seq16"])
def test_oracle_gradient_matches_central_differences(name):
    """20 seeded pixels: (f(x + h) - f(x - h)) / 2h against autograd, 1e-6 relative
    to the gradient's largest entry (uniform and wide contents: no |x - y| kink
    within h of a sampled pixel is asserted below)."""
    d, c = LC.build(name), LC.TABLE[name]
    want = LC.oracle64(name)["grad"]
    x0 = d.img.double()

    def f(x):
        if c.entry == "sl1":
            S, L1 = O.ssim_and_l1(x, d.gt.double())
            return float(LC.SL1_WEIGHTS[0] * S + LC.SL1_WEIGHTS[1] * L1)
        xc = O.compose(x, d.mask, O._f64(d.alphas), O._f64(d.back))
        return float(c.scale * O.loss_of(xc, d.gt.double(), c.lam))

    g = torch.Generator().manual_seed(11)
    live = torch.ones_like(x0, dtype=torch.bool) if d.mask is None else \
        d.mask[..., None].expand_as(x0)
    idx = live.reshape(-1).nonzero()[:, 0]
    idx = idx[torch.randperm(idx.numel(), generator=g)[:20]]
    h = 1e-6
    xc0 = x0 if c.entry == "sl1" else O.compose(x0, d.mask, O._f64(d.alphas), O._f64(d.back))
    scale = float(want.abs().max())
    for i in idx.tolist():
        assert abs(float((xc0 - d.gt.double()).reshape(-1)[i])) > 10 * h
        xp, xm = x0.clone(), x0.clone()
        xp.reshape(-1)[i] += h
        xm.reshape(-1)[i] -= h
        fd = (f(xp) - f(xm)) / (2 * h)
        assert abs(fd - float(want.reshape(-1)[i])) <= 1e-6 * scale, (i, fd)


def test_dispatch_refuses_what_the_library_refuses():
    for args in (("fused", 2), ("fused", 4), ("fused", 1, 4), ("masked", 2), ("masked", 3, 4)):
        with pytest.raises(ValueError):
            LC.dispatch(*args)
    assert LC.dispatch("two", 4)[0] == "fwd_kernel" and LC.dispatch("sl1", 3)[0] == "fwd_c_kernel<3>"
    assert LC.dispatch("masked", 3, bkgd=True).count("fused_scale_kernel") == 2


def test_every_kernel_is_reached_twice():
    seen = Counter(k for c in LC.TABLE.values() for k in set(LC.kernels_of(c)))
    assert set(seen) == set(LC.KERNELS), set(LC.KERNELS) ^ set(seen)
    assert all(n >= 2 for n in seen.values()), seen


def test_table_covers_contents_edges_tails_and_ring():
    cs = list(LC.TABLE.values())
    by_kind = {k: {(c.H, c.W) for c in cs if c.kind == k} for k in LC.KINDS}
    assert all(len(v) >= 2 for v in by_kind.values()), by_kind
    assert set(LC.SHAPES) <= by_kind["uniform"] and set(LC.SHAPES) <= by_kind["flat"]
    assert {c.H for c in cs} >= set(LC.EDGES) and {c.W for c in cs} >= set(LC.EDGES)
    assert all(h != w for h, w in LC.SHAPES)
    assert {c.B for c in cs if c.B <= 3} == {1, 2, 3}
    for entry, want in (("sl1", {1, 2, 3, 4, 5}), ("two", {1, 2, 3, 4, 5}),
                        ("fused", {(1, 1), (3, 3), (3, 4)}), ("masked", {1, 3})):
        got = {((c.C, c.XS) if entry == "fused" else c.C) for c in cs if c.entry == entry}
        assert got == want, (entry, got)
    for entry in ("fused", "masked"):
        assert {LC.scale_tail(c) for c in cs if c.entry == entry} == {0, 1, 2, 3}
    assert {c.index for c in cs if c.index is not None} >= {0, LC.STACK - 1}
    slots = {LC.ring_slot(c) for c in cs if c.seq is not None}
    assert {0, LC.RING_LEN - 1} <= slots
    assert {c.lam for c in cs} == {0.0, 0.2, 1.0}
    assert sum(c.scale == 2.5 for c in cs) >= 2
    # reduce_partials_kernel's second trip, through each forward
    big = {LC.kernels_of(c)[0] for c in cs if LC.partials(c.entry, c.B, c.H, c.W, c.C) > 1024}
    assert {"fwd_c_kernel<3>", "fwd_kernel"} <= big and any(k.startswith("fused_kernel") for k in big)
    small = [c for c in cs if c.B <= 3]
    assert all(LC.partials(c.entry, c.B, c.H, c.W, c.C) <= 1024 for c in small)
    assert {m for c in cs for m in [c.mask] if m} == set(LC.MASKS)


def test_contents_are_what_they_say():
    flats = [n for n in LC.NAMES if "_flat_" in n]
    zero = same = differ = 0
    for n in flats[:8]:
        d = LC.build(n)
        x, y = d.img[..., :d.case.C], d.gt
        zero += int((x == 0).sum())
        same += int((x == y).sum())
        differ += int((x != y).sum())
        assert float((x[:, :, 1:] == x[:, :, :-1]).float().mean()) > 0.8  # piecewise constant
    assert zero > 0 and same > 0 and differ > 0
    for n in LC.NAMES:
        d, c = LC.build(n), LC.TABLE[n]
        x = d.img[..., :c.C]
        if c.kind == "equal":
            assert torch.equal(x, d.gt)
        if c.kind == "dark":
            assert 0.0 <= float(x.min()) and float(x.max()) <= 0.02
        if c.kind == "wide":
            assert float(x.min()) < 0.0 and float(x.max()) > 1.0
        if c.index is not None:
            assert torch.equal(d.gts[c.index], d.gt[0]) and d.gts.shape[0] == LC.STACK


@pytest.mark.parametrize("name", LC.NAMES)
def test_bars_are_finite_and_the_composition_meets_its_bound(name):
    """bar > 0 wherever the oracle's output is not identically zero-by-equality
    (img == gt: both run the same exact arithmetic and agree to the bit)."""
    c = LC.TABLE[name]
    own, want = LC.composition32(name), LC.oracle64(name)
    for k in LC.outputs(c):
        bar, bd = LC.bars(name)[k], LC.bound(name, k)
        assert math.isfinite(bar) and bar >= 0.0 and math.isfinite(bd), (k, bar, bd)
        assert bool(torch.isfinite(want[k]).all())
        if c.kind != "equal":
            assert bar > 0.0, (k, bar)
        assert LC.max_err(own[k], want[k]) <= bd
    if c.kind == "equal" and c.entry != "sl1":
        # the loss's own floor: what is left where bar and |want| both vanish
        assert LC.bound(name, "loss") >= LC.FLOOR * c.lam * 0.99
