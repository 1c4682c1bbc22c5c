"""GPU: every kernel variant of the photometric loss (csrc/ssim.hip,
csrc/ssim_fused_body.h) against the float64 oracle, over the case table of
tests/loss_cases.py -- through ssim_and_l1 and l1_ssim_loss only.

An output's maximum absolute error is held to max(FACTOR x bar, FLOOR x
max|want|), bar the float32 CPU composition's own error on the same inputs
(loss_cases.bound; the scalar loss's floor is on the terms it sums, derived
there).  Beside the bounds, with no tolerance: the ring slots a call does not
own, img == gt, the render's channels past C, and what a mask hides.

Measured on an MI355X (profiles/loss_matrix/parity.txt): see MEASURED below."""

import pytest
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda"

MEASURED = """167 cases, 535 compared outputs, all inside their bounds.  Largest error /
bound per output: S 0.011 (sl1_dark_b1_33x65_c2; largest error 4.6e-06), L1 0.11
(6.4e-08), loss 0.063 (two_wide_b1_33x65_c5; largest error 2.7e-06, on
fused_flat_b2_74x12_c3s4, bar 5.8e-08), grad 0.35 (masked_flat_b1_64x52_c3_disc;
largest error 1.2e-06), grad_alpha 0.16 (3.4e-08).  By content, the largest
ratio: uniform 0.098, render 0.098, flat 0.35, equal 0.17, dark 0.12, wide 0.098.
Before the derived floor on S and the loss, two flat cases missed the plain
bound on the loss alone: fused_flat_b2_74x12_c3s4 2.67e-06 against 5.79e-07, and
fused_flat_b1_42x53_c3 through the two-pass kernels 5.56e-07 against 4.93e-07.
Every exact assertion held.  The file runs in 3.5 s."""


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401


def _dev(t, grad=False):
    return None if t is None else t.to(DEV).requires_grad_(grad)


def _run(name, img=None, entry=None, masks="case", weights=LC.SL1_WEIGHTS):
    """One forward + backward of the case through the public functions.
    img: another render than the case's; entry: another entry point on the
    case's inputs ("two" / "fused" / "masked"); masks: "case" or "all" (every
    pixel valid, no background).  Returns {output: GPU tensor} (+ ring)."""
    from gsplat_hip.losses import l1_ssim_loss, ssim_and_l1
    d = LC.build(name)
    c = d.case
    entry = c.entry if entry is None else entry
    x = _dev(d.img if img is None else img, True)
    if entry == "sl1":
        S, L1 = ssim_and_l1(x, _dev(d.gt))
        (weights[0] * S + weights[1] * L1).backward()
        return {"S": S.detach(), "L1": L1.detach(), "grad": x.grad}
    kw, gt, out = {}, d.gt, {}
    if c.index is not None:
        kw["gt_index"], gt = torch.tensor([c.index], device=DEV), d.gts
    if c.seq is not None:
        out["ring"] = torch.arange(LC.RING_LEN, dtype=torch.float32, device=DEV) + 100.0
        kw["_out_ring"] = (out["ring"], torch.tensor([c.seq], dtype=torch.int64, device=DEV))
    if c.XS != c.C:
        kw["_channels"] = c.C
    alphas = None
    if entry == "masked":
        if masks == "all":
            n = LC.STACK if c.index is not None else c.B
            kw.update(masks=torch.ones(n, c.H, c.W, dtype=torch.bool, device=DEV))
        else:
            alphas = _dev(d.alphas, c.bkgd)
            kw.update(masks=_dev(d.masks), alphas=alphas, backgrounds=_dev(d.back))
    loss = l1_ssim_loss(x, _dev(gt), c.lam, fused=entry != "two", **kw)
    assert loss.dim() == 0
    (c.scale * loss if c.scale != 1.0 else loss).backward()
    out.update(loss=loss.detach(), grad=x.grad)
    if entry == "masked" and masks == "case" and c.bkgd:
        out["galpha"] = alphas.grad
    return out


def _check(name, got, label=""):
    c, want = LC.TABLE[name], LC.oracle64(name)
    bad = []
    for k in LC.outputs(c):
        assert got[k].shape == want[k].shape, (k, got[k].shape)
        err, bd = LC.max_err(got[k], want[k]), LC.bound(name, k)
        print(f"{name}{label} {k}: err {err:.3e} bound {bd:.3e} bar {LC.bars(name)[k]:.3e} "
              f"max|want| {float(want[k].abs().max()):.3e}")
        if not err <= bd:
            bad.append((k, err, bd))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", LC.NAMES)
def test_case_meets_the_oracle(name):
    c = LC.TABLE[name]
    got = _run(name)
    _check(name, got)
    zero = torch.zeros_like(got["grad"])
    if c.seq is not None:  # the loss in its slot, every other slot as it was
        ring, k = got["ring"], LC.ring_slot(c)
        assert torch.equal(ring[k], got["loss"])
        rest = torch.arange(LC.RING_LEN, device=DEV) != k
        assert torch.equal(ring[rest], (torch.arange(LC.RING_LEN, device=DEV) + 100.0)[rest])
    if c.XS != c.C:  # the render's other channels: no loss term
        assert torch.equal(got["grad"][..., c.C:], zero[..., c.C:])
    if c.kind == "equal":
        if c.entry == "sl1":  # L1 is 0 and its part of the gradient is nothing
            assert float(got["L1"]) == 0.0
            assert torch.equal(_run(name, weights=(0.0, 1.0))["grad"], zero)
        elif c.lam == 0.0:  # sign(0) = 0 everywhere the render is let through
            assert torch.equal(got["grad"], zero)
            if c.entry != "masked":
                assert float(got["loss"]) == 0.0


_PLAIN_FUSED = [n for n in LC.NAMES if LC.TABLE[n].entry == "fused" and LC.TABLE[n].XS == LC.TABLE[n].C]


@pytest.mark.parametrize("name", [n for n in _PLAIN_FUSED if LC.TABLE[n].index is None])
def test_two_pass_meets_the_fused_cases_bounds(name):
    """The same inputs through the two-pass kernels: the same bounds against
    the oracle, not a comparison of the two with each other."""
    _check(name, _run(name, entry="two"), " (two-pass)")


@pytest.mark.parametrize("name", _PLAIN_FUSED)
def test_all_true_mask_is_the_plain_fused_loss_bit_for_bit(name):
    a, b = _run(name), _run(name, entry="masked", masks="all")
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["grad"], b["grad"])
    if "ring" in a:
        assert torch.equal(a["ring"], b["ring"])


@pytest.mark.parametrize("name", [n for n in LC.NAMES if LC.TABLE[n].XS != LC.TABLE[n].C])
def test_nan_in_the_depth_channel_changes_nothing(name):
    c, d = LC.TABLE[name], LC.build(name)
    dirty = d.img.clone()
    dirty[..., c.C:] = float("nan")
    a, b = _run(name), _run(name, img=dirty)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["grad"], b["grad"])
    assert bool(torch.isfinite(b["grad"]).all())
    assert float(b["grad"][..., c.C:].abs().max()) == 0.0


@pytest.mark.parametrize("name", [n for n in LC.NAMES if LC.TABLE[n].mask in ("disc", "pixels")])
def test_what_the_mask_hides_changes_nothing(name):
    d = LC.build(name)
    dead = ~d.mask
    assert bool(dead.any())
    dirty = d.img.clone()
    dirty[dead] = float("nan")
    dirty[:, 0, 0][dead[:, 0, 0]] = float("inf")
    dirty[:, -1, -1][dead[:, -1, -1]] = -float("inf")
    a, b = _run(name), _run(name, img=dirty)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert bool(torch.isfinite(b["loss"])) and bool(torch.isfinite(b["grad"]).all())
    assert float(b["grad"][dead.to(DEV)].abs().max()) == 0.0
    _check(name, b, " (non-finite under the mask)")
