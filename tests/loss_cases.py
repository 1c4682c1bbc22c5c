"""Float64-oracle case table of the photometric loss kernels (csrc/ssim.hip,
csrc/ssim_fused_body.h).  Host only: torch on the CPU, no GPU import.

The oracle is tests/masked_loss_oracle.py (float64, autograd).  A case names
its entry point, shape, content and options; its inputs are built from a seed
derived from that name.

Entry points (what the GPU test calls) and what `dispatch` says runs:

    sl1     ssim_and_l1(img, gt)                 outputs S, L1, d(a S + b L1)/dimg
    two     l1_ssim_loss(img, gt, lam, fused=False)
    fused   l1_ssim_loss(..., fused=True, gt_index=, _out_ring=, _channels=)
    masked  l1_ssim_loss(..., fused=True, masks=, alphas=, backgrounds=)

Bounds.  Per case and output, `bar` is the maximum absolute error of the
float32 torch composition on the CPU (train_step.ssim, losses.compose_masked,
autograd) against the oracle, and an output's maximum absolute error is held
to

    max(FACTOR * bar, FLOOR * max|want|)

with one exception, derived here and not measured: the scalar loss.  It is
formed as (1 - lam) L1 + lam (1 - S) from the float32 means S and L1, so it
carries the rounding of those two terms however small it is itself: S is a
float32 number near 1 (its representation alone is u |S|, u = 2^-24 = 6e-8,
and every pixel's SSIM value A1 A2 * (1 / (B1 B2)) is three roundings on a
value near 1), and where img == gt the loss is exactly 0 in the oracle and in
the float32 composition (both divide N by the identical N), so both bar and
max|want| vanish while a kernel that multiplies by the reciprocal is right to
1 - S = O(u) only.  The loss's floor is therefore taken on the magnitudes of
the terms it sums, not on their difference:

    FLOOR * max(|L|, lam |S|, (1 - lam) |L1|)

The second derived floor is the mean SSIM's conditioning, on S and (times lam)
on the loss.  Each pixel's variances are differences s11 = E[x^2] - mu1^2 of
two 121-term float32 sums; in a flat block both are a^2 and the difference
is their rounding, about 1e-7 a^2, added to C2 = 9e-4: the pixel's SSIM is
then right to 1e-4, and the same for every pixel of the block, so the mean
does not average it away.  The float32 composition has the same conditioning
but one draw of its error (bar) does not bound another summation order's.
masked_loss_oracle.ssim_rounding_floor is the first-order worst case from the
count of roundings in the kernels' fma chains (11 + 11 per window sum, one
more per product term) and the magnitudes of the sums, evaluated on the
case's float64 statistics: about 1e-5 on uniform noise, 3e-6 on dark images,
up to 1e-3 on flat blocks.  A worst case, so it is loose where it bites; the
gradients, whose bars already carry that conditioning pixel by pixel, do not
get it.  (Found on the MI355X: the flat cases fused_flat_b2_74x12_c3s4 and,
through the two-pass kernels, fused_flat_b1_42x53_c3 missed the plain bound on
the loss alone -- profiles/loss_matrix/parity.txt.)

L1 of ssim_and_l1 and every gradient take the plain bound.
"""

import functools
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import masked_loss_oracle as O

FACTOR = 10.0   # tests/test_gpu_masked_loss.py's factor on the float32 composition's error
FLOOR = 1e-6    # the SH and projection matrices' floor, relative to max|want|
SL1_WEIGHTS = (0.3, 0.7)  # a, b of d(a S + b L1)/dimg (test_ssim_l1_matches_torch's)

# ------------------------------------------------------------------ dispatch
# the ten kernels of ssim.hip by the variants the host code launches them in
KERNELS = (
    "fwd_c_kernel<3>", "fwd_kernel", "bwd_kernel[l1_index=0]", "bwd_kernel[l1_index=1]",
    "fused_kernel<3,4,3,3>", "fused_kernel<3,2,3,4>", "fused_kernel<1,2,1,1>",
    "fused_masked_kernel<3,4>", "fused_masked_kernel<1,2>",
    "reduce_partials_kernel[sums]", "reduce_partials_kernel[loss]",
    "reduce_partials_kernel[loss+ring]", "fused_scale_kernel",
)


def dispatch(entry, C, XS=None, masked=False, bkgd=False, ring=False):
    """The kernels one forward + backward of that call launches, in order --
    ssim.hip's host dispatch (ssim_fwd, ssim_bwd, fused_fwd, the masked entry
    points) and losses.l1_ssim_loss's choice of entry point restated."""
    XS = C if XS is None else XS
    if entry in ("sl1", "two"):
        if XS != C or masked or bkgd or ring:
            raise ValueError(f"{entry}: contiguous images, no mask / background / ring")
        fwd = "fwd_c_kernel<3>" if C == 3 else "fwd_kernel"
        red, l1i = ("sums", 1) if entry == "sl1" else ("loss", 0)
        return (fwd, f"reduce_partials_kernel[{red}]", f"bwd_kernel[l1_index={l1i}]")
    red = "reduce_partials_kernel[loss+ring]" if ring else "reduce_partials_kernel[loss]"
    if entry == "fused":
        if masked or bkgd:
            raise ValueError("fused: masks / backgrounds go to the masked entry point")
        k = {(3, 3): "fused_kernel<3,4,3,3>", (3, 4): "fused_kernel<3,2,3,4>",
             (1, 1): "fused_kernel<1,2,1,1>"}.get((C, XS))
        if k is None:
            raise ValueError(f"fused: C = {C} with pixel stride {XS} is refused")
        return (k, red, "fused_scale_kernel")
    if entry == "masked":
        if XS != C or C not in (1, 3):
            raise ValueError(f"masked: C = {C}, stride {XS} is refused")
        k = "fused_masked_kernel<3,4>" if C == 3 else "fused_masked_kernel<1,2>"
        return (k, red, "fused_scale_kernel") + (("fused_scale_kernel",) if bkgd else ())
    raise ValueError(entry)


def partials(entry, B, H, W, C):
    """The number of (ssim, l1) pairs reduce_partials_kernel sums (it strides
    by 1024: more than that takes its loop round again)."""
    if entry in ("sl1", "two"):
        tiles = ((W - 10 + 31) // 32) * ((H - 10 + 31) // 32)  # the map's tiles
        return tiles * B * (1 if C == 3 else C)
    return ((W + 31) // 32) * ((H + 31) // 32) * B  # the image's tiles


# --------------------------------------------------------------------- table
KINDS = ("uniform", "render", "flat", "equal", "dark", "wide")
EDGES = (11, 12, 32, 33, 42, 43, 52, 53, 64, 65, 74, 75)
# map of 1 / 2 / 32 / 33 / 64 / 65 pixels, image of 1 / 1 + / 2 / 2 + tiles; each
# pair and its transpose, so every edge size is met as a height and as a width
_PAIRS = ((11, 75), (12, 74), (43, 32), (33, 65), (42, 53), (52, 64))
SHAPES = tuple(_PAIRS) + tuple((w, h) for h, w in _PAIRS)
RING_LEN = 8
STACK = 3  # targets in a gt_index stack
MASKS = ("disc", "pixels", "all")


def _case(entry, kind, B, H, W, C, XS=None, lam=0.2, scale=1.0, index=None, seq=None,
          mask=None, bkgd=False):
    XS = C if XS is None else XS
    name = f"{entry}_{kind}_b{B}_{H}x{W}_c{C}"
    name += f"s{XS}" if XS != C else ""
    name += f"_lam{lam:g}" if lam != 0.2 else ""
    name += f"_g{scale:g}" if scale != 1.0 else ""
    name += f"_idx{index}" if index is not None else ""
    name += f"_seq{seq}" if seq is not None else ""
    name += f"_{mask}" if mask is not None else ""
    name += "_bkgd" if bkgd else ""
    return SimpleNamespace(name=name, entry=entry, kind=kind, B=B, H=H, W=W, C=C, XS=XS,
                           lam=lam, scale=scale, index=index, seq=seq, mask=mask, bkgd=bkgd)


def _table():
    t = []
    two_c = (3, 1, 2, 4, 5)  # C = 3 first: fwd_c_kernel<3> is the trainer's forward
    for i, (H, W) in enumerate(SHAPES):
        for kind in ("uniform", "flat"):
            j = i + (kind == "flat")
            t.append(_case("sl1", kind, 1 + j % 3, H, W, two_c[j % 5]))
            t.append(_case("two", kind, 1 + (j + 1) % 3, H, W, two_c[(j + 2) % 5]))
            C, XS = ((3, 3), (1, 1), (3, 4))[j % 3]
            t.append(_case("fused", kind, 1 + (j + 2) % 3, H, W, C, XS))
            t.append(_case("masked", kind, 1 + j % 3, H, W, (3, 1)[j % 2], mask=MASKS[j % 3],
                           bkgd=bool((j // 2) % 2)))
    # the other contents, each at a one-tile and a two-tiles-and-one shape
    for k, kind in enumerate(("render", "equal", "dark", "wide")):
        for s, (H, W) in enumerate(((33, 65), (75, 11), (43, 32))):
            j = k + s
            t.append(_case("sl1", kind, 1 + j % 2, H, W, two_c[j % 5]))
            t.append(_case("two", kind, 1 + (j + 1) % 2, H, W, two_c[(j + 1) % 5]))
            C, XS = ((3, 3), (1, 1), (3, 4))[j % 3]
            t.append(_case("fused", kind, 1 + j % 2, H, W, C, XS))
            t.append(_case("masked", kind, 1 + (j + 1) % 2, H, W, (3, 1)[j % 2],
                           mask=MASKS[(j + 1) % 3], bkgd=bool(j % 2)))
    # more than 1024 partials: batches of the smallest image (a 1 x 2 map),
    # 132 to 405 thousand floats -- an image of 1322 x 810 has 3.2 million
    t.append(_case("two", "uniform", 1025, 11, 12, 3))     # fwd_c_kernel<3>: one per image
    t.append(_case("sl1", "uniform", 205, 11, 12, 5))      # fwd_kernel: one per channel
    t.append(_case("fused", "uniform", 1025, 11, 12, 3))   # one per image tile
    # fused_scale_kernel's scalar tail: B H W XS % 4 = 1, 2, 3 in either backward
    for entry, kw in (("fused", {}), ("masked", dict(mask="disc", bkgd=True))):
        t.append(_case(entry, "uniform", 1, 11, 75, 1, scale=2.5, **kw))  # 825 = 4 * 206 + 1
        t.append(_case(entry, "flat", 1, 42, 53, 3, **kw))                # 6678 = 4 * 1669 + 2
        t.append(_case(entry, "uniform", 1, 33, 65, 3, **kw))             # 6435 = 4 * 1608 + 3
    t.append(_case("two", "render", 2, 43, 32, 3, scale=2.5))
    # lambda 0 (on img == gt: nothing left) and 1 (SSIM alone)
    for entry, kw in (("two", {}), ("fused", {}), ("masked", dict(mask="pixels", bkgd=False))):
        t.append(_case(entry, "equal", 2, 43, 32, 3, lam=0.0, **kw))
        t.append(_case(entry, "uniform", 1, 33, 65, 3, lam=1.0, **kw))
    # the first and the last target of a stack, and the loss ring's two ends
    t.append(_case("fused", "uniform", 1, 43, 32, 3, index=0))
    t.append(_case("fused", "flat", 1, 33, 65, 3, 4, index=STACK - 1))
    t.append(_case("masked", "uniform", 1, 65, 33, 3, index=STACK - 1, mask="disc", bkgd=True))
    t.append(_case("fused", "render", 1, 43, 32, 3, index=1, seq=1))
    t.append(_case("fused", "wide", 1, 33, 65, 1, index=0, seq=2 * RING_LEN))
    t.append(_case("masked", "uniform", 1, 43, 32, 3, index=STACK - 1, seq=RING_LEN + 1,
                   mask="pixels", bkgd=True))
    t.append(_case("masked", "flat", 1, 52, 64, 1, index=0, seq=3 * RING_LEN, mask="disc"))
    names = [c.name for c in t]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return {c.name: c for c in t}


TABLE = _table()
NAMES = tuple(TABLE)


def kernels_of(c):
    return dispatch(c.entry, c.C, c.XS, c.mask is not None, c.bkgd, c.seq is not None)


def ring_slot(c):
    return (c.seq - 1) % RING_LEN


def scale_tail(c):
    """B H W XS % 4 of a case whose backward is fused_scale_kernel, else None."""
    return (c.B * c.H * c.W * c.XS) % 4 if c.entry in ("fused", "masked") else None


def outputs(c):
    if c.entry == "sl1":
        return ("S", "L1", "grad")
    return ("loss", "grad") + (("galpha",) if c.bkgd else ())


# ------------------------------------------------------------------ contents
def _flat(g, B, H, W, C):
    """Blocks of 8 to 16 pixels, constant per channel: a quarter exactly 0;
    gt equals img in four blocks of ten and differs by a constant elsewhere."""
    def cuts(n):
        out, at = [], 0
        while at < n:
            at += int(torch.randint(8, 17, (1,), generator=g))
            out.append(min(at, n))
        return out

    img, gt = torch.zeros(B, H, W, C), torch.zeros(B, H, W, C)
    for b in range(B):
        i0 = 0
        for i1 in cuts(H):
            j0 = 0
            for j1 in cuts(W):
                v = torch.rand(C, generator=g)
                if float(torch.rand(1, generator=g)) < 0.25:
                    v = torch.zeros(C)
                d = (torch.rand(C, generator=g) - 0.5) * 0.4
                if float(torch.rand(1, generator=g)) < 0.4:
                    d = torch.zeros(C)
                img[b, i0:i1, j0:j1] = v
                gt[b, i0:i1, j0:j1] = v + d
                j0 = j1
            i0 = i1
    return img, gt


def _content(kind, g, B, H, W, C):
    if kind == "uniform":
        return torch.rand(B, H, W, C, generator=g), torch.rand(B, H, W, C, generator=g)
    if kind == "render":  # blurred noise and a copy of it shifted by two pixels
        base = F.avg_pool2d(torch.rand(B, C, H, W + 2, generator=g), 5, 1, 2)
        return (base[..., 2:].permute(0, 2, 3, 1).contiguous(),
                base[..., :-2].permute(0, 2, 3, 1).contiguous())
    if kind == "flat":
        return _flat(g, B, H, W, C)
    if kind == "equal":
        img = torch.rand(B, H, W, C, generator=g)
        return img, img.clone()
    if kind == "dark":
        return (torch.rand(B, H, W, C, generator=g) * 0.02,
                torch.rand(B, H, W, C, generator=g) * 0.02)
    if kind == "wide":
        return (torch.rand(B, H, W, C, generator=g) * 3.0 - 0.5,
                torch.rand(B, H, W, C, generator=g) * 3.0 - 0.5)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def build(name):
    """The float32 CPU inputs of a case.  img [B,H,W,XS] (channels past C are
    the render's other channels: uniform noise), gt [B,H,W,C] or, with an
    index, a stack [STACK,H,W,C] whose entry `index` is the target (the others
    noise), masks [B or STACK,H,W] bool, alphas [B,H,W,1], back [B,C]."""
    c = TABLE[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    img, gt = _content(c.kind, g, c.B, c.H, c.W, c.C)
    if c.XS != c.C:
        img = torch.cat([img, torch.rand(c.B, c.H, c.W, c.XS - c.C, generator=g)], -1)
    mask = None
    if c.mask is not None:
        mask = {"disc": O.disc_mask, "pixels": O.pixel_mask,
                "all": lambda *s: torch.ones(*s, dtype=torch.bool)}[c.mask](c.B, c.H, c.W)
    alphas = torch.rand(c.B, c.H, c.W, 1, generator=g) if c.entry == "masked" else None
    back = (torch.rand(c.B, c.C, generator=g) * 0.8 + 0.1) if c.bkgd else None
    gts, masks = gt, mask
    if c.index is not None:
        assert c.B == 1
        gts = torch.rand(STACK, c.H, c.W, c.C, generator=g)
        gts[c.index] = gt[0]
        if mask is not None:
            masks = torch.rand(STACK, c.H, c.W, generator=g) < 0.5
            masks[c.index] = mask[0]
    return SimpleNamespace(case=c, img=img, gt=gt, gts=gts, mask=mask, masks=masks,
                           alphas=alphas, back=back)


# -------------------------------------------------------------------- oracle
@functools.lru_cache(maxsize=None)
def oracle64(name):
    """{output: float64 tensor} of a case, computed once and shared read-only.
    grad is img-shaped (zero in the channels past C)."""
    d = build(name)
    c = d.case
    x = d.img[..., :c.C]
    if c.entry == "sl1":
        a, b = SL1_WEIGHTS
        S, L1, gx = O.ssim_and_l1_grads(x, d.gt, a, b)
        return {"S": S, "L1": L1, "grad": gx,
                "_cond": O.ssim_rounding_floor(x.double(), d.gt.double())}
    L, gx, ga = O.loss_and_grads(x, d.gt, c.lam, d.mask, d.alphas, d.back, scale=c.scale)
    if c.XS != c.C:
        gx = torch.cat([gx, torch.zeros(c.B, c.H, c.W, c.XS - c.C, dtype=gx.dtype)], -1)
    out = {"loss": L, "grad": gx}
    if c.bkgd:
        out["galpha"] = ga
    # the magnitudes of the terms the loss sums (its floor, see the module docstring)
    with torch.no_grad():
        xc = O.compose(O._f64(x), d.mask, O._f64(d.alphas), O._f64(d.back))
        S, L1 = O.ssim_and_l1(xc, d.gt.double())
        out["_cond"] = c.lam * O.ssim_rounding_floor(xc, d.gt.double())
    out["_terms"] = torch.stack([L.abs(), c.lam * S.abs(), (1.0 - c.lam) * L1.abs()]).max()
    return out


def composition32(name):
    """{output: float32 tensor}: the torch composition the kernels replace,
    float32 on the CPU -- train_step.ssim, losses.compose_masked, autograd."""
    from gsplat_hip.losses import compose_masked
    from gsplat_hip.train_step import ssim
    d = build(name)
    c = d.case
    x = d.img[..., :c.C].clone().requires_grad_(True)
    y = d.gt
    if c.entry == "sl1":
        a, b = SL1_WEIGHTS
        S = ssim(x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2))
        L1 = (x - y).abs().mean()
        (a * S + b * L1).backward()
        return {"S": S.detach(), "L1": L1.detach(), "grad": x.grad}
    al = None if d.alphas is None else d.alphas.clone().requires_grad_(c.bkgd)
    xc = compose_masked(x, d.mask, al, d.back)
    L = (xc - y).abs().mean() * (1 - c.lam) + (1 - ssim(xc.permute(0, 3, 1, 2),
                                                        y.permute(0, 3, 1, 2))) * c.lam
    (c.scale * L).backward()
    gx = x.grad
    if c.XS != c.C:
        gx = torch.cat([gx, torch.zeros(c.B, c.H, c.W, c.XS - c.C)], -1)
    out = {"loss": L.detach(), "grad": gx}
    if c.bkgd:
        out["galpha"] = al.grad
    return out


def max_err(got, want):
    return float((got.detach().double().cpu() - want).abs().max())


@functools.lru_cache(maxsize=None)
def bars(name):
    """{output: the float32 composition's maximum absolute error}, once per case."""
    want, own = oracle64(name), composition32(name)
    return {k: max_err(own[k], want[k]) for k in outputs(TABLE[name])}


def bound(name, output):
    want = oracle64(name)
    mag = float(want["_terms"]) if output == "loss" else float(want[output].abs().max())
    cond = float(want["_cond"]) if output in ("loss", "S") else 0.0
    return max(FACTOR * bars(name)[output], FLOOR * mag, cond)
