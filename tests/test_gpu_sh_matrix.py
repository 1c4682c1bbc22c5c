"""GPU: every instantiation of the SH colour kernels (csrc/sh.hip) against the
float64 oracle of tests/sh_cases.py.

sh.hip compiles sh_fwd_kernel<DEG, FUSED>, sh_bwd_kernel<DEG, FUSED> and
sh_bwd_staged_kernel<DEG, FUSED, KR, ADAM, CAMS> behind seven entry points.
Cases (rows 1 / 65 / 321, cameras 1 / 3, masks all on / 30 % off / a dead
wave, directions on the axes and diagonals and of lengths 1e-3 .. 1e3) and
the oracle: sh_cases.py.  Bound of every output: max(FACTOR x bar, FLOOR)
relative to the largest |oracle value|, bar being the float32 error of the
reference's torch implementation on the same case (tests/golden/
sh_matrix.npz); tests/test_sh_cases_host.py shows on the CPU that plain
float32 arithmetic meets it.

  a  spherical_harmonics, degrees 0-4: staged backward (K == (deg+1)^2, KR =
     0, 3, 8, 15, 24) and unstaged (K above, or coefficient rows broadcast
     over 3 cameras); one tensor and the pair (sh0, shN); with and without
     masks; with and without v_dirs
  b  sh_colors, degrees 0-4: 1 and 3 cameras, shared and per-camera
     coefficients, K equal to and above (deg+1)^2; rows with radii <= 0
     give exactly 0.5 and exactly zero gradients
  c  gsplat_hip_sh_colors_bwd_sum, degrees 0-3, against the oracle's
     gradients summed over cameras
  d  gsplat_hip_sh_colors_bwd_adam and _adam_dev, degrees 0-3: three steps
     against torch.optim.Adam's update in float64; zero-gradient rows; skip
  e  the clamp gate at equality, forward and every backward

The largest error of every output per group, with its bar and bound, is
printed as one JSON line when the module finishes (pytest -s shows it).
"""

import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import sh_cases as SC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERRORS = {}  # group -> output -> the entry with the largest err / bound
BARS = SC.load_bars(os.path.join(GOLDEN, "sh_matrix.npz"))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gsplat_hip  # noqa: F401  (fails loudly if the .so is missing)
    yield
    line = {g: {k: {f: float(f"{r[f]:.3g}") for f in ("err", "bar", "bound")} for k, r in o.items()}
            for g, o in ERRORS.items()}
    print("\nsh_matrix_errors " + json.dumps(line, sort_keys=True, separators=(",", ":")))
    for g, o in sorted(ERRORS.items()):
        k = max(o, key=lambda k: o[k]["ratio"])
        print(f"sh_matrix group {g}: largest err / bound {o[k]['ratio']:.3f} ({k}, {o[k]['case']})")


def T(x, grad=False):
    return torch.from_numpy(np.array(x)).to(DEV).requires_grad_(grad)  # the cases stay read-only


def npy(t):
    return t.detach().cpu().numpy()


def _gpu(fn):
    """fn() and a synchronize; a HIP error (a fault on the card) ends the
    session: no further kernel is launched on a card that has faulted."""
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"GPU fault, stopping: {e}", returncode=3)
        raise


def check(group, name, what, pairs):
    """pairs: {output: (ours, oracle)} or {output: (ours, oracle, bar key)}.
    Prints and records every figure, then asserts each against
    max(FACTOR x bar, FLOOR)."""
    bad = []
    for k, pr in pairs.items():
        ours, ref = pr[0], pr[1]
        bar = BARS[f"{name}:{pr[2] if len(pr) > 2 else k}"]
        assert ours.shape == ref.shape, (name, what, k, ours.shape, ref.shape)
        assert np.isfinite(ours).all(), (name, what, k)
        e, b = SC.rel_err(ours, ref), SC.bound(bar)
        print(f"{name} {what}: {k}: err {e:.3e}  bound {b:.3e}  (bar {bar:.3e})")
        rec = ERRORS.setdefault(group, {})
        if k not in rec or e / b > rec[k]["ratio"]:
            rec[k] = {"err": e, "bar": bar, "bound": b, "ratio": e / b, "case": f"{name} {what}"}
        if not e <= b:
            bad.append((k, e, b))
    assert not bad, (name, what, bad)


# ------------------------------------------------- a: spherical_harmonics
def _run_nf(c, pair, want_dirs):
    import gsplat_hip
    dirs = T(c.dirs, want_dirs)
    lead = dirs.shape[:-1]
    if pair:
        leaves = [T(c.coeffs[:, :1], True), T(c.coeffs[:, 1:], True)]
        cf = tuple(t.expand(*lead, -1, -1) for t in leaves)
    else:
        leaves = [T(c.coeffs, True)]
        cf = leaves[0].expand(*lead, -1, -1)
    if c.C > 1:
        assert (cf[0] if pair else cf).stride(0) == 0  # read in place: n_coeff_rows < n
    masks = None if c.masks is None else T(c.masks)
    col = gsplat_hip.spherical_harmonics(c.deg, dirs, cf, masks=masks)
    gr = torch.autograd.grad((col * T(c.v_colors)).sum(), leaves + ([dirs] if want_dirs else []))
    out = {"colors": npy(col), "v_coeffs": npy(torch.cat(gr[:len(leaves)], -2))}
    if want_dirs:
        norm = np.linalg.norm(c.dirs.astype(np.float64), axis=-1, keepdims=True)
        out["v_dirs"] = npy(gr[-1]).astype(np.float64) * norm
    return out


@pytest.mark.parametrize("name", SC.NF_NAMES)
def test_spherical_harmonics_vs_float64_oracle(name):
    c, ref = SC.build(name), SC.oracle64(name)
    off = None if c.masks is None else ~c.masks
    for pair in ((False, True) if c.K > 1 else (False,)):
        for want_dirs in (True, False):
            got = _gpu(lambda: _run_nf(c, pair, want_dirs))
            what = ("pair" if pair else "one") + ("" if want_dirs else " no-v_dirs")
            check("a", name, what, {k: (v, ref[k]) for k, v in got.items()})
            nb = (c.deg + 1) ** 2
            assert not got["v_coeffs"][:, nb:].any()  # above the active degree
            if off is not None:  # masked rows: exact zeros
                assert not got["colors"][off].any()
                if want_dirs:
                    assert not got["v_dirs"][off].any()
                if c.C == 1:
                    assert not got["v_coeffs"][off].any()
            if want_dirs and c.deg == 0:
                assert not got["v_dirs"].any()


# ------------------------------------------------------------ b: sh_colors
def _run_fz(c, pair, want_means):
    from gsplat_hip._wrapper import sh_colors
    means = T(c.means, want_means)
    if pair:
        leaves = [T(c.coeffs[..., :1, :], True), T(c.coeffs[..., 1:, :], True)]
        cf = tuple(leaves)
    else:
        leaves = [T(c.coeffs, True)]
        cf = leaves[0]
    col = sh_colors(c.deg, means, T(c.viewmats), cf, T(c.radii))
    gr = torch.autograd.grad((col * T(c.v_colors)).sum(), leaves + ([means] if want_means else []))
    out = {"colors": npy(col), "v_coeffs": npy(torch.cat(gr[:len(leaves)], -2))}
    if want_means:
        out["v_means"] = npy(gr[-1])
    return out


def _check_invisible(c, got):
    """Exact values where radii <= 0: colours 0.5; zero gradient rows for
    per-camera coefficients, and for Gaussians no camera sees."""
    off = ~(c.radii > 0)
    assert (got["colors"][off] == 0.5).all()
    unseen = off.all(0)
    if "v_coeffs" in got:
        if c.percam:
            assert not got["v_coeffs"][off].any()
        else:
            assert not got["v_coeffs"][unseen].any()
        assert not got["v_coeffs"][..., (c.deg + 1) ** 2:, :].any()
    if "v_means" in got:
        assert not got["v_means"][unseen].any()


@pytest.mark.parametrize("name", SC.FZ_NAMES)
def test_sh_colors_vs_float64_oracle(name):
    c, ref = SC.build(name), SC.oracle64(name)
    for pair in ((False, True) if c.K > 1 else (False,)):
        for want_means in (True, False):
            got = _gpu(lambda: _run_fz(c, pair, want_means))
            what = ("pair" if pair else "one") + ("" if want_means else " no-v_means")
            check("b", name, what, {k: (v, ref[k]) for k, v in got.items()})
            _check_invisible(c, got)


# --------------------------------------------------------- c: bwd_sum
SUM_NAMES = [n for n in SC.FZ_NAMES if "_k16_" in n and n.endswith("_sh")]


def _ptrs():
    from gsplat_hip._wrapper import _ptr, _stream
    return _ptr, _stream


@pytest.mark.parametrize("name", SUM_NAMES)
def test_bwd_sum_vs_float64_oracle(name):
    from gsplat_hip import _lib
    _ptr, _stream = _ptrs()
    c, ref = SC.build(name), SC.oracle64(name)
    assert c.deg <= 3 and c.coeffs.shape == (c.N, 16, 3)
    means, vm, radii, vcol = T(c.means), T(c.viewmats), T(c.radii), T(c.v_colors)
    sh0, shN = T(c.coeffs[:, :1]), T(c.coeffs[:, 1:])
    for want_means in (True, False):
        s0 = torch.full((c.N, 1, 3), float("nan"), device=DEV)
        sr = torch.full((c.N, 15, 3), float("nan"), device=DEV)
        sd = torch.full((c.N, 3), float("nan"), device=DEV) if want_means else None
        _gpu(lambda: _lib.call("gsplat_hip_sh_colors_bwd_sum", c.deg, c.C, c.N, _ptr(means),
                               _ptr(vm), _ptr(sh0), _ptr(shN), _ptr(radii), _ptr(vcol), _ptr(s0),
                               _ptr(sr), _ptr(sd), _stream()))
        got = {"v_coeffs": npy(torch.cat([s0, sr], 1))}
        if want_means:
            got["v_means"] = npy(sd)
        check("c", name, "sum" + ("" if want_means else " no-v_means"),
              {k: (v, ref[k]) for k, v in got.items()})
        unseen = ~(c.radii > 0).any(0)
        for v in got.values():
            assert not v[unseen].any()
        assert not got["v_coeffs"][:, (c.deg + 1) ** 2:].any()


# ------------------------------------------------------------- d: Adam
def _hyper(step, abi_floats=False):
    """{lr0 / bc1, lr_rest / bc1, 1 / sqrt(bc2)}: from the settings as given
    (what a caller hands gsplat_hip_sh_colors_bwd_adam_dev), or as
    gsplat_hip_sh_colors_bwd_adam forms them from its float arguments."""
    a = SC.ADAM
    lr0, lrr, b1, b2 = a["lr0"], a["lr_rest"], a["betas"][0], a["betas"][1]
    if abi_floats:
        lr0, lrr, b1, b2 = (float(np.float32(x)) for x in (lr0, lrr, b1, b2))
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return [lr0 / bc1, lrr / bc1, 1 / math.sqrt(bc2)]


class _AdamState:
    def __init__(self, c, m_init=None, v_init=None):
        self.c = c
        self.means, self.vm, self.radii, self.vcol = (T(c.means), T(c.viewmats), T(c.radii),
                                                      T(c.v_colors))
        self.p0, self.pr = T(c.coeffs[:, :1]), T(c.coeffs[:, 1:])
        m = np.zeros_like(c.coeffs) if m_init is None else m_init
        v = np.zeros_like(c.coeffs) if v_init is None else v_init
        self.m0, self.mr = T(m[:, :1]), T(m[:, 1:])
        self.v0, self.vr = T(v[:, :1]), T(v[:, 1:])
        self.vd = torch.full((c.N, 3), float("nan"), device=DEV)

    def step(self, step, dev, skip=None):
        from gsplat_hip import _lib
        _ptr, _stream = _ptrs()
        a, c = SC.ADAM, self.c
        head = (c.deg, c.C, c.N, _ptr(self.means), _ptr(self.vm), _ptr(self.p0), _ptr(self.pr),
                _ptr(self.radii), _ptr(self.vcol), _ptr(self.vd), _ptr(self.m0), _ptr(self.v0),
                _ptr(self.mr), _ptr(self.vr))
        f = ctypes.c_float
        if dev:
            hyper = torch.tensor(_hyper(step), dtype=torch.float32, device=DEV)
            flag = None if skip is None else torch.tensor([skip], dtype=torch.int32, device=DEV)
            _gpu(lambda: _lib.call("gsplat_hip_sh_colors_bwd_adam_dev", *head, _ptr(hyper),
                                   f(a["betas"][0]), f(a["betas"][1]), f(a["eps"]), _ptr(flag),
                                   _stream()))
        else:
            _gpu(lambda: _lib.call("gsplat_hip_sh_colors_bwd_adam", *head, f(a["lr0"]),
                                   f(a["lr_rest"]), f(a["betas"][0]), f(a["betas"][1]),
                                   f(a["eps"]), int(step), _stream()))

    def state(self):
        return {"p": npy(torch.cat([self.p0, self.pr], 1)),
                "m": npy(torch.cat([self.m0, self.mr], 1)),
                "v": npy(torch.cat([self.v0, self.vr], 1)), "v_means": npy(self.vd)}


_ADAM_RUNS = {}  # (case, dev) -> state after three steps, shared by the two tests below


def _adam_three_steps(name, dev):
    """(exp_avg after step 1, state after step 3), run once per case and form."""
    if (name, dev) not in _ADAM_RUNS:
        st = _AdamState(SC.build(name))
        st.step(1, dev)
        m1 = st.state()["m"]
        for step in (2, 3):
            st.step(step, dev)
        _ADAM_RUNS[name, dev] = (m1, st.state())
    return _ADAM_RUNS[name, dev]


F32_BETAS = tuple(float(np.float32(b)) for b in SC.ADAM["betas"])


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("name", SC.ADAM_NAMES)
def test_adam_in_backward_vs_float64_oracle(name, dev):
    """exp_avg after step 1, and exp_avg, the parameters and v_dirs after step
    3, against torch.optim.Adam's update in float64 with betas (0.9, 0.999).
    exp_avg_sq against that oracle is the next test's; here it is held to the
    same bound against the same oracle with the betas the entry points
    receive, float32(0.9) and float32(0.999) (their ABI type is float)."""
    c, ref = SC.build(name), SC.oracle64(name)
    m1, got = _adam_three_steps(name, dev)
    what = "dev" if dev else "host"
    # exp_avg after the first step is 0.1 x the gradient: every
    # instantiation's gradient, at the gradient's bar
    check("d", name, what, {"m1": (m1, ref["m1"], "v_coeffs")})
    check("d", name, what, {k: (got[k], ref[k]) for k in ("m", "p", "v_means")})
    v32 = SC.oracle_adam(c, betas=F32_BETAS)["v"]
    check("d", name, what, {"v_float32_betas": (got["v"], v32, "v")})
    # no gradient (unseen Gaussians, coefficients above the active degree):
    # zero moments stay zero and the parameter does not move
    unseen = ~(c.radii > 0).any(0)
    nb = (c.deg + 1) ** 2
    for k in ("m", "v"):
        assert not got[k][unseen].any() and not got[k][:, nb:].any()
    assert np.array_equal(got["p"][unseen], c.coeffs[unseen])
    assert np.array_equal(got["p"][:, nb:], c.coeffs[:, nb:])
    assert not got["v_means"][unseen].any()


@pytest.mark.xfail(strict=True, reason="exp_avg_sq is 1.29e-5 from the float64 oracle at betas "
                   "(0.9, 0.999): beta2 reaches the kernels as float32(0.999) = 0.999 + 1.29e-8, "
                   "so their 1 - beta2 is 0.001 x (1 - 1.29e-5); rounding of the hyperparameter "
                   "alone, see the docstring")
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("name", SC.ADAM_NAMES)
def test_adam_exp_avg_sq_vs_float64_oracle(name, dev):
    """exp_avg_sq after step 3 against the float64 oracle at betas (0.9,
    0.999).  Measured on the MI355X: 1.27e-5 .. 1.33e-5 of the largest value
    on all 48 cases, bound 1e-6 .. 2.9e-6.  The entry points take beta2 as a
    C float: float32(0.999) = 0.99900001287, and 1 - that (exact in float32)
    is 0.00099998713 = 0.001 x (1 - 1.29e-5), the factor of every g^2 term.
    The kernels are an exact Adam for that beta2 (bias correction included):
    against the oracle with the float32 betas exp_avg_sq is inside the same
    bound (the test above).  torch's float32 Adam rounds 1 - beta2 from the
    double instead, hence the bar.  The parameters feel it as 6.4e-6 of a step
    of at most lr: they pass.  Matching betas (0.9, 0.999) would take 1 -
    beta2 as a separate argument of every Adam entry point (the element
    update is shared with the FusedAdam kernels, bit for bit)."""
    _, got = _adam_three_steps(name, dev)
    check("d_exp_avg_sq", name, "dev" if dev else "host", {"v": (got["v"], SC.oracle64(name)["v"])})


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("name", [n for n in SC.ADAM_NAMES if "_n321_" in n and "_dead" in n])
def test_adam_zero_gradient_rows_decay_only(name, dev):
    """From non-zero moments, one update (step 2) of rows without a gradient:
    exp_avg = fma(1 - b1, 0 - m, m) and exp_avg_sq = b2 v with float32's
    single roundings, which float64 reproduces exactly (a 24 x 24-bit product
    plus a 24-bit addend of about the same exponent fits 53 bits).  The
    parameter moves by ss m' / (sqrt(v') ib + eps) alone: against float64
    from those m', v' the kernel's multiply, square root, fma and division
    each round once (4 x 2^-24 of the step, taken as 8) and the subtraction
    once more (half an ulp of the parameter before or after, whichever is in
    the larger binade)."""
    c = SC.build(name)
    g = torch.Generator().manual_seed(11)
    m_init = (torch.randn(c.N, 16, 3, generator=g) * 1e-2).numpy()
    v_init = (torch.randn(c.N, 16, 3, generator=g) * 1e-2).square().numpy()
    st = _AdamState(c, m_init, v_init)
    st.step(2, dev)
    got = st.state()
    nograd = np.zeros((c.N, 16), bool)
    nograd[~(c.radii > 0).any(0)] = True
    nograd[:, (c.deg + 1) ** 2:] = True
    assert nograd[64:128].all() and not nograd.all()
    b1, b2 = (np.float64(np.float32(b)) for b in SC.ADAM["betas"])
    one_b1 = np.float64(np.float32(1) - np.float32(SC.ADAM["betas"][0]))
    m64, v64, p64 = (a.astype(np.float64) for a in (m_init, v_init, c.coeffs))
    want_m = (one_b1 * (0.0 - m64) + m64).astype(np.float32)
    want_v = (b2 * v64).astype(np.float32)
    assert np.array_equal(got["m"][nograd], want_m[nograd])
    assert np.array_equal(got["v"][nograd], want_v[nograd])
    ss0, ssr, ib = (np.float64(np.float32(h)) for h in _hyper(2, abi_floats=not dev))
    ss = np.full((16, 1), ssr)
    ss[0] = ss0
    upd = ss * want_m.astype(np.float64) / (np.sqrt(want_v.astype(np.float64)) * ib
                                            + np.float64(np.float32(SC.ADAM["eps"])))
    want_p = p64 - upd
    big = np.maximum(np.abs(c.coeffs), np.abs(want_p).astype(np.float32))  # either binade
    tol = 8 * 2.0 ** -24 * np.abs(upd) + 0.5 * np.spacing(big).astype(np.float64)
    diff = np.abs(got["p"].astype(np.float64) - want_p)
    assert (np.abs(upd[nograd]) > 1e-5).mean() > 0.5  # the decay does move them
    assert (diff[nograd] <= tol[nograd]).all(), float((diff / tol)[nograd].max())
    # the rows with a gradient got another update
    assert not np.array_equal(got["m"][~nograd], want_m[~nograd])


@pytest.mark.parametrize("name", [n for n in SC.ADAM_NAMES if "_n321_" in n and "_rand" in n])
def test_adam_dev_skip_leaves_state_and_writes_v_dirs(name):
    c = SC.build(name)
    g = torch.Generator().manual_seed(12)
    m_init = (torch.randn(c.N, 16, 3, generator=g) * 1e-2).numpy()
    v_init = (torch.randn(c.N, 16, 3, generator=g) * 1e-2).square().numpy()
    st = _AdamState(c, m_init, v_init)
    st.step(1, True, skip=1)
    got = st.state()
    assert np.array_equal(got["p"], c.coeffs)
    assert np.array_equal(got["m"], m_init) and np.array_equal(got["v"], v_init)
    # v_dirs as without the flag (group d holds that one to the oracle)
    ref = _AdamState(c, m_init, v_init)
    ref.step(1, True, skip=0)
    assert np.isfinite(got["v_means"]).all() and (c.deg == 0 or got["v_means"].any())
    assert np.array_equal(got["v_means"], ref.state()["v_means"])
    assert not np.array_equal(ref.state()["p"], c.coeffs)


# --------------------------------------------------- e: the gate at equality
def _gate_coefficient():
    """float32 c with fl(B0 c) == -0.5 exactly, B0 the kernel's float32
    constant; and its neighbour one ulp further below."""
    b0 = np.float32(0.28209479177387814)
    c = np.float32(-0.5) / b0
    for _ in range(4):
        c = np.nextafter(c, np.float32(0))
    for _ in range(9):
        if np.float32(b0 * c) == np.float32(-0.5):
            below = np.nextafter(c, np.float32(-np.inf))
            while np.float32(b0 * below) == np.float32(-0.5):
                below = np.nextafter(below, np.float32(-np.inf))
            return c, below
        c = np.nextafter(c, np.float32(-np.inf))
    raise AssertionError("no float32 c with fl(B0 c) == -0.5")


@pytest.mark.parametrize("K,C,pair", [(1, 1, False), (16, 1, False), (16, 1, True), (16, 3, True),
                                      (1, 3, False)])
def test_clamp_gate_at_equality(K, C, pair):
    """Degree 0, sh + 0.5 == 0 exactly in one channel of one row: the colour
    is exactly 0 and the gradient passes (torch.clamp_min at equality); one
    ulp below, the colour is 0 and the gradient exactly zero.  K = 1, C = 1:
    the staged backward; K = 16: the unstaged one; the pair at C = 3: the sum
    over cameras; C = 3, K = 1: shared rows, unstaged."""
    from gsplat_hip._wrapper import sh_colors
    at, below = _gate_coefficient()
    assert np.float32(np.float32(0.28209479177387814) * at) + np.float32(0.5) == 0
    assert np.float32(np.float32(0.28209479177387814) * below) + np.float32(0.5) < 0
    base = SC.build("fz_d0_k16_n65_c3_on_sh")
    N, row, ch = base.N, 37, 1
    for value, passes in ((at, True), (below, False)):
        coeffs = np.array(base.coeffs[:, :K])
        coeffs[row, 0, ch] = value
        means = T(base.means, True)
        leaves = [T(coeffs[:, :1], True), T(coeffs[:, 1:], True)] if pair else [T(coeffs, True)]
        radii, vcol = T(base.radii[:C]), T(base.v_colors[:C])
        col = _gpu(lambda: sh_colors(0, means, T(base.viewmats[:C]),
                                     tuple(leaves) if pair else leaves[0], radii))
        gr = _gpu(lambda: torch.autograd.grad((col * vcol).sum(), leaves))
        colors, v_dc = npy(col), npy(gr[0])[:, 0]
        assert (colors[:, row, ch] == 0).all(), colors[:, row, ch]
        b0 = np.float32(0.28209479177387814)
        want = (b0 * base.v_colors[:C, row, ch]).astype(np.float64).sum() if passes else 0.0
        if passes:
            assert abs(v_dc[row, ch] - want) <= 4 * 2.0 ** -24 * np.abs(b0 * base.v_colors[:C, row, ch]).sum()
            assert v_dc[row, ch] != 0
        else:
            assert v_dc[row, ch] == 0
        if pair and K == 16:  # the fused Adam's backward: exp_avg = 0.1 x gradient
            c = SimpleCase(base, coeffs, C)
            st = _AdamState(c)
            st.step(1, False)
            m1 = st.state()["m"][row, 0, ch]
            assert (m1 != 0) == passes, m1
            if passes:
                assert abs(m1 / 0.1 - want) <= 1e-6 * abs(want)


class SimpleCase:
    """The first C cameras of a fused case with other coefficients."""

    def __init__(self, base, coeffs, C):
        self.deg, self.N, self.C, self.K = base.deg, base.N, C, coeffs.shape[1]
        self.means, self.viewmats = base.means, base.viewmats[:C]
        self.radii, self.v_colors, self.coeffs = base.radii[:C], base.v_colors[:C], coeffs
