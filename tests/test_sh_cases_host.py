"""Host checks of the SH test matrix's oracle and case builder
(tests/sh_cases.py), none of which needs a GPU or the reference:

  - the oracle reproduces the reference's stored float64 outputs of one case;
  - its basis is orthonormal on the sphere, by a quadrature that is exact
    for the products (no table of constants involved);
  - its autograd v_dirs equals central differences on the fixed directions;
  - run in float32 it stays inside the bound the GPU tests use, on every case
    and output, so plain float32 arithmetic can meet that bound;
  - the builder's conditions: gates, distances, fixed directions, masks.
"""

import os

import numpy as np
import pytest
import torch

import sh_cases as SC
from conftest import GOLDEN

NPZ = os.path.join(GOLDEN, "sh_matrix.npz")


@pytest.fixture(scope="module")
def bars():
    return SC.load_bars(NPZ)


def test_every_case_and_output_has_a_bar(bars):
    want = {f"{n}:{k}" for n in SC.ALL_NAMES for k in SC.OUTPUTS[SC.build(n).kind]}
    assert set(bars) == want
    assert all(0.0 <= b < 1e-5 for b in bars.values()), max(bars.values())


def test_oracle_reproduces_the_reference_float64_sample():
    z = np.load(NPZ)
    got = SC.oracle64(SC.SAMPLE)
    assert SC.build(SC.SAMPLE).deg == 4 and SC.build(SC.SAMPLE).N == 65
    for k in SC.OUTPUTS["nf"]:
        e = SC.rel_err(got[k], z["sample_" + k])
        print(f"{SC.SAMPLE}: {k}: oracle vs reference float64 {e:.2e}")
        assert e <= 1e-12, (k, e)


def test_basis_is_orthonormal_on_the_sphere():
    """Gauss-Legendre in z (8 nodes: exact to degree 15) x 16 uniform angles
    (exact for trigonometric degree 15): exact for products of two degree-4
    harmonics."""
    zs, wz = np.polynomial.legendre.leggauss(8)
    phi = 2 * np.pi * np.arange(16) / 16
    z, p = np.meshgrid(zs, phi, indexing="ij")
    s = np.sqrt(1 - z * z)
    d = torch.from_numpy(np.stack([s * np.cos(p), s * np.sin(p), z], -1))
    w = torch.from_numpy(np.broadcast_to(wz[:, None] * (2 * np.pi / 16), z.shape).copy())
    Y = SC.basis(d, 4)
    gram = torch.einsum("zp,zpi,zpj->ij", w, Y, Y).numpy()
    assert gram.shape == (25, 25)
    assert np.abs(gram - np.eye(25)).max() <= 1e-12, np.abs(gram - np.eye(25)).max()
    for deg in range(4):  # lower degrees are the leading functions
        assert torch.equal(SC.basis(d, deg), Y[..., :(deg + 1) ** 2])


def test_basis_values_at_the_pole_and_on_the_axes():
    """Y_l^0(pole) = sqrt((2l+1)/(4 pi)), every m != 0 vanishes there; the sign
    convention (-1)^|m| puts -y, z, -x at l = 1."""
    Y = SC.basis(torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64), 4)[0].numpy()
    k = 0
    for l in range(5):
        for m in range(-l, l + 1):
            want = np.sqrt((2 * l + 1) / (4 * np.pi)) if m == 0 else 0.0
            assert abs(Y[k] - want) <= 1e-15, (l, m, Y[k])
            k += 1
    d = torch.tensor([[0.3, -0.5, 0.2]], dtype=torch.float64)
    c1 = np.sqrt(3 / (4 * np.pi))
    np.testing.assert_allclose(SC.basis(d, 1)[0, 1:].numpy(), c1 * np.array([0.5, 0.2, -0.3]),
                               rtol=1e-15)


def test_autograd_v_dirs_equals_central_differences():
    """Fourth-order central differences (h = 1e-3: truncation h^4 f^(5) / 30
    and rounding 1e-16 / h both below 1e-9) on the fixed directions, poles
    included, at degree 4 with lengths 1, 0.5 and 3."""
    g = torch.Generator().manual_seed(5)
    fixed = torch.from_numpy(SC.fixed_dirs())
    dirs = torch.cat([fixed, 0.5 * fixed, 3.0 * fixed])
    n = dirs.shape[0]
    coeffs = torch.randn(n, 25, 3, generator=g, dtype=torch.float64) * 0.3
    v_col = torch.randn(n, 3, generator=g, dtype=torch.float64)

    def f(d):
        return (SC.sh_eval(4, d, coeffs) * v_col).sum(-1)  # per row

    d = dirs.clone().requires_grad_(True)
    (auto,) = torch.autograd.grad(f(d).sum(), d)
    h = 1e-3
    fd = torch.zeros_like(dirs)
    for a in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[a] = h
        fd[:, a] = (-f(dirs + 2 * e) + 8 * f(dirs + e) - 8 * f(dirs - e) + f(dirs - 2 * e)) / (12 * h)
    err = SC.rel_err(auto.numpy(), fd.numpy())
    print(f"autograd vs central differences: {err:.2e}")
    assert float(auto.abs().max()) > 0.1
    assert err <= 1e-7, err


@pytest.mark.parametrize("kind", ["nf", "fz", "adam"])
def test_float32_oracle_is_inside_the_gpu_bound(kind, bars):
    names = {"nf": SC.NF_NAMES, "fz": SC.FZ_NAMES, "adam": SC.ADAM_NAMES}[kind]
    bad, worst = [], 0.0
    for name in names:
        case, ref = SC.build(name), SC.oracle64(name)
        got = SC.oracle(case, torch.float32)
        for k in SC.OUTPUTS[kind]:
            assert np.isfinite(ref[k]).all() and np.isfinite(got[k]).all(), (name, k)
            e, b = SC.rel_err(got[k], ref[k]), SC.bound(bars[f"{name}:{k}"])
            worst = max(worst, e / b)
            if not e <= b:
                bad.append((name, k, e, b))
    print(f"{kind}: largest float32-oracle error / bound {worst:.3f}")
    assert not bad, bad


@pytest.mark.parametrize("name", SC.FZ_NAMES + SC.ADAM_NAMES)
def test_fused_case_conditions(name):
    c = SC.build(name)
    assert c.means.dtype == np.float32 and c.viewmats.dtype == np.float32
    assert c.radii.dtype == np.int32 and c.radii.shape == (c.C, c.N)
    assert c.coeffs.shape == ((c.C, c.N, c.K, 3) if c.percam else (c.N, c.K, 3))
    assert np.abs(c.coeffs).min() > 0  # also above the active degree
    r = SC.fused_distance_ratio(c)
    assert 0.25 <= r.min() and r.max() <= 4.0, (r.min(), r.max())
    R = c.viewmats[:, :3, :3].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
    nearest, share = SC.gate_stats(c)
    assert nearest >= SC.GATE_MARGIN, nearest
    on = c.radii > 0
    if on.sum() >= 8:  # a share needs rows: N = 1 has one
        assert 0.2 <= share <= 0.8, share
    if c.mask == "dead":
        assert not on[:, 64:128].any() and on[:, :64].all() and on[:, 128:].all()
    elif c.mask == "rand":
        assert 0.15 < 1 - on.mean() < 0.45
    else:
        assert on.all()
    if c.kind == "fz":  # the fixed directions, as far as the float32 means allow
        assert c.nfix == min(SC.NFIX, c.N)
        ctr = SC.camera_centres(c.viewmats)[0].numpy()
        d = c.means[:c.nfix].astype(np.float64) - ctr
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        assert np.abs(d - SC.fixed_dirs()[:c.nfix]).max() < 1e-6


@pytest.mark.parametrize("name", SC.NF_NAMES)
def test_unfused_case_conditions(name):
    c = SC.build(name)
    lead = (c.N,) if c.C == 1 else (c.C, c.N)
    assert c.dirs.dtype == np.float32 and c.dirs.shape == lead + (3,)
    assert c.coeffs.shape == (c.N, c.K, 3) and np.abs(c.coeffs).min() > 0
    nfix = min(SC.NFIX, c.N)
    flat = c.dirs.reshape(-1, 3)
    assert np.array_equal(flat[:nfix], SC.fixed_dirs()[:nfix].astype(np.float32))
    norm = np.linalg.norm(flat[nfix:].astype(np.float64), axis=-1)
    if norm.size:
        assert 1e-3 * (1 - 1e-6) <= norm.min() and norm.max() <= 1e3 * (1 + 1e-6)
    if norm.size > 200:  # the six decades are used
        assert norm.min() < 1e-2 and norm.max() > 1e2
    if c.mask == "on":
        assert c.masks is None
    else:
        assert c.masks.dtype == np.bool_ and c.masks.shape == lead
        assert c.masks.reshape(-1)[:nfix].all()
        if c.mask == "dead":
            assert not c.masks[64:128].any() and c.masks[:64].all() and c.masks[128:].all()
        else:
            assert 0.15 < 1 - c.masks.mean() < 0.45


def test_cases_are_deterministic():
    for name in (SC.NF_NAMES[3], SC.FZ_NAMES[4], SC.ADAM_NAMES[2]):
        a = SC.build(name)
        b = SC.build.__wrapped__(name)
        for k, v in vars(a).items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, getattr(b, k)), (name, k)
