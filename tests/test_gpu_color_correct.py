"""gsplat_hip.color_correct (csrc/color_correct.hip) against the float64 oracle
of tests/color_correct_cases.py on every case, and Trainer.evaluate's
`color_correct=True`.

Bounds: max |kernel - oracle| <= max(FACTOR x bar, FLOOR), bar = the
reference's own float32 error on the case (tests/golden/color_correct.npz);
the kernel sums, solves and warps in float64 and rounds the iterate to float32
once per iteration, so it sits well inside (the oracle with that rounding:
<= 1.2e-7 from the float64 run on the CPU)."""

import os

import numpy as np
import pytest
import torch

from conftest import load_golden

import color_correct_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return load_golden("color_correct")


def _run(name, **kw):
    import gsplat_hip
    img, ref, _ = CC.build(name)
    out, info = gsplat_hip.color_correct(torch.from_numpy(img.copy()).to(DEV),
                                         torch.from_numpy(ref.copy()).to(DEV),
                                         return_info=True, **kw)
    torch.cuda.synchronize()
    return img, out, info["fallbacks"]


@pytest.mark.parametrize("name", CC.REGULAR)
def test_kernel_matches_oracle(golden, name):
    img, out, fb = _run(name)
    want, want_fb = CC.expected(name)
    assert out.dtype == torch.float32 and tuple(out.shape) == img.shape
    assert fb.dtype == torch.int32 and tuple(fb.shape) == (CC.NUM_ITERS, 3)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max())
    bound = CC.bound(float(golden["bar_" + name]))
    print(f"{name}: max |kernel - oracle| = {err:.2e}  bound {bound:.2e}")
    assert np.array_equal(fb.cpu().numpy(), want_fb)
    assert err <= bound


@pytest.mark.parametrize("name", CC.SINGULAR)
def test_singular_cases_keep_the_input_bits(name):
    img, out, fb = _run(name)
    want, want_fb = CC.expected(name)
    assert np.array_equal(fb.cpu().numpy(), want_fb) and want_fb.all()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), img.view(np.uint32))
    assert float(np.abs(out.cpu().numpy() - want).max()) <= CC.FLOOR


@pytest.mark.parametrize("name", ["affine_37x53", "clipped_131x257"])
def test_num_iters(golden, name):
    import gsplat_hip
    img, ref, _ = CC.build(name)
    bound = CC.bound(float(golden["bar_" + name]))
    for n in (0, 1, 5):
        _, out, fb = _run(name, num_iters=n)
        want, want_fb = CC.oracle(img, ref, num_iters=n)
        assert tuple(fb.shape) == (n, 3) and np.array_equal(fb.cpu().numpy(), want_fb)
        err = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max())
        print(f"{name} num_iters={n}: max |kernel - oracle| = {err:.2e}  bound {bound:.2e}")
        assert err <= bound
        if n == 0:
            assert np.array_equal(out.cpu().numpy(), img)
    x = torch.from_numpy(img.copy()).to(DEV)
    out0 = gsplat_hip.color_correct(x, torch.from_numpy(ref.copy()).to(DEV), num_iters=0)
    assert out0.data_ptr() != x.data_ptr()  # a copy


@pytest.mark.parametrize("name", ["affine_131x257", "clipped_37x53", "constchan_37x53"])
def test_two_runs_are_bit_equal(name):
    _, a, fa = _run(name)
    _, b, fb = _run(name)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(fa, fb)


def test_other_layouts_and_dtypes_give_the_same_result():
    import gsplat_hip
    img, ref, _ = CC.build("gamma_37x53")
    x, r = torch.from_numpy(img.copy()).to(DEV), torch.from_numpy(ref.copy()).to(DEV)
    want = gsplat_hip.color_correct(x, r)
    # channel-first storage viewed as [H,W,3], and a view with an odd offset
    x_nc = x.permute(2, 0, 1).contiguous().permute(1, 2, 0)
    r_nc = r.permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert not x_nc.is_contiguous()
    assert torch.equal(gsplat_hip.color_correct(x_nc, r_nc), want)
    pad = torch.zeros(x.numel() + 1, device=DEV)
    pad[1:] = x.reshape(-1)
    x_off = pad[1:].view(x.shape)
    assert x_off.data_ptr() % 16 != 0
    assert torch.equal(gsplat_hip.color_correct(x_off, r), want)
    # float64 inputs are rounded to float32 (here: exactly)
    got = gsplat_hip.color_correct(x.double(), r.double())
    assert got.dtype == torch.float32 and torch.equal(got, want)
    # no autograd
    xg = x.clone().requires_grad_(True)
    assert not gsplat_hip.color_correct(xg, r).requires_grad


def _trainer_scene(n_cams=3, W=64, H=64, stride=56):
    """The garden crop's every 56th point at 64 x 64: ~2,000 Gaussians."""
    from gsplat_hip.train_step import camera_pool, load_garden_scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    means, rgbs, vms, Ks, sw, sh_ = load_garden_scene(
        os.path.join(root, "tests", "golden", "garden_scene.npz"), scene_grid=1)
    means, rgbs = means[::stride].contiguous(), rgbs[::stride].contiguous()
    vm, K = camera_pool(vms, Ks, sw, sh_, W, H, n=n_cams)
    return means, rgbs, vm.float(), K.float(), W, H


def test_trainer_evaluate_color_correct():
    """Targets that are an affine map of the trainer's own clamped renders: the
    map is inside the fit's span and nothing clips, so the corrected render is
    the target up to float32 rounding."""
    import gsplat_hip
    from gsplat_hip.losses import ssim_and_l1
    from gsplat_hip.train_step import Trainer
    means, rgbs, vm, K, W, H = _trainer_scene()
    tr = Trainer(means, rgbs, vm, K, W, H, device=DEV, max_steps=100)
    with torch.no_grad():
        renders = torch.cat([torch.clamp(tr.render(i, world_ci=[i])[0], 0.0, 1.0)
                             for i in range(len(vm))])
    assert float(renders.std()) > 0.05  # textured, not constant
    images = 0.7 * renders + 0.05
    plain = tr.evaluate(viewmats=vm, Ks=K, images=images)
    assert set(plain) == {"psnr", "ssim", "num_images"}
    res = tr.evaluate(viewmats=vm, Ks=K, images=images, color_correct=True)
    assert set(res) == {"psnr", "ssim", "num_images", "cc_psnr", "cc_ssim"}
    print(f"psnr {res['psnr']:.2f} dB  cc_psnr {res['cc_psnr']:.2f} dB  "
          f"ssim {res['ssim']:.4f}  cc_ssim {res['cc_ssim']:.4f}")
    # the default's keys and values are untouched by the keyword
    assert {k: res[k] for k in plain} == plain
    assert plain["num_images"] == len(vm)
    manual = {"psnr": [], "ssim": [], "cc_psnr": [], "cc_ssim": []}
    for i in range(len(vm)):
        c, gt = renders[i:i + 1], images[i:i + 1]
        cc = gsplat_hip.color_correct(c, gt)
        for key, a in (("", c), ("cc_", cc)):
            manual[key + "psnr"].append(float(-10.0 * torch.log10(torch.mean((a - gt) ** 2))))
            manual[key + "ssim"].append(float(ssim_and_l1(a, gt)[0]))
    for key, v in manual.items():
        assert res[key] == pytest.approx(sum(v) / len(v), rel=1e-6), key
    assert res["cc_psnr"] > 60.0
    assert res["cc_psnr"] > res["psnr"] + 20.0
