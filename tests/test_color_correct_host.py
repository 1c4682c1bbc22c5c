"""CPU checks of the colour-corrected evaluation: this project's float64
oracle of `color_correct` (tests/color_correct_cases.py) against the
reference's float64 output (tests/golden/color_correct.npz), the gates of the
case builder, the singular rule, and the Python surface's argument handling."""

import inspect

import numpy as np
import pytest
import torch

from conftest import load_golden

import color_correct_cases as CC


@pytest.fixture(scope="module")
def golden():
    return load_golden("color_correct")


@pytest.mark.parametrize("name", CC.GOLDEN_OUT)
def test_oracle_matches_reference_float64(golden, name):
    """The normal equations in float64 against the reference's QR in float64
    on the stored inputs: <= 1e-10 (measured: 8e-14 .. 2.2e-13)."""
    img, ref = golden["img_" + name], golden["ref_" + name]
    out, fb = CC.oracle(img, ref)
    err = np.abs(out - golden["out_" + name]).max()
    print(f"{name}: max |oracle - reference| = {err:.2e}")
    assert err <= 1e-10
    assert not fb.any()
    # the builder still draws the scene the golden was made from
    b_img, b_ref, _ = CC.build(name)
    assert np.array_equal(b_img, img) and np.array_equal(b_ref, ref)


def test_golden_holds_a_bar_for_every_regular_case(golden):
    for name in CC.REGULAR:
        bar = float(golden["bar_" + name])
        assert 0.0 < bar < 1e-5, (name, bar)  # a float32 error, not a different fit
    assert not any(("bar_" + n) in golden for n in CC.SINGULAR)


def test_case_list_covers_the_shapes():
    shapes = {s for _, s, _ in CC.CASES.values()}
    assert {(24, 40), (37, 53), (64, 96), (131, 257), (421, 411), (2, 16, 24), (1,)} <= shapes
    kinds = {k for k, _, _ in CC.CASES.values()}
    assert kinds == {"affine", "gamma", "clipped", "constant", "constchan", "fewrows"}


@pytest.mark.parametrize("name", list(CC.CASES))
def test_gate_leaves_no_undecided_value(name):
    img, ref, share = CC.build(name)
    print(f"{name}: redrawn {100 * share:.2f} %")
    assert share <= CC.REDRAW_CAP
    assert CC.undecided_rows(img, ref).size == 0
    assert img.dtype == np.float32 and ref.dtype == np.float32
    assert img.shape == CC.CASES[name][1] + (3,) and ref.shape == img.shape
    assert img.min() >= 0.0 and img.max() <= 1.0 and ref.min() >= 0.0 and ref.max() <= 1.0


def test_clipped_scene_saturates_about_a_third():
    img, _, _ = CC.build("clipped_131x257")
    share = float((img >= 1.0).mean())
    print(f"saturated: {100 * share:.1f} %")
    assert 0.25 <= share <= 0.45


@pytest.mark.parametrize("name", list(CC.CASES))
def test_float32_iterate_takes_the_float64_decisions(name):
    """With the iterate rounded to float32 per iteration (the kernel's
    storage) every mask and every fallback is the float64 run's."""
    img, ref, _ = CC.build(name)
    o64, f64, i64 = CC.oracle(img, ref, info=True)
    o32, f32, i32 = CC.oracle(img, ref, round32=True, info=True)
    assert np.array_equal(f64, f32)
    for a, b in zip(i64["masks"], i32["masks"]):
        assert np.array_equal(a, b)
    err = np.abs(o64 - o32).max()
    print(f"{name}: max |float32 iterate - float64| = {err:.2e}")
    assert err <= CC.FLOOR


@pytest.mark.parametrize("name", CC.SINGULAR)
def test_singular_cases_keep_the_input(name):
    img, ref, _ = CC.build(name)
    for r32 in (False, True):
        out, fb = CC.oracle(img, ref, round32=r32)
        assert np.array_equal(fb, np.ones((CC.NUM_ITERS, 3), np.int32))
        assert np.array_equal(out.astype(np.float32), img)


def test_regular_cases_improve_and_do_not_fall_back():
    for name in CC.REGULAR:
        img, ref, _ = CC.build(name)
        out, fb = CC.expected(name)
        assert not fb.any(), name

        def psnr(a):
            return -10.0 * np.log10(np.mean((a.astype(np.float64) - ref) ** 2))
        assert psnr(out) > psnr(img) + 3.0, (name, psnr(img), psnr(out))


def test_num_iters_zero_is_the_input():
    img, ref, _ = CC.build("affine_24x40")
    out, fb = CC.oracle(img, ref, num_iters=0)
    assert np.array_equal(out.astype(np.float32), img) and fb.shape == (0, 3)


# ---------------------------------------------------------- Python surface --
def test_exported():
    import gsplat_hip
    assert "color_correct" in gsplat_hip.__all__
    assert callable(gsplat_hip.color_correct)
    sig = inspect.signature(gsplat_hip.color_correct)
    assert list(sig.parameters) == ["img", "ref", "num_iters", "eps", "return_info"]
    assert sig.parameters["num_iters"].default == 5
    assert sig.parameters["eps"].default == 0.5 / 255
    assert sig.parameters["return_info"].default is False


def test_argument_errors():
    import gsplat_hip
    with pytest.raises(ValueError, match="img's 3 and ref's 4 channels must match"):
        gsplat_hip.color_correct(torch.zeros(4, 4, 3), torch.zeros(4, 4, 4))
    with pytest.raises(ValueError):  # a last dimension other than 3
        gsplat_hip.color_correct(torch.zeros(4, 4, 1), torch.zeros(4, 4, 1))
    with pytest.raises(ValueError):  # shapes that differ
        gsplat_hip.color_correct(torch.zeros(4, 4, 3), torch.zeros(4, 5, 3))
    with pytest.raises(ValueError):
        gsplat_hip.color_correct(torch.zeros(4, 4, 3), torch.zeros(4, 4, 3), num_iters=-1)
    for eps in (0.0, 0.5, -1.0):
        with pytest.raises(ValueError):
            gsplat_hip.color_correct(torch.zeros(4, 4, 3), torch.zeros(4, 4, 3), eps=eps)


def test_cpu_tensors_are_refused():
    import gsplat_hip
    from gsplat_hip._lib import GsplatHipError
    with pytest.raises(GsplatHipError):
        gsplat_hip.color_correct(torch.rand(4, 4, 3), torch.rand(4, 4, 3))
    with pytest.raises(GsplatHipError):  # no CPU copy for num_iters = 0 either
        gsplat_hip.color_correct(torch.rand(4, 4, 3), torch.rand(4, 4, 3), num_iters=0)


def test_c_entry_points_refuse_bad_arguments():
    """The host-side checks run before any device work."""
    from gsplat_hip import _lib
    lib = _lib.load()
    assert lib.gsplat_hip_color_correct_workspace_bytes(0) == 0
    assert lib.gsplat_hip_color_correct_workspace_bytes(-5) == 0
    small, large = (lib.gsplat_hip_color_correct_workspace_bytes(p) for p in (1, 1 << 22))
    assert small == (3 * 65 + 30) * 8 and large > small and large % 8 == 0
    # the workspace is a function of P alone, capped
    assert lib.gsplat_hip_color_correct_workspace_bytes(1 << 30) == large
    a, b, c, w = 0x1000, 0x2000, 0x3000, 0x4000  # never dereferenced: every call fails first
    bad = [
        (0, a, b, 5, 0.5 / 255, c, w),     # P < 1
        (16, 0, b, 5, 0.5 / 255, c, w),    # null pointers
        (16, a, 0, 5, 0.5 / 255, c, w),
        (16, a, b, 5, 0.5 / 255, 0, w),
        (16, a, b, 5, 0.5 / 255, c, 0),
        (16, a, b, -1, 0.5 / 255, c, w),   # num_iters < 0
        (16, a, b, 5, 0.0, c, w),          # eps outside (0, 0.5)
        (16, a, b, 5, 0.5, c, w),
        (16, a, b, 5, 0.5 / 255, a, w),    # out aliases img
        (16, a, b, 5, 0.5 / 255, a + 16, w),
        (16, a + 4, b, 5, 0.5 / 255, c, w),  # misaligned
    ]
    for P, img, ref, n, eps, out, ws in bad:
        with pytest.raises(_lib.GsplatHipError, match="color_correct"):
            _lib.call("gsplat_hip_color_correct", P, img, ref, n, eps, out, ws, 0, 0)


def test_evaluate_signature():
    from gsplat_hip.train_step import Trainer
    for fn in (Trainer.evaluate, Trainer.evaluate_compressed):
        p = inspect.signature(fn).parameters
        assert "color_correct" in p and p["color_correct"].default is False


def test_abi_version_unchanged():
    from gsplat_hip import _lib
    assert _lib.ABI_VERSION == 38
    assert _lib.load().gsplat_hip_abi_version() == 38
