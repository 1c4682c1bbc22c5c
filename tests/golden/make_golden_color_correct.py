"""Golden vectors for gsplat_hip.color_correct from the REFERENCE's own
`color_correct` (examples/lib_bilagrid.py:56-126).  Run in the build container
only:

    python tests/golden/make_golden_color_correct.py

The module imports `tensorly`, which `color_correct` does not use; an empty
stand-in (one no-op `set_backend`) is placed in sys.modules for the import.

The scenes are tests/color_correct_cases.py's, float32 cast up, so the kernels
under test read exactly the numbers the float64 run read.  Stored in
color_correct.npz (arrays only, below 1 MB):
    img_<case>, ref_<case>   the inputs of the small cases (float32)
    out_<case>               the reference's float64 output on them
    bar_<case>               max |reference float32 - reference float64| for
                             every non-singular case: the reference's own
                             float32 error, which the GPU tests scale their
                             bounds from
"""

import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))

import color_correct_cases as CC  # noqa: E402


def _reference():
    tl = types.ModuleType("tensorly")
    tl.set_backend = lambda *a, **k: None
    sys.modules.setdefault("tensorly", tl)
    spec = importlib.util.spec_from_file_location(
        "lib_bilagrid", os.path.join(REF, "examples", "lib_bilagrid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.color_correct


def main():
    color_correct = _reference()
    arrs = {}
    for name in CC.REGULAR:
        img, ref, share = CC.build(name)
        o64 = color_correct(torch.from_numpy(img.copy()).double(),
                            torch.from_numpy(ref.copy()).double(),
                            num_iters=CC.NUM_ITERS, eps=CC.EPS).numpy()
        o32 = color_correct(torch.from_numpy(img.copy()), torch.from_numpy(ref.copy()),
                            num_iters=CC.NUM_ITERS, eps=CC.EPS).numpy()
        bar = float(np.abs(o32.astype(np.float64) - o64).max())
        arrs["bar_" + name] = np.float64(bar)
        mine = CC.oracle(img, ref)[0]
        print(f"{name}: redrawn {100 * share:.2f} %  bar {bar:.2e}  "
              f"|oracle - reference| {np.abs(mine - o64).max():.2e}")
        if name in CC.GOLDEN_OUT:
            arrs["img_" + name], arrs["ref_" + name], arrs["out_" + name] = img, ref, o64
    path = os.path.join(OUT, "color_correct.npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print(f"color_correct.npz: {size} bytes")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
