"""Golden PLY files from the REFERENCE's own `save_ply` (gsplat/utils.py:10-98)
run on seeded inputs.  Run in the build container only:

    python tests/golden/make_golden_ply.py

Each .npz holds the inputs and the bytes of the file the reference wrote, as
a uint8 array `ply`; only arrays are written, each file below 1 MB.

    ply_sh3.npz     N = 1000, K = 16.  Non-finite means at rows 0 (NaN), 255
                    (+Inf), 256 (-Inf) and 999 (NaN); rows 512-767 of shN all
                    Inf (a whole 256-row workgroup dropped); finite opacities.
                    740 rows written.
    ply_sh0.npz     N = 300, shN [N,0,3]
    ply_colors.npz  N = 300 with `colors` and no invalid row (only there is
                    the reference's colour path right: it indexes `colors`
                    unfiltered)

The reference's filter tests `opacities` with `.any(axis=0)`; with finite
opacities, as here, it is the per-row filter.
"""

import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def _utils():
    pkg = types.ModuleType("gsplat")
    pkg.__path__ = [os.path.join(REF, "gsplat")]
    sys.modules["gsplat"] = pkg
    from gsplat import utils
    return utils


def splats(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(means=torch.randn(N, 3, generator=g) * 2.0,
                scales=torch.log(torch.rand(N, 3, generator=g) * 0.05 + 1e-3),
                quats=torch.randn(N, 4, generator=g),
                opacities=torch.logit(torch.rand(N, generator=g).clamp(1e-3, 1 - 1e-3)),
                sh0=torch.randn(N, 1, 3, generator=g) * 0.5,
                shN=torch.randn(N, K - 1, 3, generator=g) * 0.05), g


def write(U, name, sp, colors=None):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ref.ply")
        with contextlib.redirect_stdout(io.StringIO()):
            U.save_ply(sp, path, colors)
        data = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
    arrs = {k: v.numpy() for k, v in sp.items()}
    if colors is not None:
        arrs["colors"] = colors.numpy()
    arrs["ply"] = data
    out = os.path.join(OUT, name + ".npz")
    np.savez_compressed(out, **arrs)
    size = os.path.getsize(out)
    print(f"{name}: {size} bytes, ply {data.size} bytes")
    assert size < 1_000_000, (name, size)
    return data


def main():
    U = _utils()
    sp, _ = splats(1000, 16, 101)
    sp["means"][0, 1] = float("nan")
    sp["means"][255, 0] = float("inf")
    sp["means"][256, 2] = float("-inf")
    sp["means"][999, 0] = float("nan")
    sp["shN"][512:768] = float("inf")
    data = write(U, "ply_sh3", sp)
    assert b"element vertex 740\n" in data.tobytes()[:200]

    sp, _ = splats(300, 1, 102)
    write(U, "ply_sh0", sp)

    sp, g = splats(300, 16, 103)
    write(U, "ply_colors", sp, torch.rand(300, 3, generator=g))


if __name__ == "__main__":
    main()
