"""Golden vectors for appearance optimisation from the REFERENCE's own
`AppearanceOptModule` (examples/utils.py:51-114), run on the CPU in fp32,
followed by the trainer's `sigmoid(colors + splats["colors"])`
(examples/simple_trainer.py:389-410).  Run in the build container only:

    python tests/golden/make_golden_app.py

Harness-only shims (nothing under /root/reference is modified or copied): the
`gsplat` and `gsplat.cuda` package roots are stubs (their __init__ pull in the
CUDA extension); `gsplat.cuda._torch_impl` (for `_eval_sh_bases_fast`) and
`examples/utils.py` are the reference's.  Only arrays are committed.

Contents of app_opt.npz: the inputs (N = 200 Gaussians, 5 images, 2 cameras,
head weights with a non-zero last layer, a random v_colors), the colours of
every (C, degree) in {1, 2} x {0..3} and of `embed_ids=None`, and every
gradient for two cases: `c2d3` (C = 2, degree 3, embeddings) and `c1d1none`
(C = 1, degree 1, embed_ids=None).
"""

import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
N, N_IMG = 200, 5
HEAD = ("W1", "b1", "W2", "b2", "W3", "b3")


def _import_reference():
    for name, sub in (("gsplat", "gsplat"), ("gsplat.cuda", "gsplat/cuda")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, sub)]
        sys.modules[name] = pkg
    sys.path.insert(0, os.path.join(REF, "examples"))
    from utils import AppearanceOptModule
    return AppearanceOptModule


def main():
    Module = _import_reference()
    torch.manual_seed(20)
    mod = Module(N_IMG, feature_dim=32, embed_dim=16, sh_degree=3)
    with torch.no_grad():  # the trainer zeroes the last layer; the fixture must not
        mod.color_head[4].weight.normal_(0.0, 0.2)
        mod.color_head[4].bias.normal_(0.0, 0.2)
    g = torch.Generator().manual_seed(21)
    features = torch.rand(N, 32, generator=g)
    base_colors = torch.logit(torch.rand(N, 3, generator=g).clamp(0.01, 0.99))
    means = torch.randn(N, 3, generator=g)
    campos = torch.randn(2, 3, generator=g) * 3.0
    ids = torch.tensor([3, 1])
    v_colors = torch.randn(2, N, 3, generator=g)
    out = {
        "features": features, "base_colors": base_colors, "means": means, "campos": campos,
        "embed_ids": ids, "v_colors": v_colors, "embeds_table": mod.embeds.weight.detach(),
    }
    layers = (mod.color_head[0], mod.color_head[2], mod.color_head[4])
    for k, t in zip(HEAD, [p for lin in layers for p in (lin.weight, lin.bias)]):
        out[k] = t.detach()

    def run(C, deg, use_ids, grads_as=None):
        leaves = [features, base_colors, means]
        for t in leaves:
            t.grad = None
            t.requires_grad_(True)
        mod.zero_grad()
        dirs = means[None, :, :] - campos[:C, None, :]
        colors = mod(features, ids[:C] if use_ids else None, dirs, deg)
        colors = torch.sigmoid(colors + base_colors)
        tag = f"c{C}d{deg}" + ("" if use_ids else "none")
        out[f"colors_{tag}"] = colors.detach()
        if grads_as:
            colors.backward(v_colors[:C])
            out[f"{tag}_v_features"] = features.grad.clone()
            out[f"{tag}_v_base_colors"] = base_colors.grad.clone()
            out[f"{tag}_v_means"] = means.grad.clone()
            if use_ids:  # dense [n_img, 16]: rows of the other images are 0
                out[f"{tag}_v_embeds_table"] = mod.embeds.weight.grad.clone()
            for k, t in zip(HEAD, [p for lin in layers for p in (lin.weight, lin.bias)]):
                out[f"{tag}_v_{k}"] = t.grad.clone()

    for C in (1, 2):
        for deg in range(4):
            run(C, deg, True, grads_as=(C, deg) == (2, 3))
    run(2, 3, False)
    run(1, 1, False, grads_as=True)
    arrays = {k: (v.numpy().astype(np.int64) if v.dtype == torch.int64
                  else v.detach().numpy().astype(np.float32)) for k, v in out.items()}
    path = os.path.join(OUT, "app_opt.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes;", len(arrays), "arrays")


if __name__ == "__main__":
    main()
