"""A plain torch re-statement of appearance optimisation, runnable in fp32 and
fp64 on the CPU: the oracle of tests/test_app_host.py (against the fixture
recorded from the reference's own module) and of the GPU tests.

    x      = cat(embeds[c] (16), features[n] (32), sh_bases(normalize(means[n] - campos[c])) (16))
    colors = sigmoid(Linear(64,3)(ReLU(Linear(64,64)(ReLU(Linear(64,64)(x))))) + base_colors[n])
"""

import torch
import torch.nn.functional as F

EMBED_DIM, FEATURE_DIM, NUM_BASES = 16, 32, 16
HEAD_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")


def sh_bases(dirs, num_to_use):
    """[..., 16] real SH bases of unit `dirs` up to degree 3; those from
    `num_to_use` on are zero."""
    x, y, z = dirs.unbind(-1)
    one = torch.ones_like(x)
    zz = z * z
    g2, h2 = 2 * x * y, x * x - y * y
    g3, h3 = x * g2 + y * h2, x * h2 - y * g2
    c31 = -2.285228997322329 * zz + 0.4570457994644658
    B = [
        0.2820947917738781 * one,
        -0.48860251190292 * y,
        0.48860251190292 * z,
        -0.48860251190292 * x,
        0.5462742152960395 * g2,
        -1.092548430592079 * z * y,
        0.9461746957575601 * zz - 0.3153915652525201,
        -1.092548430592079 * z * x,
        0.5462742152960395 * h2,
        -0.5900435899266435 * g3,
        1.445305721320277 * z * g2,
        c31 * y,
        z * (1.865881662950577 * zz - 1.119528997770346),
        c31 * x,
        1.445305721320277 * z * h2,
        -0.5900435899266435 * h3,
    ]
    B = [b if k < num_to_use else torch.zeros_like(b) for k, b in enumerate(B)]
    return torch.stack(B, dim=-1)


def app_colors(features, base_colors, embeds, means, campos, head, sh_degree, masks=None):
    """colors [C, N, 3] in the dtype of `features`.  `embeds` [C, 16] or None
    (zeros); `head` = (W1, b1, W2, b2, W3, b3) in torch Linear layout; rows
    that `masks` [C, N] hides are 0 and get no gradient."""
    C, N = campos.shape[0], features.shape[0]
    W1, b1, W2, b2, W3, b3 = head
    if embeds is None:
        embeds = torch.zeros(C, EMBED_DIM, dtype=features.dtype)
    dirs = F.normalize(means[None, :, :] - campos[:, None, :], dim=-1)
    x = torch.cat([embeds[:, None, :].expand(-1, N, -1), features[None].expand(C, -1, -1),
                   sh_bases(dirs, (sh_degree + 1) ** 2)], dim=-1)
    h = torch.relu(F.linear(x, W1, b1))
    h = torch.relu(F.linear(h, W2, b2))
    colors = torch.sigmoid(F.linear(h, W3, b3) + base_colors[None])
    if masks is not None:
        colors = colors * masks[..., None].to(colors.dtype)
    return colors


GRAD_NAMES = ("features", "base_colors", "embeds", "means") + HEAD_NAMES


def run(inputs, v_colors, sh_degree, dtype, masks=None, use_embeds=True):
    """Forward and every gradient in `dtype` from a dict of fp32 tensors
    (features, base_colors, embeds [C,16], means, campos, W1..b3).  Returns
    (colors, {name: grad}); the embeds' gradient is absent without embeds."""
    t = {k: torch.as_tensor(v).detach().to(dtype).clone() for k, v in inputs.items()}
    names = [n for n in GRAD_NAMES if use_embeds or n != "embeds"]
    for n in names:
        t[n].requires_grad_(True)
    colors = app_colors(t["features"], t["base_colors"], t["embeds"] if use_embeds else None,
                        t["means"], t["campos"], [t[k] for k in HEAD_NAMES], sh_degree, masks)
    colors.backward(torch.as_tensor(v_colors).to(dtype))
    # an input the colours do not depend on (the means at degree 0) has grad None
    return colors.detach(), {n: t[n].grad if t[n].grad is not None else torch.zeros_like(t[n])
                             for n in names}
