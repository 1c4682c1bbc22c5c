"""Scenes and the float64 oracle for gsplat_hip.color_correct (the reference's
examples/lib_bilagrid.py:56-126), shared by tests/test_color_correct_host.py,
tests/test_gpu_color_correct.py and tests/golden/make_golden_color_correct.py.

The definition (img, ref [..., 3] float32 in [0, 1], flattened to P rows):
lo = float32(eps), hi = float32(1 - eps), unclipped(z) = lo <= z <= hi;
m0 = unclipped(img); x = img; num_iters times: a(x) = [x0x0, x0x1, x0x2, x1x1,
x1x2, x2x2, x0, x1, x2, 1]; per channel c the rows with m0[:, c],
unclipped(x[:, c]) and unclipped(ref[:, c]) give G = sum a a^T, h = sum a
ref_c and w_c = G^-1 h; x = clip(a(x) [w_0 w_1 w_2], 0, 1) for every row.
A channel is singular when fewer than 10 rows are left, a diagonal entry of G
is not positive, or the Cholesky factorisation of D^-1/2 G D^-1/2 (D = diag G)
meets a pivot below 1e-10; it then keeps its values for that iteration (w_c =
the unit vector of linear term c) and fallbacks[it, c] = 1.

`oracle(img, ref)` evaluates this in float64 throughout (what the reference's
float64 run computes: tests/golden/color_correct.npz); with `round32=True` the
iterate is rounded to float32 once per iteration, the kernel's storage.

Gates: every value compared with lo or hi is a discrete decision -- the input,
the reference and each iteration's iterate.  `build(name)` redraws any pixel
that holds such a value within GATE_MARGIN of a threshold in the float64 run,
and runs again until none is left; the share of redrawn pixels is capped at
REDRAW_CAP.  A float32 evaluation then takes the decisions of the float64 one,
and errors are bounded by max(FACTOR x bar, FLOOR) as in tests/proj_cases.py,
bar = the reference's own float32 error on the case (stored in the golden).
"""

import functools

import numpy as np

FACTOR = 4.0
FLOOR = 1e-6
GATE_MARGIN = 1e-5
REDRAW_CAP = 0.01
EPS = 0.5 / 255
NUM_ITERS = 5
PIVOT_MIN = 1e-10

# name -> (kind, shape of img without the channel dimension, seed)
CASES = {
    "affine_24x40": ("affine", (24, 40), 1),       # below one workgroup per channel-block
    "affine_37x53": ("affine", (37, 53), 2),       # odd P: a ragged last pixel group
    "affine_64x96": ("affine", (64, 96), 3),
    "affine_131x257": ("affine", (131, 257), 4),   # several workgroups: two-stage reduction
    "affine_2x16x24": ("affine", (2, 16, 24), 5),  # leading dimensions fitted jointly
    "gamma_24x40": ("gamma", (24, 40), 6),
    "gamma_37x53": ("gamma", (37, 53), 7),
    "gamma_64x96": ("gamma", (64, 96), 8),
    # more pixel groups than the accumulate pass has lanes (168 workgroups x 256
    # lanes x 4 pixels = 172,032): some lanes take a second group
    "gamma_421x411": ("gamma", (421, 411), 16),
    "clipped_24x40": ("clipped", (24, 40), 9),
    "clipped_37x53": ("clipped", (37, 53), 10),
    "clipped_131x257": ("clipped", (131, 257), 11),
    "constant_24x40": ("constant", (24, 40), 12),
    "constchan_37x53": ("constchan", (37, 53), 13),
    "fewrows_24x40": ("fewrows", (24, 40), 14),
    "single_pixel": ("affine", (1,), 15),          # P = 1: fewer than 10 rows
}
SINGULAR = ("constant_24x40", "constchan_37x53", "fewrows_24x40", "single_pixel")
REGULAR = tuple(n for n in CASES if n not in SINGULAR)
# the cases whose reference float64 output is stored in the golden
GOLDEN_OUT = tuple(n for n in REGULAR if n.endswith(("24x40", "37x53")))


def thresholds(eps=EPS):
    return np.float32(eps), np.float32(1.0 - eps)


def features(x):
    x0, x1, x2 = x[:, 0], x[:, 1], x[:, 2]
    return np.stack([x0 * x0, x0 * x1, x0 * x2, x1 * x1, x1 * x2, x2 * x2, x0, x1, x2,
                     np.ones_like(x0)], axis=1)


def solve_channel(G, h, rows):
    """w of G w = h by the scaled Cholesky factorisation, or None (singular)."""
    n = G.shape[0]
    d = np.diag(G)
    if rows < n or not np.all(d > 0.0):
        return None
    s = 1.0 / np.sqrt(d)
    Gs = G * s[:, None] * s[None, :]
    L = np.zeros_like(Gs)
    for j in range(n):
        p = Gs[j, j] - np.dot(L[j, :j], L[j, :j])
        if not p >= PIVOT_MIN:
            return None
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, n):
            L[i, j] = (Gs[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    y = np.zeros(n)
    hs = h * s
    for i in range(n):
        y[i] = (hs[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    z = np.zeros(n)
    for i in range(n - 1, -1, -1):
        z[i] = (y[i] - np.dot(L[i + 1:, i], z[i + 1:])) / L[i, i]
    return z * s


def oracle(img, ref, num_iters=NUM_ITERS, eps=EPS, round32=False, info=False):
    """The corrected image (float64, img's shape) and fallbacks int32
    [num_iters, 3]; with info=True also {"masks": [num_iters] of bool [P,3],
    "compared": the float64 values that met a threshold, [2 + num_iters, P, 3]
    (img, ref, then the iterate each iteration starts from)}."""
    lo, hi = (np.float64(t) for t in thresholds(eps))
    shape = img.shape
    x = np.asarray(img, np.float32).reshape(-1, 3).astype(np.float64)
    r = np.asarray(ref, np.float32).reshape(-1, 3).astype(np.float64)

    def unclipped(z):
        return (z >= lo) & (z <= hi)

    m0 = unclipped(x)
    mr = unclipped(r)
    fallbacks = np.zeros((num_iters, 3), np.int32)
    masks, compared = [], [x.copy(), r.copy()]
    for it in range(num_iters):
        compared.append(x.copy())
        a = features(x)
        m = m0 & unclipped(x) & mr
        masks.append(m)
        W = np.zeros((10, 3))
        for c in range(3):
            am = a[m[:, c]]
            w = solve_channel(am.T @ am, am.T @ r[m[:, c], c], am.shape[0])
            if w is None:
                fallbacks[it, c] = 1
                w = np.zeros(10)
                w[6 + c] = 1.0
            W[:, c] = w
        x = np.clip(a @ W, 0.0, 1.0)
        if round32:
            x = x.astype(np.float32).astype(np.float64)
    out = x.reshape(shape)
    if info:
        return out, fallbacks, {"masks": masks, "compared": np.stack(compared)}
    return out, fallbacks


# ------------------------------------------------------------------ scenes --
def _texture(rng, shape):
    """A smooth textured reference in about [0.08, 0.92] plus noise, [P,3]."""
    P = int(np.prod(shape))
    t = np.arange(P, dtype=np.float64) / max(P, 2)
    u = (np.arange(P) % shape[-1]) / float(shape[-1])
    ph = rng.uniform(0.0, 2.0 * np.pi, (3, 3))
    fr = rng.uniform(1.0, 4.0, (3, 3))
    tex = np.stack([0.5 + 0.2 * np.sin(2 * np.pi * fr[c, 0] * t + ph[c, 0])
                    + 0.14 * np.sin(2 * np.pi * fr[c, 1] * u + ph[c, 1])
                    + 0.06 * np.sin(2 * np.pi * 3 * fr[c, 2] * (t + u) + ph[c, 2])
                    for c in range(3)], axis=1)
    return tex + rng.normal(0.0, 0.02, (P, 3))


def _draw_ref(rng, n):
    return rng.uniform(0.08, 0.92, (n, 3))


def _make_img(kind, rng, ref, par):
    """The image of `ref` rows under the scene's colour map, before clipping."""
    n = ref.shape[0]
    noise = rng.normal(0.0, 0.01, (n, 3))
    if kind == "affine":
        return ref @ par["M"] + par["b"] + noise
    if kind == "gamma":
        return par["gain"] * np.clip(ref, 1e-3, 1.0) ** par["gamma"] + noise
    if kind == "clipped":  # about a third of the values saturate at 1
        return par["gain"] * ref + noise
    if kind == "constant":
        return np.full((n, 3), 0.5)
    if kind == "constchan":
        out = 0.8 * ref + 0.1 + noise
        out[:, 0] = 0.4
        return out
    if kind == "fewrows":  # every row saturated; build() opens 6 of them
        return (rng.uniform(size=(n, 3)) < 0.5).astype(np.float64)
    raise KeyError(kind)


def _params(kind, rng):
    if kind == "affine":
        return {"M": np.eye(3) * 0.7 + rng.uniform(-0.08, 0.08, (3, 3)),
                "b": rng.uniform(0.02, 0.1, 3)}
    if kind == "gamma":
        return {"gain": rng.uniform(0.8, 0.95, 3), "gamma": rng.uniform(1.4, 2.0, 3)}
    if kind == "clipped":
        return {"gain": rng.uniform(1.65, 1.8, 3)}
    return {}


def _f32(a):
    return np.clip(a, 0.0, 1.0).astype(np.float32)


def undecided_rows(img, ref, num_iters=NUM_ITERS, eps=EPS):
    """Rows holding a compared value within GATE_MARGIN of a threshold in the
    float64 run."""
    lo, hi = (np.float64(t) for t in thresholds(eps))
    _, _, inf = oracle(img, ref, num_iters, eps, info=True)
    v = inf["compared"]
    near = (np.abs(v - lo) < GATE_MARGIN) | (np.abs(v - hi) < GATE_MARGIN)
    return np.nonzero(near.any(axis=(0, 2)))[0]


@functools.lru_cache(maxsize=None)
def build(name):
    """(img, ref, share): float32 arrays of the case's shape + (3,), read-only,
    and the share of pixels the gate redrew."""
    kind, shape, seed = CASES[name]
    rng = np.random.RandomState(seed)
    P = int(np.prod(shape))
    par = _params(kind, rng)
    ref = _texture(rng, shape)
    img = _make_img(kind, rng, ref, par)
    if kind == "fewrows":
        rows = rng.choice(P, 6, replace=False)
        img[rows] = rng.uniform(0.2, 0.8, (6, 3))
    img, ref = _f32(img), _f32(ref)
    redrawn = set()
    for _ in range(100):
        rows = undecided_rows(img.reshape(shape + (3,)), ref.reshape(shape + (3,)))
        if rows.size == 0:
            break
        redrawn.update(rows.tolist())
        new_ref = _draw_ref(rng, rows.size)
        ref[rows] = _f32(new_ref)
        if kind != "fewrows":
            img[rows] = _f32(_make_img(kind, rng, new_ref, par))
    else:
        raise AssertionError(f"{name}: the gate did not settle")
    img, ref = img.reshape(shape + (3,)), ref.reshape(shape + (3,))
    img.setflags(write=False)
    ref.setflags(write=False)
    return img, ref, len(redrawn) / P


@functools.lru_cache(maxsize=None)
def expected(name):
    """The float64 oracle's (out, fallbacks) of the case, computed once."""
    img, ref, _ = build(name)
    out, fb = oracle(img, ref)
    out.setflags(write=False)
    fb.setflags(write=False)
    return out, fb


def bound(bar):
    return max(FACTOR * bar, FLOOR)
