"""Float64 oracle, rounding bounds and seeded cases for the multi-tensor Adam
(csrc/adam.hip, adam_update in csrc/common.h).  Host only: numpy and torch on
the CPU, no GPU import, nothing from gsplat_hip.losses.

Oracle.  One step of torch.optim.Adam (amsgrad=False, no weight decay, the
lerp form of the first moment) in float64 from the float32 state (p, m, v)
and the float32 g, aux, lr, beta1, beta2, eps, all promoted:

    g'  = g | g + aux | g aux | g (1 - aux) aux            (the gradient mode)
    m'  = m + (1 - beta1) (g' - m)
    v'  = beta2 v + (1 - beta2) g'^2
    upd = lr / (1 - beta1^t) * m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)
    p'  = p - upd

The tests step the kernel and compare each step with the oracle's step *from
the state the kernel had before it*, so the bounds are those of one step.

Bounds.  adam_update is

    m = fma(1 - b1, g - m, m)            v = fma(b2, v, ((1 - b2) g) g)
    den = fma(sqrtf(v), ib, eps)         p = p - (ss m) / den

every operation a correctly rounded float32 one (relative error <= u = 2^-24;
1 - b1 and 1 - b2 are exact for betas in [0.5, 1]) but sqrtf (<= 1 ulp = 2u),
and ss, ib are float32 roundings of the float64 factors (u each).  The
transformed gradient g' takes k roundings (k = 0, 1, 1, 3 for the four
modes), each on a product or on the exact sum, so it is right to k u |g'|.
A result below FLT_MIN is right to T = 2^-149 absolutely (gradual underflow;
gfx950 keeps float32 denormals).  With e = 1.01 u (second-order terms):

    |m' - m'64| <= e [(1 - b1) |g' - m| + |m'| + k (1 - b1) |g'|] + T        =: Bm
        -- the subtraction's and the fma's rounding and the gradient's error;
           each term is at most max(|m'|, |g'|, |m|), so Bm <= 4u max(..) + T.
    |v' - v'64| <= e (3 + 2k) v' + 3T                                         =: Bv
        -- two roundings on (1 - b2) g'^2 (plus 2k from g'), one on the sum,
           all terms non-negative so each is at most v'; <= 4u max(v', g^2)
           for the plain gradient.
    |sqrtf(v') - sqrt(v'64)| <= sqrt(v'64) [e (3 + 2k) / 2 + 2u] + sqrt(3T)
        -- sqrt(a + d) - sqrt(a) <= min(d / (2 sqrt a), sqrt d)
    |den - den64| <= ib [that] + e ib sqrt(v'64) + e den64                   =: Bd
        -- ib's own rounding and the fma's
    |upd - upd64| <= 1.01 |upd64| (3e + Bd / den64) + 1.01 (ss / den64) Bm + T   =: Bu
        -- ss's rounding, the product's, the quotient's, the denominator's
           error, and the first moment's error carried through ss / den.
           Bm is absolute: where g' and m cancel, m' is small and its error is
           not, so a bound of the form c u |upd64| alone cannot hold there.
    |p' - p'64| <= Bu + e |p'64| + T
        -- the final subtraction (half an ulp of p')

A float32 numpy restatement of adam_update (its fma emulated through float64:
the double rounding adds at most 2^-29 u, inside e) meets these on every
case: tests/test_adam_cases_host.py.
"""

import functools
import zlib
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
E = 1.01 * U
T = 2.0 ** -149
BETAS = (0.9, 0.999)
# the trainer's six learning rates: means, scales, quats, opacities, sh0, shN
LRS = (1.6e-4, 5e-3, 1e-3, 5e-2, 2.5e-3, 1.25e-4)
MODE_ROUNDINGS = (0, 1, 1, 3)
STARTS = (1, 1000, 30000)  # runs of RUN steps start at these step counts
RUN = 3
MAX_GROUPS = 8
BIG = 17_000_000  # one pass of the grid covers 16384 * 256 * 4 = 16,777,216 elements


def f32(x):
    return float(np.float32(x))


def xform(mode, g, aux):
    if mode == 0:
        return g
    if mode == 1:
        return g + aux
    if mode == 2:
        return g * aux
    return g * (1.0 - aux) * aux


def factors64(lr, betas, t):
    """lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t) in float64 from the float32 values."""
    b1, b2 = f32(betas[0]), f32(betas[1])
    return f32(lr) / (1.0 - b1 ** t), 1.0 / np.sqrt(1.0 - b2 ** t)


def oracle_step(p, m, v, g, aux, mode, lr, betas, eps, t):
    """One float64 step from float32 arrays; g None: zero.  Returns a
    namespace of p, m, v (the new state) and the bounds bp, bm, bv."""
    p, m, v = (np.asarray(a, np.float64) for a in (p, m, v))
    g = np.zeros_like(p) if g is None else np.asarray(g, np.float64)
    aux = None if aux is None else np.asarray(aux, np.float64)
    b1, b2, eps = f32(betas[0]), f32(betas[1]), f32(eps)
    ss, ib = factors64(lr, betas, t)
    k = MODE_ROUNDINGS[mode]
    gx = xform(mode, g, aux)
    m1 = m + (1.0 - b1) * (gx - m)
    v1 = b2 * v + (1.0 - b2) * gx * gx
    rv = np.sqrt(v1)
    den = rv * ib + eps
    upd = ss * m1 / den
    p1 = p - upd
    bm = E * ((1.0 - b1) * np.abs(gx - m) + np.abs(m1) + k * (1.0 - b1) * np.abs(gx)) + T
    bv = E * (3 + 2 * k) * v1 + 3 * T
    brv = rv * (E * (3 + 2 * k) / 2 + 2 * U) + np.sqrt(3 * T)
    bd = ib * brv + E * ib * rv + E * den
    bu = 1.01 * np.abs(upd) * (3 * E + bd / den) + 1.01 * (ss / den) * bm + T
    bp = bu + E * np.abs(p1) + T
    return SimpleNamespace(p=p1, m=m1, v=v1, bp=bp, bm=bm, bv=bv, upd=upd)


def step32(p, m, v, g, aux, mode, ss, ib, betas, eps):
    """adam_update restated in float32 numpy (the host check of the bounds):
    ss, ib the float32 factors the library computes.  Returns new (p, m, v)."""
    f = np.float32
    p, m, v = (np.asarray(a, f) for a in (p, m, v))
    g = np.zeros_like(p) if g is None else np.asarray(g, f)
    b1, b2, eps, ss, ib = f(betas[0]), f(betas[1]), f(eps), f(ss), f(ib)
    one = f(1.0)
    if mode == 1:
        g = g + aux
    elif mode == 2:
        g = g * aux
    elif mode == 3:
        g = (g * (one - aux)) * aux

    def fma(a, b, c):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64)
                + np.asarray(c, np.float64)).astype(f)

    with np.errstate(under="ignore"):
        m1 = fma(one - b1, g - m, m)
        v1 = fma(b2, v, ((one - b2) * g) * g)
        den = fma(np.sqrt(v1), ib, eps)
        p1 = p - (ss * m1) / den
    return p1, m1, v1


def factors32(lr, betas, t):
    """The float32 factors as gsplat_hip_adam_step forms them: float64 from
    the float32 lr and betas, rounded once."""
    ss, ib = factors64(lr, betas, t)
    return f32(ss), f32(ib)


# --------------------------------------------------------------------- cases
def _g(numel, lr=LRS[0], mode=0, mag=1.0, grad="randn"):
    """A group: grad "randn" (mag * randn), "none" (no gradient tensor) or
    "then_zero" (randn for the first run of steps, exactly 0 from then on)."""
    return SimpleNamespace(numel=numel, lr=lr, mode=mode, mag=mag, grad=grad)


MAGS = (1e-25, 1e-20, 1e-12, 1.0, 1e4)
CASES = {
    # around the 4-element slot, and the trainer's group widths; kMaxGroups at once
    "sizes8": dict(groups=[_g(n, LRS[i % 6]) for i, n in
                           enumerate((1, 3, 4, 5, 7, 8, 1001 * 3, 1001 * 4))]),
    "shN": dict(groups=[_g(1001 * 45, LRS[5])]),
    "lrs": dict(groups=[_g(1003, lr) for lr in LRS]),
    "no_grad": dict(groups=[_g(1001 * 3, LRS[0]), _g(1001, LRS[3], grad="none"),
                            _g(7, LRS[2]), _g(5, LRS[1], grad="none")]),
    "then_zero": dict(groups=[_g(1001 * 3, LRS[4], grad="then_zero"), _g(6, LRS[0])],
                      starts=(1, 4)),
    "mags_eps1e-15": dict(groups=[_g(1001, LRS[i], mag=s) for i, s in enumerate(MAGS)]),
    "mags_eps1e-8": dict(groups=[_g(1001, LRS[i], mag=s) for i, s in enumerate(MAGS)], eps=1e-8),
    "modes": dict(groups=[_g(1001, LRS[0], 0), _g(1002, LRS[1], 1), _g(1003, LRS[1], 2),
                          _g(1005, LRS[3], 3)]),
    "modes_small": dict(groups=[_g(5, LRS[3], 3), _g(3, LRS[1], 2), _g(1, LRS[0], 1),
                                _g(7, LRS[2], 0)], eps=1e-8),
}
NAMES = tuple(CASES)


def case(name):
    d = CASES[name]
    return SimpleNamespace(name=name, groups=d["groups"], eps=d.get("eps", 1e-15),
                           starts=d.get("starts", STARTS), betas=BETAS)


def _rng(name, *extra):
    return np.random.default_rng([zlib.crc32(name.encode()), *extra])


@functools.lru_cache(maxsize=None)
def initial(name):
    """[(p, m, v)] float32 per group: p ~ N(0, 1); m, v those of a gradient
    stream of the group's magnitude (m ~ 0.3 mag N(0, 1), v ~ mag^2 U(0, 1)) --
    a state any step count may meet, with g - m free to cancel."""
    out = []
    for i, gr in enumerate(case(name).groups):
        r = _rng(name, i)
        p = r.standard_normal(gr.numel).astype(np.float32)
        m = (0.3 * gr.mag * r.standard_normal(gr.numel)).astype(np.float32)
        v = ((gr.mag * gr.mag) * r.random(gr.numel)).astype(np.float32)
        for a in (p, m, v):
            a.setflags(write=False)
        out.append((p, m, v))
    return out


def grads(name, run, s):
    """[(g or None, aux or None)] float32 for step s (0-based) of run `run`.
    aux: N(0, 1) mag for the sum, exp(N(0, 1)) for the exp VJP, a sigmoid's
    value for the sigmoid VJP with exactly 0, 0.5 and 1 in front."""
    out = []
    for i, gr in enumerate(case(name).groups):
        r = _rng(name, i, 1 + run, s)
        g = (gr.mag * r.standard_normal(gr.numel)).astype(np.float32)
        if gr.grad == "none":
            g = None
        elif gr.grad == "then_zero" and run > 0:
            g = np.zeros(gr.numel, np.float32)
        aux = None
        if gr.mode == 1:
            aux = (gr.mag * r.standard_normal(gr.numel)).astype(np.float32)
        elif gr.mode == 2:
            aux = np.exp(r.standard_normal(gr.numel)).astype(np.float32)
        elif gr.mode == 3:
            aux = (1.0 / (1.0 + np.exp(-3.0 * r.standard_normal(gr.numel)))).astype(np.float32)
            aux[:3] = (0.0, 0.5, 1.0)[:gr.numel]
        out.append((g, aux))
    return out


def big_sample():
    """Indices of the 17 M group the oracle is checked on: every 17th element
    (1 M of them), the first and the last 4096."""
    idx = np.concatenate([np.arange(4096), np.arange(0, BIG, 17), np.arange(BIG - 4096, BIG)])
    return np.unique(idx)


def worst(got, want, bd):
    """(index, error / bound there) of the largest excess."""
    r = np.abs(np.asarray(got, np.float64) - want) / bd
    i = int(np.argmax(r))
    return i, float(r[i])
