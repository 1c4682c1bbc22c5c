"""float64 numpy oracles of the splat compression (gsplat_hip/compression.py,
csrc/compress.hip): the L1 assignment with lowest-index ties, the mean update
that keeps empty centroids, the Lloyd loop, the Morton order and the quantise /
dequantise formulas of each file type.  Written from the format's definition,
independent of the code under test."""

import numpy as np


# ------------------------------------------------------------------ k-means
def l1_distances(x, c, chunk=512):
    """[N, K] float64 Manhattan distances."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    out = np.empty((x.shape[0], c.shape[0]))
    for s in range(0, x.shape[0], chunk):
        out[s:s + chunk] = np.abs(x[s:s + chunk, None, :] - c[None, :, :]).sum(-1)
    return out


def assign_l1(x, c):
    """(labels, distance matrix): argmin over k, the lowest k on a tie
    (np.argmin returns the first minimum)."""
    d = l1_distances(x, c)
    return d.argmin(1), d


def update_means(x, labels, c):
    """(new centroids, counts): the mean of each centroid's members; a
    centroid without members keeps its row."""
    x = np.asarray(x, np.float64)
    out = np.asarray(c, np.float64).copy()
    K = out.shape[0]
    counts = np.bincount(labels, minlength=K)
    sums = np.stack([np.bincount(labels, weights=x[:, d], minlength=K)
                     for d in range(x.shape[1])], 1)
    has = counts > 0
    out[has] = sums[has] / counts[has, None]
    return out, counts


def lloyd(x, c0, max_iters, tol):
    """(centroids, labels, iterations): assign then update per iteration; stops
    once the fraction of changed labels is below tol."""
    c = np.asarray(c0, np.float64).copy()
    labels = np.full(len(x), -1)
    iters = 0
    for _ in range(max_iters):
        new, _ = assign_l1(x, c)
        changed = int((new != labels).sum())
        labels = new
        c, _ = update_means(x, labels, c)
        iters += 1
        if changed / len(x) < tol:
            break
    return c, labels, iters


def optimality_bar(dmin):
    """A chosen centroid's float64 distance may exceed the optimum by this:
    the fp32 sum of D <= 72 non-negative terms errs by about D * 2^-24
    relative (4.3e-6 at D = 72), on each of the two distances compared."""
    return dmin * (1 + 1e-5) + 1e-6


# ------------------------------------------------------------- Morton order
def morton_codes(means_log):
    x = np.asarray(means_log, np.float64)
    lo, hi = x.min(0), x.max(0)
    span = hi - lo
    t = (x - lo) / np.where(span > 0, span, 1.0)
    q = np.clip(np.floor(t * 1023.999), 0, 1023).astype(np.int64)
    code = np.zeros(len(x), np.int64)
    for b in range(10):
        for axis in range(3):  # x in the lowest bit
            code |= ((q[:, axis] >> b) & 1) << (3 * b + axis)
    return code


def morton_order(means_log):
    return np.argsort(morton_codes(means_log), kind="stable")


# ----------------------------------------------------------- file formulas
def log_transform(x):
    x = np.asarray(x, np.float64)
    return np.sign(x) * np.log1p(np.abs(x))


def inverse_log_transform(y):
    y = np.asarray(y, np.float64)
    return np.sign(y) * np.expm1(np.abs(y))


def quantize(values, mins, maxs, bits):
    """round(norm * (2^bits - 1)), norm over [mins, maxs]; a constant channel
    quantises to 0."""
    v = np.asarray(values, np.float64)
    mins, maxs = np.asarray(mins, np.float64), np.asarray(maxs, np.float64)
    span = maxs - mins
    norm = np.where(span > 0, (v - mins) / np.where(span > 0, span, 1.0), 0.0)
    return np.round(norm * (2 ** bits - 1))


def dequantize(q, mins, maxs, bits):
    """The reference's decode: img / (2^b - 1) * (maxs - mins) + mins."""
    mins, maxs = np.asarray(mins, np.float64), np.asarray(maxs, np.float64)
    return np.asarray(q, np.float64) / (2 ** bits - 1) * (maxs - mins) + mins


def half_step(mins, maxs, bits, ulps=4):
    """The format's error bar: half a quantisation step, plus a few fp32 ulps
    of the largest magnitude of the channel."""
    mins, maxs = np.asarray(mins, np.float64), np.asarray(maxs, np.float64)
    mag = np.maximum(np.abs(mins), np.abs(maxs))
    return (maxs - mins) / (2 * (2 ** bits - 1)) + ulps * 2.0 ** -23 * np.maximum(mag, 1e-30)
