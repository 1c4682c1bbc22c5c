"""Bars and finite differences for the 2DGS rasterizer's test matrix
(tests/surfel_cases.py).  Run on the CPU:

    python tests/golden/make_golden_surfel_matrix.py

Written to surfel_matrix.npz (numbers and names only; the inputs are rebuilt
from the seed and the float64 oracle runs at test time):

    bar_names, bar_values   per "<case>:<tile size>:<variant>:<output>", the
                            larger of two float32 errors against the float64
                            oracle, as max error / max |float64|: the oracle's
                            own torch formulation run in float32 and oracle/
                            surfel_oracle.py's numpy raster2dgs_fwd / _bwd in
                            their native float32 (hand-derived backward, another
                            operation order).  Variants: fwd; bwd (a cotangent
                            on all five outputs) and lean (colours and alphas
                            only), both with backgrounds and absgrad, at 33
                            channels.
    fd_names, fd_<case>_rows, fd_<case>_<input>
                            central finite differences in float64 of
                            sum(cotangent x output) of two cases, for every
                            entry of a few surfels' inputs, so the host test
                            can compare the oracle's autograd with them
                            without recomputing

The reference's own torch 2DGS rasterizer cannot run (it needs the CUDA
extension and nerfacc), so these two pin the oracle.  The script also prints
the populations, gate distances and redraw shares that DESIGN.md tabulates.
"""

import copy
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(OUT), os.path.dirname(os.path.dirname(OUT))]

import surfel_cases as SC  # noqa: E402
from make_golden_proj_matrix import save_npz  # noqa: E402

FD_CASES = (("sparse", 16), ("sparse_c2", 16))
FD_INPUTS = ("m2", "rt", "opac", "nr", "colors")
FD_ROWS = 4
FD_CHANNELS = (0, 5, SC.DMAX - 1)


def case_bars(name, ts):
    f64, b64, l64 = SC.fwd64(name, ts, bg=True), SC.bwd64(name, ts, bg=True), \
        SC.bwd64(name, ts, bg=True, lean=True)
    g32 = SC.torch32(name, ts)
    c = SC.build(name)
    t32 = g32.forward(bg=c.bg)
    n32 = SC.numpy_fwd(name, ts, bg=True)
    for f in (t32, n32):
        for k in ("last_ids", "median_ids", "ncon", "jsum"):
            assert np.array_equal(f[k], f64[k]), (name, ts, k)
    bars = {}
    for k in SC.FWD_OUT:
        bars[f"{name}:{ts}:fwd:{k}"] = max(SC.rel_err(t32[k], f64[k]), SC.rel_err(n32[k], f64[k]))
    for key, ref, lean in (("bwd", b64, False), ("lean", l64, True)):
        bt = g32.backward(bg=c.bg, lean=lean)
        bn = SC.numpy_bwd(name, ts, n32, bg=True, lean=lean)
        for k in ref:
            bars[f"{name}:{ts}:{key}:{k}"] = max(SC.rel_err(bt[k], ref[k]), SC.rel_err(bn[k], ref[k]))
    return bars


def _loss(c, geo):
    with torch.no_grad():
        _, o, _ = SC._walk(c, geo, torch.float64, False)
        t = lambda a: torch.from_numpy(np.array(a)).double()  # noqa: E731
        colors = o.col + o.T * t(c.bg)[:, None, None, :]
        loss = float((colors * t(c.v_colors)).sum() + ((1.0 - o.T) * t(c.v_alphas)).sum()
                     + (o.normals * t(c.v_normals)).sum() + (o.distort * t(c.v_distort)).sum()
                     + (o.median * t(c.v_median)).sum())
        # every decision: contributor sets, ids, the g3 / g2 branch and the clamp
        return loss, torch.stack([o.ncon, o.jsum, o.last_ids, o.median_ids, o.bsum])


def finite_differences(name, ts):
    """Rows: the two surfels with the most isects and the two with the largest
    2-D mean gradient (pairs decided by g2).  Central differences at a step h
    and at h / 2, Richardson-extrapolated (the ray transform's third row moves
    s by far more than its own relative size: at h = 1e-6 of the entry the
    plain difference is still 2e-3 off).  h is 1e-7 of the entry (or of its
    row's largest), or 1e-8 if an evaluation at 1e-7 decides a pair otherwise
    than the unperturbed case does; an entry with no such step is NaN."""
    c0, geo = SC.build(name), SC.tiles(name, ts)
    G = c0.C * c0.N
    many = np.argsort(-np.bincount(geo.fids, minlength=G), kind="stable")
    vm = np.abs(SC.bwd64(name, ts, bg=True)["v_means2d"]).reshape(G, 2).max(-1)
    rows = list(many[:FD_ROWS // 2])
    rows += [r for r in np.argsort(-vm, kind="stable") if r not in rows][:FD_ROWS - len(rows)]
    rows = np.array(rows)
    out = {f"fd_{name}_rows": rows.astype(np.int64)}
    _, decided = _loss(c0, geo)
    shapes = {"m2": (G, 2), "rt": (G, 9), "opac": (G,), "nr": (G, 3), "colors": (G, SC.DMAX)}
    for which in FD_INPUTS:
        base = np.array(getattr(c0, which), np.float64).reshape(shapes[which])
        cols = [()] if which == "opac" else [(j,) for j in (FD_CHANNELS if which == "colors"
                                                            else range(shapes[which][1]))]
        fd = np.zeros((len(rows), len(cols)))
        for i, row in enumerate(rows):
            for jj, j in enumerate(cols):
                fd[i, jj] = np.nan
                for rel in (1e-7, 1e-8):
                    h = rel * max(abs(base[(row,) + j]), np.abs(base[row]).max())
                    d, same = [], True
                    for step in (h, 0.5 * h):
                        vals = []
                        for sgn in (1, -1):
                            x = base.copy()
                            x[(row,) + j] += sgn * step
                            c = copy.copy(c0)
                            setattr(c, which, x.reshape(getattr(c0, which).shape))
                            loss, dec = _loss(c, geo)
                            vals.append(loss)
                            same = same and bool(torch.equal(dec, decided))
                        d.append((vals[0] - vals[1]) / (2 * step))
                    if same:
                        fd[i, jj] = (4.0 * d[1] - d[0]) / 3.0
                        break
        out[f"fd_{name}_{which}"] = fd
    return out


def main():
    bars, fixture = {}, {"fd_names": np.array([n for n, _ in FD_CASES])}
    for name in SC.ALL_NAMES:
        c = SC.build(name)
        for ts in c.ts_list:
            bars.update(case_bars(name, ts))
            tr = SC.gates(name, ts)
            print(f"{name} ts {ts}: N {c.N} C {c.C} {c.W}x{c.H} pairs {tr['pairs']} isects "
                  f"{tr['isects']} longest {tr['longest']} terminated {tr['terminated']}/"
                  f"{tr['pixels']} clamped {tr['clamped']} g3 {tr['by_g3']} g2 {tr['by_g2']} rz0 "
                  f"{tr['rz0']} redrawn {c.redrawn:.4f} nearest gate "
                  + " ".join(f"{k} {v:.1e}" for k, v in tr["min"].items()))
        if c.pop == "cull":
            for ts in c.ts_list:
                print(f"{name} ts {ts} surfel_keep branches: {SC.keep_population(name, ts)}")
    for name, ts in FD_CASES:
        fixture.update(finite_differences(name, ts))
    names = sorted(bars)
    values = np.array([bars[k] for k in names], np.float64)
    assert np.isfinite(values).all()
    for part in ("fwd", "bwd", "lean"):
        for k in sorted({n.split(":")[3] for n in names if n.split(":")[2] == part}):
            v = np.array([bars[n] for n in names if n.split(":")[2:] == [part, k]])
            print(f"{part:5s} {k:17s} bars: min {v.min():.2e}  median {np.median(v):.2e}  max {v.max():.2e}")
    print("largest share of redrawn surfels:", max(SC.build(n).redrawn for n in SC.ALL_NAMES))
    path = os.path.join(OUT, "surfel_matrix.npz")
    save_npz(path, dict(bar_names=np.array(names), bar_values=values, **fixture))
    size = os.path.getsize(path)
    print(f"surfel_matrix: {len(names)} bars, {size} bytes")
    assert size < 100_000, size


if __name__ == "__main__":
    main()
