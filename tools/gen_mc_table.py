#!/usr/bin/env python3
"""Generates gsplat-triton_amd/csrc/mc_table.h: the marching-cubes case table
of csrc/tsdf.hip, 256 rows of up to 5 triangles ([256][16] int8, -1 ends a
row).  Nothing is typed in: every row follows from the rules below.

Numbering
    corner  c = x + 2 y + 4 z                      (x, y, z in {0, 1})
    edge    e = 4 axis + r: along `axis` from the corner whose other two
            coordinates (in x, y, z order) are (r & 1, r >> 1)
    case    bit c set iff corner c is inside (tsdf < 0)

Rules
  * a vertex sits on every cube edge whose two corners differ in sign;
  * on each cube face the crossed edges are joined in pairs.  A face with four
    crossings (two inside corners on a diagonal) joins the two edges around
    each INSIDE corner: the links separate the inside corners.  The choice
    reads that face's four signs only, so the two cells sharing it agree;
  * every crossed edge lies on two faces and so has two links: they close into
    loops;
  * each loop is fan-triangulated from the first apex (walking the loop from
    its lowest edge) none of whose fan diagonals joins two vertices on the
    same cube face -- such a diagonal lies in the face, where the neighbouring
    cell may lay a triangle over it (a flat pair, a non-manifold edge);
  * each loop is wound so that its normal points along the trilinear gradient
    of the corner signs (inside -1, outside +1): towards positive tsdf.

Usage: gen_mc_table.py [--check] [path]   (default path: the header in the tree)
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT = os.path.join(HERE, "..", "gsplat-triton_amd", "csrc", "mc_table.h")


def corner_xyz(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_corners(e):
    """(the edge's lower corner, its upper corner)."""
    axis, r = e >> 2, e & 3
    others = [a for a in range(3) if a != axis]
    p = [0, 0, 0]
    p[others[0]], p[others[1]] = r & 1, r >> 1
    q = list(p)
    q[axis] = 1
    return p[0] + 2 * p[1] + 4 * p[2], q[0] + 2 * q[1] + 4 * q[2]


def edge_faces(e):
    """The two cube faces (axis, side) the edge lies on."""
    axis, r = e >> 2, e & 3
    others = [a for a in range(3) if a != axis]
    return {(others[0], r & 1), (others[1], r >> 1)}


def edge_mid(e):
    a, b = edge_corners(e)
    pa, pb = corner_xyz(a), corner_xyz(b)
    return tuple(0.5 * (pa[i] + pb[i]) for i in range(3))


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def face_cycle(axis, side):
    """The face's four corners in cyclic order."""
    u, v = [a for a in range(3) if a != axis]
    out = []
    for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
        p = [0, 0, 0]
        p[axis], p[u], p[v] = side, du, dv
        out.append(p[0] + 2 * p[1] + 4 * p[2])
    return out


def gradient(signs, p):
    """Trilinear gradient of the corner values at p in [0, 1]^3."""
    g = [0.0, 0.0, 0.0]
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for du in (0, 1):
            for dv in (0, 1):
                lo = [0, 0, 0]
                lo[u], lo[v] = du, dv
                hi = list(lo)
                hi[axis] = 1
                w = (p[u] if du else 1.0 - p[u]) * (p[v] if dv else 1.0 - p[v])
                g[axis] += w * (signs[hi[0] + 2 * hi[1] + 4 * hi[2]]
                                - signs[lo[0] + 2 * lo[1] + 4 * lo[2]])
    return g


def links_of(case):
    inside = [(case >> c) & 1 for c in range(8)]
    links = {}

    def link(a, b):
        links.setdefault(a, []).append(b)
        links.setdefault(b, []).append(a)

    for axis in range(3):
        for side in (0, 1):
            cyc = face_cycle(axis, side)
            crossed = [EDGE_OF[frozenset((cyc[i], cyc[(i + 1) % 4]))] for i in range(4)
                       if inside[cyc[i]] != inside[cyc[(i + 1) % 4]]]
            if len(crossed) == 2:
                link(*crossed)
            elif len(crossed) == 4:
                for i in range(4):  # the two edges around each inside corner
                    if inside[cyc[i]]:
                        link(EDGE_OF[frozenset((cyc[i - 1], cyc[i]))],
                             EDGE_OF[frozenset((cyc[i], cyc[(i + 1) % 4]))])
            else:
                assert not crossed
    return links


def loops_of(case):
    links = links_of(case)
    assert all(len(v) == 2 for v in links.values()), case
    seen, loops = set(), []
    for start in sorted(links):
        if start in seen:
            continue
        loop, prev, cur = [start], None, start
        seen.add(start)
        while True:
            a, b = links[cur]  # two cube edges share at most one face: a != b
            nxt = min(a, b) if prev is None else (a if b == prev else b)
            if nxt == start:
                break
            assert nxt not in seen, case
            loop.append(nxt)
            seen.add(nxt)
            prev, cur = cur, nxt
        assert len(loop) >= 3, case
        loops.append(loop)
    return loops


def orient(case, loop):
    signs = [-1.0 if (case >> c) & 1 else 1.0 for c in range(8)]
    pts = [edge_mid(e) for e in loop]
    n = [0.0, 0.0, 0.0]
    for i in range(len(pts)):  # Newell: twice the area vector, counter-clockwise from its tip
        a, b = pts[i], pts[(i + 1) % len(pts)]
        n[0] += a[1] * b[2] - a[2] * b[1]
        n[1] += a[2] * b[0] - a[0] * b[2]
        n[2] += a[0] * b[1] - a[1] * b[0]
    dot = 0.0
    for p in pts:
        g = gradient(signs, p)
        dot += n[0] * g[0] + n[1] * g[1] + n[2] * g[2]
    assert abs(dot) > 1e-9, (case, loop)
    return loop if dot > 0 else [loop[0]] + loop[:0:-1]


def fan(case, loop):
    n = len(loop)
    for s in range(n):
        r = loop[s:] + loop[:s]
        if all(not (edge_faces(r[0]) & edge_faces(r[j])) for j in range(2, n - 1)):
            return [(r[0], r[j], r[j + 1]) for j in range(1, n - 1)]
    raise AssertionError(f"case {case}: no apex for loop {loop}")


def table():
    rows = []
    for case in range(256):
        tris = []
        for loop in loops_of(case):
            tris += fan(case, orient(case, loop))
        assert len(tris) <= 5, (case, len(tris))
        flat = [e for t in tris for e in t]
        rows.append(flat + [-1] * (16 - len(flat)))
    return rows


def render():
    out = ["// Generated by tools/gen_mc_table.py -- do not edit; the rules are in that file.",
           "// Marching-cubes triangles per sign case: corner c = x + 2y + 4z, case bit c set iff",
           "// corner c is inside (tsdf < 0); edge e = 4 axis + r starts at the corner whose other",
           "// two coordinates are (r & 1, r >> 1).  -1 ends a row.",
           "#pragma once",
           "",
           "#define GS_MC_TABLE_ROWS \\"]
    rows = table()
    for i, r in enumerate(rows):
        out.append("  {" + ", ".join(f"{v:2d}" for v in r) + "}" + (", \\" if i < 255 else ""))
    return "\n".join(out) + "\n"


def main(argv):
    check = "--check" in argv
    paths = [a for a in argv if not a.startswith("--")]
    path = paths[0] if paths else DEFAULT
    text = render()
    if check:
        same = os.path.exists(path) and open(path).read() == text
        print("up to date" if same else "STALE", path)
        return 0 if same else 1
    with open(path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
