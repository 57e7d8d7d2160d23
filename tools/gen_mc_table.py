#!/usr/bin/env python3
"""Generate the marching-cubes case table text2nerf_amd/csrc/t2n_mc_table.h from rules (nothing is typed in).

    python tools/gen_mc_table.py            # rewrites the header
    python tools/gen_mc_table.py --check    # exit 1 if the committed header differs

Rules ("Mesh export"):
  corners   corner c of a cell sits at offset (c & 1, c >> 1 & 1, c >> 2 & 1) in (i, j, k); bit c of the case is set iff
            v(corner) > level (strict: NaN is outside)
  edges     edge e = 4 a + u + 2 v runs along axis a from the corner whose offsets on the other two axes, in increasing axis order,
            are (u, v); it is crossed iff its two ends differ in their bit
  faces     a face with two crossed edges joins them; a face with four has two inside corners on a diagonal and cuts each of them
            off (joins the two face edges that meet at it). The rule reads the face's four corner bits only, so the two cells
            that share a face agree on its segments
  loops     every crossed edge then has degree two: the segments form closed loops. A loop is oriented so that its area vector
            (edge midpoints as positions) points from the inside ends of its edges to their outside ends: the right-hand normal
            of every triangle points towards LOWER values
  triangles each loop is triangulated without a diagonal that joins two cube edges of one cube face (the neighbouring cell could
            put the same diagonal into that face, and four triangles would share one edge); of the admissible triangulations the
            first in the enumeration order below is taken
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "text2nerf_amd", "csrc", "t2n_mc_table.h")

EXPECT = {"empty_cases": 2, "triangles": 820, "max_triangles": 5, "longest_loop": 7}   # functions of the face rule only


def corner_offset(c):
    return (c & 1, c >> 1 & 1, c >> 2 & 1)


def corner_index(off):
    return off[0] | off[1] << 1 | off[2] << 2


def edge_corners(e):
    """(lower corner, upper corner) of cube edge e."""
    a, u, v = e >> 2, e & 1, e >> 1 & 1
    others = [b for b in range(3) if b != a]
    lo = [0, 0, 0]
    lo[others[0]], lo[others[1]] = u, v
    hi = list(lo)
    hi[a] = 1
    return corner_index(lo), corner_index(hi)


def edge_owner_offset(e):
    """Offset from the cell's lowest node of the node that owns cube edge e (its lower end)."""
    return corner_offset(edge_corners(e)[0])


def faces():
    """The six cube faces as (corners, edges): axis d, side s."""
    out = []
    for d in range(3):
        for s in range(2):
            cs = [c for c in range(8) if corner_offset(c)[d] == s]
            es = [e for e in range(12) if all(corner_offset(c)[d] == s for c in edge_corners(e))]
            assert len(cs) == 4 and len(es) == 4
            out.append((cs, es))
    return out


FACES = faces()


def same_face(e0, e1):
    return any(e0 in es and e1 in es for _, es in FACES)


def face_segments(case, face):
    """The segments (pairs of cube edges) the face rule puts on one face: a function of the face's four corner bits."""
    cs, es = face
    crossed = [e for e in es if (case >> edge_corners(e)[0] & 1) != (case >> edge_corners(e)[1] & 1)]
    if not crossed:
        return []
    if len(crossed) == 2:
        return [tuple(sorted(crossed))]
    assert len(crossed) == 4
    segs = []
    for c in cs:
        if case >> c & 1:                       # an inside corner: cut it off
            at = [e for e in es if c in edge_corners(e)]
            assert len(at) == 2
            segs.append(tuple(sorted(at)))
    assert len(segs) == 2
    return segs


def midpoint(e):
    lo, hi = edge_corners(e)
    a, b = corner_offset(lo), corner_offset(hi)
    return tuple((a[k] + b[k]) / 2 for k in range(3))


def out_minus_in(case, e):
    lo, hi = edge_corners(e)
    inside, outside = (lo, hi) if case >> lo & 1 else (hi, lo)
    a, b = corner_offset(inside), corner_offset(outside)
    return tuple(b[k] - a[k] for k in range(3))


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def loops_of(case):
    """Closed, oriented loops of cube edges; each starts at its lowest edge."""
    adj = {}
    for face in FACES:
        for e0, e1 in face_segments(case, face):
            adj.setdefault(e0, []).append(e1)
            adj.setdefault(e1, []).append(e0)
    assert all(len(v) == 2 for v in adj.values()), case
    loops, seen = [], set()
    for start in sorted(adj):
        if start in seen:
            continue
        loop, prev, cur = [start], start, min(adj[start])
        seen.add(start)
        while cur != start:
            assert cur not in seen, case
            loop.append(cur)
            seen.add(cur)
            a, b = adj[cur]
            prev, cur = cur, (b if a == prev else a)
        assert len(loop) >= 3, case
        pts = [midpoint(e) for e in loop]
        area = [0.0, 0.0, 0.0]
        for i in range(len(pts)):
            c = cross(pts[i], pts[(i + 1) % len(pts)])
            area = [area[k] + c[k] / 2 for k in range(3)]
        sign = sum(sum(area[k] * d[k] for k in range(3)) for d in (out_minus_in(case, e) for e in loop))
        assert sign != 0, case
        if sign < 0:
            loop = [loop[0]] + loop[:0:-1]
        loops.append(loop)
    return loops


def triangulations(idx):
    """Every triangulation of the convex polygon idx (positions in the loop), as lists of index triples in loop order. Enumeration
    order: the apex of the triangle on the side (first, last) ascending, the left part before the right."""
    if len(idx) < 3:
        yield []
        return
    for m in range(1, len(idx) - 1):
        for left in triangulations(idx[:m + 1]):
            for right in triangulations(idx[m:]):
                yield [(idx[0], idx[m], idx[-1])] + left + right


def triangulate(loop):
    n = len(loop)
    for tris in triangulations(list(range(n))):
        ok = True
        for t in tris:
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                if (b - a) % n in (1, n - 1):
                    continue                    # a side of the loop: lies in a face by construction
                if same_face(loop[a], loop[b]):
                    ok = False
        if ok:
            return [tuple(loop[i] for i in t) for t in tris]
    raise AssertionError(f"no admissible triangulation of {loop}")


def case_triangles(case):
    out = []
    for loop in loops_of(case):
        out += triangulate(loop)
    return out


def build_table():
    """(ntri [256], tri [256][5][3], stats): unused triples are zero."""
    ntri, tri = [], []
    longest = 0
    for case in range(256):
        for loop in loops_of(case):
            longest = max(longest, len(loop))
        ts = case_triangles(case)
        ntri.append(len(ts))
        tri.append([list(t) for t in ts] + [[0, 0, 0]] * (5 - len(ts)))
    stats = {"empty_cases": sum(1 for n in ntri if n == 0), "triangles": sum(ntri), "max_triangles": max(ntri), "longest_loop": longest}
    assert stats == EXPECT, stats
    return ntri, tri, stats


def render():
    ntri, tri, stats = build_table()
    L = ["// Marching-cubes case table. GENERATED by tools/gen_mc_table.py from the rules stated there: do not edit.",
         "// Corner c of a cell: offset (c & 1, c >> 1 & 1, c >> 2 & 1) in (i, j, k); bit c of the case: v(corner) > level.",
         "// Edge e = 4 a + u + 2 v: along axis a from the corner with offsets (u, v) on the other two axes in increasing axis order.",
         "// Right-hand normals of the triangles point towards lower values.",
         f"// {stats['empty_cases']} cases without a triangle, {stats['triangles']} triangles over all cases, at most {stats['max_triangles']} in a case,"
         f" longest loop {stats['longest_loop']}.",
         "#pragma once",
         "#ifndef T2N_MC_TABLE_QUAL",
         "#define T2N_MC_TABLE_QUAL static const",
         "#endif",
         "",
         "T2N_MC_TABLE_QUAL unsigned char t2n_mc_ntri[256] = {"]
    for r in range(0, 256, 32):
        L.append("    " + ", ".join(str(n) for n in ntri[r:r + 32]) + ",")
    L += ["};", "", "T2N_MC_TABLE_QUAL unsigned char t2n_mc_tri[256][5][3] = {"]
    for case in range(256):
        L.append("    {" + ", ".join("{" + ", ".join(f"{e:2d}" for e in t) + "}" for t in tri[case]) + "},   // " + format(case, "08b"))
    L += ["};", ""]
    return "\n".join(L)


def main():
    text = render()
    if "--check" in sys.argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("t2n_mc_table.h", "is up to date" if same else "DIFFERS from the generator's output")
        sys.exit(0 if same else 1)
    with open(HEADER, "w") as fh:
        fh.write(text)
    print("wrote", HEADER)


if __name__ == "__main__":
    main()
