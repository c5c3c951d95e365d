"""Generates shapegan_amd/csrc/mc_tables.h, the marching-cubes tables shared by csrc/mesh.hip and the CPU twin.

    python scripts/gen_mc_tables.py            # rewrite the header
    python scripts/gen_mc_tables.py --check    # exit 1 if the committed header differs

Cube corner n sits at offset ((n >> 2) & 1, (n >> 1) & 1, n & 1) along axes (0, 1, 2); a corner is inside when v < level.
Edge e = 4 * axis + (u << 1 | w) runs along `axis` from the corner whose other two offsets (in increasing axis order) are u, w.

Every case is built the same way, so that the surface is closed across cells:
  1. On each of the six faces, each maximal run of inside corners (in the face's cyclic corner order) is cut off by one segment
     between the two face edges that bound the run.  Two diagonal inside corners are therefore always separated, and this
     depends only on the four corner signs of the face: both cells that share a face produce the same segments on it, and
     traverse them in opposite directions.
  2. The directed segments of the six faces form closed loops (every crossing edge ends one segment and starts one).
  3. Each loop is triangulated without a diagonal between two vertices that lie on one cube face: a neighbouring cell sees
     only the vertices of the shared face, so no mesh edge other than the shared face segments can appear in two cells.
  4. The loop direction is chosen so that (v1 - v0) x (v2 - v0) points from the inside corners toward the outside corners,
     i.e. toward increasing values.
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "shapegan_amd", "csrc", "mc_tables.h")


def corner_pos(n):
    return np.array([(n >> 2) & 1, (n >> 1) & 1, n & 1], dtype=float)


def edge_corners(e):
    axis, j = e // 4, e % 4
    others = [a for a in range(3) if a != axis]
    off = [0, 0, 0]
    off[others[0]], off[others[1]] = (j >> 1) & 1, j & 1
    c0 = (off[0] << 2) | (off[1] << 1) | off[2]
    return c0, c0 | (1 << (2 - axis))


EDGE = {frozenset(edge_corners(e)): e for e in range(12)}


def faces():
    """(axis, side, corners in counter-clockwise order seen from outside the cube)."""
    out = []
    for axis in range(3):
        for side in (0, 1):
            cs = [n for n in range(8) if ((n >> (2 - axis)) & 1) == side]
            normal = np.zeros(3)
            normal[axis] = 1.0 if side else -1.0
            centre = sum(corner_pos(n) for n in cs) / 4
            others = [a for a in range(3) if a != axis]
            ang = {n: np.arctan2(*(corner_pos(n) - centre)[others][::-1]) for n in cs}
            order = sorted(cs, key=lambda n: ang[n])
            p = [corner_pos(n) - centre for n in order]
            if np.dot(np.cross(p[0], p[1]), normal) < 0:
                order = order[::-1]
            out.append((axis, side, order))
    return out


FACES = faces()
EDGE_FACES = {e: {f for f, (_, _, cs) in enumerate(FACES) if set(edge_corners(e)) <= set(cs)} for e in range(12)}


def segments(case):
    inside = [(case >> n) & 1 for n in range(8)]
    segs = []
    for _, _, cs in FACES:
        ins = [inside[n] for n in cs]
        if all(ins) or not any(ins):
            continue
        for i in range(4):
            if ins[i] and not ins[(i + 1) % 4]:           # the run of inside corners ends at cs[i]
                j = i
                while ins[(j - 1) % 4]:
                    j -= 1
                start = EDGE[frozenset((cs[(j - 1) % 4], cs[j % 4]))]
                end = EDGE[frozenset((cs[i], cs[(i + 1) % 4]))]
                segs.append((start, end))
    return segs


def loops(case):
    nxt = {}
    for a, b in segments(case):
        assert a not in nxt
        nxt[a] = b
    out, seen = [], set()
    for a in sorted(nxt):
        if a in seen:
            continue
        loop = [a]
        seen.add(a)
        b = nxt[a]
        while b != a:
            loop.append(b)
            seen.add(b)
            b = nxt[b]
        out.append(loop)
    return out


def allowed(a, b):
    return not (EDGE_FACES[a] & EDGE_FACES[b])


def triangulate(poly):
    """Triangles of the polygon `poly` (vertex order kept) with every diagonal `allowed`; None if impossible."""
    n = len(poly)
    if n == 3:
        return [tuple(poly)]
    for k in range(2, n):
        if k > 2 and not allowed(poly[1], poly[k]):
            continue
        if k < n - 1 and not allowed(poly[0], poly[k]):
            continue
        left = triangulate(poly[1:k + 1]) if k > 2 else []
        right = triangulate(poly[k:] + [poly[0]]) if k < n - 1 else []
        if left is None or right is None:
            continue
        return [(poly[0], poly[1], poly[k])] + left + right
    return None


def edge_mid(e):
    a, b = edge_corners(e)
    return (corner_pos(a) + corner_pos(b)) / 2


def case_triangles(case, flip):
    tris = []
    for loop in loops(case):
        if flip:
            loop = loop[::-1]
        t = triangulate(loop)
        if t is None:
            raise RuntimeError("case %d: loop %s has no triangulation without a same-face diagonal" % (case, loop))
        tris += t
    return tris


def orientation_flip():
    """True when the loops as traced must be reversed so that face normals point toward the outside corners."""
    tris = case_triangles(1, False)       # corner 0 inside: the outside corners lie toward +(1, 1, 1)
    p = [edge_mid(e) for e in tris[0]]
    return float(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), np.ones(3))) < 0


def generate():
    flip = orientation_flip()
    table = [case_triangles(c, flip) for c in range(256)]
    maxt = max(len(t) for t in table)
    lines = ["// shapegan_amd/csrc/mc_tables.h -- generated by scripts/gen_mc_tables.py; do not edit.",
             "// Marching-cubes tables shared by csrc/mesh.hip and csrc_cpu/shapegan_cpu.cpp (plain data, no code).",
             "// Corner n: offset ((n >> 2) & 1, (n >> 1) & 1, n & 1) along axes (0, 1, 2); case bit n set: corner n inside (v < level).",
             "// Edge e: along axis e / 4 from the corner whose other two offsets (increasing axis order) are ((e >> 1) & 1, e & 1).",
             "// Ambiguous faces always separate their two inside corners, so neighbouring cells agree on every shared face and",
             "// closed surfaces come out watertight; (v1 - v0) x (v2 - v0) points toward increasing values.",
             "#pragma once",
             "",
             "#define SG_MC_MAX_TRIS %d" % maxt,
             "",
             "// triangles per case",
             "static const unsigned char sg_mc_tri_count[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join("%d" % len(table[c]) for c in range(r, min(r + 32, 256))) + ",")
    lines.append("};")
    lines.append("")
    lines.append("// edges of each triangle, in table order (-1: unused)")
    lines.append("static const signed char sg_mc_tri_edges[256][%d] = {" % (3 * maxt))
    for c in range(256):
        flat = [e for t in table[c] for e in t]
        flat += [-1] * (3 * maxt - len(flat))
        lines.append("    {" + ", ".join("%d" % e for e in flat) + "},")
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = generate()
    if "--check" in sys.argv:
        ok = os.path.exists(OUT) and open(OUT).read() == text
        print("mc_tables.h is current" if ok else "mc_tables.h differs from the generator")
        sys.exit(0 if ok else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote", os.path.normpath(OUT))
