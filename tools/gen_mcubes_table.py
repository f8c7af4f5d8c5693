"""Generate uforecon_amd/csrc/mcubes_table.h: the 256-case triangle table of the marching-cubes kernel (csrc/mcubes.hip).

``python tools/gen_mcubes_table.py`` rewrites the header; ``--check`` only compares it with what would be written.

Conventions (shared with the kernel and with tests/mcubes_ref.py):
  corner c = dx | dy << 1 | dz << 2 of the cube whose lowest corner is voxel (x, y, z); the case index has bit c set iff
  corner c is *below* (v < level).
  edge e = 4 * axis + r joins corner c and c + (1 << axis), where bit axis of c is 0 and the other two bits of c, the lower
  axis first, are r & 1 and r >> 1.  The vertex on it is owned by voxel (x, y, z) + offset(c).

The table is derived, not copied.  On each of the six cube faces the crossing edges are joined by segments that cut off
the runs of below corners along the face's boundary; an ambiguous face (two below corners on a diagonal) thus gets two
segments, one around each below corner.  The rule looks at one face's four corners only, so the two cubes that share a
face draw the same segments on it, in opposite directions.  Each segment is oriented so that, seen from outside the cube,
the below corners lie on its right; chained through the cube the segments form closed loops, and each loop is
triangulated in loop order.  A triangle's right-hand normal then points away from the below corners, towards increasing
f.  A diagonal of a loop's triangulation never joins two vertices that lie on one cube face (the neighbouring cube could
draw the same diagonal): the loop is fanned from the first vertex that allows it, else triangulated by search.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "uforecon_amd", "csrc", "mcubes_table.h")


def corner_offset(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def edge_corners(e):
    axis, r = e // 4, e % 4
    others = [a for a in range(3) if a != axis]
    c = ((r & 1) << others[0]) | ((r >> 1) << others[1])
    return c, c | (1 << axis), axis


def edge_of(c0, c1):
    lo, hi = min(c0, c1), max(c0, c1)
    axis = (hi ^ lo).bit_length() - 1
    others = [a for a in range(3) if a != axis]
    return 4 * axis + ((lo >> others[0]) & 1) + 2 * ((lo >> others[1]) & 1)


def edge_mid(e):
    c0, c1, _ = edge_corners(e)
    return (corner_offset(c0) + corner_offset(c1)) / 2.0


FACES = []   # (outward normal, the four corners in boundary order)
for axis in range(3):
    u, v = [a for a in range(3) if a != axis]
    for side in (0, 1):
        cyc = [(side << axis) | (du << u) | (dv << v) for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1))]
        n = np.zeros(3)
        n[axis] = 1.0 if side else -1.0
        FACES.append((n, cyc))
EDGE_FACES = {e: {i for i, (_, cyc) in enumerate(FACES) if {edge_corners(e)[0], edge_corners(e)[1]} <= set(cyc)}
              for e in range(12)}


def face_segments(case):
    """Directed segments (start edge, end edge) on every face for one case."""
    segs = []
    for n, cyc in FACES:
        below = [(case >> c) & 1 for c in cyc]
        if all(below) or not any(below):
            continue
        start = next(i for i in range(4) if below[i] and not below[i - 1])   # first corner of a run of below corners
        for k in range(4):
            i = (start + k) % 4
            if not (below[i] and not below[i - 1]):
                continue
            j = i
            while below[(j + 1) % 4]:
                j = (j + 1) % 4
            run = [cyc[(i + m) % 4] for m in range((j - i) % 4 + 1)]
            ea = edge_of(cyc[i - 1], cyc[i])           # entering the run
            eb = edge_of(cyc[j], cyc[(j + 1) % 4])     # leaving it
            P, Q = edge_mid(ea), edge_mid(eb)
            B = np.mean([corner_offset(c) for c in run], axis=0)
            s = float(np.dot(np.cross(n, Q - P), B - P))
            assert s != 0.0
            segs.append((ea, eb) if s < 0 else (eb, ea))
    return segs


def loops_of(case):
    segs = face_segments(case)
    nxt = {}
    for a, b in segs:
        assert a not in nxt, (case, "edge leaves twice")
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), (case, "segments do not close")
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        lp = [e]
        seen.add(e)
        while nxt[lp[-1]] != e:
            lp.append(nxt[lp[-1]])
            seen.add(lp[-1])
        loops.append(lp)
    return loops


def _share_face(a, b):
    return bool(EDGE_FACES[a] & EDGE_FACES[b])


def _triangulate(poly):
    """Triangles (loop order kept) of polygon ``poly`` with no diagonal between two vertices of one cube face."""
    n = len(poly)
    if n == 3:
        return [tuple(poly)]
    for s in range(n):                      # fans first
        rot = poly[s:] + poly[:s]
        if all(not _share_face(rot[0], rot[i]) for i in range(2, n - 1)):
            return [(rot[0], rot[i], rot[i + 1]) for i in range(1, n - 1)]

    def search(p):
        if len(p) == 3:
            return [tuple(p)]
        if len(p) < 3:
            return []
        for i in range(1, len(p) - 1):      # apex of the triangle on the base (p[0], p[-1])
            if i > 1 and _share_face(p[0], p[i]):
                continue
            if i < len(p) - 2 and _share_face(p[i], p[-1]):
                continue
            left = search(p[:i + 1]) if i > 1 else []
            right = search(p[i:]) if i < len(p) - 2 else []
            if (i > 1 and left is None) or (i < len(p) - 2 and right is None):
                continue
            return (left or []) + [(p[0], p[i], p[-1])] + (right or [])
        return None

    for s in range(n):
        t = search(poly[s:] + poly[:s])
        if t is not None:
            return t
    raise AssertionError(f"no admissible triangulation of loop {poly}")


def build_table():
    tris = []
    for case in range(256):
        t = []
        for lp in loops_of(case):
            t += _triangulate(lp)
        tris.append(t)
    return tris


def emit_header(tris) -> str:
    max_tri = max(len(t) for t in tris)
    row = 3 * max_tri + 1
    lines = [
        "// Generated by tools/gen_mcubes_table.py -- do not edit.  Marching-cubes case table of csrc/mcubes.hip.",
        "// corner c = dx | dy << 1 | dz << 2; case bit c set iff corner c is below the level; edge e = 4 * axis + r joins",
        "// corner c and c + (1 << axis) (bit axis of c clear, the other two bits of c, lower axis first, = r & 1, r >> 1).",
        "// kMcTable[case]: up to UFR_MC_MAX_TRI triangles as edge triples, right-hand normal towards increasing f, then -1.",
        "#pragma once",
        "#include <stdint.h>",
        "",
        f"#define UFR_MC_MAX_TRI {max_tri}",
        f"#define UFR_MC_TABLE_ROW {row}",
        "",
        "namespace ufr {",
        "static constexpr uint8_t kMcTriCount[256] = {",
    ]
    for i in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in tris[i:i + 32]) + ",")
    lines += ["};", f"static constexpr int8_t kMcTable[256][{row}] = {{"]
    for case, t in enumerate(tris):
        flat = [e for tri in t for e in tri]
        flat += [-1] * (row - len(flat))
        lines.append("    {" + ", ".join(str(v) for v in flat) + f"}},  // {case}")
    lines += ["};", "}  // namespace ufr", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="exit 1 if the committed header differs from a fresh one")
    a = ap.parse_args()
    text = emit_header(build_table())
    if a.check:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print("mcubes_table.h is " + ("up to date" if same else "STALE"))
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print(OUT)


if __name__ == "__main__":
    main()
