"""Marching-cubes case table of the mesh stage (kt_mesh.hip), generated from a face rule rather than copied.

Cell corners: corner i = (i & 1, i >> 1 & 1, i >> 2 & 1); a corner is INSIDE when its tsdf is negative, and bit i of the case
index is set for an inside corner.  Edge e = 4 * axis + k joins corner base(e) and base(e) | (1 << axis), where k = bit_b + 2 * bit_c
over the two other axes b < c; the edge's vertex is owned by the voxel at base(e) (kt_mesh.hip / mesh_ref.py).

The rule:
  - on each of the six faces, the crossed edges (one end inside, one outside) are joined by segments: two crossed edges by one
    segment; on an ambiguous face (four crossed edges, alternating signs) each INSIDE corner is cut off by a segment of its own;
  - a segment runs in the direction o x n_f, o pointing from the segment towards the face's outside corners and n_f the face's
    outward normal; so the segments of a cell close into directed loops through its crossed edges;
  - each loop starts at its smallest edge index and is fan-triangulated from there: (l0, l1, l2), (l0, l2, l3), ...;
    the geometric normal (v1 - v0) x (v2 - v0) then points from the inside corners towards the outside ones.
The decision on a face depends only on its four signs, so two cells sharing a face join the same edges there: no cracks.

`python -m kintinuous_amd.mc_table` rewrites kintinuous_amd/csrc/kt_mc_table.hpp.
"""
from __future__ import annotations

import os
from collections import Counter

import numpy as np

MAX_TRIS = 5
HISTOGRAM = {0: 2, 1: 16, 2: 50, 3: 80, 4: 76, 5: 32}
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "kt_mc_table.hpp")


def corner_pos(i: int) -> np.ndarray:
    return np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1], dtype=np.int64)


def _edges():
    out = []
    for axis in range(3):
        b, c = [a for a in range(3) if a != axis]
        for k in range(4):
            out.append((((k & 1) << b) | ((k >> 1) << c), axis))
    return out


EDGES = _edges()                                   # (base corner, axis) per edge index
EDGE_OF = {(base, base | (1 << axis)): e for e, (base, axis) in enumerate(EDGES)}


def edge_between(c0: int, c1: int) -> int:
    return EDGE_OF[(min(c0, c1), max(c0, c1))]


def faces():
    """(axis, side, corners in cyclic order, outward normal) for the six faces."""
    out = []
    for axis in range(3):
        b, c = [a for a in range(3) if a != axis]
        for side in range(2):
            base = side << axis
            cyc = [base, base | (1 << b), base | (1 << b) | (1 << c), base | (1 << c)]
            n = np.zeros(3, dtype=np.int64)
            n[axis] = 1 if side else -1
            out.append((axis, side, cyc, n))
    return out


FACES = faces()


def face_segments(case: int, face) -> list:
    """Directed segments (edge_from, edge_to) of one face under the rule above."""
    _, _, cyc, n = face
    ins = [(case >> ci) & 1 for ci in cyc]
    segs = []
    # the four face edges in cyclic order: fe[j] joins cyc[j] and cyc[j + 1]
    fe = [edge_between(cyc[j], cyc[(j + 1) % 4]) for j in range(4)]
    crossed = [ins[j] != ins[(j + 1) % 4] for j in range(4)]
    nin = sum(ins)
    pairs = []
    if sum(crossed) == 2:
        pairs.append(tuple(j for j in range(4) if crossed[j]))
    elif sum(crossed) == 4:
        assert nin == 2
        for j in range(4):   # inside corner cyc[j] is cut off by the segment joining its two face edges fe[j - 1] and fe[j]
            if ins[j]:
                pairs.append(((j - 1) % 4, j))
    for ja, jb in pairs:
        mid = lambda j: (corner_pos(cyc[j]) + corner_pos(cyc[(j + 1) % 4])) / 2.0
        pa, pb = mid(ja), mid(jb)
        # o: in the face plane, perpendicular to the segment, towards the outside side -- away from the cut-off inside corner on an
        # ambiguous face, towards the outside corners otherwise (they all lie on one side then)
        segm = (pa + pb) / 2.0
        o = np.cross(n, pb - pa)
        if sum(crossed) == 4:
            ref = segm - corner_pos(cyc[jb])   # the corner between face edges ja = jb - 1 and jb
        else:
            ref = np.mean([corner_pos(cyc[j]) for j in range(4) if not ins[j]], axis=0) - segm
        if np.dot(o, ref) < 0:
            o = -o
        assert np.dot(o, ref) > 0
        d = np.cross(o, n)
        if np.dot(pb - pa, d) > 0:
            segs.append((fe[ja], fe[jb]))
        else:
            assert np.dot(pb - pa, d) < 0
            segs.append((fe[jb], fe[ja]))
    return segs


def case_loops(case: int) -> list:
    nxt = {}
    for f in FACES:
        for a, b in face_segments(case, f):
            assert a not in nxt
            nxt[a] = b
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    return loops


def case_triangles(case: int) -> list:
    tris = []
    for loop in case_loops(case):
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def build_table():
    """tri[256][MAX_TRIS][3] edge indices (-1 = unused), ntri[256]."""
    tri = np.full((256, MAX_TRIS, 3), -1, dtype=np.int8)
    ntri = np.zeros(256, dtype=np.uint8)
    for case in range(256):
        t = case_triangles(case)
        assert len(t) <= MAX_TRIS, (case, len(t))
        ntri[case] = len(t)
        for i, tr in enumerate(t):
            tri[case, i] = tr
    hist = dict(sorted(Counter(ntri.tolist()).items()))
    assert hist == HISTOGRAM, hist
    assert int((ntri > 0).sum()) == 254
    return tri, ntri


def header_text() -> str:
    tri, ntri = build_table()
    lines = [
        "// kt_mc_table.hpp -- GENERATED by kintinuous_amd/mc_table.py (python -m kintinuous_amd.mc_table); do not edit.",
        "// Marching-cubes case table of the mesh stage (kt_mesh.hip): the rule, the corner and edge numbering are documented there.",
        "// kt_mc_tri[case][t] packs triangle t as edge0 | edge1 << 4 | edge2 << 8; kt_mc_ntri[case] triangles per case.",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "#ifndef KT_MC_STORAGE",
        "#define KT_MC_STORAGE static const",
        "#endif",
        "",
        f"#define KT_MC_MAX_TRIS {MAX_TRIS}",
        "",
        "KT_MC_STORAGE uint8_t kt_mc_ntri[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(int(v)) for v in ntri[r:r + 32]) + ",")
    lines.append("};")
    lines.append("")
    lines.append(f"KT_MC_STORAGE uint16_t kt_mc_tri[256][{MAX_TRIS}] = {{")
    for case in range(256):
        words = []
        for t in range(MAX_TRIS):
            e = tri[case, t]
            words.append(0 if e[0] < 0 else int(e[0]) | (int(e[1]) << 4) | (int(e[2]) << 8))
        lines.append("    {" + ", ".join(f"0x{w:03x}" for w in words) + f"}},  // {case}")
    lines.append("};")
    return "\n".join(lines) + "\n"


def parse_header(text: str):
    """(tri[256][MAX_TRIS][3], ntri[256]) from the header's text (the tests compare it with build_table())."""
    import re
    body = text.split("kt_mc_ntri[256] = {", 1)[1].split("};", 1)[0]
    ntri = np.array([int(v) for v in re.findall(r"\d+", body)], dtype=np.uint8)
    body = text.split(f"kt_mc_tri[256][{MAX_TRIS}] = {{", 1)[1].split("};", 1)[0]
    words = [int(v, 16) for v in re.findall(r"0x([0-9a-f]+)", body)]
    tri = np.full((256, MAX_TRIS, 3), -1, dtype=np.int8)
    for case in range(256):
        for t in range(int(ntri[case])):
            w = words[case * MAX_TRIS + t]
            tri[case, t] = (w & 15, (w >> 4) & 15, (w >> 8) & 15)
    return tri, ntri


if __name__ == "__main__":
    with open(HEADER, "w") as f:
        f.write(header_text())
    print(HEADER)
