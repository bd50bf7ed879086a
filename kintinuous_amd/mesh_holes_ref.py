"""numpy restatement of the boundary report and small-hole fill of the -m mesh (kt_mesh_holes.hip, kt_mesh_holes / kt_mesh_holes_device):
the definition the device equals on every byte, on every call.

The definition (include/kt_abi.h):
  - input: n vertices (16 bytes each), m triangles (uint32[3]), the span table of kt_mesh_weld (span_first only) and max_edges in
    [0, 256]; an index >= n is an error;
  - triangle t, corner k gives half-edge h = 3 t + k from a = tri[t][k] to b = tri[t][(k + 1) % 3]; a triangle with two equal indices is
    degenerate: it has no half-edges, it is counted, and it is copied to the output like any other;
  - an undirected edge {a, b} with f half-edges min -> max and r the other way is interior when f == r == 1, boundary when f + r == 1 and
    non-manifold otherwise; a non-manifold edge is counted once and BLOCKS both its vertices;
  - out[v], in[v] count the boundary half-edges that leave and enter v; a vertex with in + out > 0 and not in == out == 1 is COMPLEX;
  - the boundary half-edges join their two vertices into boundary components; the label is the component's smallest vertex index.  A
    component none of whose vertices is COMPLEX or BLOCKED is a simple loop (one cycle) of L = its vertex count edges; any other is an
    open component, counted and never filled;
  - a simple loop is filled when 3 <= L <= max_edges and every vertex of it is valid (x, y, z finite, |coordinate| < 8192);
  - the centre of a filled loop: per coordinate q = rint((double)x * 2^32) as int64, S = the sum of q over the loop (exact: |S| < 2^53),
    c = (float)((double)S / (double)L * 2^-32); each of the four bytes of rgb is (2 * sum + L) / (2 L) in integers;
  - one fill triangle (b, a, centre) per boundary half-edge a -> b of a filled loop;
  - output vertices stay in their spans: span s holds its input vertices in input order, then the centres of the filled loops whose label
    lies in span s, ascending by label; span_first_out is the new first vertex per span;
  - output triangles: the m input triangles in input order through the index map, then the fill triangles ascending by h;
  - loop_out[v]: the label for a vertex of a simple loop, OPEN (0xfffffffe) for a boundary vertex of an open component, NONE (0xffffffff)
    otherwise;
  - stats: boundary_edges, nonmanifold_edges, degenerate_triangles, loops, open_components, filled, longest (edges of the longest simple
    loop), new_vertices, new_triangles.
With n = 0 the triangles are not looked at.  max_edges of 0, 1 or 2 fills nothing: the call only reports.
"""
from __future__ import annotations

import numpy as np

from .mesh_components_ref import labels_of
from .mesh_ref import MESH_VERTEX_DTYPE
from .mesh_simplify_ref import check_table

MAX_VERTICES = 1 << 29
MAX_TRIANGLES = 1 << 29
MAX_EDGES = 256
COORD_LIMIT = 8192.0
FIXED_ONE = float(1 << 32)
OPEN = 0xfffffffe
NONE = 0xffffffff
STAT_NAMES = ("boundary_edges", "nonmanifold_edges", "degenerate_triangles", "loops", "open_components", "filled", "longest", "new_vertices", "new_triangles")


def half_edges(n, triangles):
    """(a int64 [3 m], b int64 [3 m], degenerate bool [m]): half-edge h = 3 t + k runs from a[h] to b[h]"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    degenerate = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    return t.reshape(-1), t[:, [1, 2, 0]].reshape(-1), degenerate


def classify(n, triangles):
    """(boundary half-edges ascending int64 [B], non-manifold edges int64 [K, 2], degenerate bool [m])"""
    a, b, degenerate = half_edges(n, triangles)
    h = np.flatnonzero(np.repeat(~degenerate, 3))
    if len(h) == 0:
        return np.zeros(0, np.int64), np.zeros((0, 2), np.int64), degenerate
    key = np.minimum(a, b) << 32 | np.maximum(a, b)
    order = h[np.argsort(key[h], kind="stable")]
    sk = key[order]
    head = np.ones(len(sk), bool)
    head[1:] = sk[1:] != sk[:-1]
    start = np.flatnonzero(head)
    length = np.diff(np.append(start, len(sk)))
    f = np.add.reduceat((a[order] < b[order]).astype(np.int64), start)
    r = length - f
    single = length == 1
    odd = ~single & ~((f == 1) & (r == 1))
    nm = sk[start[odd]]
    return np.sort(order[start[single]]), np.stack([nm >> 32, nm & 0xffffffff], axis=1), degenerate


def valid_vertices(v) -> np.ndarray:
    x = v["xyz"]
    return (np.isfinite(x) & (np.abs(x) < np.float32(COORD_LIMIT))).all(axis=1)


def span_of(f, i):
    """the last s in [0, S) with f[s] <= i (kt_span_of)"""
    return np.searchsorted(f[:-1], i, side="right") - 1


def holes(vertices, triangles, span_first, max_edges):
    """(vertices_out MESH_VERTEX_DTYPE [n_out], triangles_out uint32 [m_out, 3], span_first_out int64 [S + 1], loop_out uint32 [n],
    stats: the nine of STAT_NAMES)"""
    v = np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3)
    n, m, k = len(v), len(tri), int(max_edges)
    if n > MAX_VERTICES or m > MAX_TRIANGLES:
        raise ValueError("n <= 2^29 vertices and m <= 2^29 triangles")
    if not 0 <= k <= MAX_EDGES:
        raise ValueError("max_edges lies in [0, 256]")
    f = check_table(n, span_first)
    if n == 0:
        return v.copy(), np.zeros((0, 3), np.uint32), np.zeros(len(f), np.int64), np.zeros(0, np.uint32), (0,) * 9
    if tri.size and int(tri.max()) >= n:
        raise ValueError("a triangle index out of range")
    a, b, _ = half_edges(n, tri)
    bh, nonmanifold, degenerate = classify(n, tri)
    blocked = np.zeros(n, bool)
    blocked[nonmanifold.reshape(-1)] = True
    out_n, in_n = np.bincount(a[bh], minlength=n), np.bincount(b[bh], minlength=n)
    bv = out_n + in_n > 0                                                        # the boundary vertices
    cplx = bv & ~((out_n == 1) & (in_n == 1))
    label = labels_of(n, np.stack([a[bh], b[bh], b[bh]], axis=1))
    root = bv & (label == np.arange(n))
    length = np.bincount(label[bv], minlength=n)                                 # per label
    is_open = np.zeros(n, bool)
    is_open[label[bv & (cplx | blocked)]] = True                                 # per label
    invalid = np.zeros(n, bool)
    invalid[label[bv & ~valid_vertices(v)]] = True
    simple = root & ~is_open
    filled = simple & ~invalid & (length >= 3) & (length <= k)                   # per root
    rank = np.cumsum(filled) - filled                                            # filled labels below each index
    total = int(filled.sum())
    below = np.append(rank, total)                                               # ... and below n
    # placement
    idx = np.arange(n)
    new = idx + below[f[span_of(f, idx)]]
    fl = np.flatnonzero(filled)
    centre_at = np.zeros(n, np.int64)
    centre_at[fl] = f[span_of(f, fl) + 1] + rank[fl]
    vout = np.zeros(n + total, MESH_VERTEX_DTYPE)
    vout[new] = v
    # centres
    mine = np.flatnonzero(bv & filled[label])                                    # the vertices of filled loops
    if total:
        L = length[fl]
        q = np.rint(v["xyz"][mine].astype(np.float64) * FIXED_ONE).astype(np.int64)
        S = np.zeros((n, 3), np.int64)
        np.add.at(S, label[mine], q)
        c = (S[fl].astype(np.float64) / L[:, None].astype(np.float64) * (1.0 / FIXED_ONE)).astype(np.float32)
        rgb = v["rgb"][mine].astype(np.int64)
        C = np.zeros((n, 4), np.int64)
        np.add.at(C, label[mine], np.stack([(rgb >> (8 * j)) & 255 for j in range(4)], axis=1))
        byte = (2 * C[fl] + L[:, None]) // (2 * L[:, None])
        centre = np.zeros(total, MESH_VERTEX_DTYPE)
        centre["xyz"] = c
        centre["rgb"] = (byte[:, 0] | byte[:, 1] << 8 | byte[:, 2] << 16 | byte[:, 3] << 24).astype(np.uint32)
        vout[centre_at[fl]] = centre
    # triangles
    fh = bh[filled[label[a[bh]]]]                                                # ascending by h
    fan = np.stack([new[b[fh]], new[a[fh]], centre_at[label[a[fh]]]], axis=1)
    tri_out = np.concatenate([new[tri.astype(np.int64)].reshape(-1, 3), fan.reshape(-1, 3)]).astype(np.uint32)
    loop_out = np.where(bv, np.where(is_open[label], OPEN, label), NONE).astype(np.uint32)
    stats = (len(bh), len(nonmanifold), int(degenerate.sum()), int(simple.sum()), int((root & is_open).sum()), total,
             int(length[simple].max()) if simple.any() else 0, total, len(fh))
    return vout, tri_out, (f + below[f]).astype(np.int64), loop_out, stats
