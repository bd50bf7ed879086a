"""numpy restatement of the mesh simplification by vertex clustering (kt_mesh_simplify.hip, kt_mesh_simplify / kt_mesh_simplify_device):
the definition the device equals on every byte.

The cell of a vertex (include/kt_abi.h): inv = 1 / (double)cell once; per axis c = floor((double)x * inv).  A vertex is valid when x, y, z
are finite, |coordinate| < 8192 and every c lies in [-2^19, 2^19); key = (cz + 2^19) << 40 | (cy + 2^19) << 20 | (cx + 2^19).  An invalid
vertex has the key INVALID_KEY (bit 63 set); any such vertex fails the call.

The clusters:
  - the occurrences of a key are taken in index order; an occurrence starts a new cluster when it is the first of its key or when its
    span differs from the previous occurrence's span: a cluster is one cell of one span; its head is its first vertex;
  - output vertices are one per cluster, in the order of their heads' indices; span_first_out[s] = the number of heads below
    span_first[s];
  - the representative, integers only: per member and axis q = rint((double)x * 2^20) (ties to even) as int64, S = the sum over the
    cluster, k = the member count, mean = floor((2 S + k) / (2 k)) (half up, FLOOR division), the coordinate (float)((double)mean * 2^-20);
    each of the four bytes of the colour word by the same rule on its own sum; a cluster of one member keeps its 16 bytes untouched;
  - every triangle index becomes its vertex's cluster index; a triangle with two equal indices is dropped; the survivors keep their
    order and orientation; duplicate survivors stay.
"""
from __future__ import annotations

import numpy as np

from .mesh_ref import MESH_VERTEX_DTYPE
from .mesh_weld_ref import check_spans, span_of

KEY_BIAS = 1 << 19
INVALID_KEY = 1 << 63
MAX_VERTICES = 1 << 29
COORD_LIMIT = 8192.0
FIXED_ONE = float(1 << 20)


def check_cell(cell) -> float:
    """1 / (double)(float)cell"""
    c = np.float32(cell)
    if not np.isfinite(c) or not c > 0:
        raise ValueError("cell is a finite float above zero")
    return 1.0 / float(c)


def check_table(n, span_first) -> np.ndarray:
    """the span table as int64 [S + 1] (the weld's rules; the simplification reads no times)"""
    f = np.asarray(span_first).reshape(-1)
    if len(f) == 0:
        raise ValueError("a span table has at least one entry")
    return check_spans(n, f, np.zeros(len(f) - 1, np.uint64))[0]


def cell_keys(xyz, cell) -> np.ndarray:
    """uint64 keys of float32 positions [n, 3]; INVALID_KEY where the vertex is not valid"""
    inv = check_cell(cell)
    x = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(x).all(axis=1) & (np.abs(x) < COORD_LIMIT).all(axis=1)
        c = np.floor(np.where(ok[:, None], x, 0.0) * inv)
    ok &= ((c >= -KEY_BIAS) & (c < KEY_BIAS)).all(axis=1)
    u = (np.where(ok[:, None], c, 0.0).astype(np.int64) + KEY_BIAS).astype(np.uint64)
    key = (u[:, 2] << np.uint64(40)) | (u[:, 1] << np.uint64(20)) | u[:, 0]
    return np.where(ok, key, np.uint64(INVALID_KEY))


def clusters(xyz, span_first, cell):
    """(order int64 [n]: the stable sort of the keys; head bool [n]: sorted entry j starts a cluster; rep int64 [n]: each vertex's head)"""
    key = cell_keys(xyz, cell)
    n = len(key)
    f = check_table(n, span_first)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool), np.zeros(0, np.int64)
    if (key >> np.uint64(63)).any():
        raise ValueError("an invalid vertex: not finite, |coordinate| >= 8192 or a cell index outside [-2^19, 2^19)")
    order = np.argsort(key, kind="stable")
    sk, ss = key[order], span_of(f, order)
    head = np.ones(n, bool)
    head[1:] = (sk[1:] != sk[:-1]) | (ss[1:] != ss[:-1])
    hp = np.maximum.accumulate(np.where(head, np.arange(n), 0))
    rep = np.empty(n, np.int64)
    rep[order] = order[hp]
    return order, head, rep


def cluster_of(xyz, span_first, cell) -> np.ndarray:
    """int64 [n]: the output vertex of each input vertex"""
    _, _, rep = clusters(xyz, span_first, cell)
    keep = rep == np.arange(len(rep))
    return (np.cumsum(keep) - keep)[rep]


def mean_half_up(S, k):
    """floor((2 S + k) / (2 k)) on int64"""
    S, k = np.asarray(S, np.int64), np.asarray(k, np.int64)
    return (2 * S + k) // (2 * k)


def simplify(vertices, triangles, span_first, cell):
    """(vertices_out MESH_VERTEX_DTYPE [n_out], triangles_out uint32 [m_out, 3], span_first_out int64 [S + 1])"""
    v = np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3)
    n = len(v)
    if n > MAX_VERTICES:
        raise ValueError("n <= 2^29 vertices")
    order, head, rep = clusters(v["xyz"], span_first, cell)
    f = check_table(n, span_first)
    if n == 0:
        assert tri.size == 0
        return v.copy(), tri.copy(), np.zeros(len(f), np.int64)
    keep = rep == np.arange(n)
    new = np.cumsum(keep) - keep                     # heads below each index
    total = int(keep.sum())
    starts = np.nonzero(head)[0]
    k = np.diff(np.concatenate([starts, [n]])).astype(np.int64)
    dest = new[order[starts]]                        # the output index of each cluster, in sorted order
    out = v[keep].copy()                             # clusters of one member: untouched
    many = k > 1
    q = np.rint(v["xyz"].astype(np.float64) * FIXED_ONE).astype(np.int64)[order]
    S = np.add.reduceat(q, starts, axis=0)
    xyz = (mean_half_up(S, k[:, None]).astype(np.float64) * (1.0 / FIXED_ONE)).astype(np.float32)
    b = np.ascontiguousarray(v["rgb"]).view(np.uint8).reshape(n, 4).astype(np.int64)[order]
    B = mean_half_up(np.add.reduceat(b, starts, axis=0), k[:, None])
    rgb = (B[:, 0] | B[:, 1] << 8 | B[:, 2] << 16 | B[:, 3] << 24).astype(np.uint32)
    out["xyz"][dest[many]] = xyz[many]
    out["rgb"][dest[many]] = rgb[many]
    assert tri.size == 0 or int(tri.max()) < n
    t = new[rep[tri.astype(np.int64)]].reshape(-1, 3)
    alive = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    first_out = np.where(f < n, new[np.minimum(f, n - 1)], total).astype(np.int64)
    return out, t[alive].astype(np.uint32), first_out
