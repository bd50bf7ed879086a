"""numpy restatement of the weld pass (kt_mesh_weld.hip, kt_mesh_weld / kt_mesh_weld_device): the definition the device equals on
every byte, and the edge key of the mesh stage (kt_extract_mesh_keyed).

The key of a vertex (include/kt_abi.h): (gz + 2^19) << 42 | (gy + 2^19) << 22 | (gx + 2^19) << 2 | axis, g = the owner voxel in
logical coordinates + real_voxel_wrap, axis 0, 1 or 2; the top two bits are zero.

The weld:
  - the occurrences of a key are taken in index order; an occurrence starts a new group when it is the first of its key, or when its
    span's time and the previous occurrence's span's time differ by more than max_gap (the larger minus the smaller, on uint64;
    NO_GATE = 2^64 - 1 never cuts);
  - the representative of a vertex is the first vertex of its group; kept vertices are the representatives, in input order, their 16
    bytes and keys untouched;
  - every triangle index becomes the new index of its vertex's representative; triangles are neither dropped nor reordered;
  - span_first_out[s] = the number of kept vertices below span_first[s].
"""
from __future__ import annotations

import numpy as np

from .mesh_ref import MESH_VERTEX_DTYPE

KEY_BIAS = 1 << 19
KEY_BITS = 62
NO_GATE = (1 << 64) - 1
MAX_VERTICES = 1 << 29


def edge_keys(owner, axis, real_voxel_wrap) -> np.ndarray:
    """uint64 keys of vertices owned by logical voxels `owner` (int [n, 3] as x, y, z) along `axis` (int [n])"""
    g = np.asarray(owner, np.int64).reshape(-1, 3) + np.asarray(real_voxel_wrap, np.int64).reshape(1, 3)
    assert ((g >= -KEY_BIAS) & (g < KEY_BIAS)).all(), "a global voxel outside [-2^19, 2^19)"
    u = (g + KEY_BIAS).astype(np.uint64)
    a = np.asarray(axis, np.int64).reshape(-1)
    assert ((a >= 0) & (a <= 2)).all()
    return (u[:, 2] << np.uint64(42)) | (u[:, 1] << np.uint64(22)) | (u[:, 0] << np.uint64(2)) | a.astype(np.uint64)


def key_fields(keys):
    """(g int64 [n, 3] as x, y, z; axis int64 [n]) of uint64 keys"""
    k = np.asarray(keys, np.uint64).reshape(-1)
    m = np.uint64((1 << 20) - 1)
    g = np.stack([(k >> np.uint64(2)) & m, (k >> np.uint64(22)) & m, (k >> np.uint64(42)) & m], axis=1).astype(np.int64) - KEY_BIAS
    return g, (k & np.uint64(3)).astype(np.int64)


def check_spans(n, span_first, span_time):
    f = np.asarray(span_first, np.uint64).reshape(-1)
    t = np.asarray(span_time, np.uint64).reshape(-1)
    if len(f) != len(t) + 1:
        raise ValueError("span_first has one entry more than span_time")
    if int(f[0]) != 0 or int(f[-1]) != n or (len(f) > 1 and (f[1:] < f[:-1]).any()):
        raise ValueError("a span table starts at 0, does not decrease and ends at n")
    if n > 0 and len(t) == 0:
        raise ValueError("vertices without a span")
    return f.astype(np.int64), t


def span_of(span_first, idx):
    """the span of each vertex index: the last s with span_first[s] <= i (empty spans share a first entry with the next span)"""
    f = np.asarray(span_first, np.int64).reshape(-1)
    return np.searchsorted(f[:-1], np.asarray(idx, np.int64), side="right") - 1


def representatives(keys, span_first, span_time, max_gap=NO_GATE) -> np.ndarray:
    """int64 [n]: each vertex's representative"""
    k = np.asarray(keys, np.uint64).reshape(-1)
    n = len(k)
    f, t = check_spans(n, span_first, span_time)
    if n == 0:
        return np.zeros(0, np.int64)
    if (k >> np.uint64(KEY_BITS)).any():
        raise ValueError("a key with a top bit set")
    order = np.argsort(k, kind="stable")
    sk = k[order]
    st = t[span_of(f, order)]
    a, b = st[1:], st[:-1]
    gap = np.where(a > b, a - b, b - a)
    head = np.ones(n, bool)
    head[1:] = (sk[1:] != sk[:-1]) | (gap > np.uint64(max_gap))
    hp = np.maximum.accumulate(np.where(head, np.arange(n), 0))
    rep = np.empty(n, np.int64)
    rep[order] = order[hp]
    return rep


def weld(vertices, keys, triangles, span_first, span_time, max_gap=NO_GATE):
    """(vertices_out MESH_VERTEX_DTYPE [n_out], keys_out uint64 [n_out], triangles_out uint32 [m, 3], span_first_out int64 [S + 1])"""
    v = np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1)
    k = np.asarray(keys, np.uint64).reshape(-1)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3)
    n = len(v)
    if len(k) != n or n > MAX_VERTICES:
        raise ValueError("n keys for n <= 2^29 vertices")
    rep = representatives(k, span_first, span_time, max_gap)
    f, _ = check_spans(n, span_first, span_time)
    keep = rep == np.arange(n)
    new = np.cumsum(keep) - keep                     # kept vertices below each index
    total = int(keep.sum())
    assert tri.size == 0 or int(tri.max()) < n
    tri_out = new[rep[tri.astype(np.int64)]].astype(np.uint32).reshape(-1, 3)
    first_out = np.where(f < n, new[np.minimum(f, max(n - 1, 0))] if n else 0, total).astype(np.int64)
    return v[keep].copy(), k[keep].copy(), tri_out, first_out
