"""numpy restatement of the connected-component filter of the -m mesh (kt_mesh_components.hip, kt_mesh_components /
kt_mesh_components_device): the definition the device equals on every byte.

The definition (include/kt_abi.h):
  - input: n vertices (16 bytes each), m triangles (uint32[3]) and the span table of kt_mesh_weld (span_first only); an index >= n is an
    error;
  - two vertices are joined when one triangle holds both; every triangle joins its three indices, one with repeated indices included;
    position plays no part;
  - label[v] = the smallest vertex index of v's component;
  - the size of a component = the number of triangles whose FIRST index carries its label (duplicates count each time); a vertex that
    no triangle references is a component of size 0;
  - a component is kept when size >= min_triangles (0 keeps everything, 1 drops exactly the unreferenced vertices);
  - output vertices: those of kept components, in input order, untouched; output triangles: those of kept components, in input order,
    orientation kept, every index replaced by the number of kept vertices below it;
  - span_first_out[s] = the number of kept vertices below span_first[s];
  - labels: label[v] for every INPUT vertex; stats: (all components, the kept ones, the largest size).
With n = 0 the triangles are not looked at.
"""
from __future__ import annotations

import numpy as np

from .mesh_ref import MESH_VERTEX_DTYPE
from .mesh_simplify_ref import check_table

MAX_VERTICES = 1 << 29
MAX_TRIANGLES = 1 << 29


def labels_of(n, triangles) -> np.ndarray:
    """int64 [n]: the smallest index of each vertex's component, by label propagation to a fixed point: the smallest label a triangle
    sees goes to its three vertices and to the vertices that ARE its three labels (so whole groups move at once and the rounds stay
    few), then every label follows its own label (pointer jumping), until nothing changes.  A label is always a vertex of the same
    component and label[v] <= v; at the fixed point a triangle's vertices share one label and label[label] = label, so the label is
    constant on a component, and the component's smallest vertex can only have itself"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    label = np.arange(n, dtype=np.int64)
    if n == 0 or len(tri) == 0:
        return label
    flat = tri.reshape(-1)
    while True:
        seen = label[tri]
        low = np.repeat(seen.min(axis=1), 3)           # the smallest label a triangle sees ...
        new = label.copy()
        np.minimum.at(new, flat, low)                  # ... goes to its three vertices
        np.minimum.at(new, seen.reshape(-1), low)      # ... and to the three labels' own entries
        while True:                                    # label[v] <= v always, so following labels only goes down
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, label):
            return label
        label = new


def components(vertices, triangles, span_first, min_triangles):
    """(vertices_out MESH_VERTEX_DTYPE [n_out], triangles_out uint32 [m_out, 3], span_first_out int64 [S + 1], labels uint32 [n],
    stats = (components, kept components, largest size))"""
    v = np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3)
    n, k = len(v), int(min_triangles)
    if n > MAX_VERTICES or len(tri) > MAX_TRIANGLES:
        raise ValueError("n <= 2^29 vertices and m <= 2^29 triangles")
    if not 0 <= k < 1 << 32:
        raise ValueError("min_triangles is a uint32")
    f = check_table(n, span_first)
    if n == 0:
        return v.copy(), np.zeros((0, 3), np.uint32), np.zeros(len(f), np.int64), np.zeros(0, np.uint32), (0, 0, 0)
    if tri.size and int(tri.max()) >= n:
        raise ValueError("a triangle index out of range")
    label = labels_of(n, tri)
    size = np.bincount(label[tri[:, 0].astype(np.int64)], minlength=n)          # per label (non-roots stay at 0)
    root = label == np.arange(n)
    keep = size[label] >= k                                                     # per vertex
    new = np.cumsum(keep) - keep                                                # kept vertices below each index
    total = int(keep.sum())
    tkeep = keep[tri[:, 0].astype(np.int64)]
    tri_out = new[tri[tkeep].astype(np.int64)].astype(np.uint32).reshape(-1, 3)
    first_out = np.where(f < n, new[np.minimum(f, n - 1)], total).astype(np.int64)
    stats = (int(root.sum()), int((root & keep).sum()), int(size[root].max()))
    return v[keep].copy(), tri_out, first_out, label.astype(np.uint32), stats
