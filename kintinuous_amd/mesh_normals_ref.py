"""numpy restatement of the vertex normals of a mesh (kt_mesh_normals.hip, kt_mesh_normals / kt_mesh_normals_device): the definition the
device equals on every byte.

Input: n vertices (MESH_VERTEX_DTYPE) and m triangles (uint32 [m, 3]).  Output: n normals (float32 [n, 3]) and n_zero, the number of
vertices whose normal is (0, 0, 0).

Per triangle (i0, i1, i2) (include/kt_abi.h):
  - an index >= n is an error;
  - a triangle with two equal indices contributes nothing;
  - otherwise each of its three vertices must be valid: x, y, z finite and |coordinate| < 8192 (the simplification's rule);
  - in double, every operation rounded once: e1 = (double)v1 - (double)v0, e2 = (double)v2 - (double)v0 per axis,
    c = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), each component two products and one subtraction: (v1 - v0) x (v2 - v0),
    which points to F > 0 on a mesh of kt_extract_mesh and whose length is twice the triangle's area (the sum is area-weighted);
  - any |c component| >= 1 is an error (1 m^2);
  - q = (int64)rint(c * 2^32) per component, ties to even; the same q is added to the sums of i0, i1 and i2.
Per vertex, S = the three int64 sums over its triangles: all zero gives (0, 0, 0), counted in n_zero; otherwise d = (double)S per axis,
len = sqrt((dx dx + dy dy) + dz dz), normal = (float)(d / len) per axis.  A vertex that no triangle references is not validated and
gets (0, 0, 0).  n = 0 gives no normals whatever the triangles hold (they are not looked at); m = 0 gives n zero normals.

|q| <= 2^32, a vertex takes at most one q per triangle and m <= 2^29, so |S| <= 2^61: the sums cannot overflow, and integer addition
commutes, so the result does not depend on the order of the triangles.
"""
from __future__ import annotations

import numpy as np

from .mesh_ref import MESH_VERTEX_DTYPE

MAX_VERTICES = 1 << 29
MAX_TRIANGLES = 1 << 29
COORD_LIMIT = 8192.0
CROSS_LIMIT = 1.0
FIXED_ONE = float(1 << 32)


def face_terms(vertices, triangles):
    """(tri int64 [k, 3], q int64 [k, 3]): the triangles with three distinct indices and the term each adds to its three vertices;
    raises ValueError on an index out of range, an invalid referenced vertex or a triangle over the bound"""
    v = np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3).astype(np.int64)
    n = len(v)
    if n > MAX_VERTICES or len(tri) > MAX_TRIANGLES:
        raise ValueError("n <= 2^29 vertices and m <= 2^29 triangles")
    if n == 0:                                           # no vertex, no normal: the triangles are not looked at
        return np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64)
    if tri.size and int(tri.max()) >= n:
        raise ValueError("a triangle index out of range")
    tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]
    x = v["xyz"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(x).all(axis=1) & (np.abs(x) < COORD_LIMIT).all(axis=1)
    if not ok[tri].all():
        raise ValueError("an invalid vertex in a triangle: not finite or |coordinate| >= 8192")
    p0 = x[tri[:, 0]]
    e1, e2 = x[tri[:, 1]] - p0, x[tri[:, 2]] - p0
    c = np.empty((len(tri), 3), np.float64)
    for a in range(3):
        b, d = (a + 1) % 3, (a + 2) % 3
        c[:, a] = e1[:, b] * e2[:, d] - e1[:, d] * e2[:, b]
    if (np.abs(c) >= CROSS_LIMIT).any():
        raise ValueError("a triangle too large: a component of (v1 - v0) x (v2 - v0) of 1 m^2 or more")
    return tri, np.rint(c * FIXED_ONE).astype(np.int64)


def sums(vertices, triangles) -> np.ndarray:
    """int64 [n, 3]: every vertex's accumulated terms"""
    n = len(np.asarray(vertices).reshape(-1))
    tri, q = face_terms(vertices, triangles)
    S = np.zeros((n, 3), np.int64)
    for e in range(3):
        np.add.at(S, tri[:, e], q)
    return S


def finish(S):
    """(normals float32 [n, 3], n_zero) of the sums"""
    S = np.asarray(S, np.int64).reshape(-1, 3)
    zero = (S == 0).all(axis=1)
    d = S.astype(np.float64)
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    out = np.zeros((len(S), 3), np.float32)
    out[~zero] = (d[~zero] / length[~zero, None]).astype(np.float32)
    return out, int(zero.sum())


def normals(vertices, triangles):
    """(normals float32 [n, 3], n_zero)"""
    return finish(sums(vertices, triangles))
