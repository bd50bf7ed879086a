"""numpy restatement of Taubin's lambda|mu smoothing of the -m mesh (kt_mesh_smooth.hip, kt_mesh_smooth / kt_mesh_smooth_device): the
definition the device equals on every byte, on every call.

The definition (include/kt_abi.h):
  - input: n vertices (16 bytes each), m triangles (uint32[3]), steps in [0, 64], lambda in (0, 1], mu in [-1.1, 1] (both float, compared
    as floats) and mode 0 or 1; output: n vertices in the same order with the same rgb;
  - half-edges as in mesh_holes_ref: a triangle with two equal indices has none; an index >= n is an error;
  - an undirected edge with exactly one half-edge each way is interior, any other rim (boundary or non-manifold); a vertex is rim when it
    is an end of a rim edge; an undirected edge counts once however many triangles hold it;
  - neighbours: an interior vertex has the other ends of all its edges; a rim vertex has none with mode 0 (it is pinned) and the other ends
    of its rim edges with mode 1; d = the number of neighbours, d > 65535 is an error, a vertex with d = 0 does not move;
  - a vertex that is an end of a half-edge must be valid: x, y, z finite and |coordinate| < 8192; any other is not validated;
  - state: q = rint((double)x * 2^32) as int64 per coordinate;
  - a half-step with factor f ((double)lambda or (double)mu), for every vertex with d > 0, from the state before the half-step:
    S = the int64 sum of the neighbours' q, D = S - d q, q' = q + (int64)rint(f * ((double)D / (double)d)): the conversion, the division
    and the product rounded once each, ties to even; |q'| >= 2^45 is an error;
  - a step is the lambda half-step, then the mu half-step;
  - output: a vertex with d = 0, and every vertex when steps = 0, keeps its 16 bytes; any other gets (float)((double)q * 2^-32);
  - stats: rim_vertices, moved_vertices (those with d > 0 when steps > 0), unique_edges.
With n = 0 the triangles are not looked at.
"""
from __future__ import annotations

import numpy as np

from .mesh_holes_ref import half_edges, valid_vertices
from .mesh_ref import MESH_VERTEX_DTYPE

MAX_VERTICES = 1 << 29
MAX_TRIANGLES = 1 << 29
MAX_STEPS = 64
MAX_VALENCE = 65535
FIXED_ONE = float(1 << 32)
RANGE = 1 << 45
LAMBDA, MU = 0.5, -0.53                                   # the driver's -mt
STAT_NAMES = ("rim_vertices", "moved_vertices", "unique_edges")


def check_params(steps, lam, mu, mode):
    """(steps, (double)lambda, (double)mu, mode) of a valid call"""
    lam, mu = np.float32(lam), np.float32(mu)
    if not (int(steps) == steps and 0 <= steps <= MAX_STEPS):
        raise ValueError("steps lies in [0, 64]")
    if not (np.float32(0.0) < lam <= np.float32(1.0)):
        raise ValueError("lambda lies in (0, 1]")
    if not (np.float32(-1.1) <= mu <= np.float32(1.0)):
        raise ValueError("mu lies in [-1.1, 1]")
    if mode not in (0, 1):
        raise ValueError("mode is 0 or 1")
    return int(steps), float(lam), float(mu), int(mode)


def edges(n, triangles):
    """the unique undirected edges: (lo int64 [E], hi int64 [E], interior bool [E])"""
    a, b, degenerate = half_edges(n, triangles)
    h = np.flatnonzero(np.repeat(~degenerate, 3))
    if len(h) == 0:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, bool)
    a, b = a[h], b[h]
    key = np.minimum(a, b) << 32 | np.maximum(a, b)
    order = np.argsort(key, kind="stable")
    sk = key[order]
    head = np.ones(len(sk), bool)
    head[1:] = sk[1:] != sk[:-1]
    start = np.flatnonzero(head)
    length = np.diff(np.append(start, len(sk)))
    f = np.add.reduceat((a[order] < b[order]).astype(np.int64), start)
    return sk[start] >> 32, sk[start] & 0xffffffff, (f == 1) & (length == 2)


def adjacency(n, triangles, mode):
    """(src int64 [A] ascending, dst int64 [A], degree int64 [n], rim bool [n], referenced bool [n], E): dst is a neighbour of src"""
    lo, hi, interior = edges(n, triangles)
    rim = np.zeros(n, bool)
    rim[lo[~interior]] = True
    rim[hi[~interior]] = True
    referenced = np.zeros(n, bool)
    referenced[lo] = True
    referenced[hi] = True
    src, dst, along = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([~interior, ~interior])
    keep = ~rim[src] | (along & (mode == 1))
    src, dst = src[keep], dst[keep]
    order = np.argsort(src, kind="stable")
    return src[order], dst[order], np.bincount(src, minlength=n).astype(np.int64), rim, referenced, len(lo)


def half_step(q, dst, start, rows, d, f):
    """q int64 [n, 3] after one half-step with factor f; rows: the vertices with d > 0, start: the first entry of each"""
    S = np.add.reduceat(q[dst], start, axis=0)
    D = S - d[:, None] * q[rows]
    qn = q.copy()
    qn[rows] = q[rows] + np.rint(f * (D.astype(np.float64) / d[:, None].astype(np.float64))).astype(np.int64)
    if (np.abs(qn[rows]) >= RANGE).any():
        raise ValueError("a coordinate left the range of 8192 m")
    return qn


def smooth(vertices, triangles, steps, lam=LAMBDA, mu=MU, mode=0):
    """(vertices_out MESH_VERTEX_DTYPE [n], stats: the three of STAT_NAMES)"""
    v = np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3)
    n, m = len(v), len(tri)
    if n > MAX_VERTICES or m > MAX_TRIANGLES:
        raise ValueError("n <= 2^29 vertices and m <= 2^29 triangles")
    steps, lam, mu, mode = check_params(steps, lam, mu, mode)
    out = v.copy()
    if n == 0:
        return out, (0, 0, 0)
    if tri.size and int(tri.max()) >= n:
        raise ValueError("a triangle index out of range")
    src, dst, degree, rim, referenced, E = adjacency(n, tri, mode)
    if (referenced & ~valid_vertices(v)).any():
        raise ValueError("a triangle's vertex that is not finite or has a coordinate of 8192 m or more")
    if (degree > MAX_VALENCE).any():
        raise ValueError("a valence over the bound of 65535")
    rows = np.flatnonzero(degree > 0)
    if steps == 0 or len(rows) == 0:
        return out, (int(rim.sum()), 0, E)
    ok = valid_vertices(v)
    q = np.zeros((n, 3), np.int64)
    q[ok] = np.rint(v["xyz"][ok].astype(np.float64) * FIXED_ONE).astype(np.int64)
    start = np.cumsum(degree) - degree
    for _ in range(steps):
        q = half_step(q, dst, start[rows], rows, degree[rows], lam)
        q = half_step(q, dst, start[rows], rows, degree[rows], mu)
    out["xyz"][rows] = (q[rows].astype(np.float64) * (1.0 / FIXED_ONE)).astype(np.float32)
    return out, (int(rim.sum()), len(rows), E)
