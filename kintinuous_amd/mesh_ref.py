"""numpy restatement of the mesh stage (kt_mesh.hip, kt_extract_mesh): topology, vertex ownership, order, and the positions and
colour words in exact float32 steps, so that the GPU result can be compared bit for bit.

Semantics (include/kt_abi.h, kt_extract_mesh):
  - a box of CELLS [lo, hi) per axis, 0 <= lo <= hi <= N - 1; cell (x, y, z) has the corners (x..x+1, y..y+1, z..z+1) in logical
    coordinates, stored at ((x + wrap_x) % N) + ((y + wrap_y) % N) * N + ((z + wrap_z) % N) * N * N;
  - a voxel is valid when its weight is non-zero and its tsdf F != 1.f (kt_extract_kernel's rule); a cell is meshed when all eight
    corners are valid; a corner is inside when F < 0 (case bit i for corner (x + (i & 1), y + (i >> 1 & 1), z + (i >> 2 & 1)));
  - one vertex per crossed edge adjacent to a meshed cell of the box, owned by the edge's lower endpoint and its axis; its position
    and colour word are those kt_extract_kernel computes for that (voxel, axis) pair;
  - vertices in the order (owner z, y, x, axis); triangles by cell (z, y, x), then table order within the cell.
"""
from __future__ import annotations

import numpy as np

from . import mc_table

MESH_VERTEX_DTYPE = np.dtype([("xyz", np.float32, 3), ("rgb", np.uint32)])
assert MESH_VERTEX_DTYPE.itemsize == 16

_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = mc_table.build_table()
    return _TABLE


def fma32(a, b, c):
    """Correctly rounded float32 fma: the product is exact in float64; the sum is rounded to odd in float64 (TwoSum error and a
    one-ulp nudge), and the final rounding to float32 is then the single rounding of a*b + c."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.uint64)
    even = (bits & np.uint64(1)) == 0
    nudge = (err != 0) & even
    s = np.where(nudge, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def unpack_tsdf(v):
    return np.asarray(v, np.int16).astype(np.float32) / np.float32(32767)


def logical(vol, col, wrap, N):
    """(tsdf float32 [z, y, x], colour uint8 [z, y, x, 4]) in logical coordinates."""
    vol = np.asarray(vol).reshape(N, N, N)
    col = np.asarray(col).reshape(N, N, N, 4)
    ix = [(np.arange(N) + int(wrap[k])) % N for k in range(3)]
    sel = np.ix_(ix[2], ix[1], ix[0])
    return unpack_tsdf(vol[sel]), col[sel]


def vertex_positions(F0, F1, c0, c1, base, axis, volume_size, N, real_wrap):
    """Positions and colour words of the extraction's point for base voxels `base` (int [n, 3] as x, y, z) along `axis` (int [n]);
    F0 / c0 of the base voxel, F1 / c1 of the far one (kt_extract_kernel and its store_point_type)."""
    N32 = np.float32(N)
    cell = np.array([np.float32(volume_size[k]) / N32 for k in range(3)], dtype=np.float32)
    V = (base.astype(np.float32) + np.float32(0.5)) * cell[None, :]
    aF, aFn = np.abs(F0), np.abs(F1)
    d_inv = np.float32(1.0) / (aF + aFn)
    ax_cell = cell[axis]
    Va = V[np.arange(len(axis)), axis]
    Vn = Va + ax_cell
    along = np.where(axis == 2, fma32(Vn, aF, Va * aFn), fma32(Va, aFn, Vn * aF)) * d_inv
    P = V.copy()
    P[np.arange(len(axis)), axis] = along
    out = np.empty((len(axis), 3), dtype=np.float32)
    for k in range(3):
        off = np.float32(real_wrap[k]) * cell[k]
        half = (cell[k] * N32) / np.float32(2)
        out[:, k] = (P[:, k] + off) - half
    rgb = (c1[:, 0].astype(np.uint32) | (c1[:, 1].astype(np.uint32) << 8) | (c1[:, 2].astype(np.uint32) << 16)
           | (c0[:, 3].astype(np.uint32) << 24))
    return out, rgb


def extract_mesh(vol, col, volume_size, voxel_wrap, lo, hi, real_voxel_wrap, N, info=False):
    """(vertices MESH_VERTEX_DTYPE[n_v], triangles uint32[n_t, 3]) of the box of cells [lo, hi).  With info=True a third item:
    {"owner": int [n_v, 3] logical x, y, z of each vertex's owner voxel, "axis": int [n_v], "strict": bool [n_v] (the edge changes
    sign strictly -- no endpoint with F == 0 -- so kt_extract_kernel emits the same point), "cells": int [n_t, 3] the cell of each
    triangle}."""
    lo = [int(v) for v in lo]
    hi = [int(v) for v in hi]
    for k in range(3):
        assert 0 <= lo[k] <= hi[k] <= N - 1, (lo, hi, N)
    verts = np.zeros(0, MESH_VERTEX_DTYPE)
    tris = np.zeros((0, 3), np.uint32)
    if any(hi[k] == lo[k] for k in range(3)):
        if info:
            return verts, tris, {"owner": np.zeros((0, 3), np.int64), "axis": np.zeros(0, np.int64), "strict": np.zeros(0, bool),
                                 "cells": np.zeros((0, 3), np.int64)}
        return verts, tris
    F, C = logical(vol, col, voxel_wrap, N)
    # the voxel box [lo, hi] (inclusive), arrays indexed [z, y, x]
    sl = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
    Fb, Cb = F[sl], C[sl]
    valid = (Cb[..., 3] != 0) & (Fb != np.float32(1.0))
    inside = Fb < 0
    nz, ny, nx = Fb.shape          # voxels; cells are one fewer
    cz, cy, cx = nz - 1, ny - 1, nx - 1
    meshed = np.ones((cz, cy, cx), bool)
    case = np.zeros((cz, cy, cx), np.int64)
    for i in range(8):
        dx, dy, dz = i & 1, (i >> 1) & 1, (i >> 2) & 1
        s = (slice(dz, dz + cz), slice(dy, dy + cy), slice(dx, dx + cx))
        meshed &= valid[s]
        case |= inside[s].astype(np.int64) << i
    # meshed cells padded to the voxel box (cells at the upper faces do not exist)
    mp = np.zeros((nz + 1, ny + 1, nx + 1), bool)   # mp[z + 1, y + 1, x + 1] = meshed cell (x, y, z); the rest False
    mp[1:cz + 1, 1:cy + 1, 1:cx + 1] = meshed

    def cell_at(dz, dy, dx):   # meshed flag of cell (x + dx, y + dy, z + dz) for every voxel (x, y, z) of the box, dx.. in {-1, 0}
        return mp[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]

    flags = np.zeros((nz, ny, nx, 3), bool)
    far_in = [np.zeros_like(inside) for _ in range(3)]
    far_in[0][:, :, :-1] = inside[:, :, 1:]
    far_in[1][:, :-1, :] = inside[:, 1:, :]
    far_in[2][:-1, :, :] = inside[1:, :, :]
    adj = [cell_at(0, 0, 0) | cell_at(0, -1, 0) | cell_at(-1, 0, 0) | cell_at(-1, -1, 0),    # x edges: cells (x, y - j, z - k)
           cell_at(0, 0, 0) | cell_at(0, 0, -1) | cell_at(-1, 0, 0) | cell_at(-1, 0, -1),    # y edges: cells (x - i, y, z - k)
           cell_at(0, 0, 0) | cell_at(0, 0, -1) | cell_at(0, -1, 0) | cell_at(0, -1, -1)]    # z edges: cells (x - i, y - j, z)
    for a in range(3):
        flags[..., a] = adj[a] & (inside != far_in[a])
    vidx = np.full(flags.shape, -1, np.int64)
    nzf = np.nonzero(flags.reshape(-1))[0]
    vidx.reshape(-1)[nzf] = np.arange(len(nzf))
    # vertex positions
    zz, yy, xx, aa = np.unravel_index(nzf, flags.shape)
    base = np.stack([xx + lo[0], yy + lo[1], zz + lo[2]], axis=1)
    step = np.eye(3, dtype=np.int64)[aa]
    far = base + step
    fz, fy, fx = far[:, 2] - lo[2], far[:, 1] - lo[1], far[:, 0] - lo[0]
    pos, rgb = vertex_positions(Fb[zz, yy, xx], Fb[fz, fy, fx], Cb[zz, yy, xx], Cb[fz, fy, fx], base, aa, volume_size, N,
                                real_voxel_wrap)
    verts = np.zeros(len(nzf), MESH_VERTEX_DTYPE)
    verts["xyz"] = pos
    verts["rgb"] = rgb
    # triangles
    tri_tab, ntri = table()
    cz_i, cy_i, cx_i = np.nonzero(meshed)
    cases = case[cz_i, cy_i, cx_i]
    tris = np.zeros(0, np.uint32)
    tcell = np.zeros((0, 3), np.int64)
    if len(cases):
        nt = ntri[cases].astype(np.int64)
        edges = tri_tab[cases].astype(np.int64)            # [cells, MAX_TRIS, 3]
        keep = np.arange(mc_table.MAX_TRIS)[None, :] < nt[:, None]
        ebase = np.array([b for b, _ in mc_table.EDGES], np.int64)
        eaxis = np.array([a for _, a in mc_table.EDGES], np.int64)
        e = np.where(edges < 0, 0, edges)
        b = ebase[e]
        ox, oy, oz = b & 1, (b >> 1) & 1, (b >> 2) & 1
        idx = vidx[cz_i[:, None, None] + oz, cy_i[:, None, None] + oy, cx_i[:, None, None] + ox, eaxis[e]]
        tris = idx[keep]
        assert (tris >= 0).all()
        tris = tris.astype(np.uint32)
        tcell = np.stack([cx_i, cy_i, cz_i], axis=1)[np.nonzero(keep)[0]] + np.array(lo)[None, :]
    if info:
        F0, F1 = Fb[zz, yy, xx], Fb[fz, fy, fx]
        strict = ((F0 > 0) & (F1 < 0)) | ((F0 < 0) & (F1 > 0))
        return verts, tris.reshape(-1, 3), {"owner": base, "axis": aa.astype(np.int64), "strict": strict, "cells": tcell}
    return verts, tris.reshape(-1, 3)

