"""Cases shared by the vertex normals' CPU and GPU tests (test_mesh_normals_ref.py, test_gpu_mesh_normals.py): random triangle lists,
fans around a hub vertex, cancelling pairs, the sphere mesh, and two implementations written apart from the restatement:
brute_normals (the definition, one triangle at a time on Python floats and exact Python integers) and float64_normals (np.add.at of the
unquantised crosses, normalised in float64: no fixed point)."""
import functools
import math

import numpy as np

import mesh_simplify_cases as sc
import mesh_weld_cases as wc
from kintinuous_amd import mesh_ref

V = mesh_ref.MESH_VERTEX_DTYPE
TRIANGLE_COUNTS = wc.SIZES                      # (0, 1, 63, 64, 65, 257, 4099, 70001)
FAN_SIZES = (1, 2, 63, 64, 65, 257, 2049, 70001)
OFFSETS = ((0.0, 0.0, 0.0), (8000.0, -8000.0, 8000.0))
SPHERE_CENTRE = (np.array([15.3, 16.6, 15.55]) + 0.5) * (3.0 / 32) - 1.5   # of mesh_weld_cases.sphere_volume(32) in metres: voxel i sits at (i + 0.5) edge - half the volume (mesh_ref)
sphere_mesh = sc.sphere_mesh


def brute_normals(vertices, triangles):
    """the definition: (normals float32 [n, 3], n_zero); raises ValueError naming the cause"""
    v = np.asarray(vertices)
    n = len(v)
    S = [[0, 0, 0] for _ in range(n)]
    for row in np.asarray(triangles).reshape(-1, 3) if n else ():       # n = 0: the triangles are not looked at
        i = [int(x) for x in row]
        if any(a >= n for a in i):
            raise ValueError("index")
        if i[0] == i[1] or i[1] == i[2] or i[0] == i[2]:
            continue
        p = [[float(x) for x in v["xyz"][a]] for a in i]
        if not all(math.isfinite(x) and abs(x) < 8192.0 for q in p for x in q):
            raise ValueError("vertex")
        e1 = [p[1][a] - p[0][a] for a in range(3)]
        e2 = [p[2][a] - p[0][a] for a in range(3)]
        c = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        if any(abs(x) >= 1.0 for x in c):
            raise ValueError("large")
        q = [round(x * 4294967296.0) for x in c]        # round(): ties to even, an exact integer
        for a in i:
            for k in range(3):
                S[a][k] += q[k]
    out = np.zeros((n, 3), np.float32)
    n_zero = 0
    for a in range(n):
        if S[a] == [0, 0, 0]:
            n_zero += 1
            continue
        assert all(abs(s) <= 1 << 61 for s in S[a])
        d = [float(s) for s in S[a]]                    # int -> float: rounded to nearest even
        length = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        out[a] = [np.float32(x / length) for x in d]
    return out, n_zero


def float64_sums(vertices, triangles):
    """(sum float64 [n, 3], valence int64 [n]): the unquantised crosses of the triangles with three distinct indices, added per vertex"""
    v = np.asarray(vertices)
    t = np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    x = v["xyz"].astype(np.float64)
    c = np.cross(x[t[:, 1]] - x[t[:, 0]], x[t[:, 2]] - x[t[:, 0]])
    S, k = np.zeros((len(v), 3)), np.zeros(len(v), np.int64)
    for e in range(3):
        np.add.at(S, t[:, e], c)
        np.add.at(k, t[:, e], 1)
    return S, k


def float64_normals(vertices, triangles):
    """float64 [n, 3]: the sums of float64_sums normalised (zero where the sum is zero)"""
    S, _ = float64_sums(vertices, triangles)
    L = np.sqrt((S * S).sum(axis=1))
    return np.where(L[:, None] > 0, S / np.where(L > 0, L, 1.0)[:, None], 0.0)


def random_case(seed, m, offset=(0.0, 0.0, 0.0)):
    """(vertices, triangles): m triangles over about m / 2 vertices in a 0.5 m box at `offset` (every cross stays below 0.25 < 1); among
    them triangles with repeated indices, duplicate triangles, and vertices that no triangle references -- two of those invalid"""
    rng = np.random.default_rng(seed)
    n = 0 if m == 0 else max(m // 2, 3) + 4
    v = np.zeros(n, V)
    v["xyz"] = (np.asarray(offset) + rng.uniform(-0.25, 0.25, (n, 3))).astype(np.float32)
    v["rgb"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    used = max(n - 4, 0)                                 # the last four vertices are never referenced
    tri = rng.integers(0, max(used, 1), (m, 3)).astype(np.uint32)
    if m >= 63:
        tri[5] = tri[4]                                  # a duplicate
        tri[7] = tri[6][[0, 2, 1]]                       # ... and a cancelling one
        tri[9, 1] = tri[9, 0]                            # repeated indices
        tri[11] = tri[11, 0]
        v["xyz"][n - 1, 0] = np.nan                      # unreferenced: not validated
        v["xyz"][n - 2, 2] = 8192.0
    return v, tri


def fan_case(k, seed=5):
    """k triangles that share vertex 0 (the hub), each with two vertices of its own on a 0.3 m ring: 2 k + 1 vertices"""
    rng = np.random.default_rng(seed + k)
    n = 2 * k + 1
    v = np.zeros(n, V)
    v["xyz"][0] = (0.01, -0.02, 0.03)
    ang = rng.uniform(0, 2 * np.pi, (k, 2))
    for e in range(2):
        v["xyz"][1 + e::2] = np.stack([0.3 * np.cos(ang[:, e]), 0.3 * np.sin(ang[:, e]), rng.uniform(-0.1, 0.1, k)], axis=1).astype(np.float32)
    v["rgb"] = np.arange(n, dtype=np.uint32)
    tri = np.stack([np.zeros(k, np.uint32), 1 + 2 * np.arange(k, dtype=np.uint32), 2 + 2 * np.arange(k, dtype=np.uint32)], axis=1)
    return v, tri


def cancelling_case():
    """the sphere mesh with every triangle (a, b, c) followed by (a, c, b), and three vertices more in a sliver whose q rounds to 0"""
    v, t = sphere_mesh()
    n = len(v)
    extra = np.zeros(3, V)
    extra["xyz"] = [(0.0, 0.0, 0.0), (2.0 ** -17, 0.0, 0.0), (0.0, 2.0 ** -17, 0.0)]      # cross = 2^-34: q = rint(2^-2) = 0
    vv = np.concatenate([v, extra])
    tt = np.concatenate([np.stack([t, t[:, [0, 2, 1]]], axis=1).reshape(-1, 3), np.array([[n, n + 1, n + 2]], np.uint32)]).astype(np.uint32)
    return vv, tt


def plane_case(flip, side=9):
    """a side x side grid in z = 0.5 at a spacing of 2^-4 m, two triangles per cell, one winding: the crosses are exact"""
    j, i = np.mgrid[0:side, 0:side]
    v = np.zeros(side * side, V)
    v["xyz"] = np.stack([i.ravel() / 16.0 - 0.25, j.ravel() / 16.0 + 1.0, np.full(side * side, 0.5)], axis=1).astype(np.float32)
    a = (j[:-1, :-1] * side + i[:-1, :-1]).ravel()
    t = np.concatenate([np.stack([a, a + 1, a + side], axis=1), np.stack([a + 1, a + side + 1, a + side], axis=1)]).astype(np.uint32)
    return v, (t[:, [0, 2, 1]] if flip else t)


def as_bytes(normals):
    return np.ascontiguousarray(normals).view(np.uint8).reshape(-1)


# ---- the PLY with normals ----
PLY_NVERTEX = np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("rgb", np.uint8, 3)])
PLY_FACE = np.dtype([("n", np.uint8), ("idx", "<i4", 3)])
PLY_PROPERTIES = ["property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz",
                  "property uchar red", "property uchar green", "property uchar blue", "property list uchar int vertex_indices"]


def read_ply_normals(path):
    """the binary PLY of kt_host_save_ply_normals: (vertices PLY_NVERTEX, faces (n, 3) int32)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int([l for l in head if l.startswith("element vertex ")][0].split()[2])
    nf = int([l for l in head if l.startswith("element face ")][0].split()[2])
    assert [l for l in head if l.startswith("property ")] == PLY_PROPERTIES
    assert head.index("property uchar blue") < head.index("element face %d" % nf)
    assert PLY_NVERTEX.itemsize == 27 and len(raw) == end + 27 * nv + PLY_FACE.itemsize * nf
    v = np.frombuffer(raw, PLY_NVERTEX, nv, end)
    f = np.frombuffer(raw, PLY_FACE, nf, end + 27 * nv)
    assert (f["n"] == 3).all()
    return v, f["idx"]
