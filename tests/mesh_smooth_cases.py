"""Cases shared by the smoothing pass's CPU and GPU tests (test_mesh_smooth_ref.py, test_gpu_mesh_smooth.py): a tetrahedron whole and minus
a face, the hole pass's random grid patches (deleted, duplicated, flipped, degenerate and fin triangles under a vertex permutation and a
triangle shuffle) with invalid vertices among the unreferenced ones, the N = 32 sphere, closed fans around a hub up to the valence bound
and one past it, a flat grid, and the independent check of the restatement (adjacency as Python sets built triangle by triangle, sums in
exact Python integers, the three float operations on Python floats)."""
import functools
import math
from collections import Counter

import numpy as np

import mesh_holes_cases as hc
import mesh_normals_cases as nc
import mesh_simplify_cases as sc
from kintinuous_amd import mesh_ref, mesh_smooth_ref as ref

V = mesh_ref.MESH_VERTEX_DTYPE
SIZES = (0, 1, 63, 64, 65, 257, 4099)           # triangles of the grid patches; the GPU tests add 70001
OFFSETS = nc.OFFSETS                            # the origin and near (8000, -8000, 8000)
STEPS = (0, 1, 2, 10)
MODES = (0, 1)
HUBS = (3, 64, 65535)                           # rim vertices of the closed fans; 65536 is the valence error
LAMBDA, MU = ref.LAMBDA, ref.MU
SPHERE_CENTRE = nc.SPHERE_CENTRE


def as_bytes(v):
    return np.ascontiguousarray(v).view(np.uint8).reshape(-1)


def moved_to(v, offset):
    out = v.copy()
    out["xyz"] = (out["xyz"].astype(np.float64) + np.asarray(offset)).astype(np.float32)
    return out


def tetra_case(closed=True):
    v, tri, _ = hc.tetra_case()
    return v, (np.concatenate([tri, [[1, 3, 2]]]).astype(np.uint32) if closed else tri)


@functools.lru_cache(maxsize=None)
def _patch(m):
    v, tri, _ = hc.random_case(m + 1, m)
    loose = np.setdiff1d(np.arange(len(v)), tri)
    if m >= 63:                                 # unreferenced vertices that are invalid: not validated, copied byte for byte
        v["xyz"][loose[0], 0] = np.nan
        v["xyz"][loose[1], 2] = 8192.0
        v["xyz"][loose[2], 1] = -np.inf
    return v, tri


def patch_case(m):
    v, tri = _patch(m)
    return v.copy(), tri.copy()


def hub_case(k):
    """k triangles (0, i, i + 1) around the hub 0, closed: every spoke is interior, so the hub is interior with valence k; the k rim
    vertices are rim, each with two rim edges"""
    rng = np.random.default_rng(700 + k)
    v = np.zeros(k + 1, V)
    a = 2.0 * np.pi * np.arange(k) / k
    v["xyz"][1:] = np.stack([0.3 * np.cos(a), 0.3 * np.sin(a), rng.uniform(-0.05, 0.05, k)], axis=1).astype(np.float32)
    v["xyz"][0] = (0.05, -0.02, 0.1)
    v["rgb"] = np.arange(k + 1, dtype=np.uint32) * np.uint32(2654435761)
    i = np.arange(k, dtype=np.int64)
    tri = np.stack([np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % k], axis=1)
    return v, tri[rng.permutation(k)].astype(np.uint32)


def flat_case(rows=9, cols=12):
    v, tri = hc.grid(rows, cols)
    return v, tri.astype(np.uint32)


def left_range_case():
    """the closed fan of 3 with the hub at x = 8191.9 and the rim at x = 8000, lambda 0.5 and mu -1.1, rims pinned: the lambda half-step
    takes the hub to about 8095.95, the mu half-step to about 8095.95 + 1.1 * 95.95 = 8201.5, past the range"""
    v, tri = hub_case(3)
    v["xyz"][:, 0] = 8000.0
    v["xyz"][0, 0] = 8191.9
    return v, tri, dict(steps=1, lam=0.5, mu=-1.1, mode=0)


def noisy_sphere():
    """the N = 32 sphere's vertices scaled radially by 1 + 0.01 * normal -> (vertices, triangles)"""
    v, tri = sc.sphere_mesh()
    v = v.copy()
    rng = np.random.default_rng(11)
    x = v["xyz"].astype(np.float64) - SPHERE_CENTRE
    v["xyz"] = (SPHERE_CENTRE + x * (1.0 + 0.01 * rng.standard_normal(len(v)))[:, None]).astype(np.float32)
    return v, tri


def radii(v):
    return np.sqrt(((v["xyz"].astype(np.float64) - SPHERE_CENTRE) ** 2).sum(axis=1))


def small_cases():
    """[(name, vertices, triangles)] at the origin: everything but the large hubs"""
    out = [("tetra", *tetra_case(True)), ("open tetra", *tetra_case(False))]
    out += [("patch %d" % m, *patch_case(m)) for m in SIZES]
    out.append(("sphere", *sc.sphere_mesh()))
    out += [("hub %d" % k, *hub_case(k)) for k in HUBS if k < 1000]
    return out


@functools.lru_cache(maxsize=None)
def _want(name, offset, steps, mode):
    v, tri = case(name, offset)
    return ref.smooth(v, tri, steps, LAMBDA, MU, mode)


def want(name, offset, steps, mode):
    """the restatement's answer for a named case, computed once"""
    out, stats = _want(name, offset, steps, mode)
    return out.copy(), stats


@functools.lru_cache(maxsize=None)
def _case(name, offset):
    if name.startswith("hub "):
        v, tri = hub_case(int(name.split()[1]))
    elif name.startswith("patch "):
        v, tri = patch_case(int(name.split()[1]))
    else:
        v, tri = {n: (a, b) for n, a, b in small_cases()}[name]
    return moved_to(v, offset), tri


def case(name, offset=OFFSETS[0]):
    v, tri = _case(name, tuple(offset))
    return v.copy(), tri.copy()


def names():
    return [n for n, _, _ in small_cases()] + ["hub %d" % k for k in HUBS if k >= 1000]


# ---- the independent check --------------------------------------------------------------------------------------------------------------
def check(vertices, triangles, steps_wanted, lam=LAMBDA, mu=MU, mode=0):
    """The definition, written apart from the restatement: {steps: (vertices_out, stats)} for every steps of steps_wanted; raises ValueError
    naming the cause"""
    v = np.asarray(vertices)
    n = len(v)
    if n == 0:
        return {s: (v.copy(), (0, 0, 0)) for s in steps_wanted}
    forward, ends = Counter(), set()
    for row in np.asarray(triangles).reshape(-1, 3).tolist():
        if any(a >= n for a in row):
            raise ValueError("index")
        if len(set(row)) < 3:
            continue
        for a, b in ((row[0], row[1]), (row[1], row[2]), (row[2], row[0])):
            forward[(a, b)] += 1
            ends |= {a, b}
    undirected = {(min(e), max(e)) for e in forward}
    interior = {e for e in undirected if forward[e] == 1 and forward[(e[1], e[0])] == 1}
    rim = set()
    for e in undirected - interior:
        rim |= set(e)
    near = [set() for _ in range(n)]
    for e in undirected:
        for x, y in (e, e[::-1]):
            if x not in rim or (e not in interior and mode == 1):
                near[x].add(y)
    xyz = [[float(c) for c in p] for p in v["xyz"]]
    if not all(math.isfinite(c) and abs(c) < 8192.0 for x in ends for c in xyz[x]):
        raise ValueError("vertex")
    if any(len(s) > 65535 for s in near):
        raise ValueError("valence")
    moving = [x for x in range(n) if near[x]]
    near = [tuple(s) for s in near]
    q = {x: [round(c * 4294967296.0) for c in xyz[x]] for x in ends}      # round(): ties to even, an exact integer
    factors = (float(np.float32(lam)), float(np.float32(mu)))
    out = {}
    for step in range(max(steps_wanted) + 1):
        if step in steps_wanted:
            o = v.copy()
            if step > 0:
                for x in moving:
                    o["xyz"][x] = [np.float32(float(c) * 2.0 ** -32) for c in q[x]]
            out[step] = (o, (len(rim), len(moving) if step > 0 else 0, len(undirected)))
        if step == max(steps_wanted):
            break
        for f in factors:
            new = {}
            for x in moving:
                d = len(near[x])
                row = []
                for c in range(3):
                    S = sum(q[y][c] for y in near[x])
                    D = S - d * q[x][c]
                    assert abs(S) < 1 << 61 and abs(d * q[x][c]) < 1 << 61 and abs(D) < 1 << 62       # what the int64 definition rests on
                    row.append(q[x][c] + round(f * (float(D) / float(d))))     # int -> float: rounded to nearest even
                if any(abs(c) >= 1 << 45 for c in row):
                    raise ValueError("range")
                new[x] = row
            q.update(new)
    return out
