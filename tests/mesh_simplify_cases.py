"""Cases shared by the mesh simplification's CPU and GPU tests (test_mesh_simplify_ref.py, test_gpu_mesh_simplify.py): random vertex
lists with a brute-force clustering on Python dicts and exact Python integers, lists with clusters of chosen sizes, the sphere mesh and
its welded split boxes, the directed-edge balance (P2) and the distance bounds (P3)."""
import functools
import math

import numpy as np

import mesh_weld_cases as wc
from kintinuous_amd import mesh_ref, mesh_simplify_ref, mesh_weld_ref

V = mesh_ref.MESH_VERTEX_DTYPE
SIZES = wc.SIZES
CLUSTER_SIZES = (1, 2, 63, 64, 65, 257, 2049)
VOXEL = 3.0 / 32                               # of the N = 32 sphere volume (3 m)
CELLS_IN_VOXELS = (1, 2, 3, 4, 8, 64)
same = wc.same


def brute_simplify(vertices, triangles, span_first, cell):
    """the definition, one vertex at a time, on Python floats (doubles) and integers: (vertices_out, triangles_out, span_first_out)"""
    v = np.asarray(vertices)
    n = len(v)
    first = [int(x) for x in span_first]
    c32 = float(np.float32(cell))
    if not (math.isfinite(c32) and c32 > 0):
        raise ValueError("cell")
    if first[0] != 0 or first[-1] != n or any(b < a for a, b in zip(first, first[1:])):
        raise ValueError("span table")
    inv = 1.0 / c32
    members, order, cluster = {}, [], []
    s = 0
    for i in range(n):
        while first[s + 1] <= i:       # skips empty spans
            s += 1
        xyz = [float(x) for x in v["xyz"][i]]
        if not all(math.isfinite(x) and abs(x) < 8192.0 for x in xyz):
            raise ValueError("vertex %d" % i)
        c = tuple(math.floor(x * inv) for x in xyz)
        if not all(-(1 << 19) <= a < (1 << 19) for a in c):
            raise ValueError("vertex %d: cell index" % i)
        if (s, c) not in members:
            members[(s, c)] = []
            order.append((s, c))           # heads in index order
        members[(s, c)].append(i)
    index = {key: k for k, key in enumerate(order)}
    heads = [members[key][0] for key in order]
    out = v[heads].copy() if n else v.copy()
    cluster = [0] * n
    for key in order:
        idx, o = members[key], index[key]
        for i in idx:
            cluster[i] = o
        k = len(idx)
        if k == 1:
            continue
        for a in range(3):
            S = sum(round(float(v["xyz"][i][a]) * 1048576.0) for i in idx)     # round(): ties to even, an exact integer
            out["xyz"][o][a] = np.float32(((2 * S + k) // (2 * k)) * 2.0 ** -20)
        word = 0
        for b in range(4):
            S = sum((int(v["rgb"][i]) >> (8 * b)) & 255 for i in idx)
            word |= ((2 * S + k) // (2 * k)) << (8 * b)
        out["rgb"][o] = word
    tri = []
    for row in np.asarray(triangles).reshape(-1, 3):
        a, b, c = (cluster[int(x)] for x in row)
        if a != b and b != c and a != c:
            tri.append([a, b, c])
    fo = [sum(1 for h in heads if h < f) for f in first]
    return out, np.array(tri, np.uint32).reshape(-1, 3), np.array(fo, np.int64)


def spans_with_empties(rng, n, n_spans):
    """a table of n_spans spans over n vertices: empty ones first, inside and last (n_spans >= 5)"""
    cuts = np.sort(rng.integers(0, n + 1, max(n_spans - 4, 1)))
    return np.concatenate([[0, 0], cuts, cuts[-1:], [n, n]]).astype(np.int64)


def random_case(seed, n, n_spans=6, cell=0.25, per_cell=3.0):
    """(vertices, triangles, span_first, cell): n vertices in random order over about n / per_cell cells around the origin (negative
    coordinates), a third of them exactly on a cell face (cell is a power of two, so x / cell is an integer there), some at 0.0 and
    -0.0; groups whose fixed-point sums are negative and tie at one half or fall between (q = -1, -2; -1, -1, -1, -2; ...), each in a
    cell of its own; colour bytes from 0 .. 3 for half the vertices (ties at one half) and any byte for the rest; a span table with
    empty spans first, inside and last, so that a cell's vertices fall into adjacent spans; about 2 n triangles"""
    rng = np.random.default_rng(seed)
    side = max(int(round((n / per_cell) ** (1 / 3))), 1)
    xyz = rng.uniform(-side / 2, side / 2, (n, 3)) * cell
    face = rng.random((n, 3)) < 1 / 3
    xyz[face] = np.round(xyz[face] / cell) * cell
    xyz = xyz.astype(np.float32)
    if n >= 8:
        xyz[0], xyz[1], xyz[2] = (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (-0.0, 0.0, cell / 2)
    # the tie groups: x = q 2^-20 with small negative q (cell -1 along x), y picks a cell per group far from the random ones
    at, u = 3, 2.0 ** -20
    for g, qs in enumerate(((-1, -2), (-1, -1, -1, -2), (-3, -4, -4, -4), (-1, -1, -2), (-7, -8), (-1, -2, -2, -2, -2, -2))):
        if at + len(qs) > n:
            break
        for q in qs:
            xyz[at] = (q * u, (side + 2 + g) * cell + (-q) * u, -(side + 2) * cell - q * u * 3)
            at += 1
    perm = rng.permutation(n)
    v = np.zeros(n, V)
    v["xyz"] = xyz[perm]
    rgb = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    small = rng.random(n) < 0.5
    rgb[small] &= np.uint32(0x03030303)
    v["rgb"] = rgb
    first = spans_with_empties(rng, n, n_spans) if n_spans >= 5 else np.linspace(0, n, n_spans + 1).astype(np.int64)
    tri = rng.integers(0, max(n, 1), (2 * n, 3)).astype(np.uint32)
    return v, tri, first, cell


def sized_clusters_case(seed=3, sizes=CLUSTER_SIZES, repeat=3):
    """clusters of exactly the given sizes (each `repeat` times), one cell each, their members spread at random over the list: one span"""
    rng = np.random.default_rng(seed)
    cell, cells = 0.125, []
    for r in range(repeat):
        for k, s in enumerate(sizes):
            cells += [r * len(sizes) + k] * s
    cells = np.array(cells)
    n = len(cells)
    xyz = np.stack([cells - 20.0, (cells % 7) - 3.0, -(cells % 5) + 0.0], axis=1) * cell + rng.uniform(0, cell, (n, 3)) * 0.999
    perm = rng.permutation(n)
    v = np.zeros(n, V)
    v["xyz"] = xyz[perm].astype(np.float32)
    v["rgb"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    tri = rng.integers(0, n, (2 * n, 3)).astype(np.uint32)
    return v, tri, np.array([0, n], np.int64), cell


def one_cluster_case(n=70001):
    """every vertex in one cell of one span: n_out = 1, m_out = 0"""
    rng = np.random.default_rng(8)
    v = np.zeros(n, V)
    v["xyz"] = (-1.0 + rng.uniform(0.001, 0.999, (n, 3))).astype(np.float32)
    v["rgb"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return v, rng.integers(0, n, (1000, 3)).astype(np.uint32), np.array([0, n], np.int64), 1.0


def many_spans_case(n=9001, S=3000):
    """a table of 3000 spans: above what the head pass stages in LDS"""
    rng = np.random.default_rng(3)
    v, tri, _, cell = random_case(77, n, per_cell=6.0)
    first = np.concatenate([[0], np.sort(rng.integers(0, n + 1, S - 1)), [n]]).astype(np.int64)
    return v, tri, first, cell


# ---- the sphere and its split boxes ----
@functools.lru_cache(maxsize=None)
def sphere_mesh(N=32):
    """(vertices, triangles) of mesh_ref.extract_mesh on mesh_weld_cases.sphere_volume(N): closed and oriented"""
    vol, col = wc.sphere_volume(N)
    v, t = mesh_ref.extract_mesh(vol, col, (3.0, 3.0, 3.0), (0, 0, 0), (0, 0, 0), (N - 1,) * 3, (0, 0, 0), N)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


@functools.lru_cache(maxsize=None)
def welded_split(axis, cut, N=32):
    """(vertices, triangles, span_first) of the two boxes of a split of the sphere, welded by the restatement: two spans, closed"""
    vol, col = wc.sphere_volume(N)
    parts = []
    for lo, hi in wc.split_boxes(N, axis, cut)[1:]:
        v, t, info = mesh_ref.extract_mesh(vol, col, (3.0, 3.0, 3.0), (0, 0, 0), lo, hi, (0, 0, 0), N, info=True)
        parts.append((v, t, mesh_weld_ref.edge_keys(info["owner"], info["axis"], (0, 0, 0))))
    v, k, t, first, times = wc.concat(*parts)
    wv, _, wt, wf = mesh_weld_ref.weld(v, k, t, first, times)
    return wv, wt, wf


def balanced(tris):
    """P2: every directed edge (a, b) occurs as often as (b, a)"""
    t = np.asarray(tris).astype(np.int64).reshape(-1, 3)
    if len(t) == 0:
        return True
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    K = int(d.max()) + 1
    fw, nf = np.unique(d[:, 0] * K + d[:, 1], return_counts=True)
    bw, nb = np.unique(d[:, 1] * K + d[:, 0], return_counts=True)
    return bool(np.array_equal(fw, bw) and np.array_equal(nf, nb))


def check_distances(v_in, span_first, cell, v_out):
    """P3: every input vertex within cell sqrt(3) of its representative, every representative within 2^-19 m of its cluster's cell"""
    c = mesh_simplify_ref.cluster_of(v_in["xyz"], span_first, cell)
    a, r = v_in["xyz"].astype(np.float64), v_out["xyz"].astype(np.float64)[c]
    assert np.sqrt(((a - r) ** 2).sum(axis=1)).max() <= float(np.float32(cell)) * math.sqrt(3.0)
    inv = 1.0 / float(np.float32(cell))
    lo = np.floor(a * inv) * float(np.float32(cell))
    hi = lo + float(np.float32(cell))
    assert (r >= lo - 2.0 ** -19).all() and (r <= hi + 2.0 ** -19).all()


# ---- a two-span mesh on the 20-node deformation graph of deform_cases ----
def deform_case():
    """(vertices, triangles, span_first, span_time, cell, graph name): 580 vertices along the graph's path in two spans"""
    import deform_cases as dc
    import deform_mesh_cases as mc
    rng = np.random.default_rng(21)
    nA, nB = 300, 280
    times = np.array([mc.span_times(20)[2], mc.span_times(20)[7]], np.uint64)
    xyz = dc.curve(rng.uniform(8, 11, nA + nB)) + rng.uniform(-0.5, 0.5, (nA + nB, 3))
    v = np.zeros(nA + nB, V)
    v["xyz"] = xyz.astype(np.float32)
    v["rgb"] = rng.integers(0, 1 << 32, nA + nB, dtype=np.uint64).astype(np.uint32)
    tri = np.concatenate([rng.integers(0, nA, (500, 3)), nA + rng.integers(0, nB, (450, 3))]).astype(np.uint32)
    return v, tri, np.array([0, nA, nA + nB], np.int64), times, 0.3, "m20_n64_c7"
