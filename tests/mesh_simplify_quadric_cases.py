"""Cases shared by the quadric simplification's CPU and GPU tests (test_mesh_simplify_quadric_ref.py, test_gpu_mesh_simplify_quadric.py):
a brute-force twin on Python dicts, exact Python integers and scalar doubles, random lists whose triangles stay below the form's bound
(every quadric term below 1) and touch 1, 2 and 3 clusters, lists with clusters of chosen sizes, one cluster that takes every triangle,
the tilted plane, the offset cube, and an unquantised float64 version of the placement."""
import functools
import math

import numpy as np

import mesh_simplify_cases as mean_cases
from kintinuous_amd import mesh_ref, mesh_simplify_ref as ref

V = mesh_ref.MESH_VERTEX_DTYPE
SIZES = (0, 1, 63, 64, 65, 257, 4099)
CLUSTER_SIZES = mean_cases.CLUSTER_SIZES
DEFAULT_BIAS = 2.0 ** -6
same = mean_cases.same


def same4(got, want):
    """every byte of (vertices, triangles, span_first_out) and n_placed"""
    same(got[:3], want[:3])
    assert int(got[3]) == int(want[3]), (got[3], want[3])


# ---- the twin ----
def brute_members(vertices, span_first, cell):
    """(cluster of every vertex, members of every cluster in output order, cell index of every cluster), the clustering of
    mesh_simplify_cases.brute_simplify once more"""
    v = np.asarray(vertices)
    first = [int(x) for x in span_first]
    inv = 1.0 / float(np.float32(cell))
    members, order, s = {}, [], 0
    for i in range(len(v)):
        while first[s + 1] <= i:
            s += 1
        c = tuple(math.floor(float(x) * inv) for x in v["xyz"][i])
        if (s, c) not in members:
            members[(s, c)] = []
            order.append((s, c))
        members[(s, c)].append(i)
    cluster = [0] * len(v)
    for o, key in enumerate(order):
        for i in members[key]:
            cluster[i] = o
    return cluster, [members[key] for key in order], [key[1] for key in order]


def brute_sums(vertices, triangles, span_first, cell):
    """a list of nine exact Python integers per cluster"""
    v = np.asarray(vertices)
    n = len(v)
    c32 = float(np.float32(cell))
    cluster, members, kcell = brute_members(v, span_first, cell)
    S = [[0] * 9 for _ in members]
    P = [[float(x) for x in p] for p in v["xyz"]]
    for row in np.asarray(triangles).reshape(-1, 3):
        i = [int(x) for x in row]
        if max(i) >= n:
            raise ValueError("index")
        if i[0] == i[1] or i[1] == i[2] or i[0] == i[2]:
            continue
        r = i.index(min(i))
        i = i[r:] + i[:r]
        p0, p1, p2 = P[i[0]], P[i[1]], P[i[2]]
        e1 = [p1[a] - p0[a] for a in range(3)]
        e2 = [p2[a] - p0[a] for a in range(3)]
        c = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        if c == [0.0, 0.0, 0.0]:
            continue
        length = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        nh = [x / length for x in c]
        done = []
        for e in range(3):
            o = cluster[i[e]]
            if o in done:
                continue
            done.append(o)
            centre = [(float(k) + 0.5) * c32 for k in kcell[o]]
            rr = [p0[a] - centre[a] for a in range(3)]
            d = (nh[0] * rr[0] + nh[1] * rr[1]) + nh[2] * rr[2]
            terms = [c[0] * nh[0], c[0] * nh[1], c[0] * nh[2], c[1] * nh[1], c[1] * nh[2], c[2] * nh[2], c[0] * d, c[1] * d, c[2] * d]
            if not all(abs(t) < 1.0 for t in terms):
                raise ValueError("term")
            for k in range(9):
                S[o][k] += round(terms[k] * 4294967296.0)       # round(): ties to even, an exact integer
    return S


def brute_quadric(vertices, triangles, span_first, cell, bias):
    """the definition, one cluster at a time: (vertices_out, triangles_out, span_first_out, n_placed)"""
    b32 = np.float32(bias)
    if not (math.isfinite(float(b32)) and 2.0 ** -20 <= float(b32) <= 1.0):
        raise ValueError("bias")
    b = float(b32)
    v = np.asarray(vertices)
    if len(v) == 0:
        out, _, fo = mean_cases.brute_simplify(v, np.zeros((0, 3), np.uint32), span_first, cell)
        return out, np.zeros((0, 3), np.uint32), fo, 0
    out, tri, fo = mean_cases.brute_simplify(v, np.zeros((0, 3), np.uint32), span_first, cell)      # (raises on vertices and tables)
    S = brute_sums(v, triangles, span_first, cell)
    out, tri, fo = mean_cases.brute_simplify(v, triangles, span_first, cell)
    c32 = float(np.float32(cell))
    inv = 1.0 / c32
    _, members, kcell = brute_members(v, span_first, cell)
    placed = 0
    for o, idx in enumerate(members):
        if len(idx) == 1:
            continue
        k = len(idx)
        centre = [(float(a) + 0.5) * c32 for a in kcell[o]]
        m = []
        for a in range(3):
            Sq = sum(round(float(v["xyz"][i][a]) * 1048576.0) for i in idx)
            m.append(float((2 * Sq + k) // (2 * k)) * 2.0 ** -20 - centre[a])
        F = [float(x) for x in S[o]]
        t = (F[0] + F[3]) + F[5]
        lam = b * t
        M00, M11, M22, M01, M02, M12 = F[0] + lam, F[3] + lam, F[5] + lam, F[1], F[2], F[4]
        r0, r1, r2 = F[6] + lam * m[0], F[7] + lam * m[1], F[8] + lam * m[2]
        c00 = M11 * M22 - M12 * M12
        c01 = M02 * M12 - M01 * M22
        c02 = M01 * M12 - M02 * M11
        c11 = M00 * M22 - M02 * M02
        c12 = M01 * M02 - M00 * M12
        c22 = M00 * M11 - M01 * M01
        det = (M00 * c00 + M01 * c01) + M02 * c02
        if not (t > 0 and det > 0):
            continue
        x = [((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det]
        with np.errstate(over="ignore"):
            res = [np.float32(centre[a] + x[a]) for a in range(3)]
        if not all(math.isfinite(float(q)) for q in res):
            continue
        if any(math.floor(float(res[a]) * inv) != kcell[o][a] for a in range(3)):
            continue
        for a in range(3):
            out["xyz"][o][a] = res[a]
        placed += 1
    return out, tri, fo, placed


# ---- lists ----
def bounded_cell(n, per_cell):
    """a power of two at which mesh_simplify_cases.random_case stays within half a metre: every quadric term of every triangle between
    its vertices is then below 1 (|c| <= 3 D^2, |d| <= D sqrt(3) + cell at an extent D)"""
    side = max(int(round((n / per_cell) ** (1 / 3))), 1)
    return 2.0 ** math.floor(math.log2(0.5 / (2 * side + 10)))


def random_case(seed, n, n_spans=6, per_cell=3.0):
    """(vertices, triangles, span_first, cell): the vertices, colours and table of mesh_simplify_cases.random_case at bounded_cell; about
    2 n triangles between any three vertices (mostly three clusters), n / 2 inside one cluster where it has three members, n / 2 with two
    vertices of one cluster, and n / 8 each with a repeated index, with two vertices at one position (c = 0) and on a line (c = 0)"""
    cell = bounded_cell(n, per_cell)
    v, tri, first, _ = mean_cases.random_case(seed, n, n_spans, cell, per_cell)
    v = v.copy()
    if n < 3:
        return v, tri, first, cell
    rng = np.random.default_rng(seed + 1000)
    cl = ref.cluster_of(v["xyz"], first, cell)
    by = np.argsort(cl, kind="stable")
    start = np.searchsorted(cl[by], np.arange(cl.max() + 2))
    extra = []
    for a in rng.integers(0, n, n // 2 + 1):
        mem = by[start[cl[a]]:start[cl[a] + 1]]
        extra.append([a, mem[rng.integers(len(mem))], mem[rng.integers(len(mem))]])          # one cluster (or a repeated index)
        extra.append([rng.integers(n), a, mem[rng.integers(len(mem))]])                      # two clusters, mostly
    for a in rng.integers(0, n, n // 8 + 1):
        extra.append([a, a, rng.integers(n)])
    dup = rng.choice(n, size=min(2 * (n // 8 + 1), n - n % 2), replace=False).reshape(-1, 2)
    inside = cl[dup[:, 0]] == cl[dup[:, 1]]                  # (a copied position must not move a vertex to another cluster)
    v["xyz"][dup[inside, 1]] = v["xyz"][dup[inside, 0]]
    for a, b in dup:
        extra.append([a, rng.integers(n), b])                # c = 0 where the copy was made
    tri = np.concatenate([tri, np.array(extra, np.int64).astype(np.uint32)])
    return v, tri[rng.permutation(len(tri))], first, cell


def sized_clusters_case(seed=3, sizes=CLUSTER_SIZES, repeat=3):
    """clusters of exactly the given sizes (each `repeat` times), one cell of 2^-7 m each, members spread at random over the list, one
    span; 2 n triangles between any three vertices and 2 n inside a window of 64 cluster-sorted vertices"""
    rng = np.random.default_rng(seed)
    cell, cells = 2.0 ** -7, []
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
    where = np.argsort(perm)                                 # where[j]: the index of sorted vertex j
    near = where[np.clip(rng.integers(0, n, (2 * n, 1)) + rng.integers(0, 64, (2 * n, 3)), 0, n - 1)]
    tri = np.concatenate([rng.integers(0, n, (2 * n, 3)), near]).astype(np.uint32)
    return v, tri[rng.permutation(len(tri))], np.array([0, n], np.int64), cell


def one_cluster_case(n=4099, m=8000):
    """every vertex in one cell of half a metre, m triangles: every term goes to the same nine sums; n_out = 1, m_out = 0"""
    rng = np.random.default_rng(8)
    v = np.zeros(n, V)
    v["xyz"] = (-0.5 + rng.uniform(0.001, 0.499, (n, 3))).astype(np.float32)
    v["rgb"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return v, rng.integers(0, n, (m, 3)).astype(np.uint32), np.array([0, n], np.int64), 0.5


def many_spans_case(n=9001, S=3000):
    """a table of 3000 spans: above what the head pass stages in LDS"""
    rng = np.random.default_rng(3)
    v, tri, _, cell = random_case(77, n, per_cell=6.0)
    first = np.concatenate([[0], np.sort(rng.integers(0, n + 1, S - 1)), [n]]).astype(np.int64)
    return v, tri, first, cell


# ---- surfaces ----
def _mesh(xyz, tri):
    v = np.zeros(len(xyz), V)
    v["xyz"] = np.asarray(xyz, np.float64).astype(np.float32)
    v["rgb"] = 0x00808080
    return v, np.asarray(tri, np.uint32).reshape(-1, 3)


PLANE_NORMAL = np.array([0.3, -0.2, 1.0]) / math.sqrt(0.3 * 0.3 + 0.2 * 0.2 + 1.0)
PLANE_POINT = np.array([0.0137, 0.0137, 0.25])


@functools.lru_cache(maxsize=None)
def plane_patch(grid=40, size=0.6):
    """(vertices, triangles) of a grid x grid patch of the plane through PLANE_POINT with PLANE_NORMAL, `size` metres along x and y"""
    g = np.arange(grid + 1) * (size / grid)
    x, y = np.meshgrid(g, g, indexing="ij")
    x, y = x.reshape(-1) + PLANE_POINT[0], y.reshape(-1) + PLANE_POINT[1]
    z = PLANE_POINT[2] - (PLANE_NORMAL[0] * (x - PLANE_POINT[0]) + PLANE_NORMAL[1] * (y - PLANE_POINT[1])) / PLANE_NORMAL[2]
    i, j = np.meshgrid(np.arange(grid), np.arange(grid), indexing="ij")
    a = (i * (grid + 1) + j).reshape(-1)
    tri = np.concatenate([np.stack([a, a + grid + 1, a + grid + 2], axis=1), np.stack([a, a + grid + 2, a + 1], axis=1)])
    return _mesh(np.stack([x, y, z], axis=1), tri)


CUBE_OFFSET = 0.0137


@functools.lru_cache(maxsize=None)
def cube_mesh(grid=40, offset=CUBE_OFFSET):
    """(vertices, triangles) of the unit cube's surface, grid x grid squares per face, two triangles each, outward, shared vertices
    along the edges, every coordinate offset by `offset`"""
    index, xyz, tri = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(xyz)
            xyz.append(p)
        return index[p]

    for axis in range(3):
        for side in (0, grid):
            u, w = (axis + 1) % 3, (axis + 2) % 3
            for i in range(grid):
                for j in range(grid):
                    def at(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        return vid(tuple(p))
                    q = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]     # counter-clockwise seen from +axis
                    if side == 0:
                        q = q[::-1]
                    tri += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return _mesh(np.array(xyz, np.float64) / grid + offset, tri)


def cube_distance(xyz, offset=CUBE_OFFSET):
    """float64 distance of every point to the surface of the unit cube at `offset`"""
    u = np.asarray(xyz, np.float64) - offset
    outside = np.sqrt((np.maximum(np.maximum(-u, u - 1.0), 0.0) ** 2).sum(axis=1))
    inside = np.minimum(u, 1.0 - u).min(axis=1)
    return np.where(outside > 0, outside, np.maximum(inside, 0.0))


def multi_member(vertices, span_first, cell):
    """bool per output vertex: its cluster has more than one member"""
    return np.bincount(ref.cluster_of(np.asarray(vertices)["xyz"], span_first, cell)) > 1


def float64_quadric(vertices, triangles, span_first, cell, bias):
    """(xyz float64 [n_out, 3], solved bool [n_out]): the placement without the fixed point -- float64 sums of the terms, the float64
    mean of the members, numpy.linalg.solve -- for the clusters of more than one member whose system is regular"""
    v = np.asarray(vertices, V).reshape(-1)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3).astype(np.int64)
    x = v["xyz"].astype(np.float64)
    cl = ref.cluster_of(v["xyz"], span_first, cell)
    total = int(cl.max()) + 1
    size = np.bincount(cl, minlength=total)
    mean = np.stack([np.bincount(cl, x[:, a], total) for a in range(3)], axis=1) / size[:, None]
    tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]
    p0 = x[tri[:, 0]]
    c = np.cross(x[tri[:, 1]] - p0, x[tri[:, 2]] - p0)
    area2 = np.linalg.norm(c, axis=1)
    tri, p0, c, area2 = tri[area2 > 0], p0[area2 > 0], c[area2 > 0], area2[area2 > 0]
    nh = c / area2[:, None]
    A, rhs = np.zeros((total, 3, 3)), np.zeros((total, 3))
    tc = cl[tri]
    use = np.stack([np.ones(len(tri), bool), tc[:, 1] != tc[:, 0], (tc[:, 2] != tc[:, 0]) & (tc[:, 2] != tc[:, 1])], axis=1)
    for e in range(3):
        u = use[:, e]
        np.add.at(A, tc[u, e], area2[u, None, None] * nh[u, :, None] * nh[u, None, :])
        np.add.at(rhs, tc[u, e], (area2[u] * (nh[u] * p0[u]).sum(axis=1))[:, None] * nh[u])      # in world coordinates: A p = sum w n (n . v0)
    out, solved = mean.copy(), np.zeros(total, bool)
    for o in np.nonzero(size > 1)[0]:
        lam = float(np.float32(bias)) * np.trace(A[o])
        if lam > 0:
            out[o] = np.linalg.solve(A[o] + lam * np.eye(3), rhs[o] + lam * mean[o])
            solved[o] = True
    return out, solved
