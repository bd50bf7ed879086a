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

The quadric form (kt_mesh_simplify_quadric / kt_mesh_simplify_quadric_device, simplify_quadric below; Lindstrom 2000): clusters, heads,
output order, span_first_out, colour bytes, the triangle map, the dropped triangles and the rule of the cluster of one are those above;
only the xyz of a cluster with more than one member can differ.  It takes a float32 bias, finite and in [2^-20, 1].
  Per input triangle: an index >= n is an error; one with two equal indices adds nothing; otherwise its indices are rotated so that the
    smallest comes first (v0, v1, v2; orientation kept), so the result depends on neither a triangle's rotation nor the list's order.
  In double, every operation rounded once: e1 = (double)v1 - (double)v0, e2 = (double)v2 - (double)v0 per axis, c = e1 x e2 as
    mesh_normals_ref forms it (c_a = e1_b e2_d - e1_d e2_b), len = sqrt((cx cx + cy cy) + cz cz); c == (0, 0, 0) adds nothing;
    nh = c / len per axis.  The six terms A = (cx nhx, cx nhy, cx nhz, cy nhy, cy nhz, cz nhz) belong to the triangle.
  For every DISTINCT cluster among the clusters of v0, v1, v2, once per cluster: k_a = floor((double)x_a * inv) of the vertex that names
    the cluster (every member of a cluster has the same k), o_a = ((double)k_a + 0.5) * (double)cell, r = (double)v0 - o,
    d = (nhx rx + nhy ry) + nhz rz, the three terms b = (cx d, cy d, cz d).  A term that is not |term| < 1 is an error (so is a NaN);
    q = (int64)rint(term * 2^32), ties to even, is added to the cluster's nine int64 sums (xx, xy, xz, yy, yz, zz, bx, by, bz).
    m <= 2^29, so |S| <= 2^61; integer addition commutes.
  Per cluster of more than one member, in double: mean_q = the integer mean above, m_a = (double)mean_q_a * 2^-20 - o_a,
    t = ((double)Sxx + (double)Syy) + (double)Szz, lam = (double)bias * t,
    M00 = (double)Sxx + lam, M11 = (double)Syy + lam, M22 = (double)Szz + lam, M01 = (double)Sxy, M02 = (double)Sxz, M12 = (double)Syz,
    r_a = (double)Sb_a + lam * m_a,
    c00 = M11 M22 - M12 M12, c01 = M02 M12 - M01 M22, c02 = M01 M12 - M02 M11, c11 = M00 M22 - M02 M02, c12 = M01 M02 - M00 M12,
    c22 = M00 M11 - M01 M01, det = (M00 c00 + M01 c01) + M02 c02,
    x0 = ((c00 r0 + c01 r1) + c02 r2) / det, x1 = ((c01 r0 + c11 r1) + c12 r2) / det, x2 = ((c02 r0 + c12 r1) + c22 r2) / det,
    out_a = (float)(o_a + x_a).  The cluster is PLACED when t > 0, det > 0, every out_a is finite and floor((double)out_a * inv) == k_a on
    all three axes; otherwise it keeps the mean's bytes.  n_placed counts the placed clusters.
  The bias pulls the minimiser towards the mean where the planes leave it free (along an edge, within a plane); on a smooth noisy surface
  the minimiser wanders tangentially and is no better than the mean.
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
QUADRIC_ONE = float(1 << 32)
QUADRIC_LIMIT = 1.0
BIAS_MIN = 2.0 ** -20
MAX_TRIANGLES = 1 << 29                          # of the quadric form: the bound behind |S| <= 2^61


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


# ---- the quadric form ----
def check_bias(bias) -> float:
    """(double)(float)bias"""
    b = np.float32(bias)
    if not np.isfinite(b) or not (np.float32(BIAS_MIN) <= b <= np.float32(1.0)):
        raise ValueError("bias is a finite float in [2^-20, 1]")
    return float(b)


def cell_centres(k, cell) -> np.ndarray:
    """o = ((double)k + 0.5) * (double)(float)cell of cell indices k (float64 or integer [.., 3])"""
    return (np.asarray(k, np.float64) + 0.5) * float(np.float32(cell))


def quadric_terms(vertices, triangles, span_first, cell):
    """(cluster int64 [p], q int64 [p, 9]): every (triangle, distinct cluster) pair's cluster and the nine terms it adds, in the
    order xx, xy, xz, yy, yz, zz, bx, by, bz; raises ValueError on an index out of range and on a term that is not below 1"""
    v = np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3).astype(np.int64)
    n = len(v)
    if n > MAX_VERTICES or len(tri) > MAX_TRIANGLES:
        raise ValueError("n <= 2^29 vertices and m <= 2^29 triangles")
    inv = check_cell(cell)
    cl = cluster_of(v["xyz"], span_first, cell)
    if n == 0:                                           # no vertex: the triangles are not looked at
        return np.zeros(0, np.int64), np.zeros((0, 9), np.int64)
    if tri.size and int(tri.max()) >= n:
        raise ValueError("a triangle index out of range")
    tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]
    lo = np.argmin(tri, axis=1)
    tri = np.take_along_axis(tri, (lo[:, None] + np.arange(3)) % 3, axis=1)      # the smallest index first, orientation kept
    x = v["xyz"].astype(np.float64)
    p0 = x[tri[:, 0]]
    e1, e2 = x[tri[:, 1]] - p0, x[tri[:, 2]] - p0
    c = np.empty((len(tri), 3), np.float64)
    for a in range(3):
        b, d = (a + 1) % 3, (a + 2) % 3
        c[:, a] = e1[:, b] * e2[:, d] - e1[:, d] * e2[:, b]
    some = (c != 0).any(axis=1)
    tri, p0, c = tri[some], p0[some], c[some]
    with np.errstate(all="ignore"):
        nh = c / np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])[:, None]
        A = np.stack([c[:, 0] * nh[:, 0], c[:, 0] * nh[:, 1], c[:, 0] * nh[:, 2], c[:, 1] * nh[:, 1], c[:, 1] * nh[:, 2], c[:, 2] * nh[:, 2]], axis=1)
        tc = cl[tri]
        use = np.stack([np.ones(len(tri), bool), tc[:, 1] != tc[:, 0], (tc[:, 2] != tc[:, 0]) & (tc[:, 2] != tc[:, 1])], axis=1)
        cluster, terms = [], []
        for e in range(3):
            u = use[:, e]
            r = p0[u] - cell_centres(np.floor(x[tri[u, e]] * inv), cell)
            d = (nh[u, 0] * r[:, 0] + nh[u, 1] * r[:, 1]) + nh[u, 2] * r[:, 2]
            cluster.append(tc[u, e])
            terms.append(np.concatenate([A[u], c[u] * d[:, None]], axis=1))
        cluster, terms = np.concatenate(cluster), np.concatenate(terms)
        if not (np.abs(terms) < QUADRIC_LIMIT).all():
            raise ValueError("a triangle too large: a quadric term of 1 or more")
    return cluster, np.rint(terms * QUADRIC_ONE).astype(np.int64)


def quadric_sums(vertices, triangles, span_first, cell) -> np.ndarray:
    """int64 [n_out, 9]: every cluster's accumulated terms"""
    cluster, q = quadric_terms(vertices, triangles, span_first, cell)
    n = len(np.asarray(vertices).reshape(-1))
    total = int(cluster_of(np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1)["xyz"], span_first, cell).max()) + 1 if n else 0
    S = np.zeros((total, 9), np.int64)
    np.add.at(S, cluster, q)
    return S


def quadric_place(S, mean_q, k, cell, bias):
    """(xyz float32 [c, 3], placed bool [c]) of clusters with the sums S int64 [c, 9], the integer means mean_q int64 [c, 3] and the cell
    indices k [c, 3]: the solve of the module's docstring, one rounding per operation"""
    inv, b = check_cell(cell), check_bias(bias)
    S = np.asarray(S, np.int64).reshape(-1, 9).astype(np.float64)
    k = np.asarray(k, np.float64).reshape(-1, 3)
    o = cell_centres(k, cell)
    m = np.asarray(mean_q, np.int64).reshape(-1, 3).astype(np.float64) * (1.0 / FIXED_ONE) - o
    with np.errstate(all="ignore"):
        t = (S[:, 0] + S[:, 3]) + S[:, 5]
        lam = b * t
        M00, M11, M22, M01, M02, M12 = S[:, 0] + lam, S[:, 3] + lam, S[:, 5] + lam, S[:, 1], S[:, 2], S[:, 4]
        r0, r1, r2 = S[:, 6] + lam * m[:, 0], S[:, 7] + lam * m[:, 1], S[:, 8] + lam * m[:, 2]
        c00 = M11 * M22 - M12 * M12
        c01 = M02 * M12 - M01 * M22
        c02 = M01 * M12 - M02 * M11
        c11 = M00 * M22 - M02 * M02
        c12 = M01 * M02 - M00 * M12
        c22 = M00 * M11 - M01 * M01
        det = (M00 * c00 + M01 * c01) + M02 * c02
        xs = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det], axis=1)
        out = (o + xs).astype(np.float32)
        placed = (t > 0) & (det > 0) & np.isfinite(out).all(axis=1)
        placed &= (np.floor(np.where(placed[:, None], out, 0).astype(np.float64) * inv) == k).all(axis=1)
    return out, placed


def simplify_quadric(vertices, triangles, span_first, cell, bias):
    """(vertices_out MESH_VERTEX_DTYPE [n_out], triangles_out uint32 [m_out, 3], span_first_out int64 [S + 1], n_placed)"""
    check_bias(bias)
    v = np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1)
    n = len(v)
    if n == 0:
        out, _, first_out = simplify(v, np.zeros((0, 3), np.uint32), span_first, cell)
        return out, np.zeros((0, 3), np.uint32), first_out, 0
    SQ = quadric_sums(v, triangles, span_first, cell)    # (the checks of the triangles come first: simplify() asserts on an index)
    out, tri, first_out = simplify(v, triangles, span_first, cell)
    inv = check_cell(cell)
    order, head, rep = clusters(v["xyz"], span_first, cell)
    keep = rep == np.arange(n)
    new = np.cumsum(keep) - keep
    starts = np.nonzero(head)[0]
    size = np.diff(np.concatenate([starts, [n]])).astype(np.int64)
    many = size > 1
    dest = new[order[starts]][many]                      # the output index of each cluster of more than one member
    q = np.rint(v["xyz"].astype(np.float64) * FIXED_ONE).astype(np.int64)[order]
    mean_q = mean_half_up(np.add.reduceat(q, starts, axis=0), size[:, None])[many]
    k = np.floor(v["xyz"][order[starts]][many].astype(np.float64) * inv)
    xyz, placed = quadric_place(SQ[dest], mean_q, k, cell, bias)
    out["xyz"][dest[placed]] = xyz[placed]
    return out, tri, first_out, int(placed.sum())
