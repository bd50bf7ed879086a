"""Cases shared by the component filter's CPU and GPU tests (test_mesh_components_ref.py, test_gpu_mesh_components.py): random meshes of
many components under a random permutation of the vertex indices, strips with adversarial indices, hubs that every union contends on,
components of exact sizes around the threshold, the connectivity and counting rules on a handful of triangles, and the independent check
of the restatement (scipy's connected components, np.minimum.at, np.bincount, boolean masks)."""
import functools

import numpy as np

import mesh_simplify_cases as sc
import mesh_weld_cases as wc
from kintinuous_amd import mesh_ref

V = mesh_ref.MESH_VERTEX_DTYPE
SIZES = wc.SIZES
THRESHOLD_SIZES = (1, 2, 63, 64, 65, 257)
same = wc.same


def _vertices(rng, n):
    v = np.zeros(n, V)
    v.view(np.uint32)[:] = rng.integers(0, 1 << 32, 4 * n, dtype=np.uint64).astype(np.uint32)   # any 16 bytes: the pass moves them untouched
    return v


def _one_span(n):
    return np.array([0, n], np.int64)


def _component(rng, k, base):
    """k triangles over the vertices base .. base + k + 1 that hang together: triangle j holds vertex j + 2 and two earlier ones, in a
    random orientation -> (triangles int64 [k, 3], vertices used)"""
    a = np.arange(2, k + 2)
    b = (rng.random(k) * a).astype(np.int64)            # below a
    c = (rng.random(k) * a).astype(np.int64)
    c = np.where(c == b, (b + 1) % a, c)                # another one below a
    t = np.stack([a, b, c], axis=1)
    roll = rng.integers(0, 3, k)
    t = np.stack([t[np.arange(k), (roll + j) % 3] for j in range(3)], axis=1)
    return t + base, k + 2


def random_case(seed, m):
    """(vertices, triangles, span_first) of about m triangles: components whose sizes are drawn from 1 up to about 300, some vertices that
    no triangle references; the vertex indices are then a random permutation (a component's smallest index sits anywhere) with
    unreferenced vertices forced to the start and the end as well, and the triangles are shuffled over the list; eleven spans with empty
    ones first, inside and last, and one span made of small components only, which loses every vertex at a threshold of 4"""
    rng = np.random.default_rng(seed)
    parts, at, left = [], 0, m
    while left > 0:
        k = min(int(rng.integers(1, 5) if rng.random() < 0.5 else rng.integers(5, 301)), left)
        t, used = _component(rng, k, at)
        parts.append(t)
        at += used
        left -= k
    loose = 3 + m // 50                                  # unreferenced vertices
    small = 0                                            # the span that loses everything: components of 1 .. 3 triangles, kept apart from the permutation
    tail = []
    if m >= 63:
        for k in (1, 2, 3, 1):
            t, used = _component(rng, k, 0)
            tail.append((t, used))
            small += used
    n_perm = at + loose
    n = n_perm + small + 2
    perm = rng.permutation(n_perm) + 1                   # index 0 and the last two stay unreferenced
    tri = perm[np.concatenate(parts)] if parts else np.zeros((0, 3), np.int64)
    base = 1 + n_perm
    for t, used in tail:
        tri = np.concatenate([tri, t + base])
        base += used
    tri = tri[rng.permutation(len(tri))].astype(np.uint32)
    first = sc.spans_with_empties(rng, 1 + n_perm, 8)
    first = np.concatenate([first, [1 + n_perm + small, n, n]]).astype(np.int64) if small else np.concatenate([first[:-1], [n, n]]).astype(np.int64)
    return _vertices(rng, n), tri, first


def all_small_span(case):
    """the span of random_case that holds components of at most 3 triangles only, or None (m < 63)"""
    first = case[2]
    return len(first) - 4 if len(first) == 12 else None


def chain_case(k, order):
    """one strip of k triangles (triangle j = strip vertices j, j + 1, j + 2) whose vertex indices are `order`: 'descending' along the
    strip, or 'random'"""
    rng = np.random.default_rng(k + 11)
    n = k + 2 if k else 0
    idx = np.arange(n)[::-1] if order == "descending" else rng.permutation(n)
    j = np.arange(k)
    tri = idx[np.stack([j, j + 1, j + 2], axis=1)].astype(np.uint32) if k else np.zeros((0, 3), np.uint32)
    return _vertices(rng, n), tri, _one_span(n)


def hub_case(k, hub):
    """k triangles that all share one vertex and are otherwise disjoint: the hub at the LARGEST index ('last') or at index 0 ('first')"""
    rng = np.random.default_rng(k + 23)
    n = 2 * k + 1 if k else 0
    j = np.arange(k)
    if hub == "last":
        tri = np.stack([2 * j, np.full(k, n - 1), 2 * j + 1], axis=1)
    else:
        tri = np.stack([2 * j + 1, 2 * j + 2, np.zeros(k, np.int64)], axis=1)
    if k:
        tri = tri[rng.permutation(k)]
    return _vertices(rng, n), tri.astype(np.uint32).reshape(-1, 3), _one_span(n)


def threshold_case():
    """components of exactly 1, 2, 63, 64, 65 and 257 triangles, permuted and shuffled; run it at THRESHOLD_SIZES and each + 1"""
    rng = np.random.default_rng(31)
    parts, at = [], 0
    for k in THRESHOLD_SIZES:
        t, used = _component(rng, k, at)
        parts.append(t)
        at += used
    perm = rng.permutation(at)
    tri = perm[np.concatenate(parts)]
    tri = tri[rng.permutation(len(tri))].astype(np.uint32)
    return _vertices(rng, at), tri, np.array([0, at // 3, at // 3, at], np.int64)


def _tetra(a, b, c, d):
    return [[a, b, c], [a, c, d], [a, d, b], [b, d, c]]


def touching_case():
    """[(name, (vertices, triangles, span_first), min_triangles, expected (components, kept components, largest), expected n_out)]"""
    rng = np.random.default_rng(41)
    out = []
    # two closed pieces that share exactly vertex 3: one component of 8 triangles
    t = np.array(_tetra(0, 1, 2, 3) + _tetra(3, 4, 5, 6), np.uint32)
    out.append(("shared vertex", (_vertices(rng, 7), t, _one_span(7)), 5, (1, 1, 8), 7))
    # the same with that vertex duplicated under index 7 (equal bytes): two components of 4
    v = _vertices(rng, 8)
    v[7] = v[3]
    t = np.array(_tetra(0, 1, 2, 3) + _tetra(7, 4, 5, 6), np.uint32)
    out.append(("duplicated vertex", (v, t, _one_span(8)), 5, (2, 0, 4), 0))
    out.append(("duplicated vertex kept", (v, t, _one_span(8)), 4, (2, 2, 4), 8))
    # a triangle and its duplicate: size 2, across the threshold; (5, 4, 3) is alone
    t = np.array([[0, 1, 2], [5, 4, 3], [0, 1, 2]], np.uint32)
    out.append(("duplicate counted twice", (_vertices(rng, 6), t, _one_span(6)), 2, (2, 1, 2), 3))
    out.append(("duplicate above the threshold", (_vertices(rng, 6), t, _one_span(6)), 3, (2, 0, 2), 0))
    # (i, i, j) joins i and j; (i, i, i) joins nothing but counts for i; vertex 5 is unreferenced
    t = np.array([[1, 1, 3], [4, 4, 4], [2, 0, 0]], np.uint32)
    out.append(("repeated indices", (_vertices(rng, 6), t, _one_span(6)), 1, (4, 3, 1), 5))
    # the size is counted at the FIRST index: all the same here, since a triangle's vertices share a label
    t = np.array([[3, 0, 1], [3, 1, 2], [4, 5, 6]], np.uint32)
    out.append(("two fans", (_vertices(rng, 7), t, np.array([0, 0, 4, 7, 7], np.int64)), 2, (2, 1, 2), 4))
    return out


def every_case():
    """[(name, (vertices, triangles, span_first), [min_triangles ...])]: all of the above, every swept size"""
    out = []
    for m in SIZES:
        out.append(("random %d" % m, random_case(m, m), [0, 1, 4, 40]))
        out.append(("chain descending %d" % m, chain_case(m, "descending"), [0, max(m, 1), m + 1]))
        out.append(("chain random %d" % m, chain_case(m, "random"), [1, m + 1]))
        out.append(("hub last %d" % m, hub_case(m, "last"), [max(m, 1), m + 1]))
        out.append(("hub first %d" % m, hub_case(m, "first"), [max(m, 1)]))
    out.append(("threshold", threshold_case(), sorted(set(list(THRESHOLD_SIZES) + [k + 1 for k in THRESHOLD_SIZES]))))
    for name, case, k, _, _ in touching_case():
        out.append((name, case, [k]))
    return out


def check(vertices, triangles, span_first, min_triangles):
    """The independent check of the restatement: scipy's partition, np.minimum.at labels, np.bincount sizes, boolean-mask compaction ->
    (vertices_out, triangles_out, span_first_out, labels, stats)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    v = np.asarray(vertices)
    tri = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    first = np.asarray(span_first).astype(np.int64)
    n = len(v)
    if n == 0:
        return v.copy(), np.zeros((0, 3), np.uint32), np.zeros(len(first), np.int64), np.zeros(0, np.uint32), (0, 0, 0)
    rows = np.concatenate([tri[:, 0], tri[:, 0]])
    cols = np.concatenate([tri[:, 1], tri[:, 2]])
    _, part = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n)), directed=False)
    lowest = np.full(part.max() + 1, n, np.int64)
    np.minimum.at(lowest, part, np.arange(n))
    label = lowest[part]
    size = np.bincount(label[tri[:, 0]], minlength=n)
    keep = size[label] >= min_triangles
    below = np.concatenate([[0], np.cumsum(keep)])              # below[i] = kept vertices under index i
    tri_out = below[tri[keep[tri[:, 0]]]].astype(np.uint32).reshape(-1, 3)
    roots = np.unique(label)
    stats = (len(roots), int((size[roots] >= min_triangles).sum()), int(size[roots].max()))
    return v[keep].copy(), tri_out, below[first], label.astype(np.uint32), stats


def same_result(got, want):
    """every byte of (vertices, triangles, span_first_out, labels) and the stats"""
    same(got[:4], want[:4])
    assert tuple(got[4]) == tuple(want[4]), (got[4], want[4])


@functools.lru_cache(maxsize=None)
def unwelded_split(axis, cut, N=32):
    """(vertices, keys, triangles, span_first, span_time) of the two boxes of a split of the sphere, concatenated and NOT welded"""
    from kintinuous_amd import mesh_weld_ref
    vol, col = wc.sphere_volume(N)
    parts = []
    for lo, hi in wc.split_boxes(N, axis, cut)[1:]:
        v, t, info = mesh_ref.extract_mesh(vol, col, (3.0, 3.0, 3.0), (0, 0, 0), lo, hi, (0, 0, 0), N, info=True)
        parts.append((v, t, mesh_weld_ref.edge_keys(info["owner"], info["axis"], (0, 0, 0))))
    return wc.concat(*parts)
