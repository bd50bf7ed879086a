"""Cases shared by the weld pass's CPU and GPU tests (test_mesh_weld_ref.py, test_gpu_mesh_weld.py): synthetic key lists with a
brute-force weld on Python dicts and lists, and the split-box volumes."""
import numpy as np

from kintinuous_amd import mesh_ref, mesh_weld_ref

V = mesh_ref.MESH_VERTEX_DTYPE
TOP = (1 << 62) - 1
NO_GATE = mesh_weld_ref.NO_GATE
SIZES = (0, 1, 63, 64, 65, 257, 4099, 70001)


def brute_weld(vertices, keys, triangles, span_first, span_time, max_gap):
    """the definition, one vertex at a time: (vertices_out, keys_out, triangles_out, span_first_out)"""
    n = len(keys)
    first = [int(x) for x in span_first]
    times = [int(x) for x in span_time]
    rep, last = [], {}
    s = 0
    for i in range(n):
        while first[s + 1] <= i:       # skips empty spans
            s += 1
        t, k = times[s], int(keys[i])
        if k in last and abs(t - last[k][0]) <= max_gap:
            rep.append(last[k][1])
            last[k] = (t, last[k][1])
        else:
            rep.append(i)
            last[k] = (t, i)
    new, kept = [], []
    for i in range(n):
        new.append(len(kept))
        if rep[i] == i:
            kept.append(i)
    tri = [[new[rep[int(a)]] for a in row] for row in np.asarray(triangles).reshape(-1, 3)]
    fo = [new[f] if f < n else len(kept) for f in first]
    return (np.asarray(vertices)[kept].copy(), np.asarray(keys, np.uint64)[kept].copy(), np.array(tri, np.uint32).reshape(-1, 3), np.array(fo, np.int64))


def _vertices(rng, n):
    v = np.zeros(n, V)
    v.view(np.uint32)[:] = rng.integers(0, 1 << 32, 4 * n, dtype=np.uint64).astype(np.uint32)   # any 16 bytes: the pass moves them untouched
    return v


def random_case(seed, n, n_spans=6, max_gap=10):
    """n vertices in n_spans spans (empty ones first, inside and last) whose times are multiples of 10 in random order; keys drawn from
    a pool of about n / 2 values, 0 and 2^62 - 1 among them: duplicates across and inside spans, at gaps below, equal to and above
    max_gap; about 2 n triangles"""
    rng = np.random.default_rng(seed)
    pool = np.unique(np.concatenate([rng.integers(0, 1 << 62, max(n // 2, 1), dtype=np.uint64), np.array([0, TOP], np.uint64)]))
    keys = pool[rng.integers(0, len(pool), n)].astype(np.uint64)
    if n >= 4:
        keys[[0, n - 1]] = 0
        keys[[1, n // 2]] = TOP
    cuts = np.sort(rng.integers(0, n + 1, max(n_spans - 4, 0)))
    first = np.concatenate([[0, 0], cuts, cuts[-1:] if len(cuts) else [], [n, n]]).astype(np.int64)   # empty: the first, the last, one inside
    if n_spans == 0:
        first = np.array([0], np.int64)
    times = (rng.permutation(len(first) - 1) * 10 + 5).astype(np.uint64)
    tri = rng.integers(0, max(n, 1), (2 * n, 3)).astype(np.uint32)
    return _vertices(rng, n), keys, tri, first, times, max_gap


def chain_cases():
    """one key at three vertices of three spans, max_gap 10: uncut, cut before the third, before the second, before both; and the same
    with the occurrences inside one span (never cut) -- each among other keys"""
    rng = np.random.default_rng(5)
    out = []
    for times in ((0, 10, 20), (0, 10, 30), (0, 20, 30), (0, 20, 40), (40, 20, 0), (10, 0, 10), (0, 11, 1)):
        keys = np.array([7, 3, 9, 7, 3, 7, 9, 1], np.uint64)
        first = np.array([0, 3, 5, 8], np.int64)
        tri = np.array([[0, 1, 2], [3, 4, 2], [5, 6, 7], [0, 3, 5]], np.uint32)
        out.append((_vertices(rng, 8), keys, tri, first, np.array(times, np.uint64), 10))
    keys = np.array([7, 7, 3, 7, 3], np.uint64)
    out.append((_vertices(rng, 5), keys, np.array([[0, 1, 3], [2, 4, 0]], np.uint32), np.array([0, 5], np.int64), np.array([99], np.uint64), 0))
    big = (1 << 64) - 2   # times at the ends of uint64: the difference is taken on uint64, and only NO_GATE never cuts
    keys = np.array([4, 4, 4], np.uint64)
    for gap in (big - 1, big, NO_GATE):
        out.append((_vertices(rng, 3), keys, np.array([[0, 1, 2]], np.uint32), np.array([0, 1, 2, 3], np.int64), np.array([0, big, 0], np.uint64), gap))
    return out


def same(got, want):
    """every byte of (vertices, keys, triangles, span_first_out)"""
    for g, w in zip(got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape, (g.shape, w.shape)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))


# ---- the split box ----
def sphere_volume(N=32):
    z, y, x = np.mgrid[0:N, 0:N, 0:N].astype(np.float64)
    r = np.sqrt((x - 15.3) ** 2 + (y - 16.6) ** 2 + (z - 15.55) ** 2) - 10.15
    vol = np.clip(np.round(r / 3.0 * 32767), -32767, 32767).astype(np.int16)
    col = np.zeros((N, N, N, 4), np.uint8)
    col[..., :3] = (np.stack([x, y, z], axis=-1) * 7).astype(np.uint8)
    col[..., 3] = 1
    return vol, col


def split_boxes(N, axis, cut):
    """(one box, box A, box B): cells [0, N - 1)^3, and the same cut at cell plane `cut` across `axis`"""
    M = N - 1
    hi_a, lo_b = [M, M, M], [0, 0, 0]
    hi_a[axis] = cut
    lo_b[axis] = cut
    return ((0, 0, 0), (M, M, M)), ((0, 0, 0), tuple(hi_a)), (tuple(lo_b), (M, M, M))


SPLITS = [(axis, cut) for axis in range(3) for cut in (1, 15, 30)]


def closed(tris):
    """every undirected edge in exactly two triangles, once in each direction"""
    t = np.asarray(tris).astype(np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    _, cnt = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    return bool((cnt == 2).all() and len(np.unique(d, axis=0)) == len(d))


def open_edges(tris):
    """the number of undirected edges used by exactly one triangle"""
    t = np.asarray(tris).astype(np.int64)
    d = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, cnt = np.unique(d, axis=0, return_counts=True)
    return int((cnt == 1).sum())


def concat(a, b):
    """two (vertices, triangles, keys) meshes as one with two spans of times 0 and 1"""
    (va, ta, ka), (vb, tb, kb) = a, b
    return (np.concatenate([va, vb]), np.concatenate([ka, kb]), np.concatenate([ta, tb + np.uint32(len(va))]).astype(np.uint32),
            np.array([0, len(va), len(va) + len(vb)], np.int64), np.array([0, 1], np.uint64))


def check_split(one, welded):
    """one = (vertices, triangles, keys) of the one-box mesh; welded = (vertices, keys, triangles, span_first_out) of the welded halves"""
    v1, t1, k1 = one
    vw, kw, tw, _ = welded
    order = np.argsort(kw, kind="stable")
    assert np.array_equal(kw[order], k1)   # (strictly increasing: no key is left twice)
    assert np.array_equal(np.ascontiguousarray(vw[order]).view(np.uint8), np.ascontiguousarray(v1).view(np.uint8))
    triples = lambda k, t: np.sort(np.ascontiguousarray(k[t.astype(np.int64)]).view(np.dtype((np.void, 24))).ravel())
    assert np.array_equal(triples(kw, tw), triples(k1, t1))
