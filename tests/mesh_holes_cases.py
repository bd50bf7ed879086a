"""Cases shared by the hole pass's CPU and GPU tests (test_mesh_holes_ref.py, test_gpu_mesh_holes.py): an open tetrahedron, fan discs with
rims around the wave and the limit, the N = 32 sphere with one-rings removed, holes that share a vertex, fins, duplicated, flipped and
degenerate triangles, unreferenced vertices and empty spans, loops across two spans, invalid vertices, random patches under a permutation,
and the independent check of the restatement (np.unique on sorted pairs, a Python walk along the loops, fractions.Fraction)."""
import functools
import math
from collections import Counter, defaultdict
from fractions import Fraction

import numpy as np

import mesh_simplify_cases as sc
import mesh_weld_cases as wc
from kintinuous_amd import mesh_ref

V = mesh_ref.MESH_VERTEX_DTYPE
SIZES = (0, 1, 63, 64, 65, 257, 4099)
RIMS = (3, 4, 63, 64, 65, 255, 256, 257)
same = wc.same


def _vertices(rng, n, box=1.5):
    """valid vertices around the origin (negative coordinates too) with random colours"""
    v = np.zeros(n, V)
    v["xyz"] = (rng.random((n, 3)) * 2.0 - 1.0).astype(np.float32) * np.float32(box)
    v["rgb"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return v


def _one_span(n):
    return np.array([0, n], np.int64)


def _thresholds(*lengths):
    """max_edges at L, L - 1, 0 and 256 for each L"""
    out = {0, 256}
    for L in lengths:
        out |= {min(L, 256), min(max(L - 1, 0), 256)}
    return sorted(out)


def tetra_case():
    """a tetrahedron minus one face: one loop of 3; filled it is closed"""
    rng = np.random.default_rng(1)
    return _vertices(rng, 4), np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1]], np.uint32), _one_span(4)


def disc_case(L, hub="last"):
    """a fan of L triangles around a hub: the rim is one loop of L edges"""
    rng = np.random.default_rng(100 + L)
    j = np.arange(L)
    ring = rng.permutation(L)                                     # the rim's indices in any order along the rim
    if hub == "last":
        tri = np.stack([np.full(L, L), ring[j], ring[(j + 1) % L]], axis=1)
    else:
        tri = np.stack([np.zeros(L, np.int64), ring[j] + 1, ring[(j + 1) % L] + 1], axis=1)
    v = _vertices(rng, L + 1)
    a = 2.0 * np.pi * np.arange(L) / L
    at = ring if hub == "last" else ring + 1
    v["xyz"][at] = np.stack([np.cos(a), np.sin(a), np.full(L, 0.25)], axis=1).astype(np.float32)
    return v, tri[rng.permutation(L)].astype(np.uint32), _one_span(L + 1)


def grid(rows, cols, rng=None):
    """(vertices, triangles int64) of a rows x cols grid of vertices in z = 0.5, two triangles per cell, one winding"""
    j, i = np.mgrid[0:rows, 0:cols]
    v = np.zeros(rows * cols, V)
    v["xyz"] = np.stack([i.reshape(-1) / 16.0 - 0.7, j.reshape(-1) / 16.0 - 0.4, np.full(rows * cols, 0.5)], axis=1).astype(np.float32)
    if rng is not None:
        v["xyz"] += (rng.random((rows * cols, 3)) * 0.01).astype(np.float32)
        v["rgb"] = rng.integers(0, 1 << 32, rows * cols, dtype=np.uint64).astype(np.uint32)
    a = (j[:-1, :-1] * cols + i[:-1, :-1]).reshape(-1)
    tri = np.concatenate([np.stack([a, a + 1, a + cols + 1], axis=1), np.stack([a, a + cols + 1, a + cols], axis=1)])
    return v, tri.astype(np.int64)


def without_rings(tri, centres):
    """the triangles that hold none of `centres`"""
    return tri[~np.isin(tri, np.asarray(centres)).any(axis=1)]


def shared_vertex_case():
    """a 9 x 9 grid without the one-rings of (2, 2) and (2, 4): the two rims share vertex (2, 3), which is COMPLEX: one open component;
    the grid's own border is a simple loop of 32"""
    v, tri = grid(9, 9, np.random.default_rng(2))
    return v, without_rings(tri, [2 * 9 + 2, 2 * 9 + 4]).astype(np.uint32), _one_span(81)


def fin_case(same_direction=True):
    """a 7 x 7 grid without the one-ring of (3, 3), and a fin triangle on one edge of that rim, running the way the rim's own triangle
    runs: the edge is non-manifold and BLOCKS its ends, so the hole is open.  The other way round the fin just moves the rim outwards"""
    v, tri = grid(7, 7, np.random.default_rng(3))
    tri = without_rings(tri, [3 * 7 + 3])
    a, b = 2 * 7 + 2, 2 * 7 + 3                                   # an edge of the rim; the triangle below holds b -> a ... find its direction
    d = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    forward = ((d[:, 0] == a) & (d[:, 1] == b)).any()
    e = (a, b) if forward == same_direction else (b, a)
    v = np.concatenate([v, _vertices(np.random.default_rng(4), 1)])
    return v, np.concatenate([tri, [[e[0], e[1], 49]]]).astype(np.uint32), _one_span(50)


def duplicate_case():
    """the open tetrahedron with one triangle twice: its three edges are non-manifold"""
    v, tri, f = tetra_case()
    return v, np.concatenate([tri, tri[:1]]), f


def flipped_case():
    """the sphere with one triangle flipped (its three edges run the same way twice) and, far from it, one one-ring removed"""
    v, tri = sc.sphere_mesh()
    tri = tri.astype(np.int64).copy()
    tri[5] = tri[5][[0, 2, 1]]
    far = int(np.argmax(np.abs(v["xyz"] - v["xyz"][tri[5, 0]]).sum(axis=1)))
    return v, without_rings(tri, [far]).astype(np.uint32), _one_span(len(v))


def degenerate_case():
    """(i, i, j) and (i, i, i) beside an open tetrahedron: no half-edges, counted, copied"""
    v, tri, _ = tetra_case()
    v = np.concatenate([v, _vertices(np.random.default_rng(5), 3)])
    return v, np.concatenate([[[4, 4, 5]], tri, [[6, 6, 6], [1, 2, 2]]]).astype(np.uint32), _one_span(7)


@functools.lru_cache(maxsize=None)
def _sphere_rings(count=7):
    """the sphere's triangles without the one-rings of `count` vertices no two of which share a neighbour -> (vertices, triangles, centres)"""
    v, tri = sc.sphere_mesh()
    tri = tri.astype(np.int64)
    assert (len(v), len(tri)) == (1946, 3888)
    near = defaultdict(set)
    for a, b, c in tri.tolist():
        near[a] |= {b, c}; near[b] |= {a, c}; near[c] |= {a, b}
    rng = np.random.default_rng(6)
    taken, centres = set(), []
    for c in rng.permutation(len(v)).tolist():
        zone = {c} | near[c] | set().union(*[near[x] for x in near[c]])
        if not zone & taken:
            centres.append(c)
            taken |= zone
        if len(centres) == count:
            break
    assert len(centres) == count
    return v, without_rings(tri, centres), centres


def sphere_case():
    """the N = 32 sphere with seven one-rings removed: seven loops of the centres' valences, every one fillable; the centres stay as
    unreferenced vertices"""
    v, tri, _ = _sphere_rings()
    return v.copy(), tri.astype(np.uint32), _one_span(len(v))


def sphere_lengths():
    v, tri, centres = _sphere_rings()
    full = sc.sphere_mesh()[1].astype(np.int64)
    return sorted(int(np.isin(full, [c]).any(axis=1).sum()) for c in centres)


def spans_case():
    """the holed sphere with unreferenced vertices first, inside and last, under a table with empty spans first, inside and last whose
    cuts run through the loops: a loop's centre lands in the span of its smallest index"""
    v, tri, centres = _sphere_rings()
    rng = np.random.default_rng(7)
    n = len(v)
    shift = np.arange(n) + 2 + (np.arange(n) >= n // 2) * 3        # two in front, three in the middle, two behind
    vv = _vertices(rng, n + 7)
    vv[shift] = v
    t = shift[tri]
    loops = check(vv, t.astype(np.uint32), _one_span(n + 7), 0)[3]
    labels = np.unique(loops[loops < 0xfffffffe])
    cuts = [int(l) + 1 for l in labels[:4]]                        # a cut right behind the smallest index of four loops: each spans two or more
    first = np.array(sorted([0, 0] + cuts + [n // 2, n // 2] + [n + 7, n + 7]), np.int64)
    return vv, t.astype(np.uint32), first


def invalid_case(kind):
    """the holed sphere with one vertex of one loop NaN ('nan'), infinite ('inf') or at a coordinate of 8192 ('far'): that loop is simple
    and is not filled"""
    v, tri, f = sphere_case()
    loops = check(v, tri, f, 0)[3]
    at = int(np.flatnonzero(loops < 0xfffffffe)[3])
    v["xyz"][at, 1] = {"nan": np.nan, "inf": -np.inf, "far": 8192.0}[kind]
    return v, tri, f


def random_case(seed, m):
    """(vertices, triangles, span_first) of exactly m triangles: a jittered grid patch with about a seventh of its triangles deleted at
    random (holes of every shape: loops, rims that touch, the patch's own border), then duplicated, flipped and degenerate triangles and
    a fin or two, the vertex indices under a random permutation with unreferenced vertices among them, the triangles shuffled; seven
    spans with empty ones first, inside and last"""
    rng = np.random.default_rng(seed)
    if m == 0:
        return _vertices(rng, 5), np.zeros((0, 3), np.uint32), np.array([0, 0, 2, 5, 5], np.int64)
    junk = min(m // 12, 40)
    side = int(math.ceil(math.sqrt((m - junk) / 0.85 / 2.0))) + 1
    v, tri = grid(side, side + 1, rng)
    keep = rng.permutation(len(tri))[:m - junk]
    tri = tri[np.sort(keep)]
    extra = []
    for k in range(junk):
        t = tri[rng.integers(len(tri))]
        kind = k % 4
        extra.append(t if kind == 0 else t[[0, 2, 1]] if kind == 1 else [t[0], t[0], t[1]] if kind == 2 else [t[0], t[1], rng.integers(len(v))])
    if extra:
        tri = np.concatenate([tri, np.array(extra, np.int64)])
    loose = 3 + m // 50
    n = len(v) + loose
    perm = rng.permutation(n)
    vv = _vertices(rng, n)
    vv[perm[:len(v)]] = v
    tri = perm[tri][rng.permutation(len(tri))]
    roll = rng.integers(0, 3, len(tri))                            # any corner first: the orientation stays
    tri = np.stack([tri[np.arange(len(tri)), (roll + j) % 3] for j in range(3)], axis=1)
    assert len(tri) == m
    return vv, tri.astype(np.uint32), sc.spans_with_empties(rng, n, 7).astype(np.int64)


def loop_lengths(case):
    """the distinct lengths of a case's simple loops, by the independent check"""
    loops = check(*case, 0)[3]
    return sorted(set(np.bincount(loops[loops < 0xfffffffe]).tolist()) - {0})


def every_case():
    """[(name, (vertices, triangles, span_first), [max_edges ...])]"""
    out = [("tetra", tetra_case(), _thresholds(3))]
    for L in RIMS:
        out.append(("disc %d" % L, disc_case(L, "last" if L % 2 else "first"), _thresholds(L)))
    out.append(("sphere", sphere_case(), _thresholds(*sphere_lengths())))
    out.append(("shared vertex", shared_vertex_case(), _thresholds(32, 6)))
    out.append(("fin", fin_case(True), _thresholds(24, 6)))
    out.append(("fin the other way", fin_case(False), _thresholds(24, 7)))
    out.append(("duplicate", duplicate_case(), _thresholds(3)))
    out.append(("flipped", flipped_case(), _thresholds(6)))
    out.append(("degenerate", degenerate_case(), _thresholds(3)))
    out.append(("spans", spans_case(), _thresholds(*sphere_lengths())))
    for kind in ("nan", "inf", "far"):
        out.append(("invalid " + kind, invalid_case(kind), _thresholds(*sphere_lengths())))
    for m in SIZES:
        case = random_case(m + 1, m)
        out.append(("random %d" % m, case, _thresholds(*loop_lengths(case))))
    return out


# ---- the independent check --------------------------------------------------------------------------------------------------------------
def _to_float32(fr):
    """the float32 nearest to a Fraction: rounded once"""
    f = np.float32(float(fr))
    near = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    return min(near, key=lambda c: abs(Fraction(float(c)) - fr))


def check(vertices, triangles, span_first, max_edges):
    """The independent check of the restatement: np.unique with counts on sorted pairs for the edge classes, a Python next-pointer walk
    for the loops, fractions.Fraction for the centres -> (vertices_out, triangles_out, span_first_out, loop_out, stats)"""
    v = np.asarray(vertices)
    tri = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    first = [int(x) for x in np.asarray(span_first)]
    n, m = len(v), len(tri)
    if n == 0:
        return v.copy(), np.zeros((0, 3), np.uint32), np.zeros(len(first), np.int64), np.zeros(0, np.uint32), (0,) * 9
    live = np.array([len(set(t)) == 3 for t in tri.tolist()], bool)
    h = np.flatnonzero(np.repeat(live, 3))
    a, b = tri.reshape(-1)[h], tri[:, [1, 2, 0]].reshape(-1)[h]
    boundary, blocked, odd = [], set(), 0
    if len(h):
        pairs = np.sort(np.stack([a, b], axis=1), axis=1)
        uniq, inverse, counts = np.unique(pairs, axis=0, return_inverse=True, return_counts=True)
        inverse = inverse.reshape(-1)
        forward = np.bincount(inverse, weights=(a < b), minlength=len(uniq)).astype(np.int64)
        for e in range(len(uniq)):
            if counts[e] == 1:
                continue
            if not (counts[e] == 2 and forward[e] == 1):
                odd += 1
                blocked |= set(uniq[e].tolist())
        boundary = [(int(h[k]), int(a[k]), int(b[k])) for k in np.flatnonzero(counts[inverse] == 1)]
    nxt, out_n, in_n, touch = defaultdict(list), Counter(), Counter(), defaultdict(set)
    for _, p, q in boundary:
        nxt[p].append(q); out_n[p] += 1; in_n[q] += 1
        touch[p].add(q); touch[q].add(p)
    loop_out = np.full(n, 0xffffffff, np.uint32)
    seen, loops, n_open, longest = set(), {}, 0, 0
    for s in sorted(touch):
        if s in seen:
            continue
        comp, todo = {s}, [s]
        while todo:
            for y in touch[todo.pop()]:
                if y not in comp:
                    comp.add(y); todo.append(y)
        seen |= comp
        simple = all(out_n[x] == 1 and in_n[x] == 1 and x not in blocked for x in comp)
        if not simple:
            n_open += 1
            loop_out[list(comp)] = 0xfffffffe
            continue
        walk, x = [s], nxt[s][0]                                  # the next pointers: back at the start after every vertex once
        while x != s:
            walk.append(x); x = nxt[x][0]
        assert sorted(walk) == sorted(comp) and s == min(comp)
        loop_out[walk] = s
        longest = max(longest, len(walk))
        ok = all(math.isfinite(float(c)) and abs(float(c)) < 8192.0 for x in walk for c in v["xyz"][x])
        loops[s] = (walk, ok and 3 <= len(walk) <= max_edges)
    filled = [s for s in sorted(loops) if loops[s][1]]
    rows, new, centre_at, first_out = [], {}, {}, []
    for s in range(len(first) - 1):
        first_out.append(len(rows))
        for x in range(first[s], first[s + 1]):
            new[x] = len(rows); rows.append(v[x])
        for l in filled:
            if first[s] <= l < first[s + 1]:
                walk = loops[l][0]
                L = len(walk)
                c = np.zeros(1, V)[0]
                for axis in range(3):
                    S = sum(round(Fraction(float(v["xyz"][x][axis])) * (1 << 32)) for x in walk)
                    assert abs(S) < 1 << 53
                    c["xyz"][axis] = _to_float32(Fraction(S, L * (1 << 32)))
                rgb = 0
                for k in range(4):
                    total = sum((int(v["rgb"][x]) >> (8 * k)) & 255 for x in walk)
                    rgb |= math.floor(Fraction(total, L) + Fraction(1, 2)) << (8 * k)
                c["rgb"] = rgb
                centre_at[l] = len(rows); rows.append(c)
    first_out.append(len(rows))
    vout = np.array(rows, V) if rows else np.zeros(0, V)
    tout = [[new[x] for x in t] for t in tri.tolist()]
    fan = 0
    for hh, p, q in sorted(boundary):
        l = int(loop_out[p])
        if l in centre_at:
            tout.append([new[q], new[p], centre_at[l]]); fan += 1
    stats = (len(boundary), odd, int((~live).sum()), len(loops), n_open, len(filled), longest, len(filled), fan)
    return vout, np.array(tout, np.uint32).reshape(-1, 3), np.array(first_out, np.int64), loop_out, stats


def same_result(got, want):
    """every byte of (vertices, triangles, span_first_out, loop_out) and the stats"""
    same(got[:4], want[:4])
    assert tuple(got[4]) == tuple(want[4]), (got[4], want[4])


def edge_counts(tris):
    """(boundary edges, V - E + F over the referenced vertices) of a triangle list"""
    t = np.asarray(tris).astype(np.int64)
    d = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    uniq, counts = np.unique(d, axis=0, return_counts=True)
    return int((counts == 1).sum()), len(np.unique(t)) - len(uniq) + len(t)
