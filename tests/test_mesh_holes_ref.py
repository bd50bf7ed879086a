"""CPU: the numpy restatement of the hole pass (kintinuous_amd/mesh_holes_ref.py) against the independent check of mesh_holes_cases.py, bit
for bit on every case, and the properties of the definition: the order of the triangles plays no part, a filled mesh is closed, a second
run finds nothing new to fill, max_edges = 0 returns the input."""
import numpy as np
import pytest

import mesh_holes_cases as cases
import mesh_weld_cases as wc
from kintinuous_amd import mesh_holes_ref as ref


@pytest.fixture(scope="module")
def every_case():
    return cases.every_case()


def test_restatement_equals_the_independent_check(every_case):
    names = [c[0] for c in every_case]
    assert len(set(names)) == len(names) and len(names) == 1 + len(cases.RIMS) + 8 + 3 + len(cases.SIZES)
    for name, case, thresholds in every_case:
        for k in thresholds:
            cases.same_result(ref.holes(*case, k), cases.check(*case, k))


def test_the_cases_are_what_they_claim(every_case):
    by_name = {name: case for name, case, _ in every_case}
    st = lambda name, k: ref.holes(*by_name[name], k)[4]
    # (boundary, non-manifold, degenerate, loops, open, filled, longest, new vertices, new triangles)
    assert st("tetra", 3) == (3, 0, 0, 1, 0, 1, 3, 1, 3) and st("tetra", 2) == (3, 0, 0, 1, 0, 0, 3, 0, 0)
    for L in cases.RIMS:
        fits = L <= 256
        assert st("disc %d" % L, min(L, 256)) == (L, 0, 0, 1, 0, int(fits), L, int(fits), L * fits)
        assert st("disc %d" % L, min(L - 1, 256))[5] == 0
    lengths = cases.sphere_lengths()
    assert len(set(lengths)) > 1
    assert st("sphere", max(lengths)) == (sum(lengths), 0, 0, 7, 0, 7, max(lengths), 7, sum(lengths))
    assert st("sphere", min(lengths))[5] == lengths.count(min(lengths)) and st("sphere", min(lengths) - 1)[5] == 0
    assert st("shared vertex", 256)[3:6] == (1, 1, 1) and st("shared vertex", 31)[5] == 0       # the two rims are one open component; the border is a loop of 32
    assert st("fin", 256)[1] == 1 and st("fin", 256)[3:6] == (1, 1, 1)                       # the fin BLOCKS the hole: only the border is filled
    assert st("fin the other way", 256)[1] == 0 and st("fin the other way", 256)[3:6] == (2, 0, 2) and st("fin the other way", 7)[5] == 1
    assert st("duplicate", 3) == (2, 3, 0, 0, 1, 0, 0, 0, 0)                                      # the two edges left of the missing face hang on BLOCKED vertices
    assert st("flipped", 256)[1] == 3 and st("flipped", 256)[4] == 0 and st("flipped", 256)[5] == 1
    assert st("degenerate", 3) == (3, 0, 3, 1, 0, 1, 3, 1, 3)
    assert st("spans", 256)[5] == 7
    for kind in ("nan", "inf", "far"):
        assert st("invalid " + kind, 256)[3:6] == (7, 0, 6)                                    # simple, and not filled
    big = st("random 4099", 256)
    assert big[1] > 0 and big[2] > 0 and big[3] >= big[5] > 0 and big[4] > 0 and 0 < st("random 4099", 4)[5] < big[5]
    # the degenerate triangles are copied like any other
    v, tri, f = by_name["degenerate"]
    assert np.array_equal(ref.holes(v, tri, f, 3)[1][:len(tri)], tri)


def test_centres_land_in_the_span_of_the_smallest_index(every_case):
    v, tri, first = [c for n, c, _ in every_case if n == "spans"][0]
    vo, to, fo, loops, st = ref.holes(v, tri, first, 256)
    labels = np.unique(loops[loops < ref.OPEN])
    assert len(labels) == 7 and st[5] == 7
    spread = 0
    for l in labels:
        members = np.flatnonzero(loops == l)
        spans = np.searchsorted(first[:-1], members, side="right") - 1
        spread += len(set(spans.tolist())) > 1
        s = spans[0]                                                                             # the smallest index is the first member
        fan = to[len(tri):]
        mine = fan[np.isin(fan[:, 0], members + (fo[spans] - first[spans]))]
        assert len(mine) == len(members) and len(set(mine[:, 2].tolist())) == 1
        c = int(mine[0, 2])
        assert fo[s] + (first[s + 1] - first[s]) <= c < fo[s + 1]                                 # behind the span's own vertices, inside the span
    assert spread >= 4
    assert np.array_equal(np.diff(fo) - np.diff(first), np.bincount(np.searchsorted(first[:-1], labels, side="right") - 1, minlength=len(first) - 1))


def test_a_shuffled_triangle_list_changes_nothing_but_the_order(every_case):
    rng = np.random.default_rng(12)
    for name, case, thresholds in every_case:
        v, tri, first = case
        if len(tri) < 2:
            continue
        k = thresholds[-1]
        a = ref.holes(v, tri, first, k)
        b = ref.holes(v, tri[rng.permutation(len(tri))], first, k)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4], name
        assert sorted(map(tuple, a[1][:len(tri)].tolist())) == sorted(map(tuple, b[1][:len(tri)].tolist()))
        rolled = lambda t: sorted(tuple(np.roll(r, -int(np.argmin(r))).tolist()) for r in t)
        assert rolled(a[1][len(tri):]) == rolled(b[1][len(tri):]), name


def test_filled_meshes_are_closed(every_case):
    by_name = {name: case for name, case, _ in every_case}
    for name in ("tetra", "disc 3", "disc 64", "disc 256", "sphere", "spans", "degenerate"):
        v, tri, first = by_name[name]
        vo, to, fo, _, st = ref.holes(v, tri, first, 256)
        again = ref.holes(vo, to, fo, 256)
        assert st[5] == st[3] > 0 and again[4][0] == 0 and again[4][3:6] == (0, 0, 0), name
        assert again[0].tobytes() == vo.tobytes() and np.array_equal(again[1], to) and np.array_equal(again[2], fo)
    vo, to, _, _, _ = ref.holes(*by_name["sphere"], 256)
    assert cases.edge_counts(to) == (0, 2) and wc.closed(to)                                     # V - E + F = 2


def test_a_second_run_fills_nothing_new_among_the_loops_it_left(every_case):
    for name, case, thresholds in every_case:
        for k in (4, 256):
            vo, to, fo, loops, st = ref.holes(*case, k)
            again = ref.holes(vo, to, fo, k)
            assert again[4][5] == 0 and again[4][7:] == (0, 0), (name, k)
            assert again[4][3] == st[3] - st[5] and again[4][4] == st[4] and again[4][1] == st[1], (name, k)   # the loops left, the open ones, the non-manifold edges


def test_max_edges_zero_returns_the_input(every_case):
    for name, case, _ in every_case:
        v, tri, first = case
        for k in (0, 1, 2):
            vo, to, fo, loops, st = ref.holes(v, tri, first, k)
            assert vo.tobytes() == v.tobytes() and np.array_equal(to, tri) and np.array_equal(fo, first) and st[5] == 0 and st[7:] == (0, 0), name


def test_bad_input_raises():
    v, tri, first = cases.tetra_case()
    for args in ((v, tri, first, 257), (v, tri, first, -1), (v, tri + 2, first, 3), (v, tri, [0, 3], 3), (v, tri, [1, 4], 3), (v, tri, [], 3)):
        with pytest.raises(ValueError):
            ref.holes(*args)
    assert ref.holes(v[:0], tri, [0, 0, 0], 3)[4] == (0,) * 9                                     # n = 0: the triangles are not looked at
