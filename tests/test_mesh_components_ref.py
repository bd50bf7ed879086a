"""CPU: the component filter's restatement (kintinuous_amd/mesh_components_ref.py) against an independently written check (scipy's
connected components for the partition, np.minimum.at for the labels, np.bincount for the sizes, boolean masks for the compaction) on
every case of mesh_components_cases.py, and the properties of the definition: a threshold of 0 returns the input, 1 drops exactly the
unreferenced vertices, the order of the triangles plays no part, the sphere is one piece, its unwelded split boxes are not, its welded
ones are."""
import numpy as np
import pytest

import mesh_components_cases as cases
import mesh_simplify_cases as sc
import mesh_weld_cases as wc
from kintinuous_amd import mesh_components_ref as ref


@pytest.fixture(scope="module")
def every_case():
    return cases.every_case()


def test_restatement_equals_the_independent_check(every_case):
    runs = 0
    for name, case, thresholds in every_case:
        for k in thresholds:
            got, want = ref.components(*case, k), cases.check(*case, k)
            try:
                cases.same_result(got, want)
            except AssertionError as e:
                raise AssertionError("%s at min_triangles %d" % (name, k)) from e
            runs += 1
    assert runs > 100


def test_the_cases_hold_what_they_say():
    for m in (257, 4099, 70001):
        case = cases.random_case(m, m)
        v, tri, first = case
        _, _, fo, labels, (comps, kept, largest) = ref.components(*case, 4)
        used = np.zeros(len(v), bool)
        used[tri.reshape(-1)] = True
        assert not used[0] and not used[-1] and (~used[1:-1]).any()                  # unreferenced vertices at the start, at the end and inside
        assert len(tri) == m + 7 and 100 < largest <= 300 and 0 < kept < comps
        roots = np.flatnonzero(labels == np.arange(len(v)))
        assert (roots[1:-1] > 8).any() and not np.array_equal(labels[tri[:, 0]], np.sort(labels[tri[:, 0]]))   # minima anywhere, triangles scattered
        s = cases.all_small_span(case)
        assert first[s + 1] > first[s] and fo[s + 1] == fo[s]                        # a span that loses every vertex
        assert first[0] == first[1] and first[-1] == first[-2] and (np.diff(first)[1:-1] == 0).any()   # empty spans first, last and inside
    for k in cases.SIZES[1:]:
        for order in ("descending", "random"):
            assert ref.components(*cases.chain_case(k, order), 1)[4] == (1, 1, k)
        for hub in ("last", "first"):
            assert ref.components(*cases.hub_case(k, hub), 1)[4] == (1, 1, k)
    v, tri, first = cases.threshold_case()
    sizes = np.bincount(ref.components(v, tri, first, 0)[3][tri[:, 0]])
    assert sorted(sizes[sizes > 0].tolist()) == list(cases.THRESHOLD_SIZES)
    for k in cases.THRESHOLD_SIZES:                                                  # >= against >: a component of exactly k stays at k and goes at k + 1
        at, above = ref.components(v, tri, first, k), ref.components(v, tri, first, k + 1)
        assert at[4][1] == sum(s >= k for s in cases.THRESHOLD_SIZES) and above[4][1] == at[4][1] - 1
        assert len(at[1]) - len(above[1]) == k


def test_the_connectivity_and_counting_rules():
    for name, case, k, stats, n_out in cases.touching_case():
        got = ref.components(*case, k)
        assert got[4] == stats and len(got[0]) == n_out, name
        cases.same_result(got, cases.check(*case, k))
    v, t, f = cases.touching_case()[1][1]
    assert v[3].tobytes() == v[7].tobytes() and ref.components(v, t, f, 0)[3].tolist() == [0, 0, 0, 0, 4, 4, 4, 4]   # equal bytes, other index: not joined


def test_errors():
    v, tri, first = cases.random_case(3, 65)
    bad = tri.copy()
    bad[7, 1] = len(v)
    for args in ((v, bad, first, 1), (v, tri, np.concatenate([[1], first[1:]]), 1), (v, tri, np.concatenate([first[:-1], [len(v) - 1]]), 1), (v, tri, first, -1), (v, tri, first, 1 << 32)):
        with pytest.raises(ValueError):
            ref.components(*args)
    out = ref.components(v[:0], tri, [0, 0, 0], 3)                                   # n = 0: zeros, the triangles are not looked at
    assert len(out[0]) == 0 and out[1].shape == (0, 3) and out[2].tolist() == [0, 0, 0] and len(out[3]) == 0 and out[4] == (0, 0, 0)
    out = ref.components(v, tri[:0], first, 1)                                       # m = 0: n components of size 0
    assert len(out[0]) == 0 and out[4] == (len(v), 0, 0) and np.array_equal(out[3], np.arange(len(v)))


def test_threshold_0_returns_the_input_and_1_drops_the_unreferenced(every_case):
    for name, case, _ in every_case:
        v, tri, first = case
        ov, ot, of, labels, stats = ref.components(v, tri, first, 0)
        cases.same((ov, ot, of), (v, tri, np.asarray(first, np.int64)))
        assert stats[0] == stats[1]
        used = np.zeros(len(v), bool)
        used[tri.reshape(-1)] = True
        ov, ot, of, _, stats1 = ref.components(v, tri, first, 1)
        cases.same((ov,), (v[used],))
        assert len(ot) == len(tri) and stats1[0] - stats1[1] == int((~used).sum()), name


def test_the_triangle_order_plays_no_part():
    rng = np.random.default_rng(5)
    for case, k in ((cases.random_case(4099, 4099), 40), (cases.chain_case(4099, "random"), 1), (cases.hub_case(257, "last"), 300), (cases.threshold_case(), 64)):
        v, tri, first = case
        a = ref.components(v, tri, first, k)
        b = ref.components(v, tri[rng.permutation(len(tri))], first, k)
        cases.same((a[0], a[2], a[3]), (b[0], b[2], b[3]))                           # the kept vertices, the table, the labels
        assert a[4] == b[4] and len(a[1]) == len(b[1])


def test_the_sphere_is_one_piece_its_unwelded_halves_are_not():
    v, t = sc.sphere_mesh(32)
    assert (len(v), len(t)) == (1946, 3888)
    out = ref.components(v, t, [0, len(v)], len(t))
    assert out[4] == (1, 1, len(t)) and not out[3].any()
    cases.same(out[:3], (v, t, np.array([0, len(v)], np.int64)))
    for axis, cut in wc.SPLITS:
        uv, _, ut, first, _ = cases.unwelded_split(axis, cut)
        stats = ref.components(uv, ut, first, 1)[4]
        if cut == 15:                                                                # the plane goes through the sphere: two open halves
            assert stats[0] == stats[1] == 2 and stats[2] < len(ut) and len(uv) > len(v)
        else:                                                                        # the plane misses it: one box holds all of it
            assert stats == (1, 1, len(ut)) and len(uv) == len(v)
        wv, wt, wf = sc.welded_split(axis, cut)
        out = ref.components(wv, wt, wf, len(wt))
        assert out[4] == (1, 1, len(wt))
        cases.same(out[:3], (wv, wt, wf))
