"""CPU: the mesh simplification's restatement (kintinuous_amd/mesh_simplify_ref.py) against a brute-force clustering on Python dicts and
exact Python integers, and the properties of the definition: P1 a cell below every spacing returns the input, P2 a closed oriented mesh
keeps its directed edges balanced, P3 the distance bounds, P4 the output table carries every representative's span time into the
deformation."""
import numpy as np
import pytest

import mesh_simplify_cases as cases
import mesh_weld_cases as wc
from kintinuous_amd import mesh_ref, mesh_simplify_ref as ref


@pytest.mark.parametrize("n", [n for n in cases.SIZES if n <= 4099])
def test_random_lists_against_brute_force(n):
    for seed, spans, cell, per in ((n, 6, 0.25, 3.0), (n + 1, 9, 0.5, 1.0), (n + 2, 1, 0.25, 20.0), (n + 3, 40, 0.125, 4.0)):
        case = cases.random_case(seed, n, spans, cell, per)
        got, want = ref.simplify(*case), cases.brute_simplify(*case)
        cases.same(got, want)
        if n >= 257:
            assert 0 < len(got[0]) < n and 0 < len(got[1]) < len(case[1])      # something merged and something dropped, something kept


def test_ties_signs_faces_and_spans():
    """what the random lists hold, one at a time"""
    V = mesh_ref.MESH_VERTEX_DTYPE
    u = 2.0 ** -20

    def mesh(xyz, rgb=None, first=None):
        v = np.zeros(len(xyz), V)
        v["xyz"] = np.array(xyz, np.float32)
        v["rgb"] = 0 if rgb is None else np.array(rgb, np.uint32)
        return v, np.zeros((0, 3), np.uint32), np.array([0, len(v)] if first is None else first, np.int64)

    # S = -3, k = 4 along x: floor((2 S + k) / (2 k)) = floor(-2 / 8) = -1 (truncation gives 0); S = -3, k = 2: exactly -1 (half up)
    for qs, want in (((-1, -1, -1, 0), None), ((-1, -1, -1, -0.0), None), ((-1, -2), -1), ((-1, -1, -1, -2), -1), ((-3, -4), -3), ((1, 2), 2), ((-5, -5, -5, -6), -5)):
        v, t, f = mesh([(q * u, 0.5, 0.5) for q in qs])
        out = ref.simplify(v, t, f, 1.0)
        cases.same(out, cases.brute_simplify(v, t, f, 1.0))
        if want is not None:
            assert len(out[0]) == 1 and out[0]["xyz"][0, 0] == np.float32(want * u)
    # the family itself, in one cell: q = 0 is cell 0 and -1 is cell -1, so S = -3 at k = 4 needs an offset that keeps 2 S + k odd-signed
    v, t, f = mesh([(-1 * u, 0.5, 0.5), (-1 * u, 0.5, 0.5), (-1 * u, 0.5, 0.5), (-u / 4, 0.5, 0.5)])   # q = -1, -1, -1, rint(-0.25) = -0.0
    out = ref.simplify(v, t, f, 1.0)
    assert len(out[0]) == 1 and out[0]["xyz"][0, 0] == np.float32(-u)                # S = -3, k = 4 -> -1
    assert int(ref.mean_half_up(-3, 4)) == -1 and int(ref.mean_half_up(-3, 2)) == -1 and int(ref.mean_half_up(3, 2)) == 2
    # a face belongs to the cell above it; -0.0 is in cell 0; a cluster of one keeps -0.0
    v, t, f = mesh([(-0.0, 0.0, 0.25), (0.1, 0.1, 0.3), (-0.25, 0.0, 0.25), (-0.2, 0.1, 0.3), (-0.0, -0.0, -0.0)])
    out = ref.simplify(v, t, f, 0.25)
    assert ref.cluster_of(v["xyz"], f, 0.25).tolist() == [0, 0, 1, 1, 2]
    assert np.signbit(out[0]["xyz"][2]).all()
    cases.same(out, cases.brute_simplify(v, t, f, 0.25))
    # colour ties: bytes 0 and 1 give 1, the weight byte alike
    v, t, f = mesh([(0.1, 0.1, 0.1), (0.2, 0.2, 0.2)], rgb=[0x00010203, 0x01000202])
    assert ref.simplify(v, t, f, 1.0)[0]["rgb"][0] == 0x01010203
    # one cell in adjacent spans: two clusters; an empty span between changes nothing
    xyz = [(0.1, 0.1, 0.1), (0.2, 0.2, 0.2), (0.3, 0.3, 0.3), (0.4, 0.4, 0.4)]
    for first, n_out, fo in (([0, 4], 1, [0, 1]), ([0, 2, 4], 2, [0, 1, 2]), ([0, 0, 2, 2, 4, 4], 2, [0, 0, 1, 1, 2, 2]), ([0, 1, 2, 3, 4], 4, [0, 1, 2, 3, 4])):
        v, t, f = mesh(xyz, first=first)
        out = ref.simplify(v, np.array([[0, 1, 2], [0, 2, 3], [3, 1, 0]], np.uint32), f, 1.0)
        assert len(out[0]) == n_out and out[2].tolist() == fo
        cases.same(out, cases.brute_simplify(v, np.array([[0, 1, 2], [0, 2, 3], [3, 1, 0]], np.uint32), f, 1.0))


def test_sized_clusters_many_spans_one_cluster():
    v, tri, first, cell = cases.sized_clusters_case()
    out = ref.simplify(v, tri, first, cell)
    sizes = np.bincount(ref.cluster_of(v["xyz"], first, cell))
    assert sorted(sizes.tolist()) == sorted(list(cases.CLUSTER_SIZES) * 3)
    cases.same(out, cases.brute_simplify(v, tri, first, cell))
    v, tri, first, cell = cases.many_spans_case()
    out = ref.simplify(v, tri, first, cell)
    assert len(out[0]) > len(np.unique(ref.cell_keys(v["xyz"], cell)))          # the spans cut cells apart
    cases.same(out, cases.brute_simplify(v, tri, first, cell))
    v, tri, first, cell = cases.one_cluster_case(4099)
    out = ref.simplify(v, tri, first, cell)
    assert len(out[0]) == 1 and len(out[1]) == 0 and out[2].tolist() == [0, 1]
    cases.same(out, cases.brute_simplify(v, tri, first, cell))


def test_p1_a_small_cell_returns_the_input():
    v, t = cases.sphere_mesh()
    assert len(v) == 1946 and len(t) == 3888 and wc.closed(t)
    out = ref.simplify(v, t, [0, len(v)], 1e-4)
    cases.same(out, (v, t, np.array([0, len(v)], np.int64)))


def test_p2_p3_sphere_and_split_boxes():
    v, t = cases.sphere_mesh()
    counts = {}
    for k in cases.CELLS_IN_VOXELS:
        cell = k * cases.VOXEL
        vo, to, fo = ref.simplify(v, t, [0, len(v)], cell)
        assert cases.balanced(to) and fo.tolist() == [0, len(vo)]
        cases.check_distances(v, [0, len(v)], cell, vo)
        counts[k] = (len(vo), len(to), int(np.bincount(ref.cluster_of(v["xyz"], [0, len(v)], cell)).max()))
    assert counts == {1: (1071, 2138, 4), 2: (380, 756, 11), 3: (188, 372, 21), 4: (115, 226, 37), 8: (32, 60, 122), 64: (8, 12, 271)}, counts
    assert not cases.balanced(t[:-1])                                            # the check sees an open edge
    sizes = {}
    for axis, cut in wc.SPLITS:
        wv, wt, wf = cases.welded_split(axis, cut)
        assert wc.closed(wt)
        for k in cases.CELLS_IN_VOXELS:
            cell = k * cases.VOXEL
            vo, to, fo = ref.simplify(wv, wt, wf, cell)
            assert cases.balanced(to)
            cases.check_distances(wv, wf, cell, vo)
            assert fo[0] == 0 and fo[-1] == len(vo) and (np.diff(fo) >= 0).all()
            # no cluster crosses the span: the heads below the cut are the clusters of the first span's vertices
            c = ref.cluster_of(wv["xyz"], wf, cell)
            assert c[:wf[1]].max(initial=-1) < fo[1] and c[wf[1]:].min(initial=fo[1]) >= fo[1]
            if k == 3 and axis == 0:
                sizes[cut] = len(vo)
    assert sizes == {1: 188, 15: 190, 30: 188}, sizes


def test_p4_the_table_carries_the_span_times():
    import deform_cases as dc
    from kintinuous_amd import deform_ref
    v, tri, first, times, cell, gname = cases.deform_case()
    vo, to, fo = ref.simplify(v, tri, first, cell)
    assert 0 < len(vo) < len(v) and 0 < fo[1] < len(vo)
    g, x = dc.graph(gname), dc.restated(gname)[0]
    moved = deform_ref.apply_mesh(g, x, vo, fo, times)
    # every representative on its own, with the time of the span its cluster's members lie in
    c = ref.cluster_of(v["xyz"], first, cell)
    span = np.full(len(vo), -1)
    span[c] = (np.arange(len(v)) >= first[1]).astype(int)
    assert (span >= 0).all() and all(len(set((np.arange(len(v))[c == k] >= first[1]).tolist())) == 1 for k in range(len(vo)))
    for s in (0, 1):
        pick = np.nonzero(span == s)[0]
        alone = deform_ref.apply_mesh(g, x, vo[pick], [0, len(pick)], times[s:s + 1])
        assert moved[pick].tobytes() == alone.tobytes()
    assert np.abs(moved["xyz"] - vo["xyz"]).max() > 0


def test_empty_and_errors():
    e = np.zeros(0, mesh_ref.MESH_VERTEX_DTYPE)
    no = np.zeros((0, 3), np.uint32)
    v, t, f = ref.simplify(e, no, [0, 0, 0], 0.1)
    assert len(v) == 0 and len(t) == 0 and f.tolist() == [0, 0, 0]
    assert ref.simplify(e, no, [0], 0.1)[2].tolist() == [0]
    two = np.zeros(2, mesh_ref.MESH_VERTEX_DTYPE)
    for first in ([1, 2], [0, 1], [0, 2, 1, 2], []):
        with pytest.raises(ValueError):
            ref.simplify(two, no, first, 0.1)
        if first:
            with pytest.raises(ValueError):
                cases.brute_simplify(two, no, first, 0.1)
    for cell in (0.0, -0.5, float("inf"), float("nan"), 1e-50):                   # (1e-50 is 0 as a float)
        with pytest.raises(ValueError):
            ref.simplify(two, no, [0, 2], cell)
        with pytest.raises(ValueError):
            cases.brute_simplify(two, no, [0, 2], cell)
    for bad, cell in ((float("nan"), 0.1), (float("inf"), 0.1), (8192.0, 1.0), (-8192.0, 1.0), (1.0, 2.0 ** -19), (-1.0 - 2.0 ** -20, 2.0 ** -19)):
        for axis in range(3):
            b = two.copy()
            b["xyz"][1, axis] = bad
            with pytest.raises(ValueError):
                ref.simplify(b, no, [0, 2], cell)
            with pytest.raises(ValueError):
                cases.brute_simplify(b, no, [0, 2], cell)
    # the last that fit: the largest float below 8192, cell indices 2^19 - 1 and -2^19
    ok = two.copy()
    ok["xyz"][0] = np.nextafter(np.float32(8192), np.float32(0))
    ok["xyz"][1] = -ok["xyz"][0]
    assert len(ref.simplify(ok, no, [0, 2], 1.0)[0]) == 2
    ok["xyz"][0], ok["xyz"][1] = 1.0 - 2.0 ** -20, -1.0
    assert len(ref.simplify(ok, no, [0, 2], 2.0 ** -19)[0]) == 2
