"""CPU: the quadric form of the mesh simplification's restatement (mesh_simplify_ref.simplify_quadric) against a brute-force twin on
Python dicts, exact Python integers and scalar doubles, and the properties of the definition: everything but the xyz of a cluster of
more than one member is simplify()'s; the result depends on neither the order of the triangles nor their rotation; a placed
representative keys into its own cell; on a plane it is the mean; on a cube it stays on the edges and corners the mean rounds off."""
import numpy as np
import pytest

import mesh_simplify_cases as mean_cases
import mesh_simplify_quadric_cases as cases
from kintinuous_amd import mesh_ref, mesh_simplify_ref as ref

BIASES = (2.0 ** -6, 2.0 ** -10)
CUBE_CELLS = (0.11, 0.2, 0.33)


def _params(n):
    return ((n, 6, 3.0, 2.0 ** -6), (n + 1, 9, 1.0, 2.0 ** -10), (n + 2, 1, 20.0, 1.0), (n + 3, 40, 4.0, 2.0 ** -20))


def _own_cell(case, out, placed_only=True):
    """every representative that differs from the mean form's keys into the cell of its cluster"""
    v, tri, first, cell = case
    want = ref.simplify(v, tri, first, cell)[0]
    moved = (out["xyz"].view(np.uint32) != want["xyz"].view(np.uint32)).any(axis=1)
    cl = ref.cluster_of(v["xyz"], first, cell)
    head_key = np.zeros(len(out), np.uint64)
    head_key[cl[::-1]] = ref.cell_keys(v["xyz"], cell)[::-1]
    assert np.array_equal(ref.cell_keys(out["xyz"][moved], cell), head_key[moved])
    return moved


@pytest.mark.parametrize("n", cases.SIZES)
def test_random_lists_against_the_twin(n):
    for seed, spans, per, bias in _params(n):
        case = cases.random_case(seed, n, spans, per)
        got, want = ref.simplify_quadric(*case, bias), cases.brute_quadric(*case, bias)
        cases.same4(got, want)
        S = ref.quadric_sums(*case)
        assert S.tolist() == cases.brute_sums(*case)
        mean = ref.simplify(*case)
        cases.same(got[1:3], mean[1:])                                                   # triangles and table: the mean form's
        assert got[0]["rgb"].tobytes() == mean[0]["rgb"].tobytes()
        single = ~cases.multi_member(*case[:1], case[2], case[3]) if n else np.zeros(0, bool)
        assert got[0][single].tobytes() == mean[0][single].tobytes()                     # a cluster of one keeps its 16 bytes
        moved = _own_cell(case, got[0])
        assert moved.sum() <= got[3] <= (~single).sum()
        if n >= 257:
            assert got[3] > 0 and 0 < len(got[1]) < len(case[1])
            tc = ref.cluster_of(case[0]["xyz"], case[2], case[3])[case[1].astype(np.int64)]
            distinct = 1 + (tc[:, 1] != tc[:, 0]) + ((tc[:, 2] != tc[:, 0]) & (tc[:, 2] != tc[:, 1]))
            assert set(distinct.tolist()) == {1, 2, 3}                                   # triangles in one, two and three clusters


def test_sized_clusters_many_spans_one_cluster():
    case = cases.sized_clusters_case()
    sizes = np.bincount(ref.cluster_of(case[0]["xyz"], case[2], case[3]))
    assert sorted(sizes.tolist()) == sorted(list(cases.CLUSTER_SIZES) * 3)
    got = ref.simplify_quadric(*case, cases.DEFAULT_BIAS)
    cases.same4(got, cases.brute_quadric(*case, cases.DEFAULT_BIAS))
    assert got[3] > 0
    case = cases.many_spans_case()
    cases.same4(ref.simplify_quadric(*case, 2.0 ** -10), cases.brute_quadric(*case, 2.0 ** -10))
    case = cases.one_cluster_case()
    got = ref.simplify_quadric(*case, cases.DEFAULT_BIAS)
    assert len(got[0]) == 1 and len(got[1]) == 0 and got[2].tolist() == [0, 1]
    cases.same4(got, cases.brute_quadric(*case, cases.DEFAULT_BIAS))
    assert np.abs(ref.quadric_sums(*case)).max() > 1 << 36                               # every triangle's terms in the same nine sums


def test_a_small_cell_returns_the_sphere():
    v, t = mean_cases.sphere_mesh()
    out = ref.simplify_quadric(v, t, [0, len(v)], 1e-4, cases.DEFAULT_BIAS)
    cases.same4(out, (v, t, np.array([0, len(v)], np.int64), 0))


def test_order_and_rotation_of_the_triangles_do_not_matter():
    rng = np.random.default_rng(5)
    for case in (cases.random_case(11, 4099, 9, 3.0), cases.sized_clusters_case(), (*mean_cases.sphere_mesh(), np.array([0, 1946]), 3 * mean_cases.VOXEL)):
        v, tri, first, cell = case
        want = ref.simplify_quadric(v, tri, first, cell, cases.DEFAULT_BIAS)
        S = ref.quadric_sums(v, tri, first, cell)
        perm = rng.permutation(len(tri))
        rolled = np.stack([np.roll(row, k) for row, k in zip(tri, rng.integers(0, 3, len(tri)))])
        assert np.array_equal(ref.quadric_sums(v, tri[perm], first, cell), S) and np.array_equal(ref.quadric_sums(v, rolled, first, cell), S)
        got = ref.simplify_quadric(v, tri[perm], first, cell, cases.DEFAULT_BIAS)
        assert got[0].tobytes() == want[0].tobytes() and got[3] == want[3]
        assert np.array_equal(got[1], ref.simplify(v, tri[perm], first, cell)[1])          # the survivors in the new order
        got = ref.simplify_quadric(v, rolled, first, cell, cases.DEFAULT_BIAS)
        assert got[0].tobytes() == want[0].tobytes() and got[3] == want[3]
        assert np.array_equal(got[1], ref.simplify(v, rolled, first, cell)[1])


def test_plane_representatives_are_the_means():
    """On a tilted plane every placed representative lies within 2^-17 m of the plane and of the float64 mean of its cluster: the planes
    fix the normal coordinate, the bias (the driver's default, 2^-6) the two tangential ones.
    What the bound has to cover, besides the integer mean's 2^-21 and a float ulp at 1 m (2^-23): the 2^-33 by which a term is rounded.
    On a plane every triangle of a cluster has the same d, so the three b terms of all its triangles are rounded the same way and the
    errors add up instead of averaging out; against the tangential stiffness bias * sum |c| that is up to sqrt(3) 2^-33 / (bias |c|),
    and the six A terms add up to 3 (2^-33 / |c|) |m| / bias with |m| <= the cell's half diagonal.  The patch is therefore one of 6 cm
    squares (|c| = 3.9e-3 m^2) clustered at 0.33 m: 3.3e-6 + 1.7e-6 + 0.5e-6 m < 2^-17 m = 7.6e-6 m.  At the 1.5 cm squares of a
    40 x 40 grid over 0.6 m (|c| = 2.4e-4 m^2, cell 0.11 m) the same sum is 3.6e-5 m and the restatement is 4.3e-5 m off the mean,
    5.2e-7 m off the plane: the fixed point of the terms, not the solve (the float64 version of the cases is 7e-9 m off the mean there)."""
    v, tri = cases.plane_patch(20, 1.2)
    first, cell = np.array([0, len(v)]), 0.33
    out, _, _, placed = ref.simplify_quadric(v, tri, first, cell, cases.DEFAULT_BIAS)
    many = cases.multi_member(v, first, cell)
    cl = ref.cluster_of(v["xyz"], first, cell)
    mean64 = np.stack([np.bincount(cl, v["xyz"][:, a].astype(np.float64)) for a in range(3)], axis=1) / np.bincount(cl)[:, None]
    assert placed == many.sum() > 9                                                      # every cluster of more than one member is placed
    xyz = out["xyz"].astype(np.float64)[many]
    off_plane = np.abs((xyz - cases.PLANE_POINT) @ cases.PLANE_NORMAL)
    off_mean = np.sqrt(((xyz - mean64[many]) ** 2).sum(axis=1))
    print("plane: %d of %d placed, off the plane %.3g m, off the mean %.3g m (bound %.3g)" % (placed, many.sum(), off_plane.max(), off_mean.max(), 2.0 ** -17))
    assert off_plane.max() <= 2.0 ** -17 and off_mean.max() <= 2.0 ** -17


@pytest.mark.parametrize("cell", CUBE_CELLS)
def test_cube_keeps_its_edges(cell):
    """the unit cube on a 40 x 40 grid per face, offset by 0.0137 m: every cluster of more than one member is placed; the largest distance
    of a representative to the cube is at most 1 / 32 of the mean form's at a bias of 2^-10 and at most 1 / 8 at 2^-6"""
    v, tri = cases.cube_mesh()
    first = np.array([0, len(v)])
    many = cases.multi_member(v, first, cell)
    mean_far = cases.cube_distance(ref.simplify(v, tri, first, cell)[0]["xyz"]).max()
    for bias, part in ((2.0 ** -10, 32.0), (2.0 ** -6, 8.0)):
        out, to, _, placed = ref.simplify_quadric(v, tri, first, cell, bias)
        far = cases.cube_distance(out["xyz"]).max()
        print("cube, cell %.2f, bias 2^%d: mean form %.4f m, quadric form %.6f m (1 / %.0f), %d clusters placed" % (cell, np.log2(bias), mean_far, far, mean_far / far, placed))
        assert placed == many.sum() >= len(out) - 1                                  # (the far corner's cell holds one vertex)
        assert far <= mean_far / part
        assert mean_cases.balanced(to)


# the gaps measured between the restatement and the unquantised float64 version (metres, the largest over the placed clusters)
FLOAT64_GAP = {"cube": 6.8e-7, "sphere": 2.5e-6}


@pytest.mark.parametrize("name", ["cube", "sphere"])
def test_against_an_unquantised_float64_solve(name):
    """the restatement against float64 sums, the float64 mean and numpy.linalg.solve: what the fixed point (2^-32 per term, 2^-20 in the
    mean) and the float result cost.  Asserted at ten times the measured gap"""
    if name == "cube":
        v, tri = cases.cube_mesh()
        cells = CUBE_CELLS
    else:
        v, tri = mean_cases.sphere_mesh()
        cells = tuple(k * mean_cases.VOXEL for k in (2, 3, 4))
    first = np.array([0, len(v)])
    worst = 0.0
    for cell in cells:
        for bias in BIASES:
            out, _, _, placed = ref.simplify_quadric(v, tri, first, cell, bias)
            mean = ref.simplify(v, tri, first, cell)[0]
            moved = (out["xyz"].view(np.uint32) != mean["xyz"].view(np.uint32)).any(axis=1)
            f64, solved = cases.float64_quadric(v, tri, first, cell, bias)
            assert moved.sum() > 0 and solved[moved].all()
            worst = max(worst, float(np.abs(out["xyz"].astype(np.float64)[moved] - f64[moved]).max()))
    print("%s: the restatement against the float64 solve: %.3g m" % (name, worst))
    assert worst <= 10 * FLOAT64_GAP[name]


def test_empty_and_errors():
    e = np.zeros(0, mesh_ref.MESH_VERTEX_DTYPE)
    no = np.zeros((0, 3), np.uint32)
    v, t, f, p = ref.simplify_quadric(e, no, [0, 0, 0], 0.1, 0.5)
    assert len(v) == 0 and len(t) == 0 and f.tolist() == [0, 0, 0] and p == 0
    case = cases.random_case(9, 257, 6, 3.0)
    v, tri, first, cell = case
    ref.simplify_quadric(*case, 2.0 ** -20)
    ref.simplify_quadric(*case, 1.0)
    for bias in (0.0, 2.0 ** -21, np.nextafter(np.float32(2.0 ** -20), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)), 2.0, -0.5, float("nan"), float("inf"), float("-inf")):
        for f in (ref.simplify_quadric, cases.brute_quadric):
            with pytest.raises(ValueError):
                f(*case, bias)
    for f in (ref.simplify_quadric, cases.brute_quadric):
        for bad in (len(v), len(v) + 7, 0xffffffff):
            tb = tri.copy()
            tb[len(tb) // 2, 1] = bad
            with pytest.raises(ValueError):
                f(v, tb, first, cell, 0.5)
        # a term of 1 or more: one 2 m triangle (c = 4 m^2)
        big = np.zeros(3, mesh_ref.MESH_VERTEX_DTYPE)
        big["xyz"][1, 0], big["xyz"][2, 1] = 2.0, 2.0
        one = np.array([[0, 1, 2]], np.uint32)
        with pytest.raises(ValueError):
            f(big, one, [0, 3], 0.25, 0.5)
        big["xyz"] *= 0.25                                                                # ... and one of half a metre fits
        assert len(f(big, one, [0, 3], 0.25, 0.5)[0]) == 3
        for val, axis in ((float("nan"), 0), (float("inf"), 1), (8192.0, 2), (-8192.0, 0)):
            vb = v.copy()
            vb["xyz"][5, axis] = val
            with pytest.raises(ValueError):
                f(vb, tri, first, cell, 0.5)
        for table in ([1] + first[1:].tolist(), first[:-1].tolist() + [len(v) - 1], [0, 9, 5] + first[3:].tolist()):
            with pytest.raises(ValueError):
                f(v, tri, table, cell, 0.5)
        for c in (0.0, -0.5, float("inf"), float("nan")):
            with pytest.raises(ValueError):
                f(v, tri, first, c, 0.5)
