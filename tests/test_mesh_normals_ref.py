"""CPU: the numpy restatement of the vertex normals (kintinuous_amd/mesh_normals_ref.py) against the definition written out one triangle
at a time (mesh_normals_cases.brute_normals), the derived bound on what the 2^-32 fixed point costs against a float64 sum, the plane,
the sphere, the permutation of the triangle list, the errors, and the PLY writer kt_host_save_ply_normals (no GPU needed)."""
import numpy as np
import pytest

import mesh_normals_cases as cases
from kintinuous_amd import mesh_normals_ref as ref

V = cases.V


@pytest.mark.parametrize("m", cases.TRIANGLE_COUNTS)
def test_restatement_equals_the_definition(m):
    for k, offset in enumerate(cases.OFFSETS):
        v, t = cases.random_case(100 * m + k, m, offset)
        got, want = ref.normals(v, t), cases.brute_normals(v, t)
        assert got[1] == want[1]
        assert np.array_equal(cases.as_bytes(got[0]), cases.as_bytes(want[0]))
        if m >= 63:
            assert 4 <= got[1] < len(v)                        # the unreferenced vertices, and not every vertex


def test_no_vertices_no_normals_whatever_the_triangles():
    """n = 0 with m > 0 is KT_OK on the device (the triangles are not looked at): the restatement and the definition say the same"""
    tri = np.array([[0, 1, 2], [7, 7, 9]], np.uint32)
    for f in (ref.normals, cases.brute_normals):
        nrm, n_zero = f(np.zeros(0, V), tri)
        assert nrm.shape == (0, 3) and nrm.dtype == np.float32 and n_zero == 0
    nrm, n_zero = ref.normals(np.zeros(5, V), tri[:0])                     # m = 0: n zero normals
    assert nrm.shape == (5, 3) and not nrm.any() and n_zero == 5


def test_fans_and_cancellation_equal_the_definition():
    for k in (1, 2, 65, 257):
        v, t = cases.fan_case(k)
        got, want = ref.normals(v, t), cases.brute_normals(v, t)
        assert got[1] == want[1] == 0 and np.array_equal(cases.as_bytes(got[0]), cases.as_bytes(want[0]))
    v, t = cases.cancelling_case()
    nrm, n_zero = ref.normals(v, t)
    assert n_zero == len(v) and not nrm.any()


def _angle(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.arctan2(np.sqrt((np.cross(a, b) ** 2).sum(axis=1)), (a * b).sum(axis=1))


def _check_quantisation_bound(v, t):
    """A triangle's q differs from c 2^32 by at most 1/2 per component, so its term by at most sqrt(3) 2^-33 in length; a vertex of valence
    k with an unquantised sum of length L: an angle of at most sqrt(3) k 2^-33 / L, plus 2^-22 for the float32 rounding of three components"""
    nrm, _ = ref.normals(v, t)
    S, k = cases.float64_sums(v, t)
    L = np.sqrt((S * S).sum(axis=1))
    slack = np.sqrt(3.0) * k * 2.0 ** -33
    zero = ~nrm.any(axis=1)
    assert (L[zero] <= slack[zero]).all()                      # a zero normal: the unquantised sum is within the fixed point's error of zero
    live = ~zero
    assert live.any()
    angle = _angle(nrm[live], S[live])
    bound = slack[live] / L[live] + 2.0 ** -22
    print("largest angle %.3g rad, smallest margin %.3g rad, at valence up to %d" % (angle.max(), (bound - angle).min(), k.max()))
    assert (angle <= bound).all()
    return nrm


def test_quantisation_bound_on_the_sphere_and_a_random_case():
    _check_quantisation_bound(*cases.sphere_mesh())
    for offset in cases.OFFSETS:
        _check_quantisation_bound(*cases.random_case(77, 4099, offset))


@pytest.mark.parametrize("flip", [False, True])
def test_plane_is_exact(flip):
    v, t = cases.plane_case(flip)
    nrm, n_zero = ref.normals(v, t)
    assert n_zero == 0
    want = np.zeros((len(v), 3), np.float32)
    want[:, 2] = -1.0 if flip else 1.0
    assert np.array_equal(cases.as_bytes(nrm), cases.as_bytes(want))


def test_sphere_normals_are_unit_and_point_outwards():
    """mesh_weld_cases.sphere_volume holds r - 10.15 voxels: F < 0 inside, F > 0 outside, so (v1 - v0) x (v2 - v0), which points to F > 0,
    points away from the centre at every vertex"""
    v, t = cases.sphere_mesh()
    nrm, n_zero = ref.normals(v, t)
    length = np.sqrt((nrm.astype(np.float64) ** 2).sum(axis=1))
    zero = ~nrm.any(axis=1)
    assert int(zero.sum()) == n_zero
    assert (np.abs(length[~zero] - 1.0) <= 2.0 ** -22).all()
    x = v["xyz"].astype(np.float64)
    tt = t.astype(np.int64)
    area = np.sqrt((np.cross(x[tt[:, 1]] - x[tt[:, 0]], x[tt[:, 2]] - x[tt[:, 0]]) ** 2).sum(axis=1))
    assert not zero[tt[area > 0]].any()                        # no vertex of a triangle with an area is left without a normal
    out = x - cases.SPHERE_CENTRE
    dots = (nrm.astype(np.float64) * out).sum(axis=1)[~zero]
    assert (dots > 0).all()
    print("sphere: %d vertices, %d zero normals, smallest cosine to the radius %.3f" % (len(v), n_zero, (dots / np.sqrt((out[~zero] ** 2).sum(axis=1))).min()))


def test_permuting_the_triangles_changes_no_byte():
    rng = np.random.default_rng(3)
    for v, t in (cases.sphere_mesh(), cases.random_case(5, 4099, cases.OFFSETS[1]), cases.fan_case(2049)):
        want = ref.normals(v, t)
        for _ in range(3):
            got = ref.normals(v, t[rng.permutation(len(t))])
            assert got[1] == want[1] and np.array_equal(cases.as_bytes(got[0]), cases.as_bytes(want[0]))


def test_errors_name_their_cause():
    v, t = cases.random_case(8, 257)
    n = len(v)
    ref.normals(v, t)
    tb = t.copy()
    tb[100, 2] = n
    for f in (ref.normals, cases.brute_normals):
        with pytest.raises(ValueError, match="index"):
            f(v, tb)
    used = int(t[50, 1])
    assert len(set(t[50].tolist())) == 3
    for val in (float("nan"), 8192.0, -8192.0, float("inf")):
        vb = v.copy()
        vb["xyz"][used, 1] = val
        for f in (ref.normals, cases.brute_normals):
            with pytest.raises(ValueError, match="vertex"):
                f(vb, t)
        vu = v.copy()                                          # the same values in a vertex no triangle references: accepted, (0, 0, 0)
        vu["xyz"][n - 3, 1] = val
        nrm, n_zero = ref.normals(vu, t)
        assert not nrm[n - 3].any() and n_zero == ref.normals(v, t)[1]
    # a right triangle with legs 1 and 1: a cross component of exactly 1.0; legs 1 and nextafter(1, 0): accepted
    tri = np.array([[0, 1, 2]], np.uint32)
    big = np.zeros(3, V)
    big["xyz"] = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]
    for f in (ref.normals, cases.brute_normals):
        with pytest.raises(ValueError, match="large"):
            f(big, tri)
    big["xyz"][2, 1] = np.nextafter(np.float32(1.0), np.float32(0.0))
    nrm, n_zero = ref.normals(big, tri)
    assert n_zero == 0 and np.array_equal(nrm, np.array([[0, 0, 1]] * 3, np.float32))
    assert np.array_equal(cases.as_bytes(cases.brute_normals(big, tri)[0]), cases.as_bytes(nrm))


# ---- the PLY with normals -------------------------------------------------------------------------------------------------------------------
def test_ply_with_normals(tmp_path):
    from kintinuous_amd import abi
    assert abi.MESH_NORMAL_DTYPE.itemsize == 12
    v, t = cases.random_case(4, 257)
    v = v.copy()
    v["xyz"][-2:] = 1.0                                        # (finite rows read back equal)
    nrm = np.zeros(len(v), abi.MESH_NORMAL_DTYPE)
    nrm["normal"] = ref.normals(v, t)[0]
    path = str(tmp_path / "n.ply")
    for vv, nn, tt in ((v, nrm, t), (v[:0], nrm[:0], t[:0]), (v, nrm, t[:0])):
        abi.save_ply_normals(path, vv, nn, tt)
        pv, pt = cases.read_ply_normals(path)
        assert np.array_equal(cases.as_bytes(pv["xyz"]), cases.as_bytes(vv["xyz"])) and np.array_equal(cases.as_bytes(pv["normal"]), cases.as_bytes(nn["normal"]))
        assert np.array_equal(pv["rgb"][:, 0], (vv["rgb"] >> 16) & 255) and np.array_equal(pv["rgb"][:, 1], (vv["rgb"] >> 8) & 255)
        assert np.array_equal(pv["rgb"][:, 2], vv["rgb"] & 255)
        assert np.array_equal(pt, tt.astype(np.int32))
    with pytest.raises(abi.KtError, match="out of range"):
        abi.save_ply_normals(path, v, nrm, np.array([[0, 1, len(v)]], np.uint32))
