"""CPU: the restatement of the smoothing pass (kintinuous_amd/mesh_smooth_ref.py) bit for bit against the independent check of
mesh_smooth_cases (Python sets, exact integers, Python floats), its invariances, what it does to a noisy sphere, and its errors."""
import numpy as np
import pytest

import mesh_smooth_cases as cases
from kintinuous_amd import mesh_smooth_ref as ref

same = lambda a, b: cases.as_bytes(a).tobytes() == cases.as_bytes(b).tobytes()


@pytest.mark.parametrize("name", cases.names())
def test_restatement_equals_the_independent_check(name):
    """(the hub of 65535 near (8000, -8000, 8000) is where |S| and |d q| come nearest to 2^61: the check's exact integers pin that the int64
    sums of the restatement hold them)"""
    for offset in cases.OFFSETS:
        v, tri = cases.case(name, offset)
        for mode in cases.MODES:
            steps = cases.STEPS
            want = cases.check(v, tri, steps, mode=mode)
            for s in steps:
                got, stats = cases.want(name, offset, s, mode)
                assert same(got, want[s][0]) and stats == want[s][1], (name, offset, mode, s)
                assert np.array_equal(got["rgb"], v["rgb"])
                if s == 0:
                    assert same(got, v) and stats[1] == 0                # steps = 0: the input's bytes
                if mode == 0:
                    lo, hi, interior = ref.edges(len(v), tri)
                    rim = np.unique(np.concatenate([lo[~interior], hi[~interior]]))
                    assert same(got[rim], v[rim]) and stats[0] == len(rim)   # pinned: every rim vertex keeps its bytes


def test_laplacian_factors_and_a_rim_that_moves():
    """mu = lambda (plain Laplacian smoothing) and the bounds of both factors against the check; with mode 1 the open tetrahedron's rim
    moves, with mode 0 it does not"""
    v, tri = cases.case("patch 257")
    for lam, mu in ((0.5, 0.5), (1.0, -1.1), (2.0 ** -20, 1.0)):
        for mode in cases.MODES:
            want = cases.check(v, tri, (2,), lam, mu, mode)[2]
            got = ref.smooth(v, tri, 2, lam, mu, mode)
            assert same(got[0], want[0]) and got[1] == want[1]
    v, tri = cases.case("open tetra")
    assert same(ref.smooth(v, tri, 3, mode=0)[0][1:], v[1:]) and ref.smooth(v, tri, 3, mode=0)[1] == (3, 1, 6)
    moved, stats = ref.smooth(v, tri, 3, mode=1)
    assert stats == (3, 4, 6) and (moved["xyz"] != v["xyz"]).any(axis=1).all()


@pytest.mark.parametrize("name", ["patch 4099", "sphere", "hub 64"])
def test_shuffled_triangles_give_the_same_bytes(name):
    v, tri = cases.case(name, cases.OFFSETS[1])
    rng = np.random.default_rng(3)
    shuffled = tri[rng.permutation(len(tri))]
    roll = rng.integers(0, 3, len(tri))
    rolled = np.stack([shuffled[np.arange(len(tri)), (roll + j) % 3] for j in range(3)], axis=1)
    for mode in cases.MODES:
        a, b = cases.want(name, cases.OFFSETS[1], 10, mode), ref.smooth(v, rolled, 10, mode=mode)
        assert same(a[0], b[0]) and a[1] == b[1]


def test_flat_grid_stays_flat_and_a_straight_rim_straight():
    rows, cols = 14, 16
    v, tri = cases.flat_case(rows, cols)
    j, i = np.mgrid[0:rows, 0:cols]
    j, i = j.reshape(-1), i.reshape(-1)
    for mode in cases.MODES:
        out, stats = ref.smooth(v, tri, 10, mode=mode)
        assert (out["xyz"][:, 2] == np.float32(0.5)).all()               # z = 0.5 exactly
        assert stats[0] == 2 * (rows + cols) - 4
        inner = (j > 0) & (j < rows - 1) & (i > 0) & (i < cols - 1)
        assert (out["xyz"][inner] != v["xyz"][inner]).any()
    # mode 1: a rim vertex has its two rim neighbours only.  A corner's lie on two lines, so it leaves both, and its move travels along the
    # rim by one vertex per half-step; after two steps a border vertex five or more from every corner has only ever seen its own line
    out = ref.smooth(v, tri, 2, mode=1)[0]
    corner = ((j == 0) | (j == rows - 1)) & ((i == 0) | (i == cols - 1))
    far = (np.minimum(i, cols - 1 - i) >= 5) | (np.minimum(j, rows - 1 - j) >= 5)
    for line, axis in (((j == 0) | (j == rows - 1), 1), ((i == 0) | (i == cols - 1), 0)):
        on = line & far
        assert on.sum() >= 4 and np.array_equal(out["xyz"][on, axis], v["xyz"][on, axis])
    assert (out["xyz"][corner, :2] != v["xyz"][corner, :2]).all()


def test_noisy_sphere_is_smoothed_and_keeps_its_size():
    """the N = 32 sphere (1946 vertices, radius 0.95 m) with 1 % radial noise, 10 steps.  The restatement gives: the radius's standard
    deviation x 0.374, the mean radius +0.088 %; with mu = lambda = 0.5 x 0.354 and -4.04 %"""
    v, tri = cases.noisy_sphere()
    r0 = cases.radii(v)
    assert 0.009 < r0.std() < 0.010
    for mode in cases.MODES:                                              # (a closed mesh: the modes agree)
        r = cases.radii(ref.smooth(v, tri, 10, mode=mode)[0])
        print("lambda|mu: std x %.4f, mean %+.4f %%" % (r.std() / r0.std(), 100 * (r.mean() / r0.mean() - 1)))
        assert r.std() < 0.5 * r0.std()                                   # measured 0.374
        assert abs(r.mean() / r0.mean() - 1) < 0.01                       # measured +0.00088
        r = cases.radii(ref.smooth(v, tri, 10, 0.5, 0.5, mode)[0])
        print("Laplacian: std x %.4f, mean %+.4f %%" % (r.std() / r0.std(), 100 * (r.mean() / r0.mean() - 1)))
        assert r.mean() / r0.mean() - 1 < -0.03                           # measured -0.0404: plain Laplacian smoothing shrinks


def test_errors_name_their_cause():
    v, tri = cases.case("patch 257")
    n = len(v)
    live = np.flatnonzero((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2]))
    loose = np.setdiff1d(np.arange(n), tri)

    def refused(cause, word, vb, tb, **kw):
        with pytest.raises(ValueError, match=cause):
            ref.smooth(vb, tb, **{**dict(steps=1), **kw})
        if word:
            with pytest.raises(ValueError, match=word):
                cases.check(vb, tb, (kw.get("steps", 1),), kw.get("lam", cases.LAMBDA), kw.get("mu", cases.MU), kw.get("mode", 0))

    tb = tri.copy()
    tb[len(tri) // 2, 1] = n
    refused("index out of range", "index", v, tb)
    for k, (axis, val) in enumerate(((0, np.nan), (1, np.inf), (2, 8192.0), (0, -8192.0), (1, -np.inf))):
        vb = v.copy()
        vb["xyz"][tri[live[7 * k], k % 3], axis] = val
        refused("not finite or has a coordinate", "vertex", vb, tri)
        vu = v.copy()                                                     # the same bad vertex, unreferenced: accepted and copied
        vu["xyz"][loose[-1], axis] = val
        got = ref.smooth(vu, tri, 1)
        assert same(got[0], cases.check(vu, tri, (1,))[1][0]) and same(got[0][loose[-1]], vu[loose[-1]])
    refused("valence over the bound", "valence", *cases.hub_case(65536))
    refused("valence over the bound", "valence", *cases.hub_case(65536), mode=1)
    lv, lt, kw = cases.left_range_case()
    refused("left the range", "range", lv, lt, **kw)
    assert ref.smooth(lv, lt, 1, 0.5, -0.9, 0)[1] == (3, 1, 6)            # 8095.95 + 0.9 * 95.95 stays inside
    for kw, cause in ((dict(steps=-1), "steps"), (dict(steps=65), "steps"), (dict(lam=0.0), "lambda"), (dict(lam=1.5), "lambda"), (dict(lam=np.nan), "lambda"),
                      (dict(mu=-1.2), "mu"), (dict(mu=1.5), "mu"), (dict(mu=np.nan), "mu"), (dict(mode=2), "mode"), (dict(mode=-1), "mode")):
        refused(cause, None, v, tri, **kw)
    assert ref.smooth(v, tri, 64, mode=1)[1][1] > 0 and ref.smooth(v, tri, 1, 1.0, -1.1, 1)[1][1] > 0     # the bounds themselves are allowed
    assert ref.smooth(v, tri, 1, 1.0, 1.0, 1)[1][1] > 0
    # n = 0: the triangles are not looked at; m = 0: the output is the input
    out, stats = ref.smooth(v[:0], tri, 5)
    assert len(out) == 0 and stats == (0, 0, 0)
    out, stats = ref.smooth(v, tri[:0], 5)
    assert same(out, v) and stats == (0, 0, 0)
