"""CPU only.  The numpy restatement of the loop-closure registration stage (kintinuous_amd/loop_icp_ref.py; DESIGN.md 4.6, the stage that
replaces PlaceRecognition::icpDepthFrames, backend/PlaceRecognition.cpp:238-276) against code that is already pinned and against an
independent float64 implementation (tests/loop_icp_cases.py: scipy cKDTree, double everywhere), on synth.render pairs of the room scene
whose relative pose is known."""
import numpy as np
import pytest

import loop_icp_cases as lc

SIZES = [(160, 120), (640, 480)]


@pytest.mark.parametrize("cols,rows", SIZES)
def test_grid_equals_the_pinned_oracle(oracle_mod, cols, rows):
    """Step b is the slice stage's VoxelGrid on points of zero colour: the oracle's kto_slice_process (pinned by tests/test_slice_process.py
    and tests/test_slice_independent.py) on the same points, weight_cull = 0, same leaf, must give the same centroids in the same order,
    bit for bit."""
    from kintinuous_amd import loop_icp_ref as ref
    cam, depth = lc.render(cols, rows, "B")
    cloud = ref.depth_to_cloud(depth, cam.fx, cam.fy, cam.cx, cam.cy, 4.0)
    assert len(cloud) > cols * rows // 2
    # the cloud itself: the reference's order (column outer) and its float expression, spot-checked against a scalar restatement
    kept = [(u, v) for u in range(cols) for v in range(rows) if depth[v, u] != 0 and depth[v, u] < 4000]
    assert len(kept) == len(cloud)
    for k in (0, 1, len(kept) // 3, len(kept) - 1):
        u, v = kept[k]
        z = np.float32(depth[v, u]) * np.float32(0.001)
        x = (np.float32(u) - np.float32(cam.cx)) * z * (np.float32(1.0) / np.float32(cam.fx))
        y = (np.float32(v) - np.float32(cam.cy)) * z * (np.float32(1.0) / np.float32(cam.fy))
        assert cloud[k].tobytes() == np.array([x, y, z], np.float32).tobytes()
    pts = np.zeros(len(cloud), oracle_mod.POINT_DTYPE)
    pts["xyz"] = cloud
    want = oracle_mod.slice_process(pts, 0, lc.LEAF, 1)["xyz"]
    got = ref.voxel_grid(cloud, lc.LEAF)
    assert got.shape == want.shape and len(got) > 1000
    assert got.tobytes() == np.ascontiguousarray(want).tobytes()


def test_nearest_tie_rule():
    from kintinuous_amd import loop_icp_ref as ref
    dst = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    src = np.array([[0.5, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)          # midway between 0 and 1; on the duplicates; midway between 0 and 3
    idx, d2 = ref.nearest(src, dst, chunk_elems=4)
    assert idx.tolist() == [0, 1, 0] and d2.tolist() == [0.25, 0.0, 1.0]


def test_host_rigid_fit_matches_the_svd_fit(ktlib):
    """kt_host_rigid_fit (Horn's quaternion, Jacobi, double; no GPU work) against the restatement's SVD fit: the same optimum, also where
    the best orthogonal matrix would be a reflection (a planar, mirrored pair)."""
    from kintinuous_amd import abi, loop_icp_ref as ref
    rng = np.random.default_rng(3)
    for case in range(6):
        s = rng.normal(size=(200, 3)) * [1.0, 1.0, 0.0 if case >= 4 else 0.3]
        t = s @ lc._rot(rng.normal(size=3), rng.uniform(0, 3.0)).T + rng.normal(size=3) + 1e-3 * rng.normal(size=s.shape)
        if case == 5:
            t = t * [1, 1, -1]
        sums = np.r_[s.sum(0), t.sum(0), (s[:, :, None] * t[:, None, :]).sum(0).ravel()]
        dM = abi.host_rigid_fit(sums, len(s))
        assert abs(np.linalg.det(dM[:3, :3]) - 1) < 1e-12 and np.abs(dM[:3, :3] @ dM[:3, :3].T - np.eye(3)).max() < 1e-12
        want = ref.rigid_fit(s, t)
        cost = lambda M: ((s @ M[:3, :3].T + M[:3, 3] - t) ** 2).sum()
        assert cost(dM) <= cost(want) * (1 + 1e-9) + 1e-18
        if case < 4:
            assert np.abs(dM - want).max() < 1e-9


@pytest.mark.parametrize("cols,rows", SIZES)
def test_restatement_against_independent_float64(cols, rows):
    """The restatement and the independent float64 run on the pair (A, B): 3 degrees and 6 cm apart, bootstrap = the truth perturbed by 1
    degree and 2 cm (seeded).  They must agree with each other far more tightly than either agrees with the truth: the restatement differs
    from the float64 run by float32 points (2^-24 of a few metres) and tie breaks only, so a tenth of the float64 run's own distance to the
    truth is a generous bound on their distance; and the restatement's distance to the truth is held to 1.5 x the float64 run's own.

    Measured (rotation rad, translation m), both sizes hit the 10-iteration cap:
      160x120  restatement - float64 (5.8e-09, 3.9e-08); float64 - truth (1.740e-02, 3.512e-02); restatement - truth (1.740e-02, 3.512e-02)
      640x480  restatement - float64 (4.4e-08, 1.8e-07); float64 - truth (1.850e-02, 3.199e-02); restatement - truth (1.850e-02, 3.199e-02)
    (Nearest-neighbour point-to-point ICP on two partly overlapping room views does not improve on a 1 degree / 2 cm bootstrap: the
    points slide along the walls.  That is the reference's method; its score, not its pose, gates the constraint.)"""
    from kintinuous_amd import loop_icp_ref as ref
    cam, d1 = lc.render(cols, rows, "A")
    _, d2 = lc.render(cols, rows, "B")
    M64, score64, its64, _ = lc.run64(cols, rows)
    M, score, info = ref.icp_depth_frames(d1, d2, cam.fx, cam.fy, cam.cx, cam.cy, lc.bootstrap(), lc.LEAF, 4.0, 10)
    e64, e, dist = lc.pose_error(M64, lc.truth()), lc.pose_error(M, lc.truth()), lc.pose_distance(M, M64)
    print(f"{cols}x{rows}: restatement-float64 {dist}, float64-truth {e64}, restatement-truth {e}, scores {score} {score64}, iterations {info} {its64}")
    assert info["n_source"] > 5000 and info["n_target"] > 5000
    assert dist[0] <= 0.1 * e64[0] and dist[1] <= 0.1 * e64[1]
    assert e[0] <= 1.5 * e64[0] and e[1] <= 1.5 * e64[1]
    assert abs(score - score64) <= 0.1 * score64


def test_score_separates_pairs():
    """(A, B) overlap; (A, C) look at different walls, same bootstrap.  The float64 run alone puts the first below 0.005 and the second
    above 0.02 -- a factor of two on either side of the reference's 0.01 gate (PlaceRecognition.cpp:196) -- and the restatement must fall
    on the same sides of 0.01."""
    from kintinuous_amd import loop_icp_ref as ref
    cam, d1 = lc.render(160, 120, "A")
    s64_b, s64_c = lc.run64(160, 120, "B")[1], lc.run64(160, 120, "C")[1]
    assert s64_b < 0.005 and s64_c > 0.02, (s64_b, s64_c)
    for to, below in (("B", True), ("C", False)):
        _, d2 = lc.render(160, 120, to)
        _, score, _ = ref.icp_depth_frames(d1, d2, cam.fx, cam.fy, cam.cx, cam.cy, lc.bootstrap(), lc.LEAF, 4.0, 10)
        assert (score < 0.01) == below, (to, score)


def test_degenerate_inputs():
    from kintinuous_amd import loop_icp_ref as ref
    cam, d1 = lc.render(160, 120, "A")
    zero = np.zeros_like(d1)
    for a, b in ((zero, d1), (d1, zero)):
        M, score, info = ref.icp_depth_frames(a, b, cam.fx, cam.fy, cam.cx, cam.cy, lc.bootstrap(), lc.LEAF)
        assert np.array_equal(M, lc.bootstrap()) and score == float("inf") and info["iterations"] == 0 and not info["converged"]
