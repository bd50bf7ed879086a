"""CPU: the tour and the legs of tests/shift_cases.py load the shift path the way they claim to -- conditions, so that a later change of a
step or a look cannot leave tests/test_gpu_shifts.py comparing empty arrays -- and the restatement of a shifting frame (slab boxes, the
extraction under the wrap of the axes before, the clears, the order) equals the oracle tracker's own slices on every slab."""
import numpy as np

import shift_cases as S
from kintinuous_amd import mesh_weld_ref


def _sign_pattern(dims):
    return tuple(d % 2 for d in sorted(dims))


def test_slab_boxes_state_the_rule():
    n, ov = S.N, S.OVERLAP
    assert S.slab_boxes(0, 3) == ([0, 0, 0], [3 + 1 + ov, n, n], [0, 0, 0], [3, n - 1, n - 1])
    assert S.slab_boxes(2, 3) == ([0, 0, 0], [n, 3 + 1 + ov, n], [0, 0, 0], [n - 1, 3, n - 1])
    assert S.slab_boxes(4, 3) == ([0, 0, 0], [n, n, 3 + 1 + ov], [0, 0, 0], [n - 1, n - 1, 3])
    assert S.slab_boxes(1, -3) == ([n - 3 - ov, 0, 0], [n, n, n], [n - 4, 0, 0], [n - 1, n - 1, n - 1])
    assert S.slab_boxes(3, -3) == ([0, n - 3 - ov, 0], [n, n, n], [0, n - 4, 0], [n - 1, n - 1, n - 1])
    assert S.slab_boxes(5, -3) == ([0, 0, n - 3 - ov - 1], [n, n, n - 1], [0, 0, n - 4], [n - 1, n - 1, n - 1])     # z-minus: one plane low
    for dim in range(6):
        lo, hi, mlo, mhi = S.slab_boxes(dim, -3 if dim % 2 else 3)
        assert all(0 <= a < b <= n for a, b in zip(lo, hi)) and all(0 <= a < b <= n - 1 for a, b in zip(mlo, mhi))    # what the restatements take


def test_tour_is_what_it_claims():
    poses = S.tour_poses()
    assert S.tour_poses() is poses and 60 <= len(poses) <= 110
    assert np.array_equal(poses[0][0], np.eye(3))
    for R, _ in poses:
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0.999
    jumps = S.jumps()
    assert jumps.max() <= S.MAX_JUMP + 1e-9 and jumps.max() >= 9
    # the camera stays inside the room, and outside the sphere and the cube
    scene = S.synth.Scene("room")
    lo, hi = scene.planes_box()
    (centre, radius), = scene.spheres()
    (clo, chi), = scene.cubes()
    for _, c in poses:
        assert ((c > lo + 0.5) & (c < hi - 0.5)).all()
        assert np.linalg.norm(c - np.asarray(centre)) > radius + 0.2 and not ((c > clo - 0.2) & (c < chi + 0.2)).all()
    d, rgb = S.tour_frames()[0]
    cam = S.camera()
    assert d.shape == (cam.rows, cam.cols) and d.dtype == np.uint16 and rgb.shape == (cam.rows, cam.cols, 3) and (d > 0).mean() > 0.9


def test_tour_loads_every_slab_kind(oracle_mod):
    """Conditions, not measurements: what the GPU tests need in order not to pass vacuously.  The figures are printed for the margin."""
    run = S.tour_oracle(oracle_mod)
    assert S.tour_oracle(oracle_mod) is run
    slabs, slices, frames = run["restated"], run["slices"], run["frames"]
    assert len(slabs) == len(slices) - 1 and slices[-1][1] == 7 and len(slices[-1][0]) > 1000
    # every restated cloud is the oracle tracker's slice
    for i, s in enumerate(slabs):
        assert s.dim == slices[i][1] and S.same_points(s.cloud, slices[i][0]), (i, s.dim, len(s.cloud), len(slices[i][0]))
        assert len(s.keys) == len(s.vertices) and (len(s.triangles) == 0 or s.triangles.max() < len(s.vertices))
    most = {d: (max(len(s.cloud) for s in slabs if s.dim == d), max(len(s.vertices) for s in slabs if s.dim == d)) for d in range(6)}
    print("frames", len(S.tour_poses()), "shifting", len(frames), "slabs", len(slabs), "largest (cloud, mesh vertices) per dimension", most)
    for d in range(6):
        assert any(s.dim == d and len(s.cloud) >= 200 and len(s.vertices) >= 100 for s in slabs), (d, most[d])
    assert any(s.dim == 5 and len(s.cloud) >= 200 for s in slabs)                                                   # Z-: the off-by-one box
    three, pairs = {}, {}
    for k, before, after, dims, first in frames:
        mine = slabs[first:first + len(dims)]
        assert [s.dim for s in mine] == dims == sorted(dims) and len({d // 2 for d in dims}) == len(dims)
        assert all(abs(s.vt) == S.SHIFT for s in mine)
        if len(dims) == 3 and all(len(s.cloud) >= 150 and len(s.triangles) > 0 for s in mine):
            three.setdefault(_sign_pattern(dims), []).append((k, [(s.dim, len(s.cloud), len(s.vertices)) for s in mine]))
        if len(dims) == 2 and all(len(s.cloud) > 0 and len(s.triangles) > 0 for s in mine):
            pairs.setdefault(tuple(d // 2 for d in dims), []).append((k, [(s.dim, len(s.cloud), len(s.vertices)) for s in mine]))
    print("three-axis frames with three full slabs:", three)
    print("two-axis frames with two full slabs:", pairs)
    assert len(three) >= 2 and sum(len(v) for v in three.values()) >= 2
    assert set(pairs) == {(0, 1), (0, 2), (1, 2)}
    # a second or third slab of a frame with data in it, on every axis that can come second: the buffer of "two slices ago" is reused
    assert {s.dim // 2 for k, _, _, dims, first in frames for s in slabs[first + 1:first + len(dims)] if len(s.vertices) >= 100} == {1, 2}
    wraps = np.array(run["wrap"])
    print("wrap from", wraps.min(axis=0).tolist(), "to", wraps.max(axis=0).tolist())
    assert (wraps.min(axis=0) < -S.N).any() and (wraps.max(axis=0) > 0).any()
    assert (wraps.min(axis=0) < -S.N).argmax() != (wraps.max(axis=0) > 0).argmax()


def test_restated_meshes_weld_on_seams_of_every_axis(oracle_mod):
    slabs = S.tour_oracle(oracle_mod)["restated"]
    v, k, tri, first, times = S.concat([(s.vertices, s.triangles) for s in slabs], [s.keys for s in slabs])
    merged, seams = S.seam_counts(slabs, k, first)
    wv, wk, wt, wf = mesh_weld_ref.weld(v, k, tri, first, times)
    print("vertices", len(v), "->", len(wv), "merged", merged, "of them across a cut along x, y, z:", seams)
    assert len(wv) == len(v) - merged and min(seams) >= 1
    # no cell is meshed twice before a plane of it has left and come back
    assert S.fresh_cells(slabs) == []
    for s in slabs:      # the keys rise strictly inside a slab: one vertex an edge
        assert (np.diff(s.keys.astype(np.int64)) > 0).all()


def test_icp_legs_shift_in_y_both_ways(oracle_mod):
    legs = {name: S.leg_oracle(oracle_mod, name) for name in S.ICP_SIGNS}
    for name, leg in legs.items():
        print(name, "camera error %.4f m" % leg["error"], "final wrap", leg["wrap"][-1], "dimensions", sorted(set(leg["dims"])), "slabs a frame at the most",
              max(leg["slabs"]))
        assert leg["error"] < 0.03, (name, leg["error"])
    dims = set().union(*(leg["dims"] for leg in legs.values()))
    assert {2, 3} <= dims and any(3 in leg["slabs"] for leg in legs.values())
