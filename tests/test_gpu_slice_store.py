"""The tracker's slice store (csrc/kt_tracker_slices.hip) over its whole life: all three stages on at once, and a reset and a close while
slab downloads are still in flight."""
import numpy as np
import pytest

from test_gpu_ownership import _held
from test_gpu_slice import _point_set

pytestmark = pytest.mark.gpu

FRAMES = 12


def test_all_stages_reset_and_close_in_flight(ktlib):
    """The first 12 frames of test_gpu_slice.py::test_stage_behind_the_tracker_with_onesweep (160 x 120, "wall", N = 128 over 7 m, a shift on
    nearly every frame: both slab buffers in flight) at the default slice capacity, with the slice stage (cull 3, k = 9), the mesh stage and
    the mesh keys on -- and place recognition, so that slices take samples with them.  Three lives on one context:
    (a) the frames, finalise, every slice read: raw, processed, mesh, keys, pose, pr_id;
    (b) the frames, reset() at once with nothing read, the frames again, finalise, every slice read: equal to (a);
    (c) the frames, close() at once with nothing read.
    After each close the library holds what it held after (a)'s (the context takes its scratch on first use), and with the context closed
    what it held before the first tracker."""
    from kintinuous_amd import abi, synth
    cam = synth.Camera.small(160, 120)
    scene = synth.Scene("wall")
    traj = synth.crabwalk_trajectory(420)
    frames = [synth.render(scene, cam, *traj[4 * i]) for i in range(FRAMES)]
    cfg = abi.TrackerConfig(cam.cols, cam.rows, 128, cam.fx, cam.fy, cam.cx, cam.cy, 7.0, 1, 2, 0, 0, 0, 0, 0, 0, 0, 1)

    def start(c):
        trk = abi.Tracker(c, cfg)
        trk.enable_slice_stage(True, weight_cull=3, k=9)
        trk.enable_mesh_stage(True)
        trk.enable_mesh_keys(True)
        return trk

    def feed(trk):
        for i, (d, rgb) in enumerate(frames):
            trk.process_frame_host(d, rgb, 33333 * i)

    def read(trk):
        trk.finalise()
        ns = trk.num_slices()
        return dict(raw=[trk.slice(i) for i in range(ns)], proc=[trk.slice_processed(i) for i in range(ns)], mesh=[trk.slice_mesh(i) for i in range(ns)],
                    keys=[trk.slice_mesh_keys(i) for i in range(ns)], spose=[trk.slice_pose(i) for i in range(ns)], pr=[trk.slice_pr_id(i) for i in range(ns)],
                    pose=trk.pose(), dense=[trk.dense_pose(i) for i in range(trk.num_poses())], vol=trk.volume().copy(), col=trk.color_volume().copy())

    base = _held()
    c = abi.Ctx(0)
    try:
        trk = start(c)
        try:
            feed(trk)
            a = read(trk)
        finally:
            trk.close()
        warm = abi.live_allocations()

        trk = start(c)
        try:
            feed(trk)
            trk.reset()                      # downloads of the last slabs are still in flight
            assert trk.num_slices() == 0
            feed(trk)
            b = read(trk)
        finally:
            trk.close()
        assert abi.live_allocations() == warm

        trk = start(c)
        try:
            feed(trk)
        finally:
            trk.close()                      # ... and here
        assert abi.live_allocations() == warm
    finally:
        c.close()
    assert abi.live_allocations() == base

    ns = len(a["raw"])
    assert ns - 1 >= 3 and a["raw"][-1][1] == 7 and a["pr"][-1] >= 0      # at least three slabs before CloudSlice::FINAL, which takes a sample
    assert all(p is not None for p in a["proc"]) and all(m is not None for m in a["mesh"])
    assert sum(len(m[0]) for m in a["mesh"]) > 0 and sum(len(p) for p in a["proc"]) > 0
    assert len(b["raw"]) == ns and b["pr"][-1] >= 0
    for run in (a, b):      # the samples that went with slabs are numbered in slab order
        ids = [p for p in run["pr"] if p >= 0]
        assert len(ids) >= 2 and all(x < y for x, y in zip(ids, ids[1:]))
    # reset() takes the global camera from the voxel wrap of the run before it, like KintinuousTracker::reset (KintinuousTracker.cpp:283-291):
    # the first dense pose and the place-recognition tap's starting point -- hence which slab takes the first sample -- are not (a)'s
    assert all(np.array_equal(x, y) for x, y in zip(a["pose"], b["pose"])) and len(a["dense"]) == len(b["dense"]) == FRAMES
    for (ts, p, loop), (ts_b, p_b, loop_b) in list(zip(a["dense"], b["dense"]))[1:]:
        assert ts == ts_b and p.tobytes() == p_b.tobytes()
    assert np.array_equal(a["vol"], b["vol"]) and np.array_equal(a["col"], b["col"])
    for i in range(ns):
        (raw, dim), (raw_b, dim_b) = a["raw"][i], b["raw"][i]
        assert dim == dim_b and _point_set(raw) == _point_set(raw_b), i      # (the extraction appends in no fixed order)
        assert a["proc"][i].tobytes() == b["proc"][i].tobytes(), i
        (v, t), (v_b, t_b) = a["mesh"][i], b["mesh"][i]
        assert v.tobytes() == v_b.tobytes() and t.tobytes() == t_b.tobytes() and len(a["keys"][i]) == len(v), i
        assert a["keys"][i].tobytes() == b["keys"][i].tobytes(), i
        (R, cam_i, ts), (R_b, cam_b, ts_b) = a["spose"][i], b["spose"][i]
        assert R.tobytes() == R_b.tobytes() and cam_i.tobytes() == cam_b.tobytes() and ts == ts_b, i
