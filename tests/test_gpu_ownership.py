"""Ownership of device memory, pinned memory, events and streams (csrc/kt_common.hpp: kt_mem): what a tracker, the integrate scratch and the
plans take comes back when their owner goes, also when the owner could not be completed.  kt_debug_live_allocations counts what all owners of
the process hold; kt_debug_fail_allocation makes one request return KT_ERR_NOMEM on the host (no HIP call, no kernel in a failing state).
Shapes: 64x48 into N = 32, the smallest a tracker takes (cols % 8 == rows % 8 == 0, N a multiple of the brick) -- a list is checked here, not
arithmetic."""
import gc
import re
import time

import numpy as np
import pytest

from test_gpu_volume import _integrate_both, _maps

pytestmark = pytest.mark.gpu

N = 32


def _scene(cols, rows, nframes):
    from kintinuous_amd import synth
    cam = synth.Camera.small(cols, rows)
    scene = synth.Scene("room")
    return cam, [synth.render(scene, cam, R, c) for (R, c) in synth.orbit_trajectory(8)[:nframes]]


def _held():
    """the counts, once trackers and contexts that earlier tests dropped without closing are gone (they are closed when collected)"""
    from kintinuous_amd import abi
    gc.collect()
    return abi.live_allocations()


@pytest.fixture(scope="module")
def tiny():
    return _scene(64, 48, 3)


def _config(cam, rgbd_icp=0):
    from kintinuous_amd import abi
    return abi.TrackerConfig(cam.cols, cam.rows, N, cam.fx, cam.fy, cam.cx, cam.cy, 6.0, 14, 2, 0, 0, rgbd_icp, 0, 0, 0)


def test_everything_comes_back(ktlib, tiny):
    """Tracker, slice stage, mesh stage (and its regrow with other bounds), three host frames, finalise, destroy: the counts of buffers, events
    and streams are exactly those from before the tracker -- without -ri (the RGB-D buffers are taken at size zero) and with it."""
    from kintinuous_amd import abi
    cam, frames = tiny

    def life(c, cfg):
        trk = abi.Tracker(c, cfg)
        trk.enable_slice_stage(True, weight_cull=2)
        trk.enable_mesh_stage(True)
        held = abi.live_allocations()
        trk.enable_mesh_stage(True, 10000, 30000)   # other bounds: the four mesh arrays are given back and taken again
        assert abi.live_allocations() == held
        for k, (d, rgb) in enumerate(frames):
            trk.process_frame_host(d, rgb, 33333 * k)
        trk.finalise()
        assert trk.num_poses() == len(frames)
        trk.close()

    base = _held()
    for rgbd_icp in (0, 1):
        c = abi.Ctx(0)
        life(c, _config(cam, rgbd_icp))       # (the context takes its lookup table, its scratch and its track state on first use)
        before = abi.live_allocations()
        assert before[0] > base[0]
        life(c, _config(cam, rgbd_icp))
        assert abi.live_allocations() == before
        c.close()
        assert abi.live_allocations() == base


def test_scratch_regrows_without_losing_anything(ktlib, oracle_mod):
    """kt_integrate_tsdf on one context at 64x48 / N = 32, at 128x96 / N = 64 (both groups of the scratch grow) and at 64x48 / N = 32 again (neither
    shrinks): every result is the oracle's, as tests/test_gpu_volume.py compares them, and the third call takes nothing."""
    from kintinuous_amd import abi
    base = _held()
    c = abi.Ctx(0)
    fresh = abi.live_allocations()
    held = []
    for cols, rows, n in ((64, 48, 32), (128, 96, 64), (64, 48, 32)):
        cam, frames = _scene(cols, rows, 1)
        depth, rgb = frames[0]
        _, _, nmap = _maps(oracle_mod, cam, depth)
        size = 6.0
        (vol, col, scaled, U), (gvol, gcol, gscaled), (dvol, dcol) = _integrate_both(c, oracle_mod, cam, depth, rgb, nmap, n, size, np.eye(3), [3, 3, 3],
                                                                                 max(0.06, 2.1 * size / n), [0, 0, 0], True)
        assert U > 0
        assert np.array_equal(scaled.view(np.uint32), gscaled.view(np.uint32))
        assert np.array_equal(vol, gvol)
        assert np.array_equal(col, gcol)
        held.append(abi.live_allocations())
    assert held[0][0] > fresh[0]
    assert held[1] == held[0] and held[2] == held[1]   # a growth gives back what it replaces; the smaller call takes nothing
    c.close()
    assert abi.live_allocations() == base
    c = abi.Ctx(0)
    assert abi.live_allocations() == fresh
    c.close()
    assert abi.live_allocations() == base


def test_failed_create_leaves_nothing_behind(ktlib, tiny):
    """Every one of the n requests that create + enable_slice_stage + enable_mesh_stage make on a fresh context (the context's lazily taken
    buffers, the scratch, the plans and the two workspaces included) is refused once: exactly one of the three calls returns KT_ERR_NOMEM with a
    file and line, and destroying what exists brings the counts back.
    Every k in 1..n is taken.  The loop's time on the MI355X has NOT been measured yet (the test prints it): should it come to more than about
    five seconds, take every k up to 20 and then every seventh, n included."""
    from kintinuous_amd import abi
    cam, frames = tiny
    cfg = _config(cam)

    def three_calls(c):
        """-> (tracker or None, [status of every call that could be made])"""
        st, trk = [], None
        for call in (lambda: abi.Tracker(c, cfg), lambda: trk.enable_slice_stage(True, weight_cull=2), lambda: trk.enable_mesh_stage(True)):
            try:
                r = call()
                trk = trk or r
                st.append(abi.KT_OK)
            except abi.KtError as e:
                st.append(e.status)
                assert re.search(r"\.(hip|hpp):\d+", str(e)), str(e)
            if trk is None:
                break
        return trk, st

    def pose_of_one_tracked_frame(trk):
        for k, (d, rgb) in enumerate(frames[:2]):   # frame 0 sets the volume up, frame 1 is tracked
            trk.process_frame_host(d, rgb, 33333 * k)
        return np.concatenate([a.ravel() for a in trk.pose()]).view(np.uint32)

    base = _held()
    c = abi.Ctx(0)
    fresh = abi.live_allocations()
    trk, st = three_calls(c)
    assert st == [abi.KT_OK] * 3
    n = sum(abi.live_allocations()) - sum(fresh)
    assert n > 100
    want = pose_of_one_tracked_frame(trk)
    trk.close()
    c.close()
    assert abi.live_allocations() == base

    t0 = time.perf_counter()
    try:
        for k in range(1, n + 1):
            c = abi.Ctx(0)
            abi.fail_allocation(k)
            trk, st = three_calls(c)
            assert st.count(abi.KT_ERR_NOMEM) == 1 and st.count(abi.KT_OK) == len(st) - 1, (k, st)
            if trk is not None:
                trk.close()
            c.close()
            assert abi.live_allocations() == base, k
    finally:
        abi.fail_allocation(-1)
    print(f"failed-create loop: n = {n}, {time.perf_counter() - t0:.2f} s")

    c = abi.Ctx(0)
    trk, st = three_calls(c)
    assert st == [abi.KT_OK] * 3
    assert np.array_equal(pose_of_one_tracked_frame(trk), want)
    trk.close()
    c.close()
    assert abi.live_allocations() == base
