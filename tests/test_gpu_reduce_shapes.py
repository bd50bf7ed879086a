"""GPU parity of the staged reduction (kt_reduce29_publish / kt_reduce29_publish2, csrc/kt_track.hip) at the shapes where the lanes of ONE
workgroup disagree about their number of k-steps, and where an LDS batch ends in half a k-pair.  A virtual thread t of the 8192 takes
the pixels t, t + 8192, ...: nk(t) = ceil((n - t) / 8192) of them.  Phase 2 walks the steps of a batch (40 per batch, staged as 20
k-pairs) over the workgroup's common count and drops the steps past a lane's own count by a select, so the cases are:
  50 x 37    n = 1850:    fewer pixels than virtual threads; 58 workgroups have any, the last one 26 live lanes; nk is 0 or 1 (half a pair alone);
  161 x 119  n = 19159:   nk is 2 or 3; workgroup 86 has lanes with 3 steps next to lanes with 2 (odd and even counts in one wave);
  697 x 479  n = 333863:  nk is 40 or 41; the second batch holds a single step for 7 lanes of workgroup 193 and nothing for the rest;
  704 x 480  n = 337920:  nk is 41 or 42; the second batch is a full pair in some workgroups and half a pair in others.
All sums against the oracle's reference-order float fold, bit for bit."""
import numpy as np
import pytest

from test_gpu_tracker import _cfgs, _run_pair, _volume_close

pytestmark = pytest.mark.gpu

DIST = 0.10
ANG = float(np.sin(np.float32(20.0 * 3.14159265 / 180.0)))
SIZES = [(50, 37), (161, 119), (697, 479), (704, 480)]


def _camera(cols, rows):
    from kintinuous_amd import synth
    s = cols / 640.0
    return synth.Camera(cols, rows, synth.FX * s, synth.FY * s, synth.CX * s, synth.CY * s)


_rendered = {}


def _pair(cols, rows):
    """The first two frames of the 8-frame orbit of the room at cols x rows (rendered once per size)."""
    from kintinuous_amd import synth
    if (cols, rows) not in _rendered:
        cam = _camera(cols, rows)
        traj = synth.orbit_trajectory(8)
        _rendered[(cols, rows)] = (cam, traj, [synth.render(synth.Scene("room"), cam, *traj[i]) for i in (0, 1)])
    return _rendered[(cols, rows)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_sizes_are_the_ragged_ones():
    """The arithmetic behind the table above (no kernel runs): which step counts meet in one workgroup, and what the last batch holds."""
    def nk(n, t):
        return max(0, (n - t + 8191) // 8192)
    n = 50 * 37
    assert [wg for wg in range(256) if nk(n, 32 * wg) > 0][-1] == 57 and sum(nk(n, 32 * 57 + v) for v in range(32)) == 26
    n = 161 * 119
    assert [nk(n, 32 * 86 + v) for v in range(32)].count(3) not in (0, 32) and {nk(n, t) for t in range(8192)} == {2, 3}
    n = 697 * 479
    assert {nk(n, t) for t in range(8192)} == {40, 41} and [nk(n, 32 * 193 + v) for v in range(32)].count(41) == 7
    assert all(nk(n, 32 * wg) == 40 for wg in range(194, 256))
    n = 704 * 480
    assert {nk(n, 32 * wg) for wg in range(256)} == {41, 42}


@pytest.mark.parametrize("cols,rows", SIZES)
def test_icp_step_at_ragged_sizes(ctx, oracle_mod, cols, rows):
    from hip_kernels import HipKernels
    from oracle.oracle import OIntr
    O, H = oracle_mod, HipKernels(ctx)
    cam, traj, ((d0, _), (d1, _)) = _pair(cols, rows)
    intr = OIntr(cam.fx, cam.fy, cam.cx, cam.cy)
    v0 = O.create_vmap(intr, O.bilateral_filter(d0)); n0 = O.create_nmap(v0)
    v1 = O.create_vmap(intr, O.bilateral_filter(d1)); n1 = O.create_nmap(v1)
    R0, t0 = np.asarray(traj[0][0], np.float32), (np.asarray(traj[0][1], np.float32) + 3).astype(np.float32)
    vg, ng = O.transform_maps(v0, n0, R0, t0)
    Ao, bo, ro = O.icp_step(R0, t0, v1, n1, O.mat33_inverse(R0), t0, intr, vg, ng, DIST, ANG, order=0)
    A, b, r = H.icp_step(R0, t0, v1, n1, O.mat33_inverse(R0), t0, intr, vg, ng, DIST, ANG)
    print(f"{cols}x{rows}: inliers {int(ro[1])} of {cols * rows}")
    assert ro[1] > 0.3 * rows * cols
    assert r[1] == ro[1], "inlier count must be exact"
    assert np.array_equal(_bits(A), _bits(Ao)) and np.array_equal(_bits(b), _bits(bo))
    assert np.array_equal(_bits(r), _bits(ro))


def test_icp_step_all_nan_at_161x119(ctx):
    """Every row is dropped in phase 1: the sums are exactly zero and the count 0 (kt_icp_kernel)."""
    from kintinuous_amd.abi import Intr
    cols, rows = 161, 119
    cam = _camera(cols, rows)
    nanmap = ctx.upload(np.full((3 * rows, cols), np.nan, np.float32))
    A, b, r = ctx.icp_step(np.eye(3), [3, 3, 3], nanmap, nanmap, np.eye(3), [3, 3, 3], Intr(cam.fx, cam.fy, cam.cx, cam.cy), nanmap, nanmap,
                           cols, rows, 0.1, 0.34)
    assert not A.any() and not b.any() and not _bits(A).any() and not _bits(b).any() and r[1] == 0 and r[0] == 0


def _rgb_inputs(O, cols, rows):
    cam, _, ((d0, rgb0), (d1, rgb1)) = _pair(cols, rows)
    dm0, dm1 = O.depth_to_metres(d0, 6000), O.depth_to_metres(d1, 6000)
    i0, i1 = O.bgr_to_intensity(rgb0), O.bgr_to_intensity(rgb1)
    dx, dy = O.derivative_images(i1)
    K = np.array([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]])
    krk = (K @ O.rodrigues(np.array([0.002, -0.003, 0.001])) @ np.linalg.inv(K)).astype(np.float32)
    kt = (K @ np.array([0.004, -0.002, 0.003])).astype(np.float32)
    return cam, dm0, dm1, i0, i1, dx, dy, krk, kt


def test_rgb_residual_and_step_at_161x119(ctx, oracle_mod):
    """kt_rgb_residual and kt_rgb_kernel (the same staged reduction behind another row functor) on a ragged workgroup."""
    from hip_kernels import HipKernels
    O, H = oracle_mod, HipKernels(ctx)
    cols, rows = 161, 119
    cam, dm0, dm1, i0, i1, dx, dy, krk, kt = _rgb_inputs(O, cols, rows)
    ms = float(np.float32(12.0 ** 2 / 0.125 ** 2))
    co, so, no = O.rgb_residual(ms, dx, dy, dm0, dm1, i0, i1, np.float32(0.07), kt, krk)
    ch, sh, nh = H.rgb_residual(ms, dx, dy, dm0, dm1, i0, i1, np.float32(0.07), kt, krk)
    print(f"rgb correspondences {no} of {cols * rows}")
    assert no > 50 and (sh, nh) == (so, no)
    m = co["valid"] != 0
    assert np.array_equal(ch["valid"] != 0, m)
    for f in ("zero", "one"):
        assert np.array_equal(ch[f][m], co[f][m])
    assert np.array_equal(ch["diff"][m].view(np.uint32), co["diff"][m].view(np.uint32))
    cloud = O.project_to_cloud(dm0, cam.fx, cam.fy, cam.cx, cam.cy, 0)
    sig = float(np.sqrt(np.float32(no)))
    Ao, bo = O.rgb_step(co, sig, cloud, np.float32(cam.fx), np.float32(cam.fy), dx, dy, 0.125, order=0)
    A, b = H.rgb_step(co, sig, cloud, np.float32(cam.fx), np.float32(cam.fy), dx, dy, 0.125)
    assert np.array_equal(_bits(A), _bits(Ao)) and np.array_equal(_bits(b), _bits(bo))
    # ... and with no correspondence at all and a NaN cloud: exactly zero (kt_rgb_kernel)
    none = np.zeros_like(co)
    A, b = H.rgb_step(none, 1.0, np.full_like(cloud, np.nan), np.float32(cam.fx), np.float32(cam.fy), dx, dy, 0.125)
    assert not _bits(A).any() and not _bits(b).any()


def _frames_168x120():
    from kintinuous_amd import synth
    cam = synth.Camera.small(168, 120)
    traj = synth.orbit_trajectory(8)
    scene = synth.Scene("room")
    return cam, [synth.render(scene, cam, R, c) for (R, c) in traj]


def test_joint_kernel_on_ragged_workgroups(ctx, oracle_mod):
    """kt_joint_kernel is reached through the tracker only (RGB-D + ICP mode): 168 x 120 = 20160 pixels are 2 or 3 steps per virtual thread,
    levels 1 and 2 leave workgroups half filled or empty -- kt_reduce29_publish2 with lanes past their last step, against the oracle tracker."""
    cam, frames = _frames_168x120()
    trk, otr, max_t, max_r = _run_pair(ctx, cam, frames[:5], 64, use_rgbd_icp=1)
    print(f"joint tracker: max_t {max_t:.3e} max_r {max_r:.3e}")
    assert max_t < 1e-6 and max_r < 1e-6, (max_t, max_r)   # (the one piece that is not bit-exact is the device's double sin / cos in Rodrigues)
    _volume_close(trk, otr)
    trk.close(); otr.close()


def test_tracker_168x120_per_level_equals_per_iteration(ctx):
    """Eight frames at 168 x 120 into a 96^3 volume: levels 1 and 2 have 5040 and 1260 pixels -- half-filled workgroups inside the resident
    kt_icp_level_kernel.  One launch for all levels and one launch per iteration: every pose and both volumes bit-equal."""
    from kintinuous_amd import abi
    cam, frames = _frames_168x120()
    g, _ = _cfgs(cam, 96)
    out = []
    for levels in (0, 1):
        abi._chk(abi.lib().kt_debug_icp_levels(levels))
        try:
            trk = abi.Tracker(ctx, g)
        finally:
            abi._chk(abi.lib().kt_debug_icp_levels(-1))
        poses = []
        for k, (d, rgb) in enumerate(frames):
            trk.process_frame_host(d, rgb, 33333 * k)
            poses.append(np.concatenate([x.ravel() for x in trk.pose()]))
        out.append((np.array(poses), trk.volume().copy(), trk.color_volume().copy()))
        trk.close()
    assert np.isfinite(out[0][0]).all() and np.abs(out[0][0][-1] - out[0][0][0]).max() > 1e-4, "the camera must have moved"
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert (out[0][2][..., 3] != 0).any()
