"""GPU.  The loop-closure registration stage (csrc/kt_loop.hip: kt_depth_to_cloud_grid, kt_cloud_nearest, kt_loop_icp_depth_frames;
DESIGN.md 4.6) against its numpy restatement (kintinuous_amd/loop_icp_ref.py), which tests/test_loop_icp_ref.py ties to the pinned oracle
and to an independent float64 implementation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loop_icp_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _intr(cam):
    from kintinuous_amd import abi
    return abi.Intr(cam.fx, cam.fy, cam.cx, cam.cy)


def _ref_grid(depth, intr, leaf, max_dist):
    from kintinuous_amd import loop_icp_ref as ref
    return ref.depth_to_cloud_grid(depth, intr.fx, intr.fy, intr.cx, intr.cy, leaf, max_dist)


def _grid_frames():
    rng = np.random.default_rng(11)
    out = {}
    for cols, rows in ((160, 120), (640, 480)):
        cam, d = lc.render(cols, rows, "B")
        out[f"{cols}x{rows}"] = (cam, d, 4.0)
    cam, d = lc.render(160, 120, "A")
    holes = d.copy()
    holes[rng.random(d.shape) < 0.3] = 0
    holes[40:60, 50:90] = 0
    out["holes"] = (cam, holes, 4.0)
    far = d.copy()                                            # max_dist = 2.5: pixels at 2499 (kept), 2500 and beyond (dropped)
    far[0:30, :] = 2499
    far[30:60, :] = 2500
    far[60:70, :] = 2501
    far[70:80, :] = 65535
    out["at_and_beyond_max_dist"] = (cam, far, 2.5)
    from kintinuous_amd import synth
    rc = synth.Camera(173, 97, 140.0, 141.0, 85.5, 50.25)
    out["ragged_173x97"] = (rc, synth.render(synth.Scene("room"), rc, lc.POSE_B[:3, :3], lc.POSE_B[:3, 3])[0], 4.0)
    out["one_pixel"] = (cam, np.where(np.arange(d.size).reshape(d.shape) == 7777, d, 0).astype(np.uint16), 4.0)
    rng = np.random.default_rng(5)                            # the column scan's edges: 1, 2 and 3 columns per thread of its 256
    for cols in (1, 255, 256, 257, 513):
        noise = rng.integers(500, 3900, (5, cols)).astype(np.uint16)
        noise[rng.random(noise.shape) < 0.3] = 0
        out[f"scan_{cols}x5"] = (synth.Camera(cols, 5, 140.0, 141.0, cols / 2 - 0.5, 2.25), noise, 4.0)
    return out


@pytest.mark.parametrize("case", ["160x120", "640x480", "holes", "at_and_beyond_max_dist", "ragged_173x97", "one_pixel",
                                  "scan_1x5", "scan_255x5", "scan_256x5", "scan_257x5", "scan_513x5"])
def test_depth_to_cloud_grid(ctx, case):
    """Point count and every float bit-equal to the restatement."""
    from kintinuous_amd import abi
    cam, depth, max_dist = _grid_frames()[case]
    intr = _intr(cam)
    want = _ref_grid(depth, intr, lc.LEAF, max_dist)
    s, got, n = ctx.depth_to_cloud_grid(depth, intr, lc.LEAF, max_dist)
    assert s == abi.KT_OK and n == len(want) and n > 0
    assert got.tobytes() == want.tobytes()
    # exact capacity fits; one short: KT_ERR_CAPACITY, the true size, an untouched buffer
    buf = np.full((n, 3), 7.0, np.float32)
    s, got, n2 = ctx.depth_to_cloud_grid(depth, intr, lc.LEAF, max_dist, capacity=n, out=buf)
    assert s == abi.KT_OK and n2 == n and buf.tobytes() == want.tobytes()
    if n > 1:
        buf = np.full((n, 3), 7.0, np.float32)
        s, got, n2 = ctx.depth_to_cloud_grid(depth, intr, lc.LEAF, max_dist, capacity=n - 1, out=buf)
        assert s == abi.KT_ERR_CAPACITY and got is None and n2 == n and (buf == 7.0).all()


def test_depth_to_cloud_grid_empty_frame(ctx):
    from kintinuous_amd import abi
    cam, depth = lc.render(160, 120, "A")
    s, got, n = ctx.depth_to_cloud_grid(np.zeros_like(depth), _intr(cam), lc.LEAF, 4.0)
    assert s == abi.KT_OK and n == 0 and len(got) == 0
    s, got, n = ctx.depth_to_cloud_grid(np.zeros_like(depth), _intr(cam), lc.LEAF, 4.0, capacity=0, out=np.zeros((1, 3), np.float32))
    assert s == abi.KT_OK and n == 0
    s, got, n = ctx.depth_to_cloud_grid(np.full_like(depth, 4000), _intr(cam), lc.LEAF, 4.0)      # every pixel AT max_dist: none kept
    assert s == abi.KT_OK and n == 0


def _nearest_cases():
    rng = np.random.default_rng(5)
    out = {}
    dst = rng.uniform(-2, 2, (3001, 3)).astype(np.float32)          # not a multiple of the 1024-point tile
    dst[100] = dst[2900]                                            # duplicates: the lower index wins
    dst[1500] = dst[1024] = dst[1023]                               # ... across a tile boundary
    src = rng.uniform(-2, 2, (777, 3)).astype(np.float32)
    src[0], src[1] = dst[2900], dst[1500]
    out["ties_and_ragged_tile"] = (src, dst)
    g = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0), np.arange(9.0), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    mid = (g[:200] + np.float32(0.5)).astype(np.float32)            # centres of lattice cells: eight targets at the same distance
    out["midway_lattice"] = (np.concatenate([mid, (g[:50] + np.array([0.5, 0, 0], np.float32))]), g)
    out["n_src_1"] = (src[5:6], dst)
    out["n_dst_1"] = (src, dst[17:18])
    out["exact_tile"] = (src[:64], dst[:2048])
    cam, d = lc.render(160, 120, "A")
    S = _ref_grid(d, _intr(cam), lc.LEAF, 4.0)
    T = _ref_grid(lc.render(160, 120, "B")[1], _intr(cam), lc.LEAF, 4.0)
    out["frame_clouds"] = (S, T)
    return out


@pytest.mark.parametrize("case", ["ties_and_ragged_tile", "midway_lattice", "n_src_1", "n_dst_1", "exact_tile", "frame_clouds"])
def test_cloud_nearest(ctx, case):
    """Indices and d2 bit-equal to the restatement (argmin's lowest-index rule)."""
    from kintinuous_amd import loop_icp_ref as ref
    src, dst = _nearest_cases()[case]
    want_i, want_d = ref.nearest(src, dst)
    got_i, got_d = ctx.cloud_nearest(src, dst)
    if case == "midway_lattice":
        d = ((src[:, None, :] - dst[None]) ** 2).sum(-1)
        assert ((d == d.min(axis=1, keepdims=True)).sum(axis=1) >= 2).all()          # the ties are real
    assert np.array_equal(got_i, want_i)
    assert got_d.tobytes() == want_d.tobytes()


def _bound_from_float64(M, cols, rows):
    """the ground-truth assertion of tests/test_loop_icp_ref.py: 1.5 x the float64 run's own error on the pair"""
    e64, e = lc.pose_error(lc.run64(cols, rows)[0], lc.truth()), lc.pose_error(M, lc.truth())
    assert e[0] <= 1.5 * e64[0] and e[1] <= 1.5 * e64[1], (e, e64)
    return e, e64


@pytest.mark.parametrize("cols,rows", [(160, 120), (640, 480)])
def test_loop_icp_against_restatement(ctx, cols, rows):
    """Iteration count and `converged` equal; every entry of the transform within 1e-5 (the only permitted difference is the order of the
    double sums, ~1e-13, which can flip an isolated float32 rounding of a transformed point); score within 1e-5 relative; the distance to the
    ground truth within 1.5 x the float64 run's own."""
    from kintinuous_amd import loop_icp_ref as ref
    cam, d1 = lc.render(cols, rows, "A")
    _, d2 = lc.render(cols, rows, "B")
    want_M, want_score, want_info = ref.icp_depth_frames(d1, d2, cam.fx, cam.fy, cam.cx, cam.cy, lc.bootstrap(), lc.LEAF, 4.0, 10)
    M, score, info = ctx.loop_icp_depth_frames(d1, d2, _intr(cam), lc.bootstrap(), lc.LEAF, 4.0, 10)
    print(f"{cols}x{rows}: max |dM| {np.abs(M.astype(np.float64) - want_M).max():.3e}, score {score!r} vs {want_score!r}, info {info}")
    assert info == want_info
    assert np.abs(M.astype(np.float64) - want_M.astype(np.float64)).max() <= 1e-5
    assert abs(score - want_score) <= 1e-5 * want_score
    print("  to the truth (rad, m):", _bound_from_float64(M, cols, rows))


def test_loop_icp_score_separates_pairs(ctx):
    cam, d1 = lc.render(160, 120, "A")
    for to, below in (("B", True), ("C", False)):
        _, score, _ = ctx.loop_icp_depth_frames(d1, lc.render(160, 120, to)[1], _intr(cam), lc.bootstrap(), lc.LEAF)
        assert (score < 0.01) == below, (to, score)


def test_loop_icp_fixed_point_and_iteration_cap(ctx):
    """A pair that reaches its fixed point before the cap (a frame against itself, bootstrap = a small shift) and runs cut short by
    max_iterations, 0 included: equal to the restatement's."""
    from kintinuous_amd import loop_icp_ref as ref
    cam, d1 = lc.render(160, 120, "A")
    boot = np.eye(4, dtype=np.float32)
    boot[0, 3] = 0.004
    for frames, b, cap in (((d1, d1), boot, 30), ((d1, lc.render(160, 120, "B")[1]), lc.bootstrap(), 3), ((d1, d1), boot, 0)):
        want_M, want_score, want_info = ref.icp_depth_frames(*frames, cam.fx, cam.fy, cam.cx, cam.cy, b, lc.LEAF, 4.0, cap)
        M, score, info = ctx.loop_icp_depth_frames(*frames, _intr(cam), b, lc.LEAF, 4.0, cap)
        assert info == want_info, (info, want_info)
        assert np.abs(M.astype(np.float64) - want_M).max() <= 1e-5 and abs(score - want_score) <= 1e-5 * want_score
    assert ref.icp_depth_frames(d1, d1, cam.fx, cam.fy, cam.cx, cam.cy, boot, lc.LEAF, 4.0, 30)[2]["converged"]


def test_determinism(ctx):
    """The same call twice, and once more after an unrelated call on the context: bit-identical output."""
    from kintinuous_amd import abi
    cam, d1 = lc.render(160, 120, "A")
    _, d2 = lc.render(160, 120, "B")
    run = lambda: ctx.loop_icp_depth_frames(d1, d2, _intr(cam), lc.bootstrap(), lc.LEAF)
    a = run()
    b = run()
    pts = np.zeros(5000, abi.POINT_DTYPE)
    pts["xyz"] = np.random.default_rng(1).uniform(-1, 1, (5000, 3))
    pts["bgra"] = 200
    assert len(abi.slice_process(ctx, pts, 8, 0.05)) > 0          # the slice stage shares the context's grid workspace
    ctx.cloud_nearest(pts["xyz"][:10], pts["xyz"])
    c = run()
    for other in (b, c):
        assert other[0].tobytes() == a[0].tobytes() and np.float32(other[1]).tobytes() == np.float32(a[1]).tobytes() and other[2] == a[2]


def test_workspace_growth():
    """A context's workspace regrows under the calls it meets -- points first, then pixels and columns, a larger frame, a smaller one
    again, the first call once more -- and no call sees a stale or undersized buffer: every result equals the same call's on a fresh
    context, bit for bit.  (Capacities are not observable from here: a capacity that shrank would regrow and still pass.)"""
    from kintinuous_amd import abi
    rng = np.random.default_rng(17)
    src, dst = rng.uniform(-2, 2, (5000, 3)).astype(np.float32), rng.uniform(-2, 2, (5000, 3)).astype(np.float32)
    small_cam, small = lc.render(32, 24, "A")
    ragged_cam, ragged, _ = _grid_frames()["ragged_173x97"]
    nearest = lambda c: ctx_bytes(c.cloud_nearest(src, dst))
    grid = lambda cam, d: lambda c: ctx_bytes(c.depth_to_cloud_grid(d, _intr(cam), lc.LEAF, 4.0)[1:])
    ctx_bytes = lambda parts: [np.asarray(p).tobytes() for p in parts]
    grown = abi.Ctx(0)
    try:
        for k, call in enumerate((nearest, grid(small_cam, small), grid(ragged_cam, ragged), grid(small_cam, small), nearest)):
            fresh = abi.Ctx(0)
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert len(want[0]) > 0 and call(grown) == want, k
    finally:
        grown.close()


def test_degenerate_and_error_paths(ctx, ktlib):
    from kintinuous_amd import abi
    cam, d1 = lc.render(160, 120, "A")
    intr, zero, boot = _intr(cam), np.zeros_like(d1), lc.bootstrap()
    for a, b, ns_zero in ((zero, d1, True), (d1, zero, False), (zero, zero, True)):
        M, score, info = ctx.loop_icp_depth_frames(a, b, intr, boot, lc.LEAF)
        assert M.tobytes() == boot.tobytes() and score == float("inf") and info["iterations"] == 0 and not info["converged"]
        assert (info["n_source"] == 0) == ns_zero
    # argument errors: KT_ERR_ARG (2), nothing written
    M, score, inf = (C.c_float * 16)(*([5.0] * 16)), C.c_float(5.0), abi.LoopIcpInfo()
    call = lambda **kw: ktlib.kt_loop_icp_depth_frames(*[kw.get(k, v) for k, v in (
        ("ctx", ctx.h), ("f1", d1.ctypes.data), ("f2", d1.ctypes.data), ("cols", 160), ("rows", 120), ("intr", C.byref(intr)), ("boot", abi._fp(boot)),
        ("leaf", lc.LEAF), ("max_dist", 4.0), ("its", 10), ("M", M), ("score", C.byref(score)), ("info", C.byref(inf)))])
    for bad in (dict(f1=None), dict(f2=None), dict(cols=0), dict(rows=-1), dict(intr=None), dict(boot=None), dict(leaf=0.0), dict(leaf=-1.0), dict(max_dist=0.0),
                dict(its=-1), dict(M=None), dict(score=None), dict(info=None), dict(ctx=None)):
        assert call(**bad) == 2, bad
    assert list(M) == [5.0] * 16 and score.value == 5.0
    assert call() == abi.KT_OK
    n = C.c_size_t(99)
    buf = np.zeros((4, 3), np.float32)
    assert ktlib.kt_depth_to_cloud_grid(ctx.h, d1.ctypes.data, 160, 120, C.byref(intr), lc.LEAF, 4.0, None, 4, C.byref(n)) == 2
    assert ktlib.kt_depth_to_cloud_grid(ctx.h, d1.ctypes.data, 160, 120, C.byref(intr), lc.LEAF, 4.0, buf.ctypes.data, 4, None) == 2
    assert ktlib.kt_depth_to_cloud_grid(ctx.h, d1.ctypes.data, 160, 120, C.byref(intr), lc.LEAF, 4.0, None, 0, C.byref(n)) == abi.KT_ERR_CAPACITY and n.value > 4
    idx, d2 = np.zeros(4, np.uint32), np.zeros(4, np.float32)
    assert ktlib.kt_cloud_nearest(ctx.h, buf.ctypes.data, 0, buf.ctypes.data, 4, idx.ctypes.data, d2.ctypes.data) == 2
    assert ktlib.kt_cloud_nearest(ctx.h, buf.ctypes.data, 4, buf.ctypes.data, 0, idx.ctypes.data, d2.ctypes.data) == 2
    assert ktlib.kt_cloud_nearest(ctx.h, buf.ctypes.data, 4, buf.ctypes.data, 4, None, d2.ctypes.data) == 2


def test_shell(ctx, tmp_path):
    """host/LoopConstraintICP.h (the reference's icpDepthFrames signature over Eigen::Matrix4f) compiled against the Eigen stand-ins and
    run on a pair written to a file: transform and score equal to the C-ABI call's, bit for bit."""
    from kintinuous_amd import build
    cam, d1 = lc.render(160, 120, "A")
    _, d2 = lc.render(160, 120, "B")
    voxel = np.float32(6.0 / 512)
    intr = _intr(cam)
    path = tmp_path / "pair.bin"
    with open(path, "wb") as f:
        f.write(np.array([160, 120], np.int32).tobytes())
        f.write(np.array([intr.fx, intr.fy, intr.cx, intr.cy, voxel], np.float32).tobytes())
        f.write(lc.bootstrap().tobytes())
        f.write(d1.tobytes())
        f.write(d2.tobytes())
    exe = str(tmp_path / "loop_icp_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "kintinuous_amd", "host"),
                        "-I", ROOT, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "stubs", "loop_icp_check.cpp"), "-o", exe,
                        "-L", os.path.dirname(build.OUT), "-lkt_hip", "-lz", "-Wl,-rpath," + os.path.dirname(build.OUT), "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines())
    got_M = np.array([float.fromhex(v) for v in lines["transform"].split()], np.float32).reshape(4, 4)
    got_score = np.float32(float.fromhex(lines["score"]))
    M, score, info = ctx.loop_icp_depth_frames(d1, d2, intr, lc.bootstrap(), float(np.float32(2.5) * voxel))
    assert got_M.tobytes() == M.tobytes() and got_score.tobytes() == np.float32(score).tobytes()
    assert [int(v) for v in lines["info"].split()] == [info["n_source"], info["n_target"], info["iterations"], int(info["converged"])]
