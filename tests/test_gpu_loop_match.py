"""GPU.  The loop-closure bootstrap stage (csrc/kt_match.hip: kt_frame_keypoints, kt_descriptor_match, kt_loop_match_frames; DESIGN.md
4.8) against its numpy restatement (kintinuous_amd/loop_match_ref.py), which tests/test_loop_match_ref.py ties to an independent
implementation and to the reference's gates.  Integer results are compared for equality; the pose passes through kt_host_rigid_fit
(an SVD in the restatement) and is held to test_gpu_loop_icp.py's 1e-5 per entry."""
import os
import subprocess

import numpy as np
import pytest

import loop_icp_cases as lc
import loop_match_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _intr(cam):
    from kintinuous_amd import abi
    return abi.Intr(cam.fx, cam.fy, cam.cx, cam.cy)


def _ref_params(p):
    from kintinuous_amd import loop_match_ref as ref
    return ref.Params(**{k: getattr(p, k) for k in ref.Params.__dataclass_fields__})


def _keypoint_frames():
    """name -> (rgb, depth, overrides of the default parameters)"""
    from kintinuous_amd import loop_match_ref as ref
    rng = np.random.default_rng(3)
    out = {}
    for cols, rows in ((160, 120), (640, 480), (173, 97)):
        _, d, rgb = mc.frame(cols, rows, "B")
        out[f"{cols}x{rows}" if cols != 173 else "ragged_173x97"] = (rgb, d, {})
    _, d, rgb = mc.frame(160, 120, "A")
    holes = d.copy()
    holes[rng.random(d.shape) < 0.3] = 0
    out["holes"] = (rgb, holes, {})
    # more corners than max_keypoints, with equal scores on both sides of the cut: identical bright squares on a flat background (the
    # crossings of a checkerboard are saddle points, which FAST-9 does not fire on; the corners of separate squares all score the same)
    grid = [(u, v) for v in range(20, 100, 12) for u in range(20, 140, 12)]
    out["equal_scores_over_cap"] = (mc.blob_frame(160, 120, grid), np.full((120, 160), 1500, np.uint16), dict(max_keypoints=100))
    out["cap_at_a_run_boundary"] = (mc.blob_frame(160, 120, grid), np.full((120, 160), 1500, np.uint16), dict(max_keypoints=1))
    out["no_corner"] = (np.full((120, 160, 3), 90, np.uint8), np.full((120, 160), 1500, np.uint16), {})
    M = ref.MARGIN
    squares = [(M, 50), (M - 1, 80), (160 - 1 - M - 5, 50), (160 - M - 5, 80), (50, M), (80, M - 1), (50, 120 - 1 - M - 5), (80, 120 - M - 5)]
    out["at_the_margin"] = (mc.blob_frame(160, 120, squares), np.full((120, 160), 1500, np.uint16), {})
    for rows in (255, 256, 257, 513):                         # the row scan's edges: 1, 2 and 3 rows per thread of its 256
        out[f"scan_48x{rows}"] = (mc.blob_frame(48, rows, [(20, v) for v in range(M + 2, rows - M - 8, 29)]), np.full((rows, 48), 1500, np.uint16), {})
    return out


@pytest.mark.parametrize("case", ["160x120", "640x480", "ragged_173x97", "holes", "equal_scores_over_cap", "cap_at_a_run_boundary", "no_corner", "at_the_margin",
                                  "scan_48x255", "scan_48x256", "scan_48x257", "scan_48x513"])
def test_frame_keypoints(ctx, case):
    """Count, coordinates, scores and descriptor words equal to the restatement's; capacity exact and one short."""
    from kintinuous_amd import abi, loop_match_ref as ref
    rgb, depth, over = _keypoint_frames()[case]
    p = abi.loop_match_params(**over)
    uv, score, desc = ref.frame_keypoints(rgb, depth, _ref_params(p))
    s, got, n = ctx.frame_keypoints(rgb, depth, p)
    assert s == abi.KT_OK and n == len(uv), (n, len(uv))
    assert np.array_equal(got[0], uv) and np.array_equal(got[1], score) and np.array_equal(got[2], desc)
    if case == "no_corner":
        assert n == 0
        return
    assert n > 0
    if case in ("equal_scores_over_cap", "cap_at_a_run_boundary"):       # the tie rule decides: corners of the cut's score were left out
        every = ref.frame_keypoints(rgb, depth, _ref_params(abi.loop_match_params(max_keypoints=4096)))[1]
        assert n == p.max_keypoints and (every == score[-1]).sum() > (score == score[-1]).sum()
    if case == "at_the_margin":
        M, kept = ref.MARGIN, {(int(u), int(v)) for u, v in uv}
        corners = ref.nms(ref.fast_scores(ref.intensity(rgb), p.fast_threshold))
        for at, off in (((M, 50), (M - 1, 80)), ((159 - M, 50), (160 - M, 80)), ((50, M), (80, M - 1)), ((50, 119 - M), (80, 120 - M))):
            assert at in kept and off not in kept and corners[off[1], off[0]], (at, off)
    s, got, n2 = ctx.frame_keypoints(rgb, depth, p, capacity=n)
    assert s == abi.KT_OK and n2 == n and np.array_equal(got[2], desc)
    s, got, n2 = ctx.frame_keypoints(rgb, depth, p, capacity=n - 1)                     # (the binding asserts the buffers stayed untouched)
    assert s == abi.KT_ERR_CAPACITY and got is None and n2 == n


def _match_cases():
    rng = np.random.default_rng(9)
    out = {}
    old = rng.integers(0, 2 ** 32, (3001, 8), dtype=np.uint64).astype(np.uint32)        # not a multiple of the 512-descriptor tile
    new = rng.integers(0, 2 ** 32, (777, 8), dtype=np.uint64).astype(np.uint32)
    flip = lambda d, bits: d ^ np.bitwise_or.reduce([np.eye(8, dtype=np.uint32)[b // 32] << np.uint32(b % 32) for b in bits])
    old[100] = old[300] = flip(new[0], [3])                   # duplicates inside a tile: the lower index wins, d2 = d1
    old[511] = old[512] = old[2000] = flip(new[1], [7, 200])  # ... across a tile boundary
    for i in range(2, 40):                                    # near copies: accepted matches among the random rest
        old[600 + 37 * i] = flip(new[i], list(range(i)))
    out["ties_and_ragged_tile"] = (new, old, dict(ratio_num=2, ratio_den=1))      # (a ratio below 1 refuses every tie of d1 and d2)
    out["n_old_1"] = (new, old[600 + 37 * 5:600 + 37 * 5 + 1], {})
    out["n_new_1"] = (new[3:4], old, {})
    out["exact_tile"] = (new[:64], old[:1024], {})
    # ratio 4 / 5: (d1, d2) = (40, 50) lands on equality and is refused, (39, 50) passes; (64, 250) is at max_hamming, (65, 250) beyond
    zero = np.zeros(8, np.uint32)
    q = np.stack([zero, zero, zero, zero])
    sets = [([40, 50], q[:1]), ([39, 50], q[:1]), ([64, 250], q[:1]), ([65, 250], q[:1])]
    for k, (counts, qq) in enumerate(sets):
        out[f"ratio_{counts[0]}_{counts[1]}"] = (qq, np.stack([flip(zero, list(range(c))) for c in counts] + [flip(zero, list(range(255)))]), {})
    return out


@pytest.mark.parametrize("case", ["ties_and_ragged_tile", "n_old_1", "n_new_1", "exact_tile", "ratio_40_50", "ratio_39_50", "ratio_64_250", "ratio_65_250"])
def test_descriptor_match(ctx, case):
    """Indices, d1 and d2 equal to the restatement's."""
    from kintinuous_amd import abi, loop_match_ref as ref
    new, old, over = _match_cases()[case]
    p = abi.loop_match_params(**over)
    want = ref.descriptor_match(new, old, _ref_params(p))
    got = ctx.descriptor_match(new, old, p)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    if case == "ties_and_ragged_tile":
        assert want[0][0] == 100 and want[1][0] == want[2][0] == 1 and want[0][1] == 511 and (want[0][2:40] >= 0).sum() > 20
    if case == "n_old_1":
        assert (want[2] == ref.NO_SECOND).all() and want[0][5] == 0
    if case.startswith("ratio_"):
        assert (want[0][0] >= 0) == (case in ("ratio_39_50", "ratio_64_250")) and [want[1][0], want[2][0]] == [int(v) for v in case.split("_")[1:]]


def test_workspace_growth():
    """A context's workspace regrows under the calls it meets -- descriptors first, then pixels and rows, a frame of fewer rows and
    more pixels per row, the first call once more -- and no call sees a stale or undersized buffer: every result equals the same
    call's on a fresh context.  (Capacities are not observable from here: a capacity that shrank would regrow and still pass.)"""
    from kintinuous_amd import abi
    new, old, _ = _match_cases()["ties_and_ragged_tile"]
    frames = _keypoint_frames()
    match = lambda c: list(c.descriptor_match(new, old))
    keypoints = lambda name: lambda c: list(c.frame_keypoints(*frames[name][:2])[1])
    grown = abi.Ctx(0)
    try:
        for k, call in enumerate((match, keypoints("160x120"), keypoints("ragged_173x97"), match)):
            fresh = abi.Ctx(0)
            try:
                want = call(fresh)
            finally:
                fresh.close()
            got = call(grown)
            assert len(want[0]) > 0 and all(np.array_equal(g, w) for g, w in zip(got, want)), k
    finally:
        grown.close()


def _check_pair(got, want):
    assert got["info"] == want["info"], (got["info"], want["info"])
    assert np.array_equal(got["matches"], want["matches"]) and np.array_equal(got["inlier"], want["inlier"])
    dp = np.abs(got["pose"].astype(np.float64) - want["pose"]).max()
    db = np.abs(got["bootstrap"].astype(np.float64) - want["bootstrap"]).max()
    assert dp <= 1e-5 and db <= 1e-5, (dp, db)
    return dp, db


@pytest.mark.parametrize("cols,rows", [(160, 120), (640, 480)])
def test_loop_match_against_restatement(ctx, cols, rows):
    """(A, B): the keypoints of both frames, the match list, the winning hypothesis and the inlier flags equal; pose and bootstrap within
    1e-5 per entry; a second call bit-identical; the bootstrap chained into the registration stage scores below the reference's 0.01."""
    want = mc.restated(cols, rows)
    cam, d_old, rgb_old = mc.frame(cols, rows, "A")
    _, d_new, rgb_new = mc.frame(cols, rows, "B")
    for rgb, d, kp in ((rgb_old, d_old, want["keypoints_old"]), (rgb_new, d_new, want["keypoints_new"])):
        s, got_kp, n = ctx.frame_keypoints(rgb, d)
        assert s == 0 and all(np.array_equal(g, w) for g, w in zip(got_kp, kp))
    got = ctx.loop_match_frames(rgb_old, d_old, rgb_new, d_new, _intr(cam))
    print(f"{cols}x{rows}: {got['info']}, max |d pose| / |d bootstrap| {_check_pair(got, want)}")
    assert got["info"]["n_matches"] >= 40 and got["info"]["n_inliers"] > 0.35 * got["info"]["n_matches"]
    again = ctx.loop_match_frames(rgb_old, d_old, rgb_new, d_new, _intr(cam))
    assert all(again[k].tobytes() == got[k].tobytes() for k in ("pose", "bootstrap", "matches", "inlier")) and again["info"] == got["info"]
    M, score, info = ctx.loop_icp_depth_frames(d_old, d_new, _intr(cam), got["bootstrap"], lc.LEAF)
    print(f"  chained registration: score {score:.3e} after {info['iterations']} iterations; bootstrap to the truth {lc.pose_error(got['bootstrap'], lc.truth())}")
    assert score < 0.01


def test_loop_match_rejects_another_wall(ctx):
    """(A, C): a gate of the caller's rejects it, exactly as the restatement's result does."""
    want = mc.restated(160, 120, "A", "C")
    cam, d_old, rgb_old = mc.frame(160, 120, "A")
    _, d_new, rgb_new = mc.frame(160, 120, "C")
    got = ctx.loop_match_frames(rgb_old, d_old, rgb_new, d_new, _intr(cam))
    _check_pair(got, want)
    assert got["info"]["n_matches"] < 40 or got["info"]["n_inliers"] <= 0.35 * got["info"]["n_matches"]


def test_loop_match_too_few_matches(ctx):
    """One frame without depth (no keypoint survives), in either place, and a single hypothesis budget of zero: identity, no inliers."""
    from kintinuous_amd import abi
    cam, d, rgb = mc.frame(160, 120, "A")
    zero = np.zeros_like(d)
    for a, b, p in ((zero, d, None), (d, zero, None), (zero, zero, None), (d, d, abi.loop_match_params(n_hypotheses=0))):
        got = ctx.loop_match_frames(rgb, a, rgb, b, _intr(cam), p)
        assert np.array_equal(got["pose"], np.eye(4, dtype=np.float32)) and np.array_equal(got["bootstrap"], np.eye(4, dtype=np.float32))
        assert got["info"]["n_inliers"] == 0 and got["info"]["best_hypothesis"] == -1 and not got["inlier"].any()
        assert (got["info"]["n_matches"] == 0) == (p is None)
        assert (got["info"]["n_kp_old"] == 0) == (a is zero) and (got["info"]["n_kp_new"] == 0) == (b is zero)


def collinear_pair():
    """Bright squares in one line over a flat wall, the new image shifted by 4 pixels: the keypoints lie on two image rows at one depth,
    so a triple drawn from one row is collinear in 3D -- exactly, y and z being equal -- and its hypothesis degenerate.  A faint blocky
    background (below the FAST threshold) tells the descriptors apart."""
    rng = np.random.default_rng(21)
    bg = np.repeat(np.repeat(rng.integers(30, 46, (30, 40)), 4, axis=0), 4, axis=1).astype(np.uint8)
    old = np.repeat(bg[..., None], 3, axis=2)
    for k, u in enumerate(range(22, 132, 9)):
        old[40:46, u:u + 6] = 215 + (k % 3) * 10
    depth = np.full((120, 160), 2000, np.uint16)
    return old, depth, np.roll(old, 4, axis=1), depth


def test_loop_match_degenerate_hypotheses(ctx):
    """Seed 27 opens with two degenerate hypotheses and about a fifth of the 500 are: the winner is the restatement's.  Then a pair whose
    matches all lie on one row (the depth below it removed): every hypothesis is degenerate, the result the identity."""
    from kintinuous_amd import abi, loop_match_ref as ref
    rgb_old, d_old, rgb_new, d_new = collinear_pair()
    cam = mc.frame(160, 120, "A")[0]
    p = abi.loop_match_params(seed=27)
    want = ref.loop_match_frames(rgb_old, d_old, rgb_new, d_new, cam.fx, cam.fy, cam.cx, cam.cy, _ref_params(p))
    m = want["match_index"]
    Pn = ref.points3d(want["keypoints_new"][0][m[:, 0]], d_new, cam.fx, cam.fy, cam.cx, cam.cy)
    Po = ref.points3d(want["keypoints_old"][0][m[:, 1]], d_old, cam.fx, cam.fy, cam.cx, cam.cy)
    deg = ref.fit_triples(Pn, Po, ref.draw_triples(27, 500, len(m)))[2]
    print(f"{len(m)} matches, {int(deg.sum())} of 500 hypotheses degenerate, winner {want['info']['best_hypothesis']}")
    assert len(m) >= 12 and 50 <= deg.sum() < 500 and want["info"]["best_hypothesis"] > 0 and deg[0:want["info"]["best_hypothesis"]].all()
    got = ctx.loop_match_frames(rgb_old, d_old, rgb_new, d_new, _intr(cam), p)
    _check_pair(got, want)
    assert got["info"]["n_inliers"] >= 0.9 * len(m)
    one_row = np.repeat(np.full((120, 160), 38, np.uint8)[..., None], 3, axis=2)
    one_row[::4, ::4] += 5
    one_row[40:46, 30:36] = 220
    one_row[40:46, 120:126] = 235
    d_top = d_old.copy()
    d_top[43:] = 0
    want = ref.loop_match_frames(one_row, d_top, np.roll(one_row, 4, axis=1), d_top, cam.fx, cam.fy, cam.cx, cam.cy, ref.Params())
    assert want["info"]["n_matches"] >= 3 and want["info"]["best_hypothesis"] == -1
    got = ctx.loop_match_frames(one_row, d_top, np.roll(one_row, 4, axis=1), d_top, _intr(cam))
    _check_pair(got, want)
    assert np.array_equal(got["bootstrap"], np.eye(4, dtype=np.float32))


def test_argument_errors(ctx, ktlib):
    import ctypes as C
    from kintinuous_amd import abi
    cam, d, rgb = mc.frame(160, 120, "A")
    intr, p = _intr(cam), abi.loop_match_params()
    pose, boot, info = (C.c_float * 16)(*([5.0] * 16)), (C.c_float * 16)(*([5.0] * 16)), abi.LoopMatchInfo()
    matches, inl = np.zeros((2048, 4), np.int32), np.zeros(2048, np.uint8)
    call = lambda **kw: ktlib.kt_loop_match_frames(*[kw.get(k, v) for k, v in (
        ("ctx", ctx.h), ("ro", rgb.ctypes.data), ("do", d.ctypes.data), ("rn", rgb.ctypes.data), ("dn", d.ctypes.data), ("cols", 160), ("rows", 120),
        ("intr", C.byref(intr)), ("p", C.byref(p)), ("pose", pose), ("boot", boot), ("m", matches.ctypes.data), ("inl", inl.ctypes.data), ("cap", 2048),
        ("info", C.byref(info)))])
    bad_p = [abi.loop_match_params(max_keypoints=0), abi.loop_match_params(max_keypoints=4097), abi.loop_match_params(ratio_den=0),
             abi.loop_match_params(reproj_px=0.0), abi.loop_match_params(max_hamming=257), abi.loop_match_params(n_hypotheses=-1)]
    for bad in [dict(ctx=None), dict(ro=None), dict(do=None), dict(rn=None), dict(dn=None), dict(cols=0), dict(rows=-1), dict(intr=None), dict(p=None),
                dict(pose=None), dict(boot=None), dict(info=None), dict(m=None)] + [dict(p=C.byref(b)) for b in bad_p]:
        assert call(**bad) == 2, bad
    assert list(pose) == [5.0] * 16 and list(boot) == [5.0] * 16
    assert call() == abi.KT_OK and info.n_matches > 3
    assert call(cap=3) == abi.KT_ERR_CAPACITY and info.n_matches > 3 and info.n_inliers == 0
    n = C.c_size_t(0)
    assert ktlib.kt_frame_keypoints(ctx.h, rgb.ctypes.data, d.ctypes.data, 160, 120, C.byref(p), None, None, None, 4, C.byref(n)) == 2
    assert ktlib.kt_frame_keypoints(ctx.h, rgb.ctypes.data, d.ctypes.data, 160, 120, C.byref(p), None, None, None, 0, C.byref(n)) == abi.KT_ERR_CAPACITY and n.value > 4
    desc, out = np.zeros((4, 8), np.uint32), np.zeros(4, np.int32)
    dm = lambda nn, no, o: ktlib.kt_descriptor_match(ctx.h, desc.ctypes.data, nn, desc.ctypes.data, no, C.byref(p), o, out.ctypes.data, out.ctypes.data)
    assert dm(0, 4, out.ctypes.data) == 2 and dm(4, 0, out.ctypes.data) == 2 and dm(4, 4, None) == 2 and dm(4, 4, out.ctypes.data) == abi.KT_OK


def test_shell(ctx, tmp_path):
    """host/loop_tool (RawLogReader -> LoopClosureDetection::processLoopClosureDetection -> LoopClosureBootstrap / LoopConstraintICP) on
    a .klg of A, B and C: the printed matches, inliers, score, verdict and constraint equal the C-ABI calls' through the binding."""
    from kintinuous_amd import build, klg
    build.build_host()
    cam = mc.frame(160, 120, "A")[0]
    frames = [(mc.frame(160, 120, w)[1], mc.frame(160, 120, w)[2]) for w in ("A", "B", "C", "C")]     # (the reader never returns a log's last frame)
    log = str(tmp_path / "abc.klg")
    klg.write_klg(log, frames, timestamps=[1000, 2000, 3000, 4000], cols=160, rows=120)
    calib = tmp_path / "calib.txt"
    calib.write_text(f"{cam.fx!r} {cam.fy!r} {cam.cx!r} {cam.cy!r}\n")
    voxel = np.float32(6.0) / np.float32(512)
    for b, verdict in ((1, "accepted"), (2, "rejected")):
        r = subprocess.run([build.LOOP_TOOL, "-l", log, "-a", "0", "-b", str(b), "-w", "160", "-h", "120", "-c", str(calib)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        f = dict(l.split(" ", 1) for l in r.stdout.strip().replace("; ", "\n").splitlines())
        got = ctx.loop_match_frames(frames[0][1], frames[0][0], frames[b][1], frames[b][0], _intr(cam))
        assert int(f["matches"]) == got["info"]["n_matches"] and int(f["inliers"]) == got["info"]["n_inliers"], (f, got["info"])
        assert f["verdict"].startswith(verdict), f
        if verdict == "accepted":
            M, score, _ = ctx.loop_icp_depth_frames(frames[0][0], frames[b][0], _intr(cam), got["bootstrap"], float(np.float32(2.5) * voxel))
            assert np.float32(float.fromhex(f["score"])).tobytes() == np.float32(score).tobytes()
            assert np.array([float.fromhex(v) for v in f["constraint"].split()], np.float32).tobytes() == M.tobytes()
            assert f["times"].split() == ["2000", "1000"] and int(f["projected"]) == got["info"]["n_inliers"]
    assert subprocess.run([build.LOOP_TOOL, "-l", log, "-a", "0", "-b", "9", "-w", "160", "-h", "120"], capture_output=True).returncode != 0
