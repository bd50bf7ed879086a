"""The voxel pass, the ray cast and the tracker's device-pose launches with the camera facing every way round the volume: the cases of
tests/heading_cases.py (tests/test_heading_cases.py asserts, without a GPU, that they are what they claim and that the oracle equals the
reference's own kernels on every one of them).

Every other GPU test that reaches integrate looks roughly down the volume's +z axis; the pre-pass of csrc/kt_volume.hip, which decides
what voxels the kernel visits at all, branches on the sign and size of b_z = Ri[8] * cell_z (kt_clip_halfline, the near slab, the depth-range
prune, the reciprocal guard of a z chunk), and a voxel it drops is silent.  The bar is the usual one -- every stored bit equals the oracle's --
plus, for the planned pre-pass (kt_integrate_plan through the hook kt_debug_tsdf_plan_ranges of csrc/kt_measure.h), that the wave-column
ranges made for a predicted pose cover every voxel the frame's own pose updates: zero misses.

Scratch mutations of kt_volume.hip, run once each on an MI355X: the near plane of kt_tsdf_interval_kernel clipped as if
b_z > 0 always fails 23 of the 44 test_integrate_heading[lean-wc4-*] cases, every -z-facing one among them, while tests/test_gpu_volume.py passes;
pm_A = 0 in kt_integrate_plan fails test_plan_ranges_cover_every_update at the (0.02, 0.02) margins (outside_yN and plan_outside_x0, aimed poses);
fabsf(bz) in the first kt_clip_halfline call passes, and is harmless: it only removes a bound that the four image sides imply.
"""
import numpy as np
import pytest

import heading_cases as H
from conftest import random_volume_state

gpu = pytest.mark.gpu
B = 32   # KT_BRICK
GUARD = 64


def tight_flags(vol, N):
    """tests/test_gpu_bricks.py: [bz, by, bx] = 1 iff the 32^3 storage brick holds a negative tsdf word"""
    nb = N // B
    return (vol.reshape(nb, B, nb, B, nb, B) < 0).any(axis=(1, 3, 5)).astype(np.uint8)


def _superset(flags, ref):
    return not (ref.astype(bool) & ~flags.astype(bool)).any()


def _same_maps(a, b):
    """tests/test_gpu_sweep.py: the same NaN positions (a NaN's sign and payload are the machine's) and the same bits everywhere else"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# conftest.py parametrises the voxel kernels by module name, so this module selects the forms itself (the fixture of tests/test_gpu_bricks.py)
FORMS = ["lean-wc4", "lean-wc5", "r3-wc4", "r3-wc5", "pointers"]


@pytest.fixture(params=FORMS)
def form(request, ktlib, monkeypatch):
    from kintinuous_amd import abi
    try:
        if request.param == "pointers":   # the pointer-addressed round-3 kernel: what N >= 1024 takes
            monkeypatch.setenv("KT_TSDF_POINTERS", "1")
        else:
            monkeypatch.delenv("KT_TSDF_POINTERS", raising=False)
            lean, wc = request.param.split("-wc")
            abi._chk(ktlib.kt_debug_tsdf_lean(1 if lean == "lean" else 0))
            abi._chk(ktlib.kt_debug_tsdf_wcl(int(wc)))
            assert ktlib.kt_debug_tsdf_kernel() == (b"kt_tsdf23_lean_kernel" if lean == "lean" else b"kt_tsdf23_kernel")
        yield request.param
    finally:
        ktlib.kt_debug_tsdf_lean(-1)
        ktlib.kt_debug_tsdf_wcl(-1)
        monkeypatch.delenv("KT_TSDF_POINTERS", raising=False)


_STATES = {}


def _state(N):
    """one random reachable volume state per N (conftest.random_volume_state), shared and left unchanged"""
    if N not in _STATES:
        vol, col = random_volume_state(np.random.default_rng(900 + N), N, True)
        for a in (vol, col):
            a.setflags(write=False)
        _STATES[N] = (vol, col)
    return _STATES[N]


def _flag_bytes(N):
    from kintinuous_amd import abi
    return abi.measure_lib().kt_debug_brick_count(N)


def _integrate_dev(ctx, O, case, which, dvol, dcol, dfl):
    """one integrate_tsdf_bricks call of a case's frame on device buffers; returns the scaled depth"""
    from kintinuous_amd.abi import Intr
    cam = H.camera(case.cam)
    depth, rgb, nmap, Rinv, t = H.inputs(O, case, which)
    dscaled = ctx.upload(np.full(depth.shape, -7.0, np.float32))
    ctx.integrate_tsdf_bricks(ctx.upload(depth), cam.cols, cam.rows, Intr(cam.fx, cam.fy, cam.cx, cam.cy), [H.SIZE] * 3, Rinv, t, H.trunc(case.N), dvol,
                              dscaled, case.wrap, dcol, ctx.upload(rgb), ctx.upload(nmap), True, case.N, dfl)
    ctx.sync()
    return ctx.download(dscaled, np.float32, depth.shape)


def _flags_buffer(N, start_vol):
    """the flags as the call finds them (N % 32 != 0: a pattern the call must leave alone) with guard bytes behind them"""
    n = _flag_bytes(N)
    if N % B:
        fl = np.full(n, 0xA5, np.uint8)
    else:
        fl = tight_flags(start_vol, N).reshape(-1)
    assert fl.size == n
    return np.concatenate([fl, np.full(GUARD, 0x5A, np.uint8)]), n


@gpu
@pytest.mark.parametrize("name", H.names())
def test_integrate_heading(ctx, oracle_mod, form, name):
    """The case's frame, then the frame from the neighbouring heading of its class, into (a) an empty volume and (b) a random reachable
    state: every tsdf word, colour byte and scaled-depth bit equals the oracle's after either frame.  Flags (N % 32 == 0): after the first
    frame into the empty volume they EQUAL tight_flags of the result (from an empty volume every stored negative is still there); after any
    other call they are a superset of it, nothing was lowered, and nothing was raised where nothing negative lies or lay.  Looking away:
    nothing changes and no flag rises."""
    O = oracle_mod
    case = H.by_name(name)
    N = case.N
    for tag, start in (("empty", None), ("state", _state(N))):
        ref = H.fused(O, case, start, tag)
        vol0, col0 = (np.zeros((N, N, N), np.int16), np.zeros((N, N, N, 4), np.uint8)) if start is None else start
        fb, n = _flags_buffer(N, vol0)
        dvol, dcol, dfl = ctx.upload(vol0), ctx.upload(col0), ctx.upload(fb)
        before_vol, before_fl = vol0, fb[:n]
        for which in (0, 1):
            rvol, rcol, rscaled, U = ref[which]
            msg = f"{form} {name} start={tag} frame {which} (U = {U})"
            scaled = _integrate_dev(ctx, O, case, which, dvol, dcol, dfl)
            gvol, gcol = ctx.download(dvol, np.int16, (N, N, N)), ctx.download(dcol, np.uint8, (N, N, N, 4))
            out = ctx.download(dfl, np.uint8, fb.shape)
            fl, guard = out[:n], out[n:]
            assert np.array_equal(scaled.view(np.uint32), rscaled.view(np.uint32)), f"{msg}: scaled depth"
            bad = gvol != rvol
            assert not bad.any(), f"{msg}: {int(bad.sum())} tsdf words differ, {int((bad & (gvol == before_vol)).sum())} of them were not updated at all"
            assert np.array_equal(gcol, rcol), f"{msg}: {int((gcol != rcol).any(axis=-1).sum())} colour / weight words differ"
            assert (guard == 0x5A).all(), f"{msg}: guard bytes"
            if N % B:
                assert (fl == 0xA5).all(), f"{msg}: N % 32 != 0 and the flags buffer was written"
            else:
                tight = tight_flags(gvol, N).reshape(-1)
                assert set(np.unique(fl)) <= {0, 1} and _superset(fl, tight), f"{msg}: a brick with a negative word is not flagged"
                assert _superset(fl, before_fl) and _superset(before_fl | tight, fl), f"{msg}: a flag was lowered, or raised where nothing negative lies or lay"
                if tag == "empty" and which == 0:
                    assert np.array_equal(fl, tight), f"{msg}: flags {fl.tolist()} tight {tight.tolist()}"
            if which == 0 and case.expect.get("away"):
                assert U == 0 and np.array_equal(gvol, vol0) and np.array_equal(gcol, col0) and np.array_equal(fl, before_fl), msg
            elif which == 0:
                assert U >= H.U_FLOOR, msg
            before_vol, before_fl = gvol, fl


def _cast_dev(ctx, case, turned, dvol, dcol, dflags):
    from kintinuous_amd.abi import Intr
    cam = H.camera(case.cam)
    v0, n0, c0 = H.prefill(cam.rows, cam.cols)
    dv, dn, dc = ctx.upload(v0), ctx.upload(n0), ctx.upload(c0)
    R, t = H.cast_pose(case, turned)
    counts = ctx.raycast_bricks(Intr(cam.fx, cam.fy, cam.cx, cam.cy), R, t, H.trunc(case.N), [H.SIZE] * 3, dvol, dv, dn, cam.cols, cam.rows, case.wrap, dc, dcol,
                                case.N, dflags)
    return ctx.download(dv, np.float32, v0.shape), ctx.download(dn, np.float32, n0.shape), ctx.download(dc, np.uint8, c0.shape), counts


@gpu
@pytest.mark.parametrize("name", H.names())
def test_raycast_heading(ctx, oracle_mod, name):
    """From the volume and the flags that the device's own two integrates left: the cast from the case's pose and from a quarter turn on,
    plain and with the flags (empty-space hops), equals the oracle's -- maps by the NaN-position rule, every colour byte, and S."""
    O = oracle_mod
    case = H.by_name(name)
    N, cam = case.N, H.camera(case.cam)
    ref = H.fused(O, case)
    vol0, col0 = np.zeros((N, N, N), np.int16), np.zeros((N, N, N, 4), np.uint8)
    fb, n = _flags_buffer(N, vol0)
    dvol, dcol, dfl = ctx.upload(vol0), ctx.upload(col0), ctx.upload(fb)
    for which in (0, 1):
        _integrate_dev(ctx, O, case, which, dvol, dcol, dfl)
    rvol, rcol = ref[1][0], ref[1][1]
    assert np.array_equal(ctx.download(dvol, np.int16, (N, N, N)), rvol) and np.array_equal(ctx.download(dcol, np.uint8, (N, N, N, 4)), rcol), name
    for turned in (False, True):
        v, nm, c, S = H.cast(O, O, case, turned, rvol, rcol, key="empty")
        hits = int(np.isfinite(v[:cam.rows]).sum())
        if H.inside(case) and not turned:
            assert hits > 1000, (name, hits)     # a camera inside the volume sees what it fused
        for flags in (None, dfl):
            msg = f"{name} turned={turned} {'flags' if flags is not None else 'plain'} (oracle hits {hits}, S {S})"
            gv, gn, gc, (gS, hopped, hop_iters, batch_iters) = _cast_dev(ctx, case, turned, dvol, dcol, flags)
            assert _same_maps(v, gv), f"{msg}: {int((v.view(np.uint32) != gv.view(np.uint32)).sum())} vertex-map words differ"
            assert _same_maps(nm, gn), f"{msg}: {int((nm.view(np.uint32) != gn.view(np.uint32)).sum())} normal-map words differ"
            assert np.array_equal(c, gc), f"{msg}: colour image"
            assert gS == S, f"{msg}: S {gS}"
            ghits = int(np.isfinite(gv[:cam.rows]).sum())
            assert ghits == hits and (hits <= 1000 or ghits > 1000), msg
            if flags is None or N % B:
                assert hopped == 0 and hop_iters == 0, msg
    out = ctx.download(dfl, np.uint8, fb.shape)
    assert (out[n:] == 0x5A).all()


# ---- the planned pre-pass ------------------------------------------------------------------------------------------------------------------------
MARGINS = [(0.0, 0.0), (1.0e-3, 3.0e-3), (0.02, 0.02)]      # (theta, tau): the values of test_gpu_tracker.py::test_plan_margins_hold_at_their_edge
FRACTIONS = [(0.9, 0.9), (0.98, 0.98)]


def _accepted(case, R, t, theta, tau):
    """the set-up kernel's test (csrc/kt_setup.hpp kt_setup_block0), in float as there: the plan is accepted iff |R - R^|_F <= 1.40 theta and
    |t - t^| <= 0.99 tau"""
    dr = np.sqrt(np.sum((R - case.R) * (R - case.R), dtype=np.float32))
    dt = np.sqrt(np.sum((t - case.t) * (t - case.t), dtype=np.float32))
    assert dr <= np.float32(1.40) * np.float32(theta) and dt <= np.float32(0.99) * np.float32(tau), (case.name, theta, tau, dr, dt)
    return float(dr), float(dt)


def _true_pose(O, case, theta, tau, fr, ft, rng):
    """the prediction (the case's pose) turned by fr theta about a seeded random axis and moved by ft tau in a seeded random direction"""
    axis, direction = rng.normal(size=3), rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    direction /= np.linalg.norm(direction)
    R = case.R if theta == 0 else np.ascontiguousarray(case.R.astype(np.float64) @ O.rodrigues(axis * (fr * theta)), np.float32)
    t = case.t if tau == 0 else (case.t.astype(np.float64) + direction * (ft * tau)).astype(np.float32)
    dr, dt = _accepted(case, R, t, theta, tau)
    if theta:
        assert dr >= 1.2 * fr * theta and dt >= 0.95 * ft * tau      # ... and it lands where it was aimed: near the edge
    return R, t


def _aligned_poses(O, case, theta, tau, fr, ft):
    """Eight more true poses at the same distance from the prediction, aimed instead of drawn: a turn about the camera's own y (x) axis with a
    step along its own x (y) axis, in the four sign combinations -- two of them push the image the same way (a random direction spends, on
    average, little of the translation margin on the side the rotation needs it)."""
    out = []
    R64 = case.R.astype(np.float64)
    for axis, other in ((1, 0), (0, 1)):
        for sr in (1, -1):
            for st in (1, -1):
                e = np.zeros(3)
                e[axis] = sr * fr * theta
                R = np.ascontiguousarray(R64 @ O.rodrigues(e), np.float32)
                t = (case.t.astype(np.float64) + R64[:, other] * (st * ft * tau)).astype(np.float32)
                _accepted(case, R, t, theta, tau)
                out.append((R, t, f"aimed: axis {'xy'[axis]} turn {sr:+d} step {st:+d}"))
    return out


@gpu
@pytest.mark.parametrize("name", H.names() + [c.name for c in H.plan_cases()])
def test_plan_ranges_cover_every_update(ctx, oracle_mod, ktlib, name):
    """kt_integrate_plan at kernel level, under both wave-column shapes: the ranges made for the predicted pose with margins (theta, tau)
    hold the logical z of every voxel that the oracle updates when it integrates the frame at a true pose 0.9 / 0.98 of both margins away --
    in a seeded random direction, and (0.98, non-zero margins) in eight aimed ones.  Zero misses is the condition.  The two cases of
    H.plan_cases run the widest margins at 0.98 only.  Against a vacuous pass (every range the whole column): for a camera inside the volume at
    least one wave-column is empty -- the half-space behind the camera guarantees it -- and at least one is not."""
    from kintinuous_amd import abi
    from kintinuous_amd.abi import Intr
    O = oracle_mod
    case = H.by_name(name)
    N, cam = case.N, H.camera(case.cam)
    big = case.cls == "plan"
    depth, rgb, nmap, Rinv_pred, t_pred = H.inputs(O, case, 0)
    ddepth, drgb, dnmap = ctx.upload(depth), ctx.upload(rgb), ctx.upload(nmap)
    rng = np.random.default_rng(77)
    updated = {}
    for (theta, tau) in (MARGINS[-1:] if big else MARGINS):
        poses = []
        for (fr, ft) in (FRACTIONS[-1:] if big else FRACTIONS):
            poses.append(_true_pose(O, case, theta, tau, fr, ft, rng) + (f"drawn at ({fr}, {ft})",))
        if theta:
            poses += _aligned_poses(O, case, theta, tau, *FRACTIONS[-1])
        plans = {}
        for wcl in (4, 5):
            abi._chk(ktlib.kt_debug_tsdf_wcl(wcl))
            try:
                plans[wcl] = ctx.tsdf_plan_ranges(ddepth, drgb, dnmap, cam.cols, cam.rows, Intr(cam.fx, cam.fy, cam.cx, cam.cy), [H.SIZE] * 3, Rinv_pred, t_pred,
                                                  H.trunc(N), case.wrap, N, theta, tau)
            finally:
                abi._chk(ktlib.kt_debug_tsdf_wcl(-1))
        for (R, t, label) in poses:
            key = R.tobytes() + t.tobytes()
            if key not in updated:
                vol, col = np.zeros((N, N, N), np.int16), np.zeros((N, N, N, 4), np.uint8)
                U, _ = O.integrate_tsdf(depth, H.intr(O, case), [H.SIZE] * 3, O.mat33_inverse(R), t, H.trunc(N), vol, case.wrap, col, rgb, nmap, True)
                sz, sy, sx = np.nonzero(col[..., 3])      # a voxel is updated where its weight byte left 0
                assert len(sz) == U, (name, len(sz), U)
                updated[key] = (sx, sy, (sz - case.wrap[2]) % N, U)
            sx, sy, z, U = updated[key]
            assert U == 0 if case.expect.get("away") else U >= H.U_FLOOR, (name, U)
            for wcl in (4, 5):
                msg = f"{name} theta={theta} tau={tau} {label} wcl={wcl} U={U}"
                assert plans[wcl] is not None, f"{msg}: KT_NO_PLAN"
                z0, z1, made_wcl = plans[wcl]
                assert made_wcl == wcl and z0.shape == z1.shape == (-(-N // (64 >> wcl)), -(-N // (1 << wcl))), msg
                assert ((z0 >= 0) & (z1 <= N)).all(), msg
                xg, yg = sx >> wcl, sy // (64 >> wcl)
                miss = (z < z0[yg, xg]) | (z >= z1[yg, xg])
                assert not miss.any(), f"{msg}: {int(miss.sum())} updated voxels lie outside their wave-column's range, first (sx, sy, z) {sx[miss][:3]}, {sy[miss][:3]}, {z[miss][:3]}"
                empty = z0 >= z1
                if H.inside(case):
                    assert empty.any() and not empty.all(), f"{msg}: {int(empty.sum())} of {empty.size} wave-columns are empty"
                elif not case.expect.get("away"):
                    assert not empty.all(), msg


# ---- the tracker's device-pose launches, round the compass -----------------------------------------------------------------------------------------
def _same_points(p, q):
    if len(p) != len(q):
        return False
    a = np.sort(np.ascontiguousarray(p).view(np.dtype((np.void, p.dtype.itemsize))).ravel())
    b = np.sort(np.ascontiguousarray(q).view(np.dtype((np.void, q.dtype.itemsize))).ravel())
    return bool(np.array_equal(a, b))


@gpu
@pytest.mark.parametrize("dynamic_cube", [0, 1])
@pytest.mark.parametrize("N", [64, 96])
def test_turn_ground_truth(ctx, oracle_mod, N, dynamic_cube):
    """The tracker and the oracle's tracker on ground-truth poses (H.turn_poses: 360 degrees of yaw, the floor, the ceiling, a roll): the
    voxel kernel and the fused ray-cast pyramid take the pose from the device, shifts and slices happen along the way.  As
    test_gpu_tracker.py::test_ground_truth_odometry: poses and wraps bit for bit every frame, slices the same points, volumes byte-identical,
    the predicted maps of all four levels equal in validity and bits.
    (In the oracle its X- and Z- slabs are empty, X+ holds 93 points at the most and Y never shifts: tests/test_gpu_shifts.py.)"""
    from kintinuous_amd import abi, synth
    from oracle import oracle
    cam = synth.Camera.small(160, 120)
    poses = H.turn_poses()
    assert len(poses) == 26
    frames = [tuple(np.ascontiguousarray(a) for a in synth.render(synth.Scene("room"), cam, R, c)) for R, c in poses]
    stamps = np.array([33333 * (k + 1) for k in range(len(frames))], np.uint64)
    rows = synth.ground_truth_rows(poses)
    g = abi.TrackerConfig(cam.cols, cam.rows, N, cam.fx, cam.fy, cam.cx, cam.cy, 6.0, 3, 2, 0, 0, 0, 0, 0, 0, dynamic_cube, 0)
    o = oracle.OTrackerConfig(cam.cols, cam.rows, N, cam.fx, cam.fy, cam.cx, cam.cy, 6.0, 3, 2, 0, 0, 0, 0, 0, 0, dynamic_cube, 0)
    trk, otr = abi.Tracker(ctx, g), oracle.OracleTracker(o)
    try:
        trk.load_trajectory(stamps, rows)
        otr.load_trajectory(stamps, rows)
        for k, (d, rgb) in enumerate(frames):
            trk.process_frame_host(d, rgb, int(stamps[k]))
            otr.process_frame(d, rgb, int(stamps[k]))
            assert trk.num_poses() == otr.num_poses() == k + 1
            R, t, gc = trk.pose()
            Ro, to, go = otr.pose()
            assert np.array_equal(R, Ro) and np.array_equal(t, to) and np.array_equal(gc, go), k
            assert np.array_equal(trk.voxel_wrap(), otr.voxel_wrap()), k
        # the camera did turn: the last pose is the roll of 180 degrees (x and y reversed)
        R, _, _ = trk.pose()
        assert np.abs(R - np.diag([-1.0, -1.0, 1.0])).max() < 1e-5
        assert trk.num_slices() == otr.num_slices()
        if dynamic_cube:
            assert trk.num_slices() >= 20
        for i in range(trk.num_slices()):
            p, dim = trk.slice(i)
            q, dim2 = otr.slice(i)
            assert dim == dim2 and _same_points(p, q), (i, len(p), len(q))
        v, ov = trk.volume(), otr.volume()
        c, oc = trk.color_volume(), otr.color_volume()
        assert int((oc[..., 3] != 0).sum()) > 10000
        assert np.array_equal(v, ov), f"{int((v != ov).sum())} tsdf words differ"
        assert np.array_equal(c, oc), f"{int((c != oc).any(axis=-1).sum())} colour / weight words differ"
        for lvl in range(4):
            for a, b in ((trk.vmap_g_prev(lvl), otr.vmap_g_prev(lvl)), (trk.nmap_g_prev(lvl), otr.nmap_g_prev(lvl))):
                n = a.shape[0] // 3
                va, vb = np.isfinite(a[:n]), np.isfinite(b[:n])
                assert np.array_equal(va, vb) and va.sum() > 0, f"level {lvl}: validity masks differ"
                for pl in range(3):
                    assert np.array_equal(a[pl * n:(pl + 1) * n][va].view(np.uint32), b[pl * n:(pl + 1) * n][va].view(np.uint32)), (lvl, pl)
    finally:
        trk.close()
        otr.close()
