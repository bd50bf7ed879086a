"""The negative-brick flags of the voxel kernels and the ray cast's empty-space hops (csrc/kt_volume.hip: the flags; csrc/kt_raycast.hip: kt_raycast_kernel<.., SKIP>), at kernel
level, through the hooks of csrc/kt_measure.h (kt_debug_integrate_bricks, kt_debug_raycast_bricks) and csrc/kt_debug.h (kt_tracker_debug_bricks).

The whole definition of a correct flag set is `tight_flags`: flag [bz, by, bx] is 1 iff the 32^3 STORAGE brick holds a negative tsdf word.  A flag
set is safe for a volume iff it is a superset of tight_flags(volume).  The bar for the ray cast is the usual one: every bit of the vertex map, the
normal map and the colour image equals the oracle's, and the sample count S too -- with hops, without hops, and with either source of flags.

The volumes of the ray cast cases are built so that a wrong hop shows: negative sheets one voxel thick ON brick faces with unflagged neighbours,
zeros directly in front of negatives, random states with empty bricks.  `test_case_conditions` (no GPU) asserts with the oracle and a numpy
restatement of the march that the committed seeds really put surfaces there, so that a later change of seeds cannot empty a case.

Not covered: the host branch nb^3 > 32768 of kt_raycast_impl (it needs N > 1024), and the pyramid-fused PYR + SKIP form of the kernel, whose extra
arguments kt_raycast does not have (the tracker tests of this module and of test_gpu_tracker.py run it, end to end).

Measured on an MI355X (a report, not a bar), the largest share of the march samples that hops replaced, volumes 1 - 6: 0.64, 0.74, 0.62, 0.88, 0.89, 0
(with the scratch mutations of the two files that each fail a test of this module).
"""
import functools

import numpy as np
import pytest

from conftest import random_rotation, random_volume_state

gpu = pytest.mark.gpu
B = 32   # KT_BRICK


# ---- the reference for flags -----------------------------------------------------------------------------------------------------------------
def tight_flags(vol, N):
    """[bz, by, bx] = 1 iff any(vol[32 bz : 32 bz + 32, 32 by : .., 32 bx : ..] < 0), over storage order"""
    nb = N // B
    assert N % B == 0 and vol.shape == (N, N, N)
    return (vol.reshape(nb, B, nb, B, nb, B) < 0).any(axis=(1, 3, 5)).astype(np.uint8)


def _superset(flags, ref):
    return not (ref.astype(bool) & ~flags.astype(bool)).any()


# ---- frames and poses ------------------------------------------------------------------------------------------------------------------------
def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)


@functools.lru_cache(maxsize=None)
def _ragged_frame():
    """one 173 x 97 render: waves of the ray cast with lanes outside the image, pixel tiles of the voxel pass that are not whole"""
    from kintinuous_amd import synth
    cam = synth.Camera.small(173, 97)
    R, c = synth.orbit_trajectory(8)[1]
    return cam, synth.render(synth.Scene("room"), cam, R, c)


def _nmap_of(oracle, cam, depth):
    from oracle.oracle import OIntr
    return oracle.create_nmap(oracle.create_vmap(OIntr(cam.fx, cam.fy, cam.cx, cam.cy), oracle.bilateral_filter(depth)))


_NMAPS = {}


def _frame(oracle, small_scene, which):
    """(cam, depth, rgb, nmap) of frame `which` of small_scene (160 x 120), or of the ragged render (which = 'ragged'); computed once"""
    if which not in _NMAPS:
        if which == "ragged":
            cam, (depth, rgb) = _ragged_frame()
        else:
            cam, (depth, rgb) = small_scene[0], small_scene[1][which]
        _NMAPS[which] = (cam, depth, rgb, _nmap_of(oracle, cam, depth))
    return _NMAPS[which]


def _trunc(N, size):
    return max(0.06, 2.1 * float(np.max(size)) / N)


# ---- voxel-kernel forms: conftest.py parametrises by module name, so this module selects the forms itself ----------------------------------
FORMS = ["lean-wc4", "lean-wc5", "r3-wc4", "r3-wc5", "pointers"]   # lean-wc5 streams its volume words with NT stores, lean-wc4 does not


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


def _integrate_dev(ctx, cam, depth, rgb, nmap, N, size, Rinv, t, trunc, wrap, vol, col, flags, guard=64):
    """one kt_debug_integrate_bricks call on host arrays: (volume, colour volume, flags, the guard bytes behind the flags)"""
    from kintinuous_amd.abi import Intr
    nbytes = flags.size
    fb = np.concatenate([flags.reshape(-1), np.full(guard, 0x5A, np.uint8)])
    dvol, dcol, dfl = ctx.upload(vol), ctx.upload(col), ctx.upload(fb)
    size3 = [size] * 3 if np.isscalar(size) else list(size)
    ctx.integrate_tsdf_bricks(ctx.upload(depth), cam.cols, cam.rows, Intr(cam.fx, cam.fy, cam.cx, cam.cy), size3, Rinv, t, trunc, dvol,
                              ctx.empty(depth.size * 4), wrap, dcol, ctx.upload(rgb), ctx.upload(nmap), True, N, dfl)
    ctx.sync()
    out = ctx.download(dfl, np.uint8, fb.shape)
    return ctx.download(dvol, np.int16, vol.shape), ctx.download(dcol, np.uint8, col.shape), out[:nbytes].reshape(flags.shape), out[nbytes:]


def _integrate_ref(oracle, cam, depth, rgb, nmap, N, size, Rinv, t, trunc, wrap, vol, col):
    from oracle.oracle import OIntr
    vol, col = vol.copy(), col.copy()
    size3 = [size] * 3 if np.isscalar(size) else list(size)
    U, _ = oracle.integrate_tsdf(depth, OIntr(cam.fx, cam.fy, cam.cx, cam.cy), size3, Rinv, t, trunc, vol, wrap, col, rgb, nmap, True)
    return vol, col, U


# ---- flags written by integrate --------------------------------------------------------------------------------------------------------------
def _one_frame_cases(N):
    rng = np.random.default_rng(11)
    Rrot = random_rotation(rng, 0.5)
    poses = [("identity", np.eye(3, dtype=np.float32), [3, 3, 3]), ("rotated", Rrot, [2.8, 3.1, 2.9]), ("outside", np.eye(3, dtype=np.float32), [3, 3, -0.45])]
    wraps = [[0, 0, 0], [32, 64, 0], [31, 1, 33], [N - 1, 0, 17]]
    cases = [(0, w, p) for w in wraps for p in poses]
    cases += [("ragged", w, poses[1]) for w in wraps]
    return cases


_ONE_FRAME_REF = {}


@gpu
@pytest.mark.parametrize("N", [64, 96, 128])
def test_one_frame_flags_equal_tight(ctx, oracle_mod, small_scene, form, N):
    """One frame into an empty volume with zeroed flags: from an empty volume every stored negative is still there afterwards, so the flags
    must EQUAL tight_flags of the result; and the stored words are the oracle's, so the flags path changes nothing that is stored."""
    size = 6.0
    trunc = _trunc(N, size)
    nb = N // B
    for i, (which, wrap, (pname, R, t)) in enumerate(_one_frame_cases(N)):
        cam, depth, rgb, nmap = _frame(oracle_mod, small_scene, which)
        Rinv = oracle_mod.mat33_inverse(R)
        zero_v, zero_c = np.zeros((N, N, N), np.int16), np.zeros((N, N, N, 4), np.uint8)
        if (N, i) not in _ONE_FRAME_REF:
            _ONE_FRAME_REF[(N, i)] = _integrate_ref(oracle_mod, cam, depth, rgb, nmap, N, size, Rinv, t, trunc, wrap, zero_v, zero_c)
        rvol, rcol, U = _ONE_FRAME_REF[(N, i)]
        tight = tight_flags(rvol, N)
        assert U > 100 and tight.any(), (which, wrap, pname)
        gvol, gcol, fl, guard = _integrate_dev(ctx, cam, depth, rgb, nmap, N, size, Rinv, t, trunc, wrap, zero_v, zero_c, np.zeros((nb, nb, nb), np.uint8))
        msg = f"{form} N={N} frame={which} wrap={wrap} pose={pname}"
        assert np.array_equal(gvol, rvol) and np.array_equal(gcol, rcol), msg
        assert np.array_equal(fl, tight), f"{msg}: flags {fl.ravel().tolist()} tight {tight.ravel().tolist()}"
        assert (guard == 0x5A).all(), msg


@gpu
@pytest.mark.parametrize("N", [64, 96])
def test_accumulated_flags(ctx, oracle_mod, small_scene, form, N):
    """Four frames with changing wraps and poses (the recipe of test_integrate_random_poses_wrapped_and_accumulated): after every frame the
    flags are a superset of tight_flags(volume), and nothing was raised where nothing negative lies or lay: flags <= flags before | bricks
    holding a word that changed to, or stayed at, a negative value in the call (= tight_flags of the new volume)."""
    rng = np.random.default_rng(7)
    size, nb = 6.0, N // B
    trunc = _trunc(N, size)
    vol, col = np.zeros((N, N, N), np.int16), np.zeros((N, N, N, 4), np.uint8)
    flags = np.zeros((nb, nb, nb), np.uint8)
    raised = 0
    for k in range(4):
        cam, depth, rgb, nmap = _frame(oracle_mod, small_scene, k)
        R = random_rotation(rng, 0.5)
        Rinv = oracle_mod.mat33_inverse(R)
        t = (np.array([3, 3, 3]) + rng.uniform(-0.4, 0.4, 3)).astype(np.float32)
        wrap = [int(w) for w in rng.integers(0, N, 3)]
        rvol, rcol, U = _integrate_ref(oracle_mod, cam, depth, rgb, nmap, N, size, Rinv, t, trunc, wrap, vol, col)
        gvol, gcol, fl, guard = _integrate_dev(ctx, cam, depth, rgb, nmap, N, size, Rinv, t, trunc, wrap, vol, col, flags)
        assert U > 100 and np.array_equal(gvol, rvol) and np.array_equal(gcol, rcol), (form, k)
        tight = tight_flags(gvol, N)
        assert _superset(fl, tight), f"{form} frame {k} wrap {wrap}: a brick with a negative word is not flagged"
        assert _superset(fl, flags), f"{form} frame {k}: a flag was lowered"
        assert _superset(flags | tight, fl), f"{form} frame {k} wrap {wrap}: a flag was raised where nothing negative lies or lay"
        assert set(np.unique(fl)) <= {0, 1} and (guard == 0x5A).all()
        raised += int(fl.sum()) - int(flags.sum())
        vol, col, flags = gvol, gcol, fl
    assert raised > 0


@gpu
def test_random_state_flags(ctx, oracle_mod, small_scene, form):
    """Into a random-state volume whose starting flags are tight_flags of that state: a superset of tight_flags afterwards."""
    N, size = 96, 6.0
    trunc = _trunc(N, size)
    rng = np.random.default_rng(23)
    vol, col = _empty_brick_state(rng, N)
    flags = tight_flags(vol, N)
    assert flags.any() and not flags.all()
    cam, depth, rgb, nmap = _frame(oracle_mod, small_scene, 1)
    R = random_rotation(rng, 0.5)
    Rinv = oracle_mod.mat33_inverse(R)
    wrap = [31, 1, 33]
    rvol, rcol, U = _integrate_ref(oracle_mod, cam, depth, rgb, nmap, N, size, Rinv, [3.1, 2.9, 3.0], trunc, wrap, vol, col)
    gvol, gcol, fl, guard = _integrate_dev(ctx, cam, depth, rgb, nmap, N, size, Rinv, [3.1, 2.9, 3.0], trunc, wrap, vol, col, flags)
    assert U > 100 and np.array_equal(gvol, rvol) and np.array_equal(gcol, rcol)
    assert _superset(fl, tight_flags(gvol, N)) and _superset(fl, flags) and (guard == 0x5A).all()
    assert int(fl.sum()) > int(flags.sum())   # the frame put negative words into bricks that had none


@gpu
def test_zero_depth_leaves_flags(ctx, oracle_mod, small_scene, form):
    N, size = 64, 6.0
    nb = N // B
    cam, depth, rgb, nmap = _frame(oracle_mod, small_scene, 0)
    rng = np.random.default_rng(5)
    for pattern in (np.zeros((nb, nb, nb), np.uint8), rng.integers(0, 2, (nb, nb, nb)).astype(np.uint8), np.full((nb, nb, nb), 0xA5, np.uint8)):
        vol, col = np.zeros((N, N, N), np.int16), np.zeros((N, N, N, 4), np.uint8)
        gvol, gcol, fl, guard = _integrate_dev(ctx, cam, np.zeros_like(depth), rgb, nmap, N, size, np.eye(3), [3, 3, 3], 0.2, [17, 5, 40], vol, col, pattern)
        assert not gvol.any() and not gcol.any()
        assert np.array_equal(fl, pattern) and (guard == 0x5A).all(), form


@gpu
def test_n80_ignores_flags(ctx, oracle_mod, small_scene, form, ktlib):
    """N % 32 != 0: the call succeeds, stores the oracle's words and leaves the flags buffer alone."""
    from kintinuous_amd import abi
    N, size = 80, 6.0
    trunc = _trunc(N, size)
    n = abi.measure_lib().kt_debug_brick_count(N)
    assert n == 27 and abi.measure_lib().kt_debug_brick_count(96) == 27 and abi.measure_lib().kt_debug_brick_count(64) == 8
    cam, depth, rgb, nmap = _frame(oracle_mod, small_scene, 0)
    vol, col = np.zeros((N, N, N), np.int16), np.zeros((N, N, N, 4), np.uint8)
    rvol, rcol, U = _integrate_ref(oracle_mod, cam, depth, rgb, nmap, N, size, np.eye(3), [3, 3, 3], trunc, [31, 1, 33], vol, col)
    gvol, gcol, fl, guard = _integrate_dev(ctx, cam, depth, rgb, nmap, N, size, np.eye(3), [3, 3, 3], trunc, [31, 1, 33], vol, col, np.full(n, 0xA5, np.uint8))
    assert U > 100 and (rvol < 0).any() and np.array_equal(gvol, rvol) and np.array_equal(gcol, rcol)
    assert (fl == 0xA5).all() and (guard == 0x5A).all()


# ---- flags kept by the tracker ---------------------------------------------------------------------------------------------------------------
def _check_tracker_flags(trk, N, where):
    fl = trk.debug_bricks()
    tight = tight_flags(trk.volume(), N)
    assert set(np.unique(fl)) <= {0, 1}
    assert _superset(fl, tight), f"{where}: bricks {np.argwhere(tight.astype(bool) & ~fl.astype(bool)).tolist()} hold negative words and are not flagged"
    return fl, tight


@gpu
def test_tracker_flags_crabwalk(ctx):
    """N = 96 on the crab-walk of test_gpu_mesh.py::test_tracker_mesh_stage: X+, X- and Z shifts move the wrap and clear slabs under the flags."""
    from kintinuous_amd import abi, synth
    cam = synth.Camera.small(160, 120)
    scene = synth.Scene("wall")
    traj = synth.crabwalk_trajectory(420)
    idx = list(range(0, 40, 2)) + list(range(40, 0, -2))
    N = 96
    trk = abi.Tracker(ctx, abi.TrackerConfig(cam.cols, cam.rows, N, cam.fx, cam.fy, cam.cx, cam.cy, 5.2, 3, 2, 0, 0, 0, 0, 0, 0))
    try:
        wraps = set()
        for k, i in enumerate(idx):
            trk.process_frame_host(*synth.render(scene, cam, *traj[i]), 33333 * k)
            if k % 6 == 5 or k == len(idx) - 1:
                fl, _ = _check_tracker_flags(trk, N, f"frame {k}")
                wraps.add(tuple(int(w) for w in trk.voxel_wrap()))
        assert len(wraps) >= 3 and fl.any()   # the checks saw the volume under several wraps
        trk.finalise()
        _check_tracker_flags(trk, N, "finalised")
    finally:
        trk.close()


@gpu
def test_tracker_flags_orbit_and_reset(ctx, small_scene):
    from kintinuous_amd import abi
    cam, frames, _ = small_scene
    N = 64
    trk = abi.Tracker(ctx, abi.TrackerConfig(cam.cols, cam.rows, N, cam.fx, cam.fy, cam.cx, cam.cy, 6.0, 14, 2, 0, 0, 0, 0, 0, 0))
    try:
        for k, (d, rgb) in enumerate(frames):
            trk.process_frame_host(d, rgb, 33333 * k)
            if k % 3 == 2 or k == len(frames) - 1:
                fl, _ = _check_tracker_flags(trk, N, f"frame {k}")
        assert fl.any()
        trk.reset()
        assert not trk.debug_bricks().any()
        trk.process_frame_host(*frames[0], 0)
        fl, tight = _check_tracker_flags(trk, N, "first frame after reset")
        assert tight.any() and np.array_equal(fl, tight)   # one frame into a cleared volume: every stored negative is still there
    finally:
        trk.close()


# ---- SKIP ray cast = no-SKIP ray cast = oracle: the volumes --------------------------------------------------------------------------------------
def _rotate_storage(vol, wrap):
    """logical volume -> storage layout for a given wrap (storage[(i + w) % N] = logical[i])"""
    return np.roll(vol, shift=(wrap[2], wrap[1], wrap[0]), axis=(0, 1, 2))


def _empty_brick_state(rng, N):
    """volume 4: a random reachable state in which a seeded 70 % of the bricks hold no negative word (v -> |v| there)"""
    vol, col = random_volume_state(rng, N, True)
    nb = N // B
    empty = rng.random((nb, nb, nb)) < 0.7
    m = np.repeat(np.repeat(np.repeat(empty, B, 0), B, 1), B, 2)
    vol[m] = np.abs(vol[m])
    return vol, col


def _sheet_volume(N, seed, zeros):
    """volume 2 (zeros = False): +20000, weight 1, everywhere; a seeded half of the storage bricks carry a one-voxel negative sheet on their first
    or last storage plane along a seeded axis.  With tight flags the brick behind such a face is unflagged unless it carries a sheet itself:
    rays hop to within the margin of the face and the first normal sample is the negative one.
    volume 3 (zeros = True): the same, and the plane just outside each sheet, where it lies in an unflagged brick, is 0: the reference sees
    0 -> negative, which is no crossing; plus isolated zeros and cleared slabs (tsdf and colour 0, as a volume shift leaves them) inside unflagged
    bricks."""
    rng = np.random.default_rng(seed)
    nb = N // B
    vol = np.full((N, N, N), 20000, np.int16)
    col = rng.integers(0, 256, (N, N, N, 4)).astype(np.uint8)
    col[..., 3] = 1
    ids = rng.permutation(nb ** 3)[: nb ** 3 // 2]
    chosen = np.zeros(nb ** 3, bool)
    chosen[ids] = True
    chosen = chosen.reshape(nb, nb, nb)
    sheets = []
    for b in ids:
        bb = np.unravel_index(b, (nb, nb, nb))
        axis, last = int(rng.integers(3)), int(rng.integers(2))
        sl = [slice(B * bb[0], B * bb[0] + B), slice(B * bb[1], B * bb[1] + B), slice(B * bb[2], B * bb[2] + B)]
        plane = B * bb[axis] + (B - 1 if last else 0)
        sl[axis] = plane
        sheets.append((bb, axis, last, tuple(sl)))
    if zeros:
        for bb, axis, last, sl in sheets:
            nbr = list(bb)
            nbr[axis] = (bb[axis] + (1 if last else -1)) % nb
            if not chosen[tuple(nbr)]:
                s2 = list(sl)
                s2[axis] = (sl[axis] + (1 if last else -1)) % N
                vol[tuple(s2)] = 0
        free = np.repeat(np.repeat(np.repeat(~chosen, B, 0), B, 1), B, 2)
        vol[free & (rng.random((N, N, N)) < 0.02)] = 0            # isolated zeros
        for b in np.flatnonzero(~chosen.reshape(-1))[::2]:          # cleared slabs, 4 planes thick, inside every other unflagged brick
            bb = np.unravel_index(b, (nb, nb, nb))
            axis, at = int(rng.integers(3)), int(rng.integers(4, 24))
            sl = [slice(B * bb[0], B * bb[0] + B), slice(B * bb[1], B * bb[1] + B), slice(B * bb[2], B * bb[2] + B)]
            sl[axis] = slice(B * bb[axis] + at, B * bb[axis] + at + 4)
            vol[tuple(sl)] = 0
            col[tuple(sl)] = 0
    for bb, axis, last, sl in sheets:
        shape = vol[sl].shape
        vol[sl] = -rng.integers(2000, 32767, shape).astype(np.int16)
    assert np.array_equal(tight_flags(vol, N), chosen.astype(np.uint8))
    return vol, col


WRAPS = [[0, 0, 0], [32, 64, 0], [17, 5, 40], [31, 1, 33]]
POSE_SEED = {1: 4, 2: 2, 3: 2, 4: 2, 5: 2, 6: 2}   # chosen so that test_case_conditions holds (it asserts that they do)


def _poses(volume_id, size3):
    """(name, R, t, integer principal point): identity near the centre (the centre column has rd.x == 0: the 1e-15 path), a random rotation up
    to pi with the camera inside, 0.45 m outside the near face, outside looking in through the x = 0 / z = 0 edge, and looking away"""
    rng = np.random.default_rng(POSE_SEED[volume_id])
    c = np.asarray(size3, np.float32) / 2
    I = np.eye(3, dtype=np.float32)
    return [("identity", I, (c + np.array([0.33, -0.21, 0.27], np.float32)).astype(np.float32), True),   # (off the brick faces that meet at the centre)
            ("rotated", random_rotation(rng, np.pi), (c + rng.uniform(-0.4, 0.4, 3)).astype(np.float32), False),
            ("outside", I, np.array([c[0], c[1], -0.45], np.float32), False),
            ("edge", _rot_y(np.pi / 4), np.array([-0.3, c[1] + 0.1, -0.3], np.float32), False),
            ("away", _rot_y(np.pi), np.array([c[0], c[1], -0.45], np.float32), False)]


VOLUMES = {1: "fused", 2: "sheets", 3: "zeros-before-negatives", 4: "random-state", 5: "all-unflagged", 6: "all-flagged"}
VOLUME_N = {1: 96, 2: 128, 3: 128, 4: 96, 5: 64, 6: 64}


@functools.lru_cache(maxsize=None)
def _small_frames():
    from kintinuous_amd import synth
    cam = synth.Camera.small(160, 120)
    traj = synth.orbit_trajectory(8)
    return cam, [synth.render(synth.Scene("room"), cam, R, c) for (R, c) in traj], traj


def _fused(oracle, N, size3, wrap, integrate=None):
    """volume 1: three integrates along the orbit, straight into the storage layout of `wrap` (equal to _rotate_storage of the wrap-0 result:
    test_volume_1_is_a_rolled_volume).  integrate = the device's (with flags) or, by default, the oracle's."""
    cam, frames, traj = _small_frames()
    trunc = _trunc(N, size3)
    vol, col = np.zeros((N, N, N), np.int16), np.zeros((N, N, N, 4), np.uint8)
    flags = np.zeros((N // B,) * 3, np.uint8)
    for k in range(3):
        depth, rgb = frames[k]
        nmap = _nmap_of(oracle, cam, depth)
        R, c = traj[k]
        Rinv = oracle.mat33_inverse(R.astype(np.float32))
        t = (c + np.asarray(size3) / 2).astype(np.float32)
        if integrate is None:
            vol, col, _ = _integrate_ref(oracle, cam, depth, rgb, nmap, N, list(size3), Rinv, t, trunc, wrap, vol, col)
        else:
            vol, col, flags, _ = integrate(cam, depth, rgb, nmap, N, list(size3), Rinv, t, trunc, wrap, vol, col, flags)
    return vol, col, flags


_VOL_CACHE = {}


def _volume(oracle, volume_id, wrap, size3=(6.0, 6.0, 6.0)):
    """(volume, colour volume, flags) of a case in storage order; the flags are tight_flags except for volume 6 (all ones)"""
    key = (volume_id, tuple(wrap), tuple(size3))
    if key not in _VOL_CACHE:
        N = VOLUME_N[volume_id]
        if volume_id == 1:
            vol, col, _ = _fused(oracle, N, size3, wrap)
        elif volume_id in (2, 3):
            vol, col = _sheet_volume(N, 40 + volume_id, volume_id == 3)
        elif volume_id == 4:
            vol, col = _empty_brick_state(np.random.default_rng(44), N)
        elif volume_id == 5:
            rng = np.random.default_rng(45)
            vol = rng.integers(1, 32768, (N, N, N)).astype(np.int16)
            col = rng.integers(0, 256, (N, N, N, 4)).astype(np.uint8)
        else:
            vol, col = random_volume_state(np.random.default_rng(46), N, True)
        if volume_id in (4, 6):
            # every ray of a camera inside the volume starts in the camera's own voxel: where the random state is negative there, all of them
            # leave (- -> +) at once.  The 5^3 voxels around the two inside cameras are made non-negative.
            for (_, _, t, _) in _poses(volume_id, size3)[:2]:
                g = np.floor(np.asarray(t, np.float64) / (np.asarray(size3) / N)).astype(int)
                ix = [(np.arange(g[k] - 2, g[k] + 3) + wrap[k]) % N for k in range(3)]
                sel = np.ix_(ix[2], ix[1], ix[0])
                vol[sel] = np.abs(vol[sel])
        flags = tight_flags(vol, N) if volume_id != 6 else np.ones((N // B,) * 3, np.uint8)
        for a in (vol, col, flags):
            a.setflags(write=False)
        _VOL_CACHE[key] = (vol, col, flags)
    return _VOL_CACHE[key]


def _cam_intr(cam, integer_pp):
    return (cam.fx, cam.fy, float(round(cam.cx)), float(round(cam.cy))) if integer_pp else (cam.fx, cam.fy, cam.cx, cam.cy)


def _cases(volume_id):
    """the ray cast cases of a volume: (name, wrap, size3, R, t, intr 4-tuple, cols, rows)"""
    from kintinuous_amd import synth
    cam = synth.Camera.small(160, 120)
    out = []
    cube = (6.0, 6.0, 6.0)
    for wrap in WRAPS:
        for (pname, R, t, ipp) in _poses(volume_id, cube):
            out.append((f"{pname}/wrap={wrap}", wrap, cube, R, t, _cam_intr(cam, ipp), cam.cols, cam.rows))
    if volume_id in (1, 2):
        rag = synth.Camera.small(173, 97)
        for (pname, R, t, ipp) in _poses(volume_id, cube)[:2]:
            out.append((f"{pname}/173x97/wrap={WRAPS[3]}", WRAPS[3], cube, R, t, _cam_intr(rag, ipp), rag.cols, rag.rows))
    if volume_id == 1:   # unequal edges
        size3 = (4.5, 5.0, 6.0)
        for (pname, R, t, ipp) in _poses(volume_id, size3)[:3]:
            out.append((f"{pname}/edges={size3}/wrap={WRAPS[2]}", WRAPS[2], size3, R, t, _cam_intr(cam, ipp), cam.cols, cam.rows))
    return out


def _prefill(rows, cols):
    rng = np.random.default_rng(3)
    return (rng.uniform(-1, 1, (3 * rows, cols)).astype(np.float32), rng.uniform(-1, 1, (3 * rows, cols)).astype(np.float32),
            rng.integers(0, 255, (rows, cols, 4)).astype(np.uint8))


_ORACLE_CAST = {}


def _oracle_cast(oracle, key, vol, col, N, wrap, size3, R, t, intr, cols, rows):
    """the oracle's maps for a case, from the pre-filled buffers; computed once (key) and shared by the tests that need it"""
    from oracle.oracle import OIntr
    if key is None or key not in _ORACLE_CAST:
        v, n, c = (a.copy() for a in _prefill(rows, cols))
        S = oracle.raycast(OIntr(*intr), R, t, _trunc(N, size3), list(size3), np.ascontiguousarray(vol), v, n, wrap, c, np.ascontiguousarray(col))
        for a in (v, n, c):
            a.setflags(write=False)
        if key is None:
            return v, n, c, S
        _ORACLE_CAST[key] = (v, n, c, S)
    return _ORACLE_CAST[key]


# ---- a numpy restatement of the march (ray_caster.cu:340-352), for the conditions only ------------------------------------------------------------
def _march(vol, N, wrap, size3, R, t, intr, cols, rows, trunc):
    """Per pixel: how the march ended (0 never entered / ran out, 1 hit (+ -> -), 2 left (- -> +)), the STORAGE voxel of the sample it ended on,
    and whether a negative sample ever followed a sample that was exactly 0.  float32 throughout with the products of p = rs + rd t rounded once
    (in double), as the reference's fused multiply-adds are; a pixel that differs from the oracle in the last bit of a coordinate can only move
    counts by a few, and the conditions that use them have margins of 5x and more (test_case_conditions also checks the hits against the oracle)."""
    f = np.float32
    fx, fy, cx, cy = (f(v) for v in intr)
    x, y = np.meshgrid(np.arange(cols, dtype=f), np.arange(rows, dtype=f))
    rn = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1).reshape(-1, 3)
    R = np.asarray(R, f)
    t = np.asarray(t, f)
    nxt = (rn[:, None, :] * R[None, :, :]).astype(f)
    nxt = ((nxt[..., 0] + nxt[..., 1]) + nxt[..., 2]) + t
    rd = nxt - t
    rd = (rd / np.sqrt((rd * rd).sum(-1, dtype=f))[:, None]).astype(f)
    rd[rd == 0] = f(1e-15)
    size = np.asarray(size3, f)
    cell = (size / f(N)).astype(f)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tmin = ((np.where(rd > 0, f(0), size) - t) / rd).astype(f)
        tmax = ((np.where(rd > 0, size, f(0)) - t) / rd).astype(f)
    t0 = np.maximum(tmin.max(-1), f(0))
    t1 = tmax.min(-1)
    step = f(f(trunc) * f(0.8))
    max_time = f(3) * (size[0] + size[1] + size[2])
    w = np.asarray(wrap) % N

    def pos(tt):
        return (rd.astype(np.float64) * tt[:, None].astype(np.float64) + t.astype(np.float64)).astype(f)

    def voxel(p):
        return np.floor((p / cell).astype(f)).astype(np.int64)

    def read(g):
        s = (g + w) % N
        return vol[s[:, 2], s[:, 1], s[:, 0]].astype(np.int32), s

    alive = t0 < t1
    tc = t0.copy()
    g = np.clip(voxel(pos(tc)), 0, N - 1)
    tsdf, _ = read(g)
    n = len(tc)
    kind = np.zeros(n, np.int8)
    end = np.full((n, 3), -1, np.int64)
    zero_neg = np.zeros(n, bool)
    while alive.any():
        alive &= tc < max_time
        g = voxel(pos((tc + step).astype(f)))
        inside = ((g >= 0) & (g < N)).all(-1)
        alive &= inside
        cur, s = read(np.clip(g, 0, N - 1))
        leave = alive & (tsdf < 0) & (cur > 0)
        hit = alive & (tsdf > 0) & (cur < 0)
        zero_neg |= alive & (tsdf == 0) & (cur < 0)
        kind[leave], kind[hit] = 2, 1
        end[leave | hit] = s[leave | hit]
        tsdf = np.where(alive, cur, tsdf)
        alive &= ~(leave | hit)
        tc = np.where(alive, (tc + step).astype(f), tc)
    return kind.reshape(rows, cols), end.reshape(rows, cols, 3), zero_neg.reshape(rows, cols)


def test_case_conditions(oracle_mod):
    """The conditions the committed seeds were chosen for, asserted with the oracle alone (no GPU): every case except 'away' and volume 5 has
    oracle hits on >= 5 % of its pixels; volumes 2 and 3 have >= 100 pixels whose march ends on a sample in the first or last voxel layer of a
    brick; volume 3 has >= 20 pixels in which a negative sample follows a sample that is exactly 0."""
    for vid in VOLUMES:
        face_px = zero_px = 0
        for (name, wrap, size3, R, t, intr, cols, rows) in _cases(vid):
            N = VOLUME_N[vid]
            vol, col, flags = _volume(oracle_mod, vid, wrap, size3)
            v, n, c, S = _oracle_cast(oracle_mod, (vid, name), vol, col, N, wrap, size3, R, t, intr, cols, rows)
            hits = int(np.isfinite(v[:rows]).sum())
            if "away" in name:
                assert S == 0 and hits == 0, (vid, name)
                continue
            assert S > rows * cols / 2, (vid, name, S)
            if vid == 5:
                assert hits == 0
                continue
            assert hits >= 0.05 * rows * cols, f"volume {vid} {name}: {hits} hits of {rows * cols}"
            if vid in (2, 3):
                kind, end, zero_neg = _march(vol, N, wrap, size3, R, t, intr, cols, rows, _trunc(N, size3))
                # the restated march finds the oracle's hits (not the reverse: a crossing in the volume's outermost voxel layers gives no vertex)
                assert (np.isfinite(v[:rows]) & (kind != 1)).sum() <= 0.002 * rows * cols, (vid, name)
                layer = end % B
                face_px += int(((kind > 0) & ((layer == 0) | (layer == B - 1)).any(-1)).sum())
                zero_px += int(zero_neg.sum())
        if vid in (2, 3):
            assert face_px >= 100, (vid, face_px)
        if vid == 3:
            assert zero_px >= 20, zero_px


def test_tight_flags_definition():
    N = 64
    vol = np.zeros((N, N, N), np.int16)
    assert not tight_flags(vol, N).any()
    vol[40, 31, 32] = -1          # storage (z, y, x): brick (1, 0, 1)
    vol[0, 0, 0] = 5
    f = tight_flags(vol, N)
    assert f.sum() == 1 and f[1, 0, 1] == 1


# ---- SKIP ray cast = no-SKIP ray cast = oracle: the GPU side ------------------------------------------------------------------------------------
def _cast_dev(ctx, dvol, dcol, N, wrap, size3, R, t, intr, cols, rows, dflags):
    from kintinuous_amd.abi import Intr
    v0, n0, c0 = _prefill(rows, cols)
    dv, dn, dc = ctx.upload(v0), ctx.upload(n0), ctx.upload(c0)
    counts = ctx.raycast_bricks(Intr(*intr), R, t, _trunc(N, size3), list(size3), dvol, dv, dn, cols, rows, wrap, dc, dcol, N, dflags)
    return ctx.download(dv, np.float32, v0.shape), ctx.download(dn, np.float32, n0.shape), ctx.download(dc, np.uint8, c0.shape), counts


def _bits_differ(a, b):
    """words that differ, bit for bit.  One exception: a NaN that ARITHMETIC made -- the normal of a zero gradient, 0 x rsqrt(0), which only the
    synthetic volumes produce -- carries the sign and payload of the machine that made it (x86: 0xffc00000, gfx950: 0x7fc00000; the maps' own
    'no value' NaN is 0x7fffffff on both), so two NaN words count as equal."""
    return (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))


def _assert_cast(ref, got, msg, skip, want_hops):
    v, n, c, S = ref
    gv, gn, gc, (gS, hopped, hop_iters, batch_iters) = got
    bad = int(_bits_differ(v, gv).sum())
    assert bad == 0, f"{msg}: {bad} vertex-map words differ from the oracle's"
    bad = _bits_differ(n, gn)
    assert not bad.any(), f"{msg}: {int(bad.sum())} normal-map words differ, first {n[bad][:4]} vs {gn[bad][:4]}"
    assert np.array_equal(c, gc), f"{msg}: colour image"
    assert gS == S, f"{msg}: S {gS} vs the oracle's {S}"
    if not skip or want_hops is False:
        assert hopped == 0 and hop_iters == 0, msg
    elif want_hops:
        assert hopped > 0 and hop_iters > 0, f"{msg}: no sample was replaced by a hop -- the path under test did not run"
    assert hopped <= gS
    return hopped / max(gS, 1)


@gpu
@pytest.mark.parametrize("volume_id", sorted(VOLUMES))
def test_skip_raycast_equals_oracle(ctx, oracle_mod, volume_id):
    """Every bit of vmap, nmap and the colour image, and S, from pre-filled buffers: no-SKIP, SKIP with tight_flags (volume 6: all ones), and
    SKIP with the flags the device's own integrate wrote -- volume 1: the device fused it; volumes 2 - 4: one more frame fused on the device
    into the volume, starting from its tight flags (a new volume, with the oracle's ray cast of its own)."""
    N = VOLUME_N[volume_id]
    share = 0.0
    dev = {}   # (wrap, size3) -> device buffers of the case's volume, and of its device-integrated variant
    for (name, wrap, size3, R, t, intr, cols, rows) in _cases(volume_id):
        vol, col, flags = _volume(oracle_mod, volume_id, wrap, size3)
        msg = f"volume {volume_id} ({VOLUMES[volume_id]}) {name}"
        key = (tuple(wrap), tuple(size3))
        if key not in dev:
            d = {"vol": ctx.upload(vol), "col": ctx.upload(col), "flags": ctx.upload(flags)}
            if volume_id == 1:
                gvol, gcol, gfl = _fused(oracle_mod, N, size3, wrap, functools.partial(_dev_integrate4, ctx))
                assert np.array_equal(gvol, vol) and np.array_equal(gcol, col) and _superset(gfl, flags), msg
                d["own"] = (d["vol"], d["col"], ctx.upload(gfl), vol, col)
            elif volume_id in (2, 3, 4):
                cam, frames, traj = _small_frames()
                depth, rgb = frames[0]
                nmap = _nmap_of(oracle_mod, cam, depth)
                args = (cam, depth, rgb, nmap, N, list(size3), np.eye(3, dtype=np.float32), [3.0, 3.0, 3.0], _trunc(N, size3), wrap, vol, col)
                gvol, gcol, gfl, _ = _integrate_dev(ctx, *args, flags.copy())
                rvol, rcol, U = _integrate_ref(oracle_mod, *args)
                assert U > 100 and np.array_equal(gvol, rvol) and np.array_equal(gcol, rcol) and _superset(gfl, tight_flags(gvol, N)), msg
                assert _superset(gfl, flags)
                d["own"] = (ctx.upload(gvol), ctx.upload(gcol), ctx.upload(gfl), gvol, gcol)
            dev[key] = d
        d = dev[key]
        away = "away" in name
        ref = _oracle_cast(oracle_mod, (volume_id, name), vol, col, N, wrap, size3, R, t, intr, cols, rows)
        _assert_cast(ref, _cast_dev(ctx, d["vol"], d["col"], N, wrap, size3, R, t, intr, cols, rows, None), msg + " no-SKIP", False, None)
        got = _cast_dev(ctx, d["vol"], d["col"], N, wrap, size3, R, t, intr, cols, rows, d["flags"])
        share = max(share, _assert_cast(ref, got, msg + " SKIP tight", True, None if away else volume_id != 6))
        if volume_id == 5 and not away:   # every ray hops from face to face and leaves: x planes NaN, y / z and the colours keep their pre-fill
            v0, n0, c0 = _prefill(rows, cols)
            assert np.isnan(got[0][:rows]).all() and np.isnan(got[1][:rows]).all()
            assert np.array_equal(got[0][rows:], v0[rows:]) and np.array_equal(got[1][rows:], n0[rows:]) and np.array_equal(got[2], c0)
        if "own" in d:
            ovol, ocol, ofl, hvol, hcol = d["own"]
            ref2 = ref if volume_id == 1 else _oracle_cast(oracle_mod, None, hvol, hcol, N, wrap, size3, R, t, intr, cols, rows)
            got = _cast_dev(ctx, ovol, ocol, N, wrap, size3, R, t, intr, cols, rows, ofl)
            share = max(share, _assert_cast(ref2, got, msg + " SKIP device-written flags", True, None if away else True))
    print(f"volume {volume_id} ({VOLUMES[volume_id]}): largest hop share {share:.3f}")


def _dev_integrate4(ctx, *args):
    return _integrate_dev(ctx, *args)


def test_volume_1_is_a_rolled_volume(oracle_mod):
    """volume 1 fused straight into a wrap's storage layout is _rotate_storage of the wrap-0 volume (what test_raycast casts)"""
    a, ac, _ = _volume(oracle_mod, 1, WRAPS[0])
    b, bc, _ = _volume(oracle_mod, 1, WRAPS[2])
    assert np.array_equal(_rotate_storage(a, WRAPS[2]), b) and np.array_equal(_rotate_storage(ac, WRAPS[2]), bc)


@gpu
def test_skip_falls_back_at_n80(ctx, oracle_mod):
    """N % 32 != 0 with a non-null flags pointer: the no-SKIP kernel, bit for bit, and no sample is hopped over.  (The other fall-back,
    nb^3 > 32768, is a host branch that needs N > 1024: not covered.)"""
    from kintinuous_amd import abi, synth
    N, size3, wrap = 80, (6.0, 6.0, 6.0), [17, 5, 40]
    vol, col = random_volume_state(np.random.default_rng(80), N, True)
    cam = synth.Camera.small(160, 120)
    dvol, dcol = ctx.upload(vol), ctx.upload(col)
    dfl = ctx.upload(np.zeros(abi.measure_lib().kt_debug_brick_count(N) + 64, np.uint8))   # all "empty": a kernel that read them would hop
    for (pname, R, t, ipp) in _poses(6, size3)[:3]:
        intr = _cam_intr(cam, ipp)
        ref = _oracle_cast(oracle_mod, None, vol, col, N, wrap, size3, R, t, intr, cam.cols, cam.rows)
        a = _cast_dev(ctx, dvol, dcol, N, wrap, size3, R, t, intr, cam.cols, cam.rows, None)
        b = _cast_dev(ctx, dvol, dcol, N, wrap, size3, R, t, intr, cam.cols, cam.rows, dfl)
        _assert_cast(ref, a, f"N=80 {pname} no flags", False, None)
        _assert_cast(ref, b, f"N=80 {pname} flags", True, False)
        assert a[3] == b[3]
