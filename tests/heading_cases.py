"""The case table of tests/test_heading_cases.py (CPU) and tests/test_gpu_headings.py (GPU): cameras that face every way round the volume.

Every other test of the voxel pass looks roughly down the volume's +z axis (rotations of 0.5 rad at the most), and the pre-pass of
csrc/kt_volume.hip -- which decides what voxels the kernel visits at all -- branches on exactly that: the sign and size of b_z = Ri[8] * cell_z
in kt_clip_halfline, the near slab cut with -b_z, the depth-range prune that walks a column from its far end, the reciprocal guard that is
checked at the ends of a z chunk.  The classes:

  axis          the six axis-exact facings (R holds 0 and +-1 only: b_z is +cell, -cell or exactly 0), three sizes, one integer principal point
  roll          90, 180 and 270 degrees about the optical axis, exact
  near_quarter  yaw and pitch of pi / 2 + d for d = +-1e-10, +-1e-4 and 0 (cos(pi / 2) = 6e-17 in double): b_z on both sides of
                kt_clip_halfline's 1e-12 and between them, non-zero
  oblique       a seeded view direction in each of the seven octants other than (+, +, +), with a seeded roll
  on_voxel      the axis rotations with the camera centre exactly ON a voxel centre (the camera-frame depth is exactly 0 on a whole plane of
                voxels, and constant along every column of a sideways camera), and a quarter of a voxel off
  outside       0.45 m outside five faces looking in, and one looking away (nothing may change)

A case is (name, cls, R, t, cam, N, wrap, expect): R the camera-to-volume rotation (float32; the view direction is its third column), t the
camera centre in volume coordinates, and the frame is rendered where the pose says: synth.render(Scene("room"), cam, R, t - SIZE / 2), with a
seeded 2 % of the depths removed.  numpy and kintinuous_amd.synth only; the helpers that need the oracle take it as an argument.
"""
import dataclasses
import functools
import zlib
from collections import namedtuple

import numpy as np

from kintinuous_amd import synth

SIZE = 6.0
CENTRE = np.array([3.1, 2.95, 3.2])     # the default camera centre: (0.1, -0.05, 0.2) off the volume's
HOLES = 0.02
CLASSES = ("axis", "roll", "near_quarter", "oblique", "on_voxel", "outside")
U_FLOOR = 500                            # voxels a case's frame must update (every case but "away")

Case = namedtuple("Case", "name cls R t cam N wrap expect")


def trunc(N):
    return max(0.06, 2.1 * SIZE / N)


def _rx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def _ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def _rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def _exact(R):
    """a rotation by multiples of a quarter turn as what it is: 0 and +-1, not cos(pi / 2) = 6e-17"""
    Q = np.round(R)
    assert np.abs(Q - R).max() < 1e-12 and np.array_equal(Q @ Q.T, np.eye(3)) and np.linalg.det(Q) > 0
    return Q.astype(np.float32) + np.float32(0)     # (+ 0: no negative zeros)


QUARTER_TURN = _exact(_ry(np.pi / 2))               # "a quarter turn on" for the ray cast: the view direction z -> x
AXIS = {"+z": _exact(np.eye(3)), "-z": _exact(_ry(np.pi)), "+x": _exact(_ry(np.pi / 2)), "-x": _exact(_ry(-np.pi / 2)),
        "+y": _exact(_rx(-np.pi / 2)), "-y": _exact(_rx(np.pi / 2))}
AXIS_DIR = {"+z": (0, 0, 1), "-z": (0, 0, -1), "+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0)}
OCTANTS = [(-1, 1, 1), (1, -1, 1), (-1, -1, 1), (1, 1, -1), (-1, 1, -1), (1, -1, -1), (-1, -1, -1)]


@functools.lru_cache(maxsize=None)
def camera(key):
    """'s' 160 x 120, 'r' the ragged 173 x 97, 'i' 160 x 120 with a whole principal point (the centre pixel's ray has two zero components),
    'h' 320 x 240 (plan_cases)"""
    if key in ("r", "h"):
        return synth.Camera.small(173, 97) if key == "r" else synth.Camera.small(320, 240)
    cam = synth.Camera.small(160, 120)
    return dataclasses.replace(cam, cx=float(round(cam.cx)), cy=float(round(cam.cy))) if key == "i" else cam


def wrap_of(N, wrapped):
    return [N - 1, 5, 40 % N] if wrapped else [0, 0, 0]


def clip_branch(Ri8, N):
    """the branch of kt_clip_halfline that the near plane's beta = Ri[8] * cell_z takes, from the float32 product: 'lo', 'hi' or 'mid'"""
    bz = np.float32(Ri8) * (np.float32(SIZE) / np.float32(N))
    return "lo" if bz > np.float32(1e-12) else "hi" if bz < np.float32(-1e-12) else "mid"


def _look(direction, roll):
    """a rotation whose third column is `direction`, rolled about it"""
    z = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], axis=1) @ _rz(roll)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, cls, R, t=CENTRE, cam="s", N=64, wrapped=False, **expect):
        R = np.ascontiguousarray(R, np.float32)
        out.append(Case(name, cls, R, np.asarray(t, np.float32), cam, N, wrap_of(N, wrapped), dict(expect)))

    # axis: six facings at 160 x 120 / N = 64, and the other sizes
    for k in AXIS:
        add(f"axis{k}", "axis", AXIS[k], facing=k, branch={"+z": "lo", "-z": "hi"}.get(k, "mid"))
    add("axis+x/N96/wrap", "axis", AXIS["+x"], N=96, wrapped=True, facing="+x", branch="mid")
    add("axis-z/173x97/N80/wrap", "axis", AXIS["-z"], cam="r", N=80, wrapped=True, facing="-z", branch="hi")
    add("axis-y/ipp", "axis", AXIS["-y"], cam="i", facing="-y", branch="mid")
    # roll about the optical axis
    add("roll90", "roll", _exact(_rz(np.pi / 2)), branch="lo")
    add("roll180/N96/wrap", "roll", _exact(_rz(np.pi)), N=96, wrapped=True, branch="lo")
    add("roll270/173x97/N80", "roll", _exact(_rz(-np.pi / 2)), cam="r", N=80, branch="lo")
    # near a quarter turn: cos(pi / 2 + d) = -d
    for d, kw in ((1e-10, {}), (-1e-10, {}), (1e-4, dict(N=96, wrapped=True)), (-1e-4, dict(N=96)), (0.0, {})):
        add(f"yaw90{d:+.0e}", "near_quarter", _ry(np.pi / 2 + d), branch="hi" if d > 0 else "lo" if d < 0 else "mid", nonzero=True, **kw)
    for d, kw in ((1e-10, dict(wrapped=True)), (-1e-10, {}), (1e-4, dict(cam="r", N=80)), (-1e-4, dict(cam="r", N=80, wrapped=True)), (0.0, dict(N=96))):
        add(f"pitch90{d:+.0e}", "near_quarter", _rx(-(np.pi / 2 + d)), branch="hi" if d > 0 else "lo" if d < 0 else "mid", nonzero=True, **kw)
    # oblique: one view direction per octant
    rng = np.random.default_rng(2024)
    sizes = [{}, {}, dict(N=96, wrapped=True), {}, dict(cam="r", N=80), dict(N=96, wrapped=True), {}]
    for octant, kw in zip(OCTANTS, sizes):
        direction = np.asarray(octant) * rng.uniform(0.35, 1.0, 3)
        add("oblique" + "".join("+" if s > 0 else "-" for s in octant), "oblique", _look(direction, rng.uniform(-np.pi, np.pi)), octant=octant,
            t=CENTRE + rng.uniform(-0.2, 0.2, 3), **kw)
    # the camera centre on a voxel centre: (k + 0.5) cell is exact in float32 at N = 64 (cell = 3 / 32)
    cell = SIZE / 64
    on = (np.array([33, 31, 34]) + 0.5) * cell
    assert np.array_equal(on.astype(np.float32).astype(np.float64), on)
    for i, k in enumerate(AXIS):
        add(f"on_voxel{k}", "on_voxel", AXIS[k], t=on, wrapped=i in (2, 5), facing=k, branch={"+z": "lo", "-z": "hi"}.get(k, "mid"), on_voxel=True)
    for k in ("+x", "-y", "-z"):
        add(f"quarter_off{k}", "on_voxel", AXIS[k], t=on + cell / 4, facing=k, branch={"+z": "lo", "-z": "hi"}.get(k, "mid"), on_voxel=False)
    # outside a face, looking in (and away)
    a, b, o = 3.1, 2.9, 0.45
    add("outside_x0", "outside", AXIS["+x"], t=(-o, a, b), facing="+x", branch="mid", outside=True)
    add("outside_xN/wrap", "outside", AXIS["-x"], t=(SIZE + o, a, b), wrapped=True, facing="-x", branch="mid", outside=True)
    add("outside_y0/N96", "outside", AXIS["+y"], t=(a, -o, b), N=96, facing="+y", branch="mid", outside=True)
    add("outside_yN", "outside", AXIS["-y"], t=(a, SIZE + o, b), facing="-y", branch="mid", outside=True)
    add("outside_zN", "outside", AXIS["-z"], t=(a, b, SIZE + o), facing="-z", branch="hi", outside=True)
    add("away", "outside", AXIS["-x"], t=(-o, a, b), facing="-x", branch="mid", outside=True, away=True)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def plan_cases():
    """Two more cases for the planned pre-pass alone (test_plan_ranges_cover_every_update), where its rotation margin is more than the
    pre-pass's fixed slack.  That slack is 2 pixels on every image side and 2 to 3 voxels at either end of a column's z interval; a turn
    of 20 mrad moves a voxel d metres away by 0.02 d, which at 160 x 120 (f = 132: 2.6 pixels) and N <= 96 (voxels of 6 cm and more) is
    inside it at every depth the room has.  At 320 x 240 and N = 256 from 0.45 m outside a face, looking through the room at a wall 5 m
    away, it is 4 voxels and 5 pixels: without the margin voxels are dropped."""
    out = []
    for name, k, t, wrapped in (("plan_outside_x0/320x240/N256", "+x", (-0.45, 3.1, 2.9), False), ("plan_outside_zN/320x240/N256/wrap", "-z", (3.1, 2.9, SIZE + 0.45), True)):
        out.append(Case(name, "plan", AXIS[k], np.asarray(t, np.float32), "h", 256, wrap_of(256, wrapped), dict(facing=k, outside=True)))
    return tuple(out)


def names():
    return [c.name for c in cases()]


def by_name(name):
    return next(c for c in cases() + plan_cases() if c.name == name)


def neighbour(case):
    """the next case of the same class (cyclic): its pose gives the second frame of the integrate tests"""
    same = [c for c in cases() if c.cls == case.cls]
    return same[(same.index(case) + 1) % len(same)]


def inside(case):
    return bool(((case.t > 0) & (case.t < SIZE)).all())


@functools.lru_cache(maxsize=None)
def _frame(name, which):
    case = by_name(name)
    pose = case if which == 0 else neighbour(case)
    cam = camera(case.cam)
    depth, rgb = synth.render(synth.Scene("room"), cam, pose.R.astype(np.float64), pose.t.astype(np.float64) - SIZE / 2)
    depth = depth.copy()
    depth[np.random.default_rng(zlib.crc32(f"{name}/{which}".encode())).random(depth.shape) < HOLES] = 0
    for arr in (depth, rgb):
        arr.setflags(write=False)
    return pose.R, pose.t, depth, np.ascontiguousarray(rgb)


def frame(case, which):
    """(R, t, depth, rgb) of the case's own frame (which = 0) or of the frame from its neighbour's pose through the case's camera (1)"""
    return _frame(case.name, which)


# ---- what the oracle makes of a case; computed once per process and left unchanged ---------------------------------------------------------------
def intr(O, case):
    cam = camera(case.cam)
    return O.OIntr(cam.fx, cam.fy, cam.cx, cam.cy)


_INPUTS, _FUSED, _CASTS = {}, {}, {}


def inputs(O, case, which):
    """(depth, rgb, nmap, Rinv, t) of a frame: what one integrate call takes"""
    key = (case.name, which)
    if key not in _INPUTS:
        R, t, depth, rgb = frame(case, which)
        nmap = O.create_nmap(O.create_vmap(intr(O, case), O.bilateral_filter(depth)))
        nmap.setflags(write=False)
        _INPUTS[key] = (depth, rgb, nmap, O.mat33_inverse(R), t)
    return _INPUTS[key]


def fused(O, case, start=None, tag="empty"):
    """the oracle's two integrates of a case, from an empty volume or from `start` = (volume, colour volume) under the cache key `tag`:
    [(volume, colour volume, scaled depth, U) after frame 0, the same after frame 1]"""
    key = (case.name, tag)
    if key not in _FUSED:
        N = case.N
        vol, col = (np.zeros((N, N, N), np.int16), np.zeros((N, N, N, 4), np.uint8)) if start is None else (start[0].copy(), start[1].copy())
        steps = []
        for which in (0, 1):
            depth, rgb, nmap, Rinv, t = inputs(O, case, which)
            U, scaled = O.integrate_tsdf(depth, intr(O, case), [SIZE] * 3, Rinv, t, trunc(N), vol, case.wrap, col, rgb, nmap, True)
            steps.append((vol.copy(), col.copy(), scaled, U))
            for arr in steps[-1][:3]:
                arr.setflags(write=False)
        _FUSED[key] = steps
    return _FUSED[key]


def prefill(rows, cols):
    rng = np.random.default_rng(3)
    return (rng.uniform(-1, 1, (3 * rows, cols)).astype(np.float32), rng.uniform(-1, 1, (3 * rows, cols)).astype(np.float32),
            rng.integers(0, 255, (rows, cols, 4)).astype(np.uint8))


def cast_pose(case, turned):
    """the case's pose, or the pose a quarter turn on (about the camera's own y axis)"""
    return (np.ascontiguousarray(case.R @ QUARTER_TURN) if turned else case.R), case.t


def cast(M, O, case, turned, vol, col, key=None):
    """(vmap, nmap, colour image, S) of module M's (the oracle's, or the reference build's: S is None) ray cast of (vol, col) from cast_pose, over
    pre-filled buffers"""
    if key is not None and (case.name, turned, key) in _CASTS:
        return _CASTS[(case.name, turned, key)]
    cam = camera(case.cam)
    v, n, c = (a.copy() for a in prefill(cam.rows, cam.cols))
    R, t = cast_pose(case, turned)
    S = M.raycast(intr(O, case), R, t, trunc(case.N), [SIZE] * 3, np.ascontiguousarray(vol), v, n, case.wrap, c, np.ascontiguousarray(col))
    if key is not None:
        for arr in (v, n, c):
            arr.setflags(write=False)
        _CASTS[(case.name, turned, key)] = (v, n, c, S)
    return v, n, c, S


# ---- the turn on the spot of test_turn_ground_truth ------------------------------------------------------------------------------------------------
def turn_poses():
    """26 camera-to-scene poses (R, c) in the room: once round the compass in yaw steps of 30 degrees while drifting 2 cm in x and 1 cm in z a
    frame, then at the last centre down to the floor, back and up to the ceiling in pitch, back to level, then a roll to 180 degrees"""
    out = []
    for k in range(13):
        out.append((_ry(np.radians(30.0 * k)), np.array([0.02 * k, 0.0, 0.01 * k])))
    c = out[-1][1]
    for p in (30, 60, 90, 60, 30, 0, -30, -60, -90):
        out.append((_rx(-np.radians(float(p))), c))
    for r in (45, 90, 135, 180):
        out.append((_rz(np.radians(float(r))), c))
    return out
