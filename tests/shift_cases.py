"""The cases of tests/test_shift_cases.py (CPU) and tests/test_gpu_shifts.py (GPU): volume shifts on every axis, both ways, and three in one frame.

The shift path -- the per-axis blocks of finish_pose (csrc/kt_tracker.hip), kt_slice_store::fetch with its double buffer
(csrc/kt_tracker_slices.hip), the slab clears and the slab extraction (csrc/kt_volume_shift.hip), the slab mesh and its keys (csrc/kt_mesh.hip) --
was held to the oracle only by sequences whose slabs are empty or nearly so (the crab-walks of test_gpu_tracker.py, test_gpu_mesh.py and
test_gpu_mesh_weld.py, heading_cases.turn_poses): no Y shift at all, no point in an X- slab, no frame that shifts three axes.

  the tour    a ground-truth trajectory (load_trajectory: the shift pattern is designed, not tracked) through the room at 160 x 120, N = 64,
              a 2 m volume (a voxel is 1 / 32 m), voxel_shift 3, overlap 2.  The volume starts with three of its faces 3.2 voxels outside three
              walls of the room, so the walls lie in the slabs that leave first; the camera looks into the corner and at each wall, steps
              away from the corner on all three axes in one frame, makes two-axis and one-axis moves (one jump of 12 voxels), and
              travels in jumps of at most 9 voxels to three more corners of mixed sign (the cube and the sphere stay 0.2 m away), repeating the steps there.  A shift moves 3
              voxels an axis a frame (voxel_trans clamps at the threshold), so a jump is followed by frames that catch up.
  the legs    two ICP runs of 22 frames (6 m volume, identity rotation, the camera half a voxel a frame along (1, 0.8, 1) with signs):
              the shift is decided on the device (csrc/kt_setup.hpp parks the frame, the host must agree).

slab_boxes and restate_frame say again what a shifting frame extracts, from the volume BEFORE the frame, with the oracle's kernels and the
numpy mesh: the definition the tracker's slab clouds, meshes and keys are held to.  numpy, kintinuous_amd.synth and the restatements only;
the helpers that need the oracle take it as an argument.
"""
import functools
from collections import namedtuple

import numpy as np

import heading_cases as H
from kintinuous_amd import mesh_ref, mesh_weld_ref, synth

N = 64
SIZE = 2.0
VOXEL = SIZE / N
SHIFT = 3
OVERLAP = 2
MARGIN = 3.2        # voxels between a face of the volume and the wall inside it, at the first corner
FRACTION = 0.37     # the camera sits this fraction of a voxel off the lattice: no floor() of the shift decision on a knife edge
MAX_JUMP = 12       # voxels an axis a frame, at the most

ICP_SIZE = 6.0
ICP_FRAMES = 22
ICP_SIGNS = {"+++": (1, 1, 1), "+-+": (1, -1, 1)}     # (-, +, -) and (-, -, -) drift 0.18 m and 0.12 m on the oracle: not used

# a restated slab: cells = the cell of each triangle in world voxels; wrap = the real wrap it was extracted under, vt = its shift
Slab = namedtuple("Slab", "cloud vertices triangles keys cells dim wrap vt")


def camera():
    return H.camera("s")


def config(cls, size=SIZE):
    """a tracker configuration (abi.TrackerConfig or oracle.OTrackerConfig) of the tour, or of the legs at size = ICP_SIZE"""
    cam = camera()
    return cls(cam.cols, cam.rows, N, cam.fx, cam.fy, cam.cx, cam.cy, size, SHIFT, OVERLAP, 0, 0, 0, 0, 0, 0, 0, 0)


def storage_wrap(wrap, n=N):
    """vWrapCopyUpdate: the wrap the kernels index storage with"""
    return [int(w) if w >= 0 else n - (-int(w)) % n for w in wrap]


# ---- the shift rule ---------------------------------------------------------------------------------------------------------------------
def slab_boxes(dim, vt, n=N, overlap=OVERLAP):
    """(lo, hi, mlo, mhi) of the slab that leaves along dimension dim (CloudSlice: 2 axis + (0 plus | 1 minus)) on a shift of vt voxels: the
    cloud's voxels [lo, hi) and the mesh's cells [mlo, mhi) as finish_pose forms them, the z-minus box one plane low included"""
    axis, minus = dim // 2, dim % 2
    assert (vt < 0) == bool(minus) and vt != 0
    lo, hi, mlo, mhi = [0, 0, 0], [n, n, n], [0, 0, 0], [n - 1, n - 1, n - 1]
    if not minus:
        hi[axis] = vt + 1 + overlap
        mhi[axis] = vt
    else:
        if axis == 2:
            lo[2], hi[2] = n + (vt - overlap) - 1, n - 1
        else:
            lo[axis] = n + (vt - overlap)
        mlo[axis] = n + vt - 1
    return lo, hi, mlo, mhi


def restate_frame(oracle, vol, col, wrap_before, wrap_after, dims, size=SIZE, n=N, overlap=OVERLAP):
    """The slabs (Slab records: cloud, mesh vertices, triangles, keys, ...) of one shifting frame, in order, from the volume before the frame:
    each axis is extracted under the wrap the axes before it left, then cleared (tsdf words and colour words), then the wrap advances -- so
    the second and third slab of a frame see what the tracker's see.  vol and col are changed."""
    wrap = [int(w) for w in wrap_before]
    out = []
    for dim in dims:
        axis = dim // 2
        vt = int(wrap_after[axis]) - wrap[axis]
        lo, hi, mlo, mhi = slab_boxes(dim, vt, n, overlap)
        sw = storage_wrap(wrap, n)
        cloud = oracle.extract_cloud_slice(vol, [size] * 3, 3 * n ** 3 // 4, sw, col, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], 1, wrap)
        v, t, info = mesh_ref.extract_mesh(vol, col, (size,) * 3, sw, mlo, mhi, wrap, n, info=True)
        keys = mesh_weld_ref.edge_keys(info["owner"], info["axis"], wrap)
        out.append(Slab(cloud, v, t, keys, info["cells"] + np.asarray(wrap)[None, :], dim, tuple(wrap), vt))
        oracle.clear_volume(vol, axis, bool(dim % 2), wrap[axis], wrap[axis] + vt)
        oracle.clear_volume(col, axis, bool(dim % 2), wrap[axis], wrap[axis] + vt)
        wrap[axis] += vt
    assert wrap == [int(w) for w in wrap_after], (wrap, wrap_after)
    return out


# ---- the tour ---------------------------------------------------------------------------------------------------------------------------
def _start():
    """the first camera centre: the volume (centred on it) has its low x, low y and high z faces MARGIN voxels outside the room"""
    lo, hi = synth.Scene("room").planes_box()
    m = MARGIN * VOXEL
    return np.array([lo[0] + SIZE / 2 - m, lo[1] + SIZE / 2 - m, hi[2] - SIZE / 2 + m])


# A wall is inside the volume, MARGIN (2.4 to 3.4) voxels from a face, at these wraps (a wrap moves in threes): x = 0 the low-x wall, x = 45
# the high-x wall, y = 0 the ceiling, y = 9 the floor, z = 0 the high-z wall, z = -102 the low-z wall.  One shift away from it the wall has
# left with the slab; a step back brings its place in again, cleared, and the looks fuse it anew.
CORNERS = {"A": (0, 0, 0), "B": (0, 0, -102), "C": (45, 0, -102), "D": (45, 9, -102)}
AWAY = {"A": (1, 1, -1), "B": (1, 1, 1), "C": (-1, 1, 1), "D": (-1, -1, 1)}      # the way out of each corner


def _simulate(wrap, p):
    """the shift decision on camera position p (voxels from the start) under `wrap`: floor, clamped at the threshold, taken at it"""
    out = list(wrap)
    for k in range(3):
        f = int(np.floor(p[k] - wrap[k]))
        vt = max(-SHIFT, f) if f < 0 else min(SHIFT, f)
        if abs(vt) >= SHIFT:
            out[k] += vt
    return out


def _towards(*direction):
    return H._look(direction, 0.0)


class _Route:
    def __init__(self):
        self.p = np.zeros(3)
        self.wrap = [0, 0, 0]
        self.out = [(np.eye(3), self.p.copy())]
        self.k = 0

    def frame(self, R, step=(0, 0, 0)):
        step = np.asarray(step, np.float64)
        assert np.abs(step).max() <= MAX_JUMP
        self.p = self.p + step
        self.wrap = _simulate(self.wrap, self.p)
        self.out.append((np.asarray(R, np.float64), self.p.copy()))

    def look(self, looks):
        for R in looks:
            self.frame(R)

    def goto(self, target, looks, jump=9):
        """to the wrap `target` in jumps of at most `jump` voxels an axis, with the frames that catch up; `looks` in turn"""
        while True:
            want = np.asarray(target, np.float64) + FRACTION - self.p
            if not np.abs(want).max() > 1e-9 and _simulate(self.wrap, self.p) == self.wrap:
                break
            self.frame(looks[self.k % len(looks)], np.clip(want, -jump, jump))
            self.k += 1
        assert self.wrap == list(target), (self.wrap, target)


def _corner_looks(away):
    """into the corner, then at each of its three walls: the view directions opposite to the way out"""
    s = -np.asarray(away)
    names = [("-" if s[k] < 0 else "+") + "xyz"[k] for k in range(3)]
    return [_towards(*(s * np.array([1.0, 0.8, 1.2])))] + [H.AXIS[n].astype(np.float64) for n in names]


@functools.lru_cache(maxsize=None)
def tour_poses():
    """the camera-to-scene poses (R, c) of the tour: pose 0 is the identity at the start (the scene's frame is the volume's, moved)"""
    r = _Route()
    r.frame(np.eye(3), (FRACTION,) * 3)
    # corner A: low x, ceiling, high z (the cube lies below the camera, the sphere a metre to its side)
    r.look(_corner_looks(AWAY["A"]))
    r.goto((3, 3, -3), [_towards(-1, -0.8, 1.2)])                    # three axes in one frame, a wall in each slab
    # along -z with the low-x wall and the ceiling inside: every Z- slab holds a strip of both
    edge = [_towards(-1, -0.8, -0.3), _towards(-1, -0.3, -0.6), _towards(-0.7, -1, 0.2), _towards(-1, -0.5, 0.5)]
    r.goto((0, 0, -6), edge)
    r.look(edge)
    r.goto((0, 0, -12), edge, jump=3)
    r.goto((0, 3, -15), edge)                                        # y and z: the ceiling leaves
    r.goto((0, 0, -18), edge)                                        # ... and its place comes back (Y-)
    r.look(edge[:3])
    r.goto((3, 0, -21), edge)                                        # x and z
    r.goto((0, 0, -24), edge)
    r.look(edge[:3])
    r.goto((3, 3, -27), edge)                                        # three axes again, mid-way: the X clear cuts into the Y and Z slabs
    r.goto((0, 0, -30), edge)
    r.look(edge[:2])
    r.goto(CORNERS["B"], edge)                                       # the jumps of 9, two frames to catch up after each
    # corner B: low x, ceiling, low z
    r.look(_corner_looks(AWAY["B"]))
    r.goto((3, 3, -99), [_towards(-1, -0.8, -1.2)])
    # along +x with the ceiling and the low-z wall inside
    edge = [_towards(0.3, -0.8, -1), _towards(0.6, -0.3, -1), _towards(-0.2, -1, -0.7), _towards(-0.5, -0.5, -1)]
    r.goto((6, 0, -102), edge)
    r.look(edge)
    r.goto((12, 0, -102), edge, jump=3)
    r.goto((15, 3, -102), edge)                                      # x and y
    r.goto((18, 0, -102), edge)
    r.look(edge[:3])
    r.goto((21, 0, -99), edge)                                       # x and z, Z+
    r.goto((24, 0, -102), edge)
    r.look(edge[:3])
    r.goto((27, 3, -99), edge)                                       # three axes, another sign pattern
    r.goto((30, 0, -102), edge)
    r.look(edge[:2])
    r.goto((42, 0, -102), edge, jump=12)                             # the jump of 12 voxels: four frames of X+
    r.goto(CORNERS["C"], edge)
    # corner C: high x, ceiling, low z
    r.look(_corner_looks(AWAY["C"]))
    r.goto((42, 3, -99), [_towards(1, -0.8, -1.2)])
    # corner D: high x, floor, low z
    r.goto(CORNERS["D"], [_towards(1, 0.8, -1.2)])
    r.look(_corner_looks(AWAY["D"]))
    r.goto((42, 6, -99), [_towards(1, 0.8, -1.2)])
    r.goto(CORNERS["D"], [_towards(1, 0.8, -1.2)])                   # back, so that the walls are in the volume for the last slice
    r.look(_corner_looks(AWAY["D"])[1:])
    start = _start()
    return tuple((R, start + p * VOXEL) for R, p in r.out)


@functools.lru_cache(maxsize=None)
def tour_frames():
    cam, scene = camera(), synth.Scene("room")
    out = []
    for R, c in tour_poses():
        d, rgb = (np.ascontiguousarray(a) for a in synth.render(scene, cam, R, c))
        for a in (d, rgb):
            a.setflags(write=False)
        out.append((d, rgb))
    return tuple(out)


def tour_trajectory():
    """(stamps uint64 [n], rows float32 [n, 7]) for load_trajectory"""
    poses = tour_poses()
    return np.array([33333 * (k + 1) for k in range(len(poses))], np.uint64), synth.ground_truth_rows(poses)


def jumps():
    """the largest step of the camera on any axis, per frame, in voxels"""
    c = np.array([c for _, c in tour_poses()])
    return np.abs(np.diff(c, axis=0)).max(axis=1) / VOXEL


def same_points(p, q):
    """two clouds hold the same records (the extraction's order is free)"""
    if len(p) != len(q):
        return False
    a = np.sort(np.ascontiguousarray(p).view(np.dtype((np.void, p.dtype.itemsize))).ravel())
    b = np.sort(np.ascontiguousarray(q).view(np.dtype((np.void, q.dtype.itemsize))).ravel())
    return bool(np.array_equal(a, b))


_TOUR = {}


def tour_oracle(oracle):
    """The oracle's tracker on the tour, once per process and left unchanged: {"pose": [(R, t, global camera)], "wrap": [wrap after each
    frame], "frames": [(frame, wrap before, wrap after, dims, first slice)] of the shifting frames, "slices": [(cloud, dim)] with the
    finalise slice last, "restated": restate_frame's items, one per slab, "maps": the predicted maps of the last frame, "final": (volume,
    colour volume, wrap) at the end}."""
    if "run" in _TOUR:
        return _TOUR["run"]
    stamps, rows = tour_trajectory()
    otr = oracle.OracleTracker(config(oracle.OTrackerConfig))
    run = dict(pose=[], wrap=[], frames=[], slices=[], restated=[])
    try:
        otr.load_trajectory(stamps, rows)
        wrap = [0, 0, 0]
        for k, (d, rgb) in enumerate(tour_frames()):
            vol, col = otr.volume().copy(), otr.color_volume().copy()
            first = otr.num_slices()
            otr.process_frame(d, rgb, int(stamps[k]))
            after = [int(w) for w in otr.voxel_wrap()]
            run["pose"].append(otr.pose())
            run["wrap"].append(after)
            if otr.num_slices() > first:
                new = [otr.slice(i) for i in range(first, otr.num_slices())]
                dims = [dim for _, dim in new]
                run["frames"].append((k, wrap, after, dims, first))
                run["slices"] += new
                run["restated"] += restate_frame(oracle, vol, col, wrap, after, dims)
            wrap = after
        run["maps"] = [(otr.vmap_g_prev(l).copy(), otr.nmap_g_prev(l).copy()) for l in range(4)]
        run["final"] = (otr.volume().copy(), otr.color_volume().copy(), wrap)
        otr.finalise()
        run["slices"].append(otr.slice(otr.num_slices() - 1))
    finally:
        otr.close()
    _TOUR["run"] = run
    return run


def concat(meshes, keys):
    """the slab meshes as one list for the weld: (vertices, keys, triangles, span_first, span_time); a slab's time is its index"""
    first = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])]).astype(np.int64)
    v = np.concatenate([v for v, _ in meshes])
    tri = np.concatenate([t.astype(np.uint32) + np.uint32(first[i]) for i, (_, t) in enumerate(meshes)]).astype(np.uint32).reshape(-1, 3)
    return v, np.concatenate(keys).astype(np.uint64), tri, first, np.arange(len(meshes), dtype=np.uint64)


def _cell_keys(cells):
    c = np.asarray(cells, np.int64).reshape(-1, 3) + (1 << 19)
    return np.unique((c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0])


def seam_counts(slabs, keys, first):
    """(merged vertices, [those on a seam cut along x, y, z]) of the weld over the restated slabs.  A slab that left along axis a was cut
    from the volume at one voxel plane (plus: wrap + vt, minus: wrap + n + vt - 1, global voxels); what is meshed next lies on the other side
    of it, so a vertex merged into a vertex of that slab across the cut sits on an edge IN that plane: its owner voxel has that
    coordinate on a, and its edge runs along another axis.  The tour comes back to places it has left, and a cell fused anew and meshed
    again repeats its keys: only pairs of slabs that share no cell are counted."""
    rep = mesh_weld_ref.representatives(keys, first, np.arange(len(first) - 1, dtype=np.uint64))
    merged = np.nonzero(rep != np.arange(len(keys)))[0]
    g, edge = mesh_weld_ref.key_fields(keys)
    span, into = mesh_weld_ref.span_of(first, merged), mesh_weld_ref.span_of(first, rep[merged])
    ck = [_cell_keys(s.cells) for s in slabs]
    disjoint = {}
    count = [0, 0, 0]
    for i, s1, s0 in zip(merged, span, into):
        pair = (int(s0), int(s1))
        if pair not in disjoint:
            disjoint[pair] = len(np.intersect1d(ck[pair[0]], ck[pair[1]])) == 0
        slab = slabs[pair[0]]
        a = slab.dim // 2
        plane = slab.wrap[a] + slab.vt + (N - 1 if slab.dim % 2 else 0)
        if disjoint[pair] and g[i, a] == plane and edge[i] != a:
            count[a] += 1
    return len(merged), count


def fresh_cells(slabs, final_cells=None):
    """The rule 'no cell is meshed twice' on a tour that returns to places it has left: a slab's cells have lost a plane of their voxels to
    the clear, so none of them may be meshed again until that plane has come back into the volume (cleared, to be fused anew).  Walks the
    slabs in order: the cells meshed since their planes last entered; a shift of vt on axis a under wrap w brings in the planes [w + n,
    w + n + vt) (plus) or [w + vt, w) (minus), and the cells with a corner in one of them start again.  Returns [(slab index, number of
    its cells that were meshed before and have not left)] of the offenders; final_cells (world voxels) are checked last, as slab -1."""
    done = np.zeros((0, 3), np.int64)
    bad = []
    for i, s in enumerate(slabs):
        cells = np.unique(np.asarray(s.cells, np.int64).reshape(-1, 3), axis=0)
        again = len(np.intersect1d(_cell_keys(done), _cell_keys(cells))) if len(done) and len(cells) else 0
        if again:
            bad.append((i, again))
        done = np.concatenate([done, cells])
        a, w = s.dim // 2, s.wrap[s.dim // 2]
        planes = np.arange(w + N, w + N + s.vt) if s.vt > 0 else np.arange(w + s.vt, w)
        done = done[~(np.isin(done[:, a], planes) | np.isin(done[:, a] + 1, planes))]
    if final_cells is not None and len(final_cells) and len(done):
        again = len(np.intersect1d(_cell_keys(done), _cell_keys(final_cells)))
        if again:
            bad.append((-1, again))
    return bad


# ---- the ICP legs -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def leg_frames(name):
    """(frames, camera centres in the scene) of a leg: the camera half a voxel a frame along sign * (1, 0.8, 1), facing +z"""
    s = np.asarray(ICP_SIGNS[name], np.float64)
    cam, scene = camera(), synth.Scene("room")
    centres = [s * 0.5 * (ICP_SIZE / N) * k * np.array([1.0, 0.8, 1.0]) for k in range(ICP_FRAMES)]
    frames = tuple(tuple(np.ascontiguousarray(a) for a in synth.render(scene, cam, np.eye(3), c)) for c in centres)
    return frames, np.array(centres)


_LEGS = {}


def leg_oracle(oracle, name):
    """the oracle's tracker on a leg, once: {"wrap": per frame, "slabs": new slices per frame, "dims", "error": the largest distance of its
    global camera from the truth, metres}"""
    if name not in _LEGS:
        frames, centres = leg_frames(name)
        otr = oracle.OracleTracker(config(oracle.OTrackerConfig, ICP_SIZE))
        out = dict(wrap=[], slabs=[], dims=[], error=0.0)
        try:
            for k, (d, rgb) in enumerate(frames):
                first = otr.num_slices()
                otr.process_frame(d, rgb, 33333 * k)
                out["wrap"].append([int(w) for w in otr.voxel_wrap()])
                out["slabs"].append(otr.num_slices() - first)
                out["dims"] += [otr.slice(i)[1] for i in range(first, otr.num_slices())]
                out["error"] = max(out["error"], float(np.linalg.norm(otr.pose()[2].astype(np.float64) - centres[k])))
        finally:
            otr.close()
        _LEGS[name] = out
    return _LEGS[name]
