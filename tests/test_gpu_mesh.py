"""GPU: the mesh stage (kt_mesh.hip) -- kt_extract_mesh bit for bit against the numpy restatement (kintinuous_amd/mesh_ref.py) on
random volume states and fused volumes, its vertices against kt_extract_cloud_slice's points, an analytic sphere, the capacity
contract, determinism, the tracker's mesh stage on a shifting sequence and the driver's -m."""
import os
import subprocess

import numpy as np
import pytest

from conftest import random_volume_state
from kintinuous_amd import abi, mesh_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kintinuous_amd", "host", "bin", "kintinuous_hip")


def _vb(v):
    return np.ascontiguousarray(v).view(np.uint8)


def _same(a, b):
    (va, ta), (vb, tb) = a, b
    assert len(va) == len(vb) and len(ta) == len(tb), (len(va), len(vb), len(ta), len(tb))
    assert np.array_equal(_vb(va), _vb(vb))
    assert np.array_equal(ta, tb)


def _closed(tris):
    """every undirected edge in exactly two triangles, once in each direction"""
    t = tris.astype(np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    u, cnt = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    dd = np.unique(d, axis=0)
    return bool((cnt == 2).all() and len(dd) == len(d)), len(u)


def _boxes(N):
    M = N - 1
    out = [((0, 0, 0), (M, M, M)), ((3, 3, 3), (4, 4, 4)), ((5, 5, 5), (5, 9, 9)), ((0, 7, 2), (M, M, M - 1))]
    for ax in range(3):
        lo, hi = [0, 0, 0], [M, M, M]
        hi[ax] = 4
        out.append((tuple(lo), tuple(hi)))
        lo, hi = [0, 0, 0], [M, M, M]
        lo[ax] = M - 3
        out.append((tuple(lo), tuple(hi)))
    return out


@pytest.mark.parametrize("N,wrap", [(64, (0, 0, 0)), (96, (5, 90, 33)), (128, (127, 0, 64))])
def test_random_state_byte_equal(ctx, N, wrap):
    rng = np.random.default_rng(N)
    vol, col = random_volume_state(rng, N, True)
    dv, dc = ctx.upload(vol), ctx.upload(col)
    vs = (4.5, 5.0, 6.0)
    real = (wrap[0] + 2 * N, -wrap[1], wrap[2] - 7)
    for lo, hi in _boxes(N):
        got = ctx.mesh(dv, vs, wrap, dc, lo, hi, real, N)
        want = mesh_ref.extract_mesh(vol, col, vs, wrap, lo, hi, real, N)
        _same(got, want)
        if all(h > l for l, h in zip(lo, hi)) and (hi[0] - lo[0]) > 8:
            assert len(want[1]) > 0


def test_fused_volume_byte_equal_and_matches_the_extraction(ctx, small_scene):
    """A tracker's fused volume: the mesh equals the restatement, and every vertex of a strictly sign-changing edge is one of
    kt_extract_cloud_slice's points over the same voxels (x, y, z and the rgb word)."""
    cam, frames, _ = small_scene
    N = 64
    cfg = abi.TrackerConfig(cam.cols, cam.rows, N, cam.fx, cam.fy, cam.cx, cam.cy, 6.0, 14, 2, 0, 0, 0, 0, 0, 0)
    trk = abi.Tracker(ctx, cfg)
    for k, (d, rgb) in enumerate(frames[:4]):
        trk.process_frame_host(d, rgb, 33333 * k)
    vol, col = trk.volume(), trk.color_volume()
    trk.close()
    dv, dc = ctx.upload(vol), ctx.upload(col)
    vs = (6.0, 6.0, 6.0)
    for wrap, lo, hi in (((0, 0, 0), (0, 0, 0), (63, 63, 63)), ((9, 0, 40), (2, 5, 0), (60, 63, 50))):
        real = (wrap[0] + 64, wrap[1], wrap[2])
        v, t = ctx.mesh(dv, vs, wrap, dc, lo, hi, real, N)
        rv, rt, info = mesh_ref.extract_mesh(vol, col, vs, wrap, lo, hi, real, N, info=True)
        _same((v, t), (rv, rt))
        assert len(t) > 1000
        # the extraction over voxels [lo, hi] (maxZ = hi + 1 <= N - 1 < N: no z-edge through the modulo)
        cap = 3 * N ** 3 // 4
        out = ctx.empty(cap * 32)
        n = ctx.extract_cloud_slice(dv, vs, out, cap, wrap, dc, lo[0], hi[0] + 1, lo[1], hi[1] + 1, lo[2], hi[2] + 1, 1, real, N)
        pts = ctx.download(out, abi.POINT_DTYPE, (n,))
        key = lambda xyz, rgb: set(zip(*(np.ascontiguousarray(xyz).view(np.uint32).T.tolist()), rgb.tolist()))
        P = key(pts["xyz"], pts["bgra"].copy().view(np.uint32).ravel())
        s = info["strict"]
        assert s.sum() > 300
        M = key(v["xyz"][s], v["rgb"][s])
        assert M <= P, len(M - P)


def test_analytic_sphere_closed(ctx):
    N = 64
    z, y, x = np.mgrid[0:N, 0:N, 0:N].astype(np.float64)
    r = np.sqrt((x - 30.6) ** 2 + (y - 33.2) ** 2 + (z - 31.1) ** 2) - 20.3
    vol = np.clip(np.round(r / 6.0 * 32767), -32767, 32767).astype(np.int16)
    col = np.zeros((N, N, N, 4), np.uint8)
    col[..., 3] = 1
    v, t = ctx.mesh(ctx.upload(vol), (3, 3, 3), (0, 0, 0), ctx.upload(col), (0, 0, 0), (N - 1,) * 3, (0, 0, 0), N)
    closed, ne = _closed(t)
    assert closed and len(v) - ne + len(t) == 2
    # outward: the normals point away from the centre
    p = v["xyz"].astype(np.float64)[t.astype(np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    c = p.mean(axis=1) - (np.array([30.6 + 0.5, 33.2 + 0.5, 31.1 + 0.5]) * 3 / N - 1.5)
    assert ((n * c).sum(axis=1) > 0).all()


def test_capacity_and_determinism(ctx):
    N = 64
    vol, col = random_volume_state(np.random.default_rng(7), N, True)
    dv, dc = ctx.upload(vol), ctx.upload(col)
    args = (dv, (3, 3, 3), (1, 2, 3), dc, (0, 0, 0), (N - 1,) * 3, (0, 0, 0), N)
    s, nv, nt = ctx.extract_mesh(*args)
    assert s == abi.KT_ERR_CAPACITY and nv > 0 and nt > 0
    guard = 64
    for cv, ct in ((nv - 1, nt), (nv, nt - 1), (0, nt), (nv // 2, nt // 2)):
        vb = ctx.upload(np.full((nv + guard) * 4, 0xA5A5A5A5, np.uint32))
        tb = ctx.upload(np.full((nt + guard) * 3, 0x5A5A5A5A, np.uint32))
        s, nv2, nt2 = ctx.extract_mesh(*args, vertices=vb, v_cap=cv, triangles=tb, t_cap=ct)
        assert s == abi.KT_ERR_CAPACITY and (nv2, nt2) == (nv, nt)
        assert (ctx.download(vb, np.uint32, ((nv + guard) * 4,)) == 0xA5A5A5A5).all()   # nothing written at all
        assert (ctx.download(tb, np.uint32, ((nt + guard) * 3,)) == 0x5A5A5A5A).all()
    vb = ctx.upload(np.full((nv + guard) * 4, 0xA5A5A5A5, np.uint32))
    tb = ctx.upload(np.full((nt + guard) * 3, 0x5A5A5A5A, np.uint32))
    s, _, _ = ctx.extract_mesh(*args, vertices=vb, v_cap=nv, triangles=tb, t_cap=nt)
    assert s == abi.KT_OK
    a = ctx.download(vb, np.uint32, ((nv + guard) * 4,))
    b = ctx.download(tb, np.uint32, ((nt + guard) * 3,))
    assert (a[nv * 4:] == 0xA5A5A5A5).all() and (b[nt * 3:] == 0x5A5A5A5A).all()
    assert ctx.extract_mesh(*args[:4], (5, 5, 5), (5, 5, 5), (0, 0, 0), N) == (abi.KT_OK, 0, 0)   # an empty box
    m1 = ctx.mesh(*args)
    m2 = ctx.mesh(*args)
    _same(m1, m2)
    with pytest.raises(abi.KtError):
        ctx.extract_mesh(dv, (3, 3, 3), (0, 0, 0), dc, (0, 0, 0), (N, N - 1, N - 1), (0, 0, 0), N)   # cells stop at N - 1


def _tri_cells(v, t, N, vsize):
    """the cell of every triangle, in world voxel units: the cell that holds its centroid (its vertices lie on the cell's edges)"""
    p = v["xyz"].astype(np.float64)[t.astype(np.int64)]
    cell = vsize / N
    return np.floor((p.mean(axis=1) + vsize / 2) / cell - 0.5).astype(np.int64)


def test_tracker_mesh_stage(ctx):
    """(In the oracle this walk's slabs are empty but for one Z- slab of 2425 points, and no oracle runs here: tests/test_gpu_shifts.py holds
    every slab's mesh to a restatement byte for byte.)"""
    from kintinuous_amd import synth
    cam = synth.Camera.small(160, 120)
    scene = synth.Scene("wall")
    traj = synth.crabwalk_trajectory(420)
    idx = list(range(0, 40, 2)) + list(range(40, 0, -2))   # out and back: X+ then X- shifts, and Z shifts from the walk's sway
    frames = [synth.render(scene, cam, *traj[i]) for i in idx]
    N, vsize = 96, 5.2   # (in this volume the Z- slab holds a piece of the wall; the X slabs lie outside the frustum)
    cfg = abi.TrackerConfig(cam.cols, cam.rows, N, cam.fx, cam.fy, cam.cx, cam.cy, vsize, 3, 2, 0, 0, 0, 0, 0, 0)

    def run(mesh):
        trk = abi.Tracker(ctx, cfg)
        if mesh:
            trk.enable_mesh_stage(True)
        for k, (d, rgb) in enumerate(frames):
            trk.process_frame_host(d, rgb, 33333 * k)
        trk.finalise()
        return trk

    off, on = run(False), run(True)
    try:
        _check_stage(off, on, frames, N, vsize)
    finally:
        off.close()
        on.close()


def _check_stage(off, on, frames, N, vsize):
    assert off.num_poses() == on.num_poses() == len(frames)
    for i in range(len(frames)):
        a, b = off.dense_pose(i), on.dense_pose(i)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert np.array_equal(off.pose()[0], on.pose()[0]) and np.array_equal(off.pose()[1], on.pose()[1])
    assert np.array_equal(off.volume(), on.volume()) and np.array_equal(off.color_volume(), on.color_volume())
    ns = on.num_slices()
    assert ns == off.num_slices() and ns >= 4
    dims = set()
    cells = []
    for i in range(ns):
        pa, da = off.slice(i)
        pb, db = on.slice(i)
        assert da == db and len(pa) == len(pb)   # the same point set (the extraction's order is unspecified)
        key = lambda p: np.sort(np.ascontiguousarray(p).view(np.dtype((np.void, p.dtype.itemsize))).ravel())
        assert np.array_equal(key(pa), key(pb))
        assert off.slice_mesh(i) is None
        v, t = on.slice_mesh(i)
        dims.add(db)
        assert on.slice_mesh_info(i) == (len(v), len(t))
        assert len(t) == 0 or t.max() < len(v)
        # the slice's strict-crossing vertices are points of its cloud: a mesh vertex that coincides with a cloud point carries its
        # colour word; the share of vertices found bounds how many could be non-strict (F == 0 ends are rare in fused volumes)
        P = set(zip(*(np.ascontiguousarray(pb["xyz"]).view(np.uint32).T.tolist()), pb["bgra"].copy().view(np.uint32).ravel().tolist()))
        M = list(zip(*(np.ascontiguousarray(v["xyz"]).view(np.uint32).T.tolist()), v["rgb"].tolist()))
        found = sum(m in P for m in M)
        assert found >= 0.99 * len(M), (i, found, len(M))
        if db != 7:
            # manifold away from the box faces: no interior edge in more than two triangles, each direction once
            tt = t.astype(np.int64)
            d = np.concatenate([tt[:, [0, 1]], tt[:, [1, 2]], tt[:, [2, 0]]])
            assert len(np.unique(d, axis=0)) == len(d)
        c = _tri_cells(v, t, N, vsize)
        cells.append(set(map(tuple, c.tolist())))
    assert {0, 1, 4, 5} <= dims and 7 in dims
    assert sum(len(c) for c in cells[:-1]) > 0 and len(cells[-1]) > 0   # the slabs together, and the final volume, have surface
    # the final mesh equals the restatement on the tracker's own volumes
    w = on.voxel_wrap()
    sw = [int(x) if x >= 0 else N - ((-int(x)) % N) for x in w]
    fv, ft = on.slice_mesh(ns - 1)
    rv, rt = mesh_ref.extract_mesh(on.volume(), on.color_volume(), (vsize,) * 3, sw, (0, 0, 0), (N - 1,) * 3, w, N)
    _same((fv, ft), (rv, rt))
    # no cell meshed twice: the slabs' cells (world voxel units) are disjoint, and disjoint from the final mesh's
    for i in range(ns):
        for j in range(i + 1, ns):
            assert not (cells[i] & cells[j]), (i, j, len(cells[i] & cells[j]))


def test_driver_writes_ply(tmp_path):
    from kintinuous_amd import klg, synth
    cam = synth.Camera.small(160, 120)
    scene = synth.Scene("wall")
    traj = synth.crabwalk_trajectory(420)
    idx = list(range(0, 30, 2)) + list(range(30, 0, -2))
    frames = [synth.render(scene, cam, *traj[i]) for i in idx]
    log = str(tmp_path / "log.klg")
    klg.write_klg(log, list(frames) + [frames[-1]], cols=cam.cols, rows=cam.rows)
    calib = str(tmp_path / "calib.txt")
    with open(calib, "w") as f:
        f.write(f"{cam.fx!r} {cam.fy!r} {cam.cx!r} {cam.cy!r}\n")
    common = ["-l", log, "-c", calib, "-n", "96", "-w", str(cam.cols), "-h", str(cam.rows), "-s", "7", "-t", "3"]
    for name, extra in (("plain", []), ("mesh", ["-m"])):
        r = subprocess.run([BIN] + common + ["-o", str(tmp_path / name)] + extra, cwd=str(tmp_path), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    assert open(tmp_path / "plain.poses").read() == open(tmp_path / "mesh.poses").read()
    assert not os.path.exists(tmp_path / "plain.ply")
    from test_mesh_table import read_ply
    v, t = read_ply(str(tmp_path / "mesh.ply"))
    # the same run through the C-ABI tracker: the file holds every slice's mesh, concatenated
    cfg = abi.TrackerConfig(cam.cols, cam.rows, 96, cam.fx, cam.fy, cam.cx, cam.cy, 7.0, 3, 2, 0, 0, 0, 0, 0, 0)
    c = abi.Ctx(0)
    trk = abi.Tracker(c, cfg)
    try:
        trk.enable_mesh_stage(True)
        for k, (d, rgb) in enumerate(frames):
            trk.process_frame_host(d, rgb, 33333 * k)
        trk.finalise()
        sizes = [trk.slice_mesh_info(i) for i in range(trk.num_slices())]
    finally:
        trk.close()
        c.close()
    assert len(v) == sum(s[0] for s in sizes) and len(t) == sum(s[1] for s in sizes) and len(t) > 0
    assert t.max() < len(v)
