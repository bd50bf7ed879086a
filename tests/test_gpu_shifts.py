"""The shift path of the cyclical volume with data in every slab: the tour and the ICP legs of tests/shift_cases.py (tests/test_shift_cases.py
asserts, without a GPU, that every dimension leaves with hundreds of points, that frames shift three axes with three full slabs, and that
the restatement of a shifting frame equals the oracle tracker's slices).

The crab-walks of test_gpu_tracker.py, test_gpu_mesh.py and test_gpu_mesh_weld.py and the turn of test_gpu_headings.py shift with empty or nearly
empty slabs, never along y, never three axes in a frame.  Here the tracker is held to the oracle after EVERY shifting frame (a clear that
took a plane too many is seen before a later frame overwrites it), and the slab meshes and keys -- so far checked by properties -- byte for
byte to shift_cases.restate_frame, the second and third slab of a frame included.

Scratch mutations of finish_pose (csrc/kt_tracker.hip), each failing here: DESIGN.md section 5.
"""
import hashlib

import numpy as np
import pytest

import mesh_weld_cases as weld_cases
import shift_cases as S
from kintinuous_amd import abi, mesh_ref, mesh_weld_ref

pytestmark = pytest.mark.gpu


def _vb(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _volumes_equal(trk, otr, what):
    v, ov = trk.volume(), otr.volume()
    c, oc = trk.color_volume(), otr.color_volume()
    assert np.array_equal(v, ov), f"{what}: {int((v != ov).sum())} tsdf words differ, planes x {np.unique(np.nonzero(v != ov)[2])[:8]} y {np.unique(np.nonzero(v != ov)[1])[:8]} z {np.unique(np.nonzero(v != ov)[0])[:8]}"
    for ch in range(4):
        assert np.array_equal(c[..., ch], oc[..., ch]), f"{what}: colour / weight byte {ch}: {int((c[..., ch] != oc[..., ch]).sum())} differ"


@pytest.mark.parametrize("readahead", [0, 1])
def test_tour_against_the_oracle(ctx, oracle_mod, readahead):
    """The tracker and the oracle's tracker on the tour's ground-truth poses: pose, global camera and wrap bit for bit every frame; the
    tsdf words and all four colour / weight bytes after every shifting frame; every slice the same dimension and point set, the finalise
    slice too; the predicted maps of the last frame equal in validity and bits.  With readahead every frame is announced one call early."""
    O = oracle_mod
    frames = S.tour_frames()
    stamps, rows = S.tour_trajectory()
    trk, otr = abi.Tracker(ctx, S.config(abi.TrackerConfig)), O.OracleTracker(S.config(O.OTrackerConfig))
    try:
        trk.load_trajectory(stamps, rows)
        otr.load_trajectory(stamps, rows)
        shifting = 0
        for k, (d, rgb) in enumerate(frames):
            if readahead and k + 1 < len(frames):
                trk.prefetch_frame_host(*frames[k + 1])
            before = otr.num_slices()
            trk.process_frame_host(d, rgb, int(stamps[k]))
            otr.process_frame(d, rgb, int(stamps[k]))
            assert trk.num_poses() == otr.num_poses() == k + 1
            for a, b in zip(trk.pose(), otr.pose()):
                assert np.array_equal(a, b), k
            assert np.array_equal(trk.voxel_wrap(), otr.voxel_wrap()), k
            if otr.num_slices() > before:
                shifting += 1
                assert trk.num_slices() == otr.num_slices(), k
                _volumes_equal(trk, otr, f"frame {k} (slabs {[otr.slice(i)[1] for i in range(before, otr.num_slices())]})")
        assert shifting >= 40
        _volumes_equal(trk, otr, "the last frame")
        a, b = trk.vmap_g_prev(0), otr.vmap_g_prev(0)
        va = np.isfinite(a)
        assert np.array_equal(va, np.isfinite(b)) and va.sum() > 1000 and np.array_equal(a[va].view(np.uint32), b[va].view(np.uint32))
        a, b = trk.nmap_g_prev(0), otr.nmap_g_prev(0)
        va = np.isfinite(a)
        assert np.array_equal(va, np.isfinite(b)) and va.sum() > 1000 and np.array_equal(a[va].view(np.uint32), b[va].view(np.uint32))
        trk.finalise()
        otr.finalise()
        assert trk.num_slices() == otr.num_slices()
        full = 0
        for i in range(trk.num_slices()):
            p, dim = trk.slice(i)
            q, dim2 = otr.slice(i)
            assert dim == dim2 and S.same_points(p, q), (i, dim, dim2, len(p), len(q))
            full += len(p) >= 200
        assert dim == 7 and len(p) > 1000 and full >= 15
    finally:
        trk.close()
        otr.close()


def _digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).view(np.uint8)).hexdigest()


def _tour_run(ctx, stages):
    """the tracker alone on the tour, stages on or off: what it showed per frame (pose, wrap, and after a shifting frame a digest of the
    tsdf volume and of the colour volume) and what it holds at the end"""
    frames = S.tour_frames()
    stamps, rows = S.tour_trajectory()
    trk = abi.Tracker(ctx, S.config(abi.TrackerConfig))
    out = dict(pose=[], wrap=[], volumes={})
    try:
        trk.load_trajectory(stamps, rows)
        if stages:
            trk.enable_mesh_keys(True)        # ahead of the stage: the key arrays follow the stage's bounds
            trk.enable_mesh_stage(True)
            trk.enable_slice_stage(True, weight_cull=2)
        for k, (d, rgb) in enumerate(frames):
            before = trk.num_slices()
            trk.process_frame_host(d, rgb, int(stamps[k]))
            out["pose"].append(trk.pose())
            out["wrap"].append(trk.voxel_wrap())
            if trk.num_slices() > before:
                out["volumes"][k] = (_digest(trk.volume()), _digest(trk.color_volume()))
        out["final"] = (trk.volume(), trk.color_volume(), [int(w) for w in trk.voxel_wrap()])
        trk.finalise()
        ns = trk.num_slices()
        out["raw"] = [trk.slice(i) for i in range(ns)]
        out["mesh"] = [trk.slice_mesh(i) for i in range(ns)]
        out["proc"] = [trk.slice_processed(i) for i in range(ns)]
        if stages:
            out["keys"] = [trk.slice_mesh_keys(i) for i in range(ns)]
            out["info"] = [trk.slice_mesh_info(i) for i in range(ns)]
    finally:
        trk.close()
    return out


@pytest.fixture(scope="module")
def staged(ctx):
    """the tour with the mesh stage, its keys and the slice stage on; computed once, left unchanged"""
    return _tour_run(ctx, True)


def _tri_cells(v, t):
    """tests/test_gpu_mesh.py: the cell of every triangle in world voxels -- the cell that holds its centroid"""
    p = v["xyz"].astype(np.float64)[t.astype(np.int64)]
    return np.floor((p.mean(axis=1) + S.SIZE / 2) / S.VOXEL - 0.5).astype(np.int64)


def test_tour_with_the_stages_on(ctx, oracle_mod, staged):
    """enable_mesh_keys, enable_mesh_stage and enable_slice_stage(weight_cull = 2) on the tour.  Poses, wraps, the volumes after every
    shifting frame and the raw slices are those of the run with everything off.  Every slab's mesh -- vertices, triangles -- and its keys
    equal shift_cases.restate_frame's byte for byte: the box of each axis as finish_pose forms it, extracted BEFORE the clears of its own
    axis and AFTER those of the axes before it in the same frame.  Every processed slice is the stand-alone kt_slice_process of the raw one
    (the rule of tests/test_slice_process.py).  No cell is meshed twice (shift_cases.fresh_cells: the check of test_gpu_mesh.py::_check_stage
    for a tour that comes back to places it has left), the last mesh included, which equals the restatement on the tracker's own volume."""
    O = oracle_mod
    on, off = staged, _tour_run(ctx, False)
    run = S.tour_oracle(O)
    slabs = run["restated"]
    assert len(on["pose"]) == len(off["pose"]) == len(S.tour_frames())
    for k, (a, b) in enumerate(zip(on["pose"], off["pose"])):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(on["wrap"][k], off["wrap"][k]), k
        assert np.array_equal(on["wrap"][k], run["wrap"][k]), k
    assert sorted(on["volumes"]) == sorted(off["volumes"]) == [f[0] for f in run["frames"]]
    for k in on["volumes"]:
        assert on["volumes"][k] == off["volumes"][k], f"frame {k}: the volumes differ with the stages on"
    assert len(on["raw"]) == len(off["raw"]) == len(slabs) + 1
    assert all(m is None for m in off["mesh"]) and all(p is None for p in off["proc"])
    leaf = S.SIZE / S.N
    compared = dict(vertices=0, second=0, third=0, processed=0)
    for i, ((raw, dim), (raw_off, dim_off)) in enumerate(zip(on["raw"], off["raw"])):
        assert dim == dim_off and S.same_points(raw, raw_off), (i, dim, len(raw), len(raw_off))
        want = abi.slice_process(ctx, raw, 2, leaf) if len(raw) else np.zeros(0, abi.NPOINT_DTYPE)
        proc = on["proc"][i]
        assert proc is not None and len(proc) == len(want) and proc.tobytes() == want.tobytes(), (i, dim, len(raw))
        ref = O.slice_process(raw.view(O.POINT_DTYPE), 2, leaf)
        assert len(ref) == len(proc) and np.array_equal(ref["xyz"], proc["xyz"]) and np.array_equal(ref["bgra"], proc["bgra"]), (i, dim)
        compared["processed"] += len(proc)
    for k, before, after, dims, first in run["frames"]:
        for j, dim in enumerate(dims):
            i = first + j
            s, (v, t), keys = slabs[i], on["mesh"][i], on["keys"][i]
            what = f"frame {k}, slab {j} of {dims} (slice {i}): restated {len(s.vertices)} vertices, {len(s.triangles)} triangles"
            assert on["raw"][i][1] == dim == s.dim and S.same_points(on["raw"][i][0], s.cloud), what
            assert on["info"][i] == (len(v), len(t)) == (len(s.vertices), len(s.triangles)), f"{what}; the tracker {on['info'][i]}"
            assert np.array_equal(_vb(v), _vb(s.vertices)), what
            assert np.array_equal(t, s.triangles), what
            assert np.array_equal(keys, s.keys), what
            compared["vertices"] += len(v)
            if j:
                compared["second" if j == 1 else "third"] += len(v)
    print("compared byte for byte:", compared)
    assert compared["vertices"] > 20000 and compared["second"] > 5000 and compared["third"] > 3000 and compared["processed"] > 3000
    # the last mesh: the restatement on the tracker's own volume
    vol, col, wrap = on["final"]
    fv, ft = on["mesh"][-1]
    rv, rt = mesh_ref.extract_mesh(vol, col, (S.SIZE,) * 3, S.storage_wrap(wrap), (0, 0, 0), (S.N - 1,) * 3, wrap, S.N)
    assert len(ft) > 1000 and np.array_equal(_vb(fv), _vb(rv)) and np.array_equal(ft, rt)
    mine = [s._replace(cells=_tri_cells(*on["mesh"][i])) for i, s in enumerate(slabs)]
    assert S.fresh_cells(mine, _tri_cells(fv, ft)) == []


def test_weld_over_the_tour(ctx, oracle_mod, staged):
    """kt_mesh_weld over the tracker's slab meshes and keys of the tour (a slab's span time is its index): the restatement's weld on every
    byte; merged pairs across cuts along x, along y and along z; fewer edges used by exactly one triangle than before."""
    ref = S.tour_oracle(oracle_mod)["restated"]      # (the wrap and the shift of each slab)
    assert len(staged["mesh"]) == len(ref) + 1
    slabs = [r._replace(cloud=None, vertices=v, triangles=t, keys=k, cells=_tri_cells(v, t)) for r, (v, t), k in zip(ref, staged["mesh"], staged["keys"])]
    v, k, tri, first, times = S.concat([(s.vertices, s.triangles) for s in slabs], [s.keys for s in slabs])
    w = abi.MeshWeld(ctx)
    try:
        got = w.weld(v, k, tri, first, times)
    finally:
        w.close()
    weld_cases.same(got, mesh_weld_ref.weld(v, k, tri, first, times))
    merged, seams = S.seam_counts(slabs, k, first)
    before, after = weld_cases.open_edges(tri), weld_cases.open_edges(got[2])
    print("slabs", len(slabs), "vertices", len(v), "->", len(got[0]), "merged", merged, "across a cut along x, y, z", seams, "open edges", before, "->", after)
    assert len(got[0]) == len(v) - merged and min(seams) >= 1
    assert after < before


@pytest.mark.parametrize("leg", list(S.ICP_SIGNS))
def test_icp_legs(ctx, oracle_mod, leg):
    """ICP odometry, so the shift is decided on the device (csrc/kt_setup.hpp parks the frame, finish_pose must agree and redo the fusion):
    along (1, 0.8, 1) with signs, Y+ and Y- among the slabs and one frame of three.  The bars of test_gpu_tracker.py: poses within 1e-6,
    the same wrap every frame, slices the same points, volumes byte-identical; no frame fell back to the stepwise odometry."""
    O = oracle_mod
    frames, _ = S.leg_frames(leg)
    want = S.leg_oracle(O, leg)
    trk, otr = abi.Tracker(ctx, S.config(abi.TrackerConfig, S.ICP_SIZE)), O.OracleTracker(S.config(O.OTrackerConfig, S.ICP_SIZE))
    try:
        fallbacks = trk.odometry_fallbacks()
        max_t = max_r = 0.0
        for k, (d, rgb) in enumerate(frames):
            trk.process_frame_host(d, rgb, 33333 * k)
            otr.process_frame(d, rgb, 33333 * k)
            R, t, gc = trk.pose()
            Ro, to, go = otr.pose()
            max_t = max(max_t, float(np.abs(t - to).max() / max(1.0, np.abs(to).max())), float(np.abs(gc - go).max()))
            max_r = max(max_r, float(np.abs(R - Ro).max()))
            assert np.array_equal(trk.voxel_wrap(), otr.voxel_wrap()) and [int(w) for w in otr.voxel_wrap()] == want["wrap"][k], f"frame {k}: shift decisions diverged"
        assert max_t < 1e-6 and max_r < 1e-6, (max_t, max_r)
        assert trk.odometry_fallbacks() == fallbacks == 0
        assert trk.num_slices() == otr.num_slices() == len(want["dims"]) >= 8
        for i in range(trk.num_slices()):
            p, dim = trk.slice(i)
            q, dim2 = otr.slice(i)
            assert dim == dim2 == want["dims"][i] and S.same_points(p, q), (i, dim, dim2, len(p), len(q))
        _volumes_equal(trk, otr, leg)
    finally:
        trk.close()
        otr.close()
