"""GPU: the seam weld of the -m mesh (kt_mesh_weld.hip) -- kt_extract_mesh_keyed against kt_extract_mesh and the restatement's keys,
kt_mesh_weld_device and kt_mesh_weld byte for byte against kintinuous_amd/mesh_weld_ref.py on synthetic lists, the split box end to end,
the tracker's keys on an out-and-back walk, the welded mesh through kt_deform_apply_mesh, and the driver's -mw."""
import os
import subprocess

import numpy as np
import pytest

import mesh_weld_cases as cases
from conftest import random_volume_state
from kintinuous_amd import abi, mesh_ref, mesh_weld_ref

pytestmark = pytest.mark.gpu

V = abi.MESH_VERTEX_DTYPE
GUARD = 5
CV, CK, CT = 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A, 0x3C3C3C3C


def _vb(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def welder(ctx):
    w = abi.MeshWeld(ctx)
    yield w
    w.close()


# ---- keyed extraction -------------------------------------------------------------------------------------------------------------------
def _volumes():
    N = 32
    return {"sphere": (cases.sphere_volume(N), (3.0, 3.0, 3.0), (0, 0, 0), (0, 0, 0), N),
            "random": (random_volume_state(np.random.default_rng(11), N, True), (4.5, 5.0, 6.0), (5, 31, 17), (-40, 3 * N + 5, -7), N)}


def _ref_keyed(vol, col, vs, wrap, lo, hi, real, N):
    v, t, info = mesh_ref.extract_mesh(vol, col, vs, wrap, lo, hi, real, N, info=True)
    return v, t, mesh_weld_ref.edge_keys(info["owner"], info["axis"], real)


@pytest.mark.parametrize("name", ["sphere", "random"])
def test_keyed_extraction_and_split_box(ctx, welder, name):
    """On the boxes of the split test: kt_extract_mesh_keyed = kt_extract_mesh's vertices and triangles and the restatement's keys; the two
    halves concatenated and welded on the device are the one-box call's mesh."""
    (vol, col), vs, wrap, real, N = _volumes()[name]
    dv, dc = ctx.upload(vol), ctx.upload(col)
    for axis, cut in cases.SPLITS:
        got = []
        for lo, hi in cases.split_boxes(N, axis, cut):
            v, t, k = ctx.mesh_keyed(dv, vs, wrap, dc, lo, hi, real, N)
            pv, pt = ctx.mesh(dv, vs, wrap, dc, lo, hi, real, N)
            rv, rt, rk = _ref_keyed(vol, col, vs, wrap, lo, hi, real, N)
            assert np.array_equal(_vb(v), _vb(pv)) and np.array_equal(t, pt)
            assert np.array_equal(_vb(v), _vb(rv)) and np.array_equal(t, rt) and np.array_equal(k, rk)
            got.append((v, t, k))
        v, k, t, first, times = cases.concat(got[1], got[2])
        welded = welder.weld(v, k, t, first, times)
        cases.same(welded, mesh_weld_ref.weld(v, k, t, first, times))
        cases.check_split(got[0], welded)
        if name == "sphere":
            assert cases.closed(welded[2]) and (cut != 15 or not cases.closed(t))


def test_keyed_capacity_canary_and_range(ctx):
    N = 32
    (vol, col), vs, wrap, real, _ = _volumes()["random"]
    dv, dc = ctx.upload(vol), ctx.upload(col)
    args = (dv, vs, wrap, dc, (0, 0, 0), (N - 1,) * 3, real, N)
    s, nv, nt = ctx.extract_mesh_keyed(*args)
    assert s == abi.KT_ERR_CAPACITY and nv > 0 and nt > 0

    def bufs():
        return (ctx.upload(np.full((nv + GUARD) * 4, CV, np.uint32)), ctx.upload(np.full((nt + GUARD) * 3, CT, np.uint32)),
                ctx.upload(np.full(nv + GUARD, CK, np.uint64)))

    def down(vb, tb, kb):
        return ctx.download(vb, np.uint32, ((nv + GUARD) * 4,)), ctx.download(tb, np.uint32, ((nt + GUARD) * 3,)), ctx.download(kb, np.uint64, (nv + GUARD,))

    for cv, ct in ((nv - 1, nt), (nv, nt - 1), (0, nt)):
        vb, tb, kb = bufs()
        s, nv2, nt2 = ctx.extract_mesh_keyed(*args, vertices=vb, v_cap=cv, triangles=tb, t_cap=ct, keys=kb)
        assert s == abi.KT_ERR_CAPACITY and (nv2, nt2) == (nv, nt)
        a, b, c = down(vb, tb, kb)
        assert (a == CV).all() and (b == CT).all() and (c == CK).all()           # nothing written at all
    vb, tb, kb = bufs()
    assert ctx.extract_mesh_keyed(*args, vertices=vb, v_cap=nv, triangles=tb, t_cap=nt, keys=kb)[0] == abi.KT_OK
    a, b, c = down(vb, tb, kb)
    assert (a[nv * 4:] == CV).all() and (b[nt * 3:] == CT).all() and (c[nv:] == CK).all()
    assert (a[:nv * 4] != CV).any() and (np.diff(c[:nv].astype(np.int64)) > 0).all()
    # a real_voxel_wrap that pushes a coordinate of the box's voxels [0, N - 1] past 2^19 - 1, or below -2^19
    lim = 1 << 19
    for bad in ((lim - N + 1, 0, 0), (0, -lim - 1, 0), (0, 0, lim)):
        with pytest.raises(abi.KtError) as e:
            ctx.extract_mesh_keyed(dv, vs, wrap, dc, (0, 0, 0), (N - 1,) * 3, bad, N)
        assert e.value.status == abi.KT_ERR_ARG
    assert ctx.extract_mesh_keyed(dv, vs, wrap, dc, (0, 0, 0), (N - 1,) * 3, (lim - N, -lim, lim - N), N)[0] == abi.KT_ERR_CAPACITY   # the last that fit
    assert ctx.extract_mesh(dv, vs, wrap, dc, (0, 0, 0), (N - 1,) * 3, (lim, 0, 0), N)[0] == abi.KT_ERR_CAPACITY                     # unkeyed: no such limit


# ---- synthetic lists --------------------------------------------------------------------------------------------------------------------
def _device(ctx, welder, case, capacity=None):
    """kt_mesh_weld_device on uploads with canaries behind every buffer -> (status, n_out, span_first_out, buffers as left, inputs as left)"""
    v, k, tri, first, times, gap = case
    n, m = len(v), len(tri)
    cap = n if capacity is None else capacity
    dv = ctx.upload(np.concatenate([v.view(np.uint32).reshape(-1), np.full(4 * GUARD, CV, np.uint32)]))
    dk = ctx.upload(np.concatenate([k, np.full(GUARD, CK, np.uint64)]))
    dt = ctx.upload(np.concatenate([tri.reshape(-1), np.full(3 * GUARD, CT, np.uint32)]))
    ov = ctx.upload(np.full(4 * (cap + GUARD), CV, np.uint32))
    ok = ctx.upload(np.full(cap + GUARD, CK, np.uint64))
    s, n_out, fo = welder.weld_device(dv, dk, n, dt, m, first, times, gap, ov, ok, cap)
    out = (ctx.download(ov, np.uint32, (4 * (cap + GUARD),)), ctx.download(ok, np.uint64, (cap + GUARD,)), ctx.download(dt, np.uint32, (3 * (m + GUARD),)))
    ins = (ctx.download(dv, np.uint32, (4 * (n + GUARD),)), ctx.download(dk, np.uint64, (n + GUARD,)))
    for b in (dv, dk, dt, ov, ok):
        b.free()
    return s, n_out, fo, out, ins


def _check_device(ctx, welder, case):
    v, k, tri, first, times, gap = case
    n, m = len(v), len(tri)
    wv, wk, wt, wf = mesh_weld_ref.weld(*case)
    s, n_out, fo, (ov, ok, ot), (iv, ik) = _device(ctx, welder, case)
    assert s == abi.KT_OK and n_out == len(wv)
    assert np.array_equal(ov[:4 * n_out], wv.view(np.uint32).reshape(-1)) and np.array_equal(ok[:n_out], wk)
    assert np.array_equal(ot[:3 * m], wt.reshape(-1)) and np.array_equal(fo, wf)
    assert (ov[4 * n_out:] == CV).all() and (ok[n_out:] == CK).all() and (ot[3 * m:] == CT).all()    # nothing behind the outputs
    assert np.array_equal(iv[:4 * n], v.view(np.uint32).reshape(-1)) and (iv[4 * n:] == CV).all()    # the inputs are read only
    assert np.array_equal(ik[:n], k) and (ik[n:] == CK).all()
    return (wv, wk, wt, wf), (ov, ok, ot, fo)


@pytest.mark.parametrize("n", cases.SIZES)
def test_lists_device_and_host_forms(ctx, welder, n):
    for seed, spans, gap in ((n, 6, 10), (n + 1, 9, 0), (n + 2, 5, cases.NO_GATE), (n + 3, 40, 30)):
        case = cases.random_case(seed, n, spans, gap)
        want, got = _check_device(ctx, welder, case)
        _, again = _check_device(ctx, welder, case)                     # a second call: the same bytes
        assert all(np.array_equal(a, b) for a, b in zip(got, again))
        s, hv, hk, ht, hf, n_out = welder.weld_host(*case[:5], case[5])
        assert s == abi.KT_OK and n_out == len(want[0])
        cases.same((hv, hk, ht, hf), want)


def test_chains_and_a_table_beyond_lds(ctx, welder):
    for case in cases.chain_cases():
        _check_device(ctx, welder, case)
    # 3000 spans: above the table the head pass stages in LDS, with a gate (so the table is searched in global memory), and without
    rng = np.random.default_rng(3)
    n, S = 9001, 3000
    v, k, tri, _, _, _ = cases.random_case(77, n)
    first = np.concatenate([[0], np.sort(rng.integers(0, n + 1, S - 1)), [n]]).astype(np.int64)
    times = rng.integers(0, 200, S).astype(np.uint64)
    for gap in (40, cases.NO_GATE):
        want, _ = _check_device(ctx, welder, (v, k, tri, first, times, gap))
        assert 0 < len(want[0]) < n
    cases.same(mesh_weld_ref.weld(v, k, tri, first, times, 40), cases.brute_weld(v, k, tri, first, times, 40))


def test_large_after_small_equals_a_fresh_object(ctx):
    small, large = cases.random_case(1, 65), cases.random_case(2, 70001, 40, 30)
    a, b = abi.MeshWeld(ctx), abi.MeshWeld(ctx)
    try:
        _check_device(ctx, a, small)
        _, got = _check_device(ctx, a, large)
        _, fresh = _check_device(ctx, b, large)
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh))
        cases.same(a.weld(*small[:5], small[5]), mesh_weld_ref.weld(*small))          # ... and a small one after it
        cases.same(a.weld(*large[:5], large[5]), b.weld(*large[:5], large[5]))
    finally:
        a.close()
        b.close()


def test_errors_leave_everything_intact(ctx, welder):
    case = cases.random_case(9, 4099, 6, 10)
    v, k, tri, first, times, gap = case
    n, m = len(v), len(tri)
    want = mesh_weld_ref.weld(*case)
    n_keep = len(want[0])

    def intact(res):
        _, _, fo, (ov, ok, ot), (iv, ik) = res
        assert (ov == CV).all() and (ok == CK).all()
        assert np.array_equal(ot[:3 * m], tri.reshape(-1)) and (ot[3 * m:] == CT).all()
        assert np.array_equal(iv[:4 * n], v.view(np.uint32).reshape(-1)) and np.array_equal(ik[:n], k)
        assert (fo == -1).all()                                                        # span_first_out untouched as well

    for cap in (n_keep - 1, n_keep // 2, 0):
        res = _device(ctx, welder, case, capacity=cap)
        assert res[0] == abi.KT_ERR_CAPACITY and res[1] == n_keep
        intact(res)
    bad_tables = [(np.array([1] + first[1:].tolist()), times), (np.array(first[:-1].tolist() + [n - 1]), times),
                  (np.array([0, 9, 5] + first[3:].tolist()), times)]
    for f, t in bad_tables:
        res = _device(ctx, welder, (v, k, tri, f, t, gap))
        assert res[0] == abi.KT_ERR_ARG
        intact(res)
    for pos, val in ((0, 1 << 62), (n // 2, 1 << 63), (n - 1, (1 << 64) - 1)):       # a key with a top bit set: found on the device
        kb = k.copy()
        kb[pos] = val
        res = _device(ctx, welder, (v, kb, tri, first, times, gap))
        assert res[0] == abi.KT_ERR_ARG
        _, _, fo, (ov, ok, ot), _ = res
        assert (ov == CV).all() and (ok == CK).all() and np.array_equal(ot[:3 * m], tri.reshape(-1)) and (fo == -1).all()
        s, hv, hk, ht, hf, _ = welder.weld_host(v, kb, tri, first, times, gap)
        assert s == abi.KT_ERR_ARG and not hv.view(np.uint32).any() and not hk.any() and np.array_equal(ht, tri) and (hf == -1).all()
    # the host form at too small a capacity: the true count, nothing written
    s, hv, hk, ht, hf, n_out = welder.weld_host(v, k, tri, first, times, gap, capacity=n_keep - 1)
    assert s == abi.KT_ERR_CAPACITY and n_out == n_keep and not hv.view(np.uint32).any() and not hk.any() and np.array_equal(ht, tri) and (hf == -1).all()
    # null pointers with n > 0, misaligned vertices, the compaction in place, n > 2^29
    dv, dk, dt = ctx.upload(v), ctx.upload(k), ctx.upload(tri)
    ov, ok = ctx.empty(16 * n + 16), ctx.empty(8 * n)
    good = dict(vertices=dv, keys=dk, n=n, triangles=dt, m=m, span_first=first, span_time=times, max_gap=gap, vertices_out=ov, keys_out=ok, capacity=n)
    for change in (dict(vertices=None), dict(keys=None), dict(triangles=None), dict(vertices_out=None), dict(keys_out=None), dict(vertices=dv.ptr + 8),
                   dict(vertices_out=ov.ptr + 4), dict(vertices_out=dv), dict(keys_out=dk), dict(n=(1 << 29) + 1, span_first=[0, (1 << 29) + 1], span_time=[0])):
        assert welder.weld_device(**{**good, **change})[0] == abi.KT_ERR_ARG, change
    assert np.array_equal(ctx.download(dt, np.uint32, (m, 3)), tri) and np.array_equal(_vb(ctx.download(dv, V, (n,))), _vb(v))
    s, n_out, fo = welder.weld_device(**good)                                           # the object is still usable
    assert s == abi.KT_OK and n_out == n_keep and np.array_equal(fo, want[3])
    assert np.array_equal(ctx.download(dt, np.uint32, (m, 3)), want[2])
    # n = 0: KT_OK with any valid table, null pointers included
    assert welder.weld_device(None, None, 0, None, 0, [0, 0, 0], [3, 4], gap, None, None, 0) [:2] == (abi.KT_OK, 0)
    s, n_out, fo = welder.weld_device(None, None, 0, None, 0, [0], [], gap, None, None, 0)
    assert (s, n_out, fo.tolist()) == (abi.KT_OK, 0, [0])
    for b in (dv, dk, dt, ov, ok):
        b.free()


def test_allocations_return(ctx):
    ctx.sync()
    start = abi.live_allocations()
    w = abi.MeshWeld(ctx)
    created = abi.live_allocations()[0]
    assert created > start[0]
    case = cases.random_case(4, 257)
    _check_device(ctx, w, case)
    device_form = abi.live_allocations()[0]
    assert device_form > created                                      # the per-vertex arrays and the span table are the object's
    w.weld(*case[:5], case[5])
    assert abi.live_allocations()[0] == device_form + 5               # ... and so is the host form's staging
    w.weld(*cases.random_case(5, 65)[:5])                             # a smaller call takes nothing
    assert abi.live_allocations()[0] == device_form + 5
    w.weld(*cases.random_case(6, 4099)[:5])                           # a larger one releases and takes again
    assert abi.live_allocations()[0] == device_form + 5
    w.close()
    assert abi.live_allocations() == start


# ---- the tracker ------------------------------------------------------------------------------------------------------------------------
def test_tracker_keys_and_weld(ctx, welder):
    """The out-and-back crab-walk of test_gpu_mesh.py::test_tracker_mesh_stage (N = 96, 160 x 120), with keys on and off.
    Every slice's mesh equals the run with keys off; keys rise strictly per slice; the off-axis coordinates are the kernel's own
    arithmetic on the key; the weld over all slices merges vertices, every merged pair shares its edge and lies less than a cell apart,
    and fewer edges are used by exactly one triangle.
    Measured on an MI355X: 9 slices, 3271 vertices -> 3153 (118 merged), the largest distance of a merged pair 0.074 of a cell, edges
    used by exactly one triangle 907 -> 679.
    (In the oracle this walk's slabs are empty but for one Z- slab: tests/test_gpu_shifts.py welds slabs of every dimension.)"""
    from kintinuous_amd import synth
    cam = synth.Camera.small(160, 120)
    scene = synth.Scene("wall")
    traj = synth.crabwalk_trajectory(420)
    idx = list(range(0, 40, 2)) + list(range(40, 0, -2))
    frames = [synth.render(scene, cam, *traj[i]) for i in idx]
    N, vsize = 96, 5.2
    cfg = abi.TrackerConfig(cam.cols, cam.rows, N, cam.fx, cam.fy, cam.cx, cam.cy, vsize, 3, 2, 0, 0, 0, 0, 0, 0)


    def run(keys):
        """(meshes, keys, times, wraps): per slice; wraps = the real voxel wrap each slice was meshed under, followed frame by frame (the
        axes shift one after the other, each slab under the wrap of the axes before it)"""
        trk = abi.Tracker(ctx, cfg)
        try:
            if keys:
                trk.enable_mesh_keys(True)        # ahead of the stage: the key arrays follow the stage's bounds
            trk.enable_mesh_stage(True)
            wraps, wrap = [], trk.voxel_wrap().astype(np.int64)
            for k, (d, rgb) in enumerate(frames):
                trk.process_frame_host(d, rgb, 33333 * k)
                after = trk.voxel_wrap().astype(np.int64)
                for i in range(len(wraps), trk.num_slices()):
                    axis = trk.slice_info(i)[1] // 2
                    wraps.append(wrap.copy())
                    wrap[axis] = after[axis]
                assert np.array_equal(wrap, after)
            trk.finalise()
            wraps.append(wrap.copy())
            ns = trk.num_slices()
            assert ns == len(wraps)
            meshes = [trk.slice_mesh(i) for i in range(ns)]
            if not keys:
                with pytest.raises(abi.KtError) as e:
                    trk.slice_mesh_keys(0)
                assert e.value.status == abi.KT_ERR_STATE
                return meshes, None, None, wraps
            return meshes, [trk.slice_mesh_keys(i) for i in range(ns)], [trk.slice_pose(i)[2] for i in range(ns)], wraps
        finally:
            trk.close()

    off, _, _, _ = run(False)
    on, keys, times, wraps = run(True)
    assert len(on) == len(off) >= 4
    cell = np.float32(vsize) / np.float32(N)
    half = (cell * np.float32(N)) / np.float32(2)
    for (v, t), (pv, pt), k, wrap in zip(on, off, keys, wraps):
        assert np.array_equal(_vb(v), _vb(pv)) and np.array_equal(t, pt) and len(k) == len(v)
        assert (np.diff(k.astype(np.int64)) > 0).all() and not (k >> np.uint64(62)).any()
        # the off-axis coordinates from the key in the kernel's own order: ((x + 0.5) cell + wrap cell) - half with x = g - wrap
        g, ax = mesh_weld_ref.key_fields(k)
        x = (g - wrap[None, :]).astype(np.float32)
        assert (x >= 0).all() and (x <= N - 1).all()
        base = ((x + np.float32(0.5)) * cell + wrap.astype(np.float32)[None, :] * cell) - half
        offax = np.arange(3)[None, :] != ax[:, None]
        assert np.array_equal(v["xyz"][offax], base[offax])
        along = (v["xyz"] - base)[~offax]
        assert (along >= -4 * np.spacing(np.float32(vsize))).all() and (along <= cell + 4 * np.spacing(np.float32(vsize))).all()   # on the edge the key names
    v = np.concatenate([m[0] for m in on])
    k = np.concatenate(keys)
    first = np.concatenate([[0], np.cumsum([len(m[0]) for m in on])]).astype(np.int64)
    tri = np.concatenate([m[1] + np.uint32(first[i]) for i, m in enumerate(on)]).astype(np.uint32)
    times = np.array(times, np.uint64)
    wv, wk, wt, wf = welder.weld(v, k, tri, first, times)
    cases.same((wv, wk, wt, wf), mesh_weld_ref.weld(v, k, tri, first, times))
    rep = mesh_weld_ref.representatives(k, first, times)
    merged = np.nonzero(rep != np.arange(len(v)))[0]
    assert len(merged) > 0 and len(wv) == len(v) - len(merged)
    d = v["xyz"][merged].astype(np.float64) - v["xyz"][rep[merged]].astype(np.float64)
    before, after = cases.open_edges(tri), cases.open_edges(wt)
    print("slices", len(on), "vertices", len(v), "->", len(wv), "merged", len(merged), "largest distance of a merged pair / cell",
          float(np.sqrt((d * d).sum(axis=1)).max() / cell), "open edges", before, "->", after)
    assert np.array_equal(k[merged], k[rep[merged]])                                    # one edge ...
    assert np.sqrt((d * d).sum(axis=1)).max() < cell                                    # ... and less than one cell apart
    assert after < before


# ---- the deformation ----------------------------------------------------------------------------------------------------------------------
def test_welded_mesh_through_the_deformation(ctx, welder):
    """A two-span mesh with a seam of 90 shared keys, welded, goes into kt_deform_apply_mesh with span_first_out on the 20-node graph of
    tests/deform_mesh_cases.py: every byte equals deform_ref.apply_mesh on the restatement's welded arrays."""
    import deform_cases as dc
    import deform_mesh_cases as mc
    from kintinuous_amd import deform_ref as ref
    gname = "m20_n64_c7"
    gc = dc.case(gname)
    rng = np.random.default_rng(21)
    nA, nB, seam = 300, 280, 90
    times = np.array([mc.span_times(20)[2], mc.span_times(20)[7]], np.uint64)
    first = np.array([0, nA, nA + nB], np.int64)
    xyz = dc.curve(rng.uniform(0, 19, nA + nB)) + rng.uniform(-0.5, 0.5, (nA + nB, 3))
    xyz[nA:nA + seam] = xyz[nA - seam:nA] + [0.01, 0.0, 0.0]           # the later slab's vertex on the same edge, a little along it
    v = np.zeros(nA + nB, V)
    v["xyz"] = xyz.astype(np.float32)
    v["rgb"] = rng.integers(0, 1 << 32, nA + nB, dtype=np.uint64).astype(np.uint32)
    k = np.concatenate([np.arange(nA) * 4 + 1, np.arange(nA - seam, nA) * 4 + 1, (nA + np.arange(nB - seam)) * 4 + 2]).astype(np.uint64)
    ta = np.concatenate([rng.integers(0, nA, (500, 3)), [[nA - 1, nA - 2, 0]]])
    tb = np.concatenate([nA + rng.integers(0, nB, (450, 3)), [[nA + seam - 1, nA + seam, nA + seam + 1]]])   # nA + seam - 1 shares nA - 1's key
    tri = np.concatenate([ta, tb]).astype(np.uint32)
    want = mesh_weld_ref.weld(v, k, tri, first, times)
    got = welder.weld(v, k, tri, first, times)
    cases.same(got, want)
    wv, wk, wt, wf = got
    assert len(wv) == nA + nB - seam and wf.tolist() == [0, nA, nA + nB - seam]
    g = abi.DeformationGraph(ctx, 20, 8)
    try:
        g.set_graph(gc["node_pos"], gc["node_time"])
        g.set_state(dc.restated(gname)[0])
        moved = g.apply_mesh(wv, wf, times)
        unwelded = g.apply_mesh(v, first, times)
    finally:
        g.close()
    ref_moved = ref.apply_mesh(dc.graph(gname), dc.restated(gname)[0], want[0], want[3], times)
    assert moved.tobytes() == ref_moved.tobytes()
    assert np.abs(moved["xyz"] - wv["xyz"]).max() > 0
    # the seam vertex nA - 1 is referenced by the last triangle of either span: one index, in the earlier span, hence one position; on the
    # unwelded mesh the two stay apart
    assert wt[len(ta) - 1, 0] == wt[-1, 0] == nA - 1 < wf[1]
    assert not np.array_equal(unwelded["xyz"][nA - 1], unwelded["xyz"][nA + seam - 1])


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def _rgb24(v):
    return v["rgb"][:, 0].astype(np.uint32) << 16 | v["rgb"][:, 1].astype(np.uint32) << 8 | v["rgb"][:, 2].astype(np.uint32)


def _driver_weld_is_the_restatements(ctx, prefix, cfg, frames, stamps, trajectory=None):
    """<prefix>_weld.ply and <prefix>.weld against the restatement's weld of <prefix>.ply with the keys of the same frames through the
    C-ABI tracker (the .ply keeps three colour bytes of the vertex's four; the weld moves whatever it is given) -> (n_in, n_out, spans,
    open edges before, after)"""
    import deform_mesh_cases as mc
    v, tri = mc.read_ply(prefix + ".ply")
    lines = [l.split() for l in open(prefix + ".weld").read().splitlines()]
    spans = [(int(a), int(b), int(c)) for tag, a, b, c in lines[:-1] if tag == "span"]
    assert len(spans) == len(lines) - 1 and lines[-1][0] == "result"
    n_in, n_out, n_tri = (int(x) for x in lines[-1][1:])
    assert n_in == len(v) and n_tri == len(tri)
    first = np.array([s[1] for s in spans] + [n_in], np.int64)
    times = np.array([s[0] for s in spans], np.uint64)
    wv, wtri = mc.read_ply(prefix + "_weld.ply")
    trk = abi.Tracker(ctx, cfg)
    try:
        if trajectory is not None:
            trk.load_trajectory(*trajectory)
        trk.enable_mesh_stage(True)
        trk.enable_mesh_keys(True)
        for (d, rgb), ts in zip(frames, stamps):
            trk.process_frame_host(d, rgb, ts)
        trk.finalise()
        ns = trk.num_slices()
        meshes = [trk.slice_mesh(i) for i in range(ns)]
        keys = np.concatenate([trk.slice_mesh_keys(i) for i in range(ns)])
        assert [trk.slice_pose(i)[2] for i in range(ns)] == times.tolist()
    finally:
        trk.close()
    assert [len(m[0]) for m in meshes] == np.diff(first).tolist()
    assert np.array_equal(np.concatenate([m[0]["xyz"] for m in meshes]), v["xyz"])       # the run's own .ply is this tracker's mesh
    full = np.zeros(n_in, V)
    full["xyz"], full["rgb"] = v["xyz"], _rgb24(v)
    rv, rk, rt, rf = mesh_weld_ref.weld(full, keys, tri.astype(np.uint32), first, times)
    assert len(rv) == n_out == len(wv) and np.array_equal(rv["xyz"], wv["xyz"]) and np.array_equal(rv["rgb"], _rgb24(wv))
    assert np.array_equal(rt.astype(np.int32), wtri)
    assert [s[2] for s in spans] == rf[:-1].tolist() and rf[-1] == n_out
    return n_in, n_out, len(spans), cases.open_edges(tri), cases.open_edges(wtri)


def test_driver_mw(ctx, tmp_path):
    """kintinuous_hip ... -lc -pg -pcd -m -mw -df on the ten-frame walk of tests/test_gpu_deform_mesh.py's driver test: _weld.ply and .weld are
    the restatement's weld of the run's own .ply with the keys of the same frames through the C-ABI tracker; _weld_def.ply has _weld.ply's
    faces; every file of the run without -mw is byte-identical; -mw without -m is ignored with a message.  That walk never shifts the
    volume (measured: 1 span, 3746 vertices, nothing to merge), so the crab-walk of test_tracker_keys_and_weld runs with -m -mw as
    well: there the file has seams, and the weld closes edges."""
    import deform_mesh_cases as mc
    import loop_db_cases as lc
    from kintinuous_amd import build, klg, synth
    build.build_host()
    frames = [lc.frames()[k] for k in range(10)]
    stamps = [1000 * (k + 1) for k in range(10)]
    log = str(tmp_path / "ten.klg")
    klg.write_klg(log, frames + [frames[-1]], timestamps=stamps + [99000], cols=lc.COLS, rows=lc.ROWS)
    cam = lc.camera()
    calib = tmp_path / "calib.txt"
    calib.write_text(f"{cam.fx!r} {cam.fy!r} {cam.cx!r} {cam.cy!r}\n")
    tfile = str(tmp_path / "traj.csv")
    rows = synth.ground_truth_rows([(T[:3, :3], T[:3, 3]) for T in lc.poses()])
    synth.write_trajectory_file(tfile, stamps, rows)

    def run(name, *extra):
        prefix = str(tmp_path / name)
        r = subprocess.run([build.HOST_BIN, "-l", log, "-c", str(calib), "-n", "96", "-w", str(lc.COLS), "-h", str(lc.ROWS), "-s", "6", "-p", tfile, "-o", prefix,
                            "-v", "vocab.yml.gz", "-lc", "-dl", "3", "-pcd", "-pg", "-df", "-dg", "0.02", "-ds", "1e-9", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (extra, r.returncode, r.stdout, r.stderr[-2000:])
        return r, prefix

    plain, p0 = run("plain", "-m")
    weld, p1 = run("weld", "-m", "-mw")
    nomesh, p2 = run("nomesh", "-mw")
    rd = lambda p: open(p, "rb").read()
    base = os.path.basename
    outputs = lambda p: sorted(f[len(base(p)):] for f in os.listdir(tmp_path) if f.startswith(base(p) + ".") or f.startswith(base(p) + "_"))
    assert outputs(p1) == sorted(outputs(p0) + [".weld", "_weld.ply", "_weld_def.ply"])
    for ext in outputs(p0):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    assert "-mw ignored without -m" in nomesh.stderr and not [e for e in outputs(p2) if "weld" in e or e.endswith(".ply")]
    cfg = abi.TrackerConfig(lc.COLS, lc.ROWS, 96, cam.fx, cam.fy, cam.cx, cam.cy, 6.0, 14, 2, 0, 0, 0, 0, 0, 0)
    got = _driver_weld_is_the_restatements(ctx, p1, cfg, frames + [frames[-1]], stamps + [99000], (np.array(stamps, np.uint64), rows))
    print("loop log: vertices %d -> %d in %d spans, open edges %d -> %d" % got)
    wv, wtri = mc.read_ply(p1 + "_weld.ply")
    dv, dtri = mc.read_ply(p1 + "_weld_def.ply")
    assert np.array_equal(wtri, dtri) and len(wv) == len(dv) and wv["rgb"].tobytes() == dv["rgb"].tobytes()
    assert np.abs(dv["xyz"] - wv["xyz"]).max() > 0                                          # ... and it was deformed
    # the out-and-back crab-walk of test_tracker_keys_and_weld (a 5.2 m volume: there the slabs that leave hold a piece of the wall)
    cam = synth.Camera.small(160, 120)
    traj = synth.crabwalk_trajectory(420)
    frames = [synth.render(synth.Scene("wall"), cam, *traj[i]) for i in list(range(0, 40, 2)) + list(range(40, 0, -2))]
    log = str(tmp_path / "crab.klg")
    klg.write_klg(log, list(frames) + [frames[-1]], cols=cam.cols, rows=cam.rows)
    calib.write_text(f"{cam.fx!r} {cam.fy!r} {cam.cx!r} {cam.cy!r}\n")
    p3 = str(tmp_path / "crab")
    r = subprocess.run([build.HOST_BIN, "-l", log, "-c", str(calib), "-n", "96", "-w", str(cam.cols), "-h", str(cam.rows), "-s", "5.2", "-t", "3", "-o", p3, "-m", "-mw"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    cfg = abi.TrackerConfig(cam.cols, cam.rows, 96, cam.fx, cam.fy, cam.cx, cam.cy, 5.2, 3, 2, 0, 0, 0, 0, 0, 0)
    got = _driver_weld_is_the_restatements(ctx, p3, cfg, frames, [33333 * k for k in range(len(frames))])
    print("crab-walk: vertices %d -> %d in %d spans, open edges %d -> %d" % got)
    n_in, n_out, n_spans, before, after = got
    assert n_spans > 1 and n_out < n_in and after < before
    assert not os.path.exists(p3 + "_weld_def.ply")
