"""GPU: Taubin's lambda|mu smoothing of the -m mesh (kt_mesh_smooth.hip) -- kt_mesh_smooth_device and kt_mesh_smooth byte for byte against
kintinuous_amd/mesh_smooth_ref.py on every case of mesh_smooth_cases in both modes, grid patches up to 70001 triangles at the origin and
near (8000, -8000, 8000), a large call after a small one, the errors with canaries, the chain from the volume to the deformed mesh on the
device, and the driver's -mt."""
import os

import numpy as np
import pytest

import mesh_driver_cases as drv
import mesh_smooth_cases as cases
from kintinuous_amd import abi, mesh_smooth_ref as ref

pytestmark = pytest.mark.gpu

V = abi.MESH_VERTEX_DTYPE
GUARD = 5
CV, CT, CO = 0xA5A5A5A5, 0x3C3C3C3C, 0x5EEDF00D
L, M = cases.LAMBDA, cases.MU
NONE = (-1, -1, -1)                                   # the stats of a call that left them alone


@pytest.fixture(scope="module")
def smo(ctx):
    w = abi.MeshSmooth(ctx)
    yield w
    w.close()


def _device(ctx, smo, v, tri, steps, lam=L, mu=M, mode=0):
    """kt_mesh_smooth_device on uploads with canaries behind every buffer -> (status, stats, output as left, inputs as left)"""
    n, m = len(v), len(tri)
    dv = ctx.upload(np.concatenate([v.view(np.uint32).reshape(-1), np.full(4 * GUARD, CV, np.uint32)]))
    dt = ctx.upload(np.concatenate([tri.reshape(-1), np.full(3 * GUARD, CT, np.uint32)]))
    do = ctx.upload(np.full(4 * (n + GUARD), CO, np.uint32))
    s, stats = smo.smooth_device(dv, n, dt, m, steps, lam, mu, mode, do)
    out = ctx.download(do, np.uint32, (4 * (n + GUARD),))
    ins = (ctx.download(dv, np.uint32, (4 * (n + GUARD),)), ctx.download(dt, np.uint32, (3 * (m + GUARD),)))
    for b in (dv, dt, do):
        b.free()
    return s, stats, out, ins


def _check_device(ctx, smo, v, tri, steps, mode=0, want=None, lam=L, mu=M):
    n, m = len(v), len(tri)
    wv, ws = ref.smooth(v, tri, steps, lam, mu, mode) if want is None else want
    s, stats, out, (iv, it) = _device(ctx, smo, v, tri, steps, lam, mu, mode)
    assert s == abi.KT_OK and stats == ws
    assert np.array_equal(out[:4 * n], wv.view(np.uint32).reshape(-1))
    assert (out[4 * n:] == CO).all()                                                                  # nothing behind the output
    assert np.array_equal(iv[:4 * n], v.view(np.uint32).reshape(-1)) and (iv[4 * n:] == CV).all()     # the inputs are read only
    assert np.array_equal(it[:3 * m], tri.reshape(-1)) and (it[3 * m:] == CT).all()
    return (wv, ws), out


def _check_both(ctx, smo, v, tri, steps, mode=0, want=None, lam=L, mu=M):
    want, got = _check_device(ctx, smo, v, tri, steps, mode, want, lam, mu)
    _, again = _check_device(ctx, smo, v, tri, steps, mode, want, lam, mu)     # a second call: the same bytes
    assert np.array_equal(got, again)
    s, hv, hs = smo.smooth_host(v, tri, steps, lam, mu, mode)
    assert s == abi.KT_OK and hs == want[1] and len(hv) == len(v)
    assert np.array_equal(cases.as_bytes(hv), cases.as_bytes(want[0]))
    return want


@pytest.mark.parametrize("name", cases.names())
def test_every_case_device_and_host_forms(ctx, smo, name):
    """(the hub of 65535, the largest valence there is, among them)"""
    for offset in cases.OFFSETS:
        v, tri = cases.case(name, offset)
        for mode in cases.MODES:
            for steps in cases.STEPS:
                _check_both(ctx, smo, v, tri, steps, mode, cases.want(name, offset, steps, mode))


@pytest.mark.parametrize("m", cases.SIZES + (70001,))
def test_patches_at_both_offsets(ctx, smo, m):
    import mesh_holes_cases as hc
    for k, offset in enumerate(cases.OFFSETS):
        v, tri, _ = hc.random_case(300 + m + k, m)
        v = cases.moved_to(v, offset)
        for mode in cases.MODES:
            for steps in (1, 10) if m > 4099 else cases.STEPS:
                (wv, ws), _ = _check_device(ctx, smo, v, tri, steps, mode)
                if m >= 257 and steps:                                              # (below that the pinned patches have no interior vertex)
                    assert 0 < ws[1] < len(v) and ws[0] > 0 and ws[2] > m
        _check_both(ctx, smo, v, tri, 2, 1, None, 0.5, 0.5)                         # plain Laplacian smoothing


def test_large_after_small_equals_a_fresh_object(ctx):
    import mesh_holes_cases as hc
    small, large = hc.random_case(1, 65)[:2], hc.random_case(2, 70001)[:2]
    a, b = abi.MeshSmooth(ctx), abi.MeshSmooth(ctx)
    try:
        _check_device(ctx, a, *small, 2)
        want, got = _check_device(ctx, a, *large, 3, 1)
        _, fresh = _check_device(ctx, b, *large, 3, 1, want)
        assert np.array_equal(got, fresh)
        _check_device(ctx, a, *small, 2)                                            # ... and a small one after it
        for case in (small, large):
            x, y = a.smooth(*case, 2), b.smooth(*case, 2)
            assert x[1] == y[1] and np.array_equal(cases.as_bytes(x[0]), cases.as_bytes(y[0]))
    finally:
        a.close()
        b.close()


def test_allocations_return(ctx):
    import mesh_holes_cases as hc
    ctx.sync()
    start = abi.live_allocations()
    w = abi.MeshSmooth(ctx)
    created = abi.live_allocations()[0]
    assert created > start[0]
    _check_device(ctx, w, *hc.random_case(4, 257)[:2], 2)
    device_form = abi.live_allocations()[0]
    assert device_form == created + 7 + 6                             # the per-vertex and the per-half-edge arrays are the object's
    w.smooth(*hc.random_case(4, 257)[:2], 2)
    assert abi.live_allocations()[0] == device_form + 3               # ... and so is the host form's staging
    w.smooth(*hc.random_case(5, 65)[:2], 2)                           # a smaller call takes nothing
    assert abi.live_allocations()[0] == device_form + 3
    w.smooth(*hc.random_case(6, 4099)[:2], 2)                         # a larger one releases and takes again
    assert abi.live_allocations()[0] == device_form + 3
    w.close()
    assert abi.live_allocations() == start


def test_errors_leave_everything_intact(ctx, smo):
    v, tri = cases.case("patch 4099")
    n, m = len(v), len(tri)
    want = cases.want("patch 4099", cases.OFFSETS[0], 2, 0)

    def refused(vb, tb, cause, steps=2, lam=L, mu=M, mode=0):
        with pytest.raises(ValueError, match=cause):
            ref.smooth(vb, tb, steps, lam, mu, mode)
        s, stats, out, (iv, it) = _device(ctx, smo, vb, tb, steps, lam, mu, mode)
        assert s == abi.KT_ERR_ARG and stats == NONE and (out == CO).all()           # the output keeps its pattern in full
        assert np.array_equal(iv[:4 * len(vb)], vb.view(np.uint32).reshape(-1)) and np.array_equal(it[:3 * len(tb)], tb.reshape(-1))
        keep = np.full(len(vb), 7.0, np.float32).repeat(4).view(V)
        s, hv, hs = smo.smooth_host(vb, tb, steps, lam, mu, mode, keep)
        assert s == abi.KT_ERR_ARG and hs == NONE and (hv["xyz"] == 7.0).all()       # ... and so does the host form's
        _check_device(ctx, smo, v, tri, 2, 0, want)                                  # the same object's next valid call is correct

    for row, col in ((0, 0), (m // 2, 1), (m - 1, 2)):                               # an index out of range
        tb = tri.copy()
        tb[row, col] = n if row else 0xffffffff
        refused(v, tb, "index out of range")
    live = np.flatnonzero((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2]))
    loose = np.setdiff1d(np.arange(n), tri)
    for k, (axis, val) in enumerate(((0, float("nan")), (1, float("inf")), (2, 8192.0), (0, -8192.0), (1, float("-inf")))):
        vb = v.copy()                                                                # an invalid vertex that a triangle references
        vb["xyz"][tri[live[17 * k], k % 3], axis] = val
        refused(vb, tri, "not finite or has a coordinate")
        vu = v.copy()                                                                # ... and the same one unreferenced: accepted
        vu["xyz"][loose[-1], axis] = val
        _check_device(ctx, smo, vu, tri, 2)
    for mode in cases.MODES:
        refused(*cases.hub_case(65536), "valence over the bound", mode=mode)         # the hub of 65536
    lv, lt, kw = cases.left_range_case()
    refused(lv, lt, "left the range", **kw)
    _check_both(ctx, smo, lv, lt, 1, 0, None, 0.5, -0.9)                             # ... and one that stays inside
    # sizes over 2^29 with dummy pointers: refused before anything is allocated
    start = abi.live_allocations()
    for nn, mm in (((1 << 29) + 1, 1), (3, (1 << 29) + 1)):
        assert smo.smooth_device(0x10000, nn, 0x20000, mm, 1, L, M, 0, 0x30000) == (abi.KT_ERR_ARG, NONE)
    assert abi.live_allocations() == start
    # null pointers with n > 0, misaligned vertices, an output that is or overlaps an input, bad steps, lambda, mu and mode
    dv, dt = ctx.upload(v), ctx.upload(tri)
    do = ctx.upload(np.full(4 * n, CO, np.uint32))
    good = dict(vertices=dv, n=n, triangles=dt, m=m, steps=2, lam=L, mu=M, mode=0, vertices_out=do)
    nan = float("nan")
    for change in (dict(vertices=None), dict(triangles=None), dict(vertices_out=None), dict(vertices=dv.ptr + 8), dict(vertices_out=do.ptr + 8, n=n - 1),
                   dict(vertices_out=dv), dict(vertices_out=dv.ptr + 16, n=2, m=0), dict(vertices_out=dt), dict(vertices_out=dt.ptr + 16 * (3 * m // 4 - 1)),
                   dict(steps=-1), dict(steps=65), dict(lam=0.0), dict(lam=-0.5), dict(lam=1.0000001), dict(lam=nan), dict(mu=-1.2), dict(mu=1.0000001), dict(mu=nan),
                   dict(mode=2), dict(mode=-1)):
        assert smo.smooth_device(**{**good, **change}) == (abi.KT_ERR_ARG, NONE), change
    assert (ctx.download(do, np.uint32, (4 * n,)) == CO).all()
    assert np.array_equal(ctx.download(dt, np.uint32, (m, 3)), tri) and np.array_equal(ctx.download(dv, V, (n,)).view(np.uint8), v.view(np.uint8))
    assert smo.smooth_device(**good) == (abi.KT_OK, want[1])                         # the object is still usable
    assert np.array_equal(ctx.download(do, V, (n,)).view(np.uint8), want[0].view(np.uint8))
    for change, stats in ((dict(steps=64), None), (dict(lam=1.0, mu=-1.1, steps=1), None), (dict(mu=1.0, steps=1), None), (dict(mode=1), None)):
        kw = {**good, **change}                                                      # the bounds themselves are allowed
        assert smo.smooth_device(**kw) == (abi.KT_OK, ref.smooth(v, tri, kw["steps"], kw["lam"], kw["mu"], kw["mode"])[1]), change
    # n = 0: nothing done; m = 0: the output is the input
    assert smo.smooth_device(None, 0, None, 0, 2, L, M, 0, None) == (abi.KT_OK, (0, 0, 0))
    assert smo.smooth_device(None, 0, dt, m, 2, L, M, 0, None) == (abi.KT_OK, (0, 0, 0))     # (the triangles are not looked at: the restatement's rule)
    assert smo.smooth_device(dv, n, None, 0, 2, L, M, 1, do) == (abi.KT_OK, (0, 0, 0))
    assert np.array_equal(ctx.download(do, V, (n,)).view(np.uint8), v.view(np.uint8))
    for b in (dv, dt, do):
        b.free()


# ---- mesh, weld, holes, smooth, simplify, normals, deform: all on the device ------------------------------------------------------------
def test_chain_on_the_device(ctx, smo):
    """kt_extract_mesh_keyed on the N = 32 sphere's split boxes, kt_mesh_weld_device, kt_mesh_holes_device, kt_mesh_smooth_device,
    kt_mesh_simplify_device at 2 voxels, kt_mesh_normals_device and kt_deform_apply_mesh_device with the 20-node graph of deform_cases,
    the span table of the hole pass unchanged behind the smoothing: every stage equal to its restatement on the stage before"""
    import deform_cases as dc
    import deform_mesh_cases as mc
    import mesh_simplify_cases as sc
    import mesh_weld_cases as wc
    from kintinuous_amd import deform_ref, mesh_holes_ref, mesh_normals_ref, mesh_ref, mesh_simplify_ref, mesh_weld_ref
    N, gname = 32, "m20_n64_c7"
    vol, col = wc.sphere_volume(N)
    dvol, dcol = ctx.upload(vol), ctx.upload(col)
    welder, holes, simp, nrm, g = abi.MeshWeld(ctx), abi.MeshHoles(ctx), abi.MeshSimplify(ctx), abi.MeshNormals(ctx), abi.DeformationGraph(ctx, 20, 8)
    bufs = [dvol, dcol]
    try:
        gc = dc.case(gname)
        g.set_graph(gc["node_pos"], gc["node_time"])
        g.set_state(dc.restated(gname)[0])
        times = np.array([mc.span_times(20)[2], mc.span_times(20)[7]], np.uint64)
        for axis, cut, mode in ((0, 15, 0), (2, 15, 1)):
            boxes = wc.split_boxes(N, axis, cut)[1:]
            parts = [ctx.mesh_keyed(dvol, (3.0, 3.0, 3.0), (0, 0, 0), dcol, lo, hi, (0, 0, 0), N) for lo, hi in boxes]
            for (pv, pt, _), (lo, hi) in zip(parts, boxes):
                rv, rt = mesh_ref.extract_mesh(vol, col, (3.0, 3.0, 3.0), (0, 0, 0), lo, hi, (0, 0, 0), N)
                wc.same((pv, pt), (rv, rt))
            v, k, t, first, _ = wc.concat(*[(p[0], p[1], p[2]) for p in parts])
            n, m = len(v), len(t)
            vcap, tcap = abi.MeshHoles.most(n, m)
            dv, dk, dt = ctx.upload(v), ctx.upload(k), ctx.upload(t)
            wv, wk, fv, ft, tv, sv, st, on = (ctx.empty(16 * n), ctx.empty(8 * n), ctx.empty(16 * vcap), ctx.empty(12 * tcap), ctx.empty(16 * vcap), ctx.empty(16 * vcap),
                                              ctx.empty(12 * tcap), ctx.empty(12 * vcap))
            bufs += [dv, dk, dt, wv, wk, fv, ft, tv, sv, st, on]
            s, nw, wf = welder.weld_device(dv, dk, n, dt, m, first, times, wc.NO_GATE, wv, wk, n)
            rw = mesh_weld_ref.weld(v, k, t, first, times)
            assert s == abi.KT_OK and 0 < nw < n
            wc.same((ctx.download(wv, V, (nw,)), ctx.download(dt, np.uint32, (m, 3)), wf), (rw[0], rw[2], rw[3]))
            s, nf, mf, ff, hstats = holes.holes_device(wv, nw, dt, m, wf, 256, fv, vcap, ft, tcap)
            rh = mesh_holes_ref.holes(rw[0], rw[2], rw[3], 256)
            assert s == abi.KT_OK and hstats == rh[4]
            hv, ht = ctx.download(fv, V, (nf,)), ctx.download(ft, np.uint32, (mf, 3))
            wc.same((hv, ht, ff), rh[:3])
            s, tstats = smo.smooth_device(fv, nf, ft, mf, 5, L, M, mode, tv)
            rs = ref.smooth(hv, ht, 5, L, M, mode)
            assert s == abi.KT_OK and tstats == rs[1] and tstats[1] > nf // 2
            smoothed = ctx.download(tv, V, (nf,))
            wc.same((smoothed,), (rs[0],))
            assert np.array_equal(ctx.download(ft, np.uint32, (mf, 3)), ht)                       # the triangles are untouched
            cell = 2 * sc.VOXEL
            s, ns, ms, sf = simp.simplify_device(tv, nf, ft, mf, ff, cell, sv, vcap, st, tcap)
            assert s == abi.KT_OK and 0 < ns < nf and 0 < ms < mf
            wc.same((ctx.download(sv, V, (ns,)), ctx.download(st, np.uint32, (ms, 3)), sf), mesh_simplify_ref.simplify(smoothed, ht, ff, cell))
            s, n_zero = nrm.normals_device(tv, nf, ft, mf, on)
            wn, wz = mesh_normals_ref.normals(smoothed, ht)
            assert s == abi.KT_OK and n_zero == wz and np.array_equal(ctx.download(on, np.float32, (nf, 3)).view(np.uint8), wn.view(np.uint8))
            g.apply_mesh_device(tv, nf, ff, times)
            moved = ctx.download(tv, V, (nf,))
            assert moved.tobytes() == deform_ref.apply_mesh(dc.graph(gname), dc.restated(gname)[0], smoothed, ff, times).tobytes()
            assert np.abs(moved["xyz"] - smoothed["xyz"]).max() > 0
    finally:
        g.close()
        nrm.close()
        simp.close()
        holes.close()
        welder.close()
        for b in bufs:
            b.free()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def _rgb24(v):
    return v["rgb"][:, 0].astype(np.uint32) << 16 | v["rgb"][:, 1].astype(np.uint32) << 8 | v["rgb"][:, 2].astype(np.uint32)


def _smooth_file(prefix):
    """<prefix>.smooth -> (n, m, steps, lambda, mu, mode, rim, moved, edges)"""
    lines = open(prefix + ".smooth").read().splitlines()
    f = lines[0].split()
    assert len(lines) == 1 and f[0] == "result" and len(f) == 10
    return tuple(int(x) for x in f[1:4]) + (float.fromhex(f[4]), float.fromhex(f[5])) + tuple(int(x) for x in f[6:])


def _driver_smooth_is_the_restatements(prefix, source, steps, mode):
    """<prefix>_smooth.ply and <prefix>.smooth against the restatement on what <prefix><source>.ply holds -> the smoothed arrays.  The .ply
    keeps three colour bytes of four, which the pass only copies"""
    import deform_mesh_cases as mc
    v, tri = mc.read_ply(prefix + source + ".ply")
    sv, stri = mc.read_ply(prefix + "_smooth.ply")
    full = np.zeros(len(v), V)
    full["xyz"], full["rgb"] = v["xyz"], _rgb24(v)
    want, stats = ref.smooth(full, tri.astype(np.uint32), steps, L, M, mode)
    assert _smooth_file(prefix) == (len(v), len(tri), steps, float(np.float32(L)), float(np.float32(M)), mode) + stats
    assert np.array_equal(tri, stri) and len(tri) > 0 and sv["rgb"].tobytes() == v["rgb"].tobytes()
    assert np.ascontiguousarray(sv["xyz"]).tobytes() == np.ascontiguousarray(want["xyz"]).tobytes()
    assert stats[1] > 0 and (sv["xyz"] != v["xyz"]).any()
    return want, tri.astype(np.uint32), stats


def test_driver_mt_on_the_welded_crab_walk(tmp_path):
    """kintinuous_hip -m -mw -mt 5 on the out-and-back crab-walk of tests/test_gpu_mesh_holes.py's driver test: _smooth.ply and .smooth are
    the restatement applied to _weld.ply, every file of the run without -mt is byte-identical; -mtb moves the rims; -mt -ms feeds the
    smoothed mesh; -mt -mn gives the smoothed file the normals of its own arrays; -mt without -m, -mt 65 and -mtb alone are ignored with a
    message"""
    import mesh_normals_cases as nc
    from kintinuous_amd import mesh_normals_ref
    run = drv.crab_walk_driver(tmp_path)

    rd = lambda p: open(p, "rb").read()
    _, p0 = run("plain", "-m", "-mw")
    out, p1 = run("smooth", "-m", "-mw", "-mt", "5")
    assert drv.outputs(tmp_path, p1) == sorted(drv.outputs(tmp_path, p0) + [".smooth", "_smooth.ply"])
    for ext in drv.outputs(tmp_path, p0):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    want, tri, stats = _driver_smooth_is_the_restatements(p1, "_weld", 5, 0)
    print("crab-walk -mt 5: %d vertices, %d triangles, %d rim vertices, %d moved, %d edges" % ((len(want), len(tri)) + stats))
    assert len([l for l in out.stdout.splitlines() if l.startswith("mesh ") and "_smooth.ply:" in l]) == 1
    # -mtb: the rims move along themselves
    _, p2 = run("rim", "-m", "-mw", "-mt", "5", "-mtb")
    _, _, stats_b = _driver_smooth_is_the_restatements(p2, "_weld", 5, 1)
    assert stats_b[0] == stats[0] and (stats_b[1] > stats[1] or stats[0] == 0)
    # -mt -ms: the simplification takes the smoothed mesh
    _, p3 = run("both", "-m", "-mw", "-mt", "5", "-ms", "0.05")
    assert drv.outputs(tmp_path, p3) == sorted(drv.outputs(tmp_path, p1) + [".simp", "_simp.ply"])
    for ext in drv.outputs(tmp_path, p1):
        assert rd(p1 + ext) == rd(p3 + ext), ext
    _, p3b = run("simp", "-m", "-mw", "-ms", "0.05")
    simp_result, plain_result = [open(p + ".simp").read().splitlines()[-1].split() for p in (p3, p3b)]
    assert simp_result[0] == "result" and (int(simp_result[1]), int(simp_result[3])) == (len(want), len(tri))
    assert rd(p3 + "_simp.ply") != rd(p3b + "_simp.ply") and plain_result[1] == simp_result[1]        # ... the same counts in, other vertices out
    # -mt -mn: rows of 27 bytes, the normals of the smoothed arrays
    _, p4 = run("nrm", "-m", "-mw", "-mt", "5", "-mn")
    nv, nf = nc.read_ply_normals(p4 + "_smooth.ply")
    assert np.ascontiguousarray(nv["xyz"]).tobytes() == np.ascontiguousarray(want["xyz"]).tobytes() and np.array_equal(nf.astype(np.uint32), tri)
    wn, n_zero = mesh_normals_ref.normals(want, tri)
    assert np.ascontiguousarray(nv["normal"]).tobytes() == wn.tobytes()
    listed = {l.split()[0]: tuple(int(x) for x in l.split()[1:]) for l in open(p4 + ".normals").read().splitlines()}
    assert listed[os.path.basename(p4) + "_smooth.ply"] == (len(want), len(tri), n_zero)
    # ignored with a message
    nomesh, p5 = run("nomesh", "-mt", "5")
    assert "-mt ignored without -m" in nomesh.stderr and not [e for e in drv.outputs(tmp_path, p5) if "smooth" in e or e.endswith(".ply")]
    big, p6 = run("big", "-m", "-mw", "-mt", "65")
    assert "-mt ignored" in big.stderr and drv.outputs(tmp_path, p6) == drv.outputs(tmp_path, p0)
    alone, p7 = run("alone", "-m", "-mw", "-mtb")
    assert "-mtb ignored without -mt" in alone.stderr and drv.outputs(tmp_path, p7) == drv.outputs(tmp_path, p0)


def test_driver_mt_with_df_on_the_loop_log(tmp_path):
    """kintinuous_hip ... -lc -pg -pcd -df -m -mt 5 on the ten-frame walk of tests/test_gpu_deform_mesh.py's driver test: _smooth.ply is the
    restatement's smoothing of .ply; _smooth_def.ply has _smooth.ply's faces and colours and its vertices where the deformation's
    restatement puts them, from the run's own .deform, whose mesh lines are the span table the smoothing left alone (the rule of
    test_gpu_mesh_holes.py for _fill_def.ply: every float the restatement's or its neighbour); every file of the run without -mt is
    byte-identical."""
    import deform_cases as dc
    import deform_mesh_cases as mc
    from kintinuous_amd import deform_ref
    run = drv.loop_log_driver(tmp_path)

    _, p0 = run("plain", "-m")
    _, p1 = run("smooth", "-m", "-mt", "5")
    rd = lambda p: open(p, "rb").read()
    assert drv.outputs(tmp_path, p1) == sorted(drv.outputs(tmp_path, p0) + [".smooth", "_smooth.ply", "_smooth_def.ply"])
    for ext in drv.outputs(tmp_path, p0):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    _driver_smooth_is_the_restatements(p1, "", 5, 0)
    before, faces = mc.read_ply(p1 + "_smooth.ply")
    after, faces_after = mc.read_ply(p1 + "_smooth_def.ply")
    assert np.array_equal(faces, faces_after) and len(faces) > 0 and len(before) == len(after) and before["rgb"].tobytes() == after["rgb"].tobytes()
    d = mc.deform_file(open(p1 + ".deform").read())
    pose_t = [p[0] for p in d["pose"]]
    orig = np.array([p[1:4] for p in d["pose"]], np.float32)
    keep = deform_ref.sample_nodes(orig, 0.02)
    graph = deform_ref.Graph(orig[keep], np.array([pose_t[k] for k in keep], np.uint64))
    src = np.array([c[1:4] for c in d["con"]], np.float32)
    x, _, _, _, _, status, _ = deform_ref.optimise(graph, src, np.array([c[0] for c in d["con"]], np.uint64), np.array([c[4:7] for c in d["con"]]), {"significant_error": 1e-9})
    assert status in (deform_ref.CONVERGED, deform_ref.MAX_STEPS)
    first = np.concatenate([[0], np.cumsum([c for _, c in d["mesh"]])]).astype(np.int64)
    assert first[-1] == len(before)
    v = np.zeros(len(before), V)
    v["xyz"] = before["xyz"]
    want = deform_ref.apply_mesh(graph, x, v, first, [t for t, _ in d["mesh"]])
    got, wanted_xyz = after["xyz"].reshape(-1), want["xyz"].reshape(-1)
    near = (got == wanted_xyz) | (got == np.nextafter(wanted_xyz, np.float32(np.inf))) | (got == np.nextafter(wanted_xyz, np.float32(-np.inf)))
    near |= np.abs(got.astype(np.float64) - wanted_xyz.astype(np.float64)) <= 10 * dc.BOUND * (1.0 + float(np.abs(before["xyz"]).max()))
    assert near.all() and np.abs(after["xyz"] - before["xyz"]).max() > 0                   # ... and it was deformed
