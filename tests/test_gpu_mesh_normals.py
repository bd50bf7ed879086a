"""GPU: the vertex normals of the -m mesh (kt_mesh_normals.hip) -- kt_mesh_normals_device and kt_mesh_normals byte for byte against
kintinuous_amd/mesh_normals_ref.py on random triangle lists, fans whose atomics all land on one vertex, cancelling pairs, a large call
after a small one, the errors with canaries, the sphere's split boxes meshed, welded, simplified and deformed on the device, and the
driver's -mn."""
import os

import numpy as np
import pytest

import mesh_driver_cases as drv
import mesh_normals_cases as cases
import mesh_weld_cases as wc
from kintinuous_amd import abi, mesh_normals_ref as ref

pytestmark = pytest.mark.gpu

V = abi.MESH_VERTEX_DTYPE
GUARD = 5
CV, CT, CN = 0xA5A5A5A5, 0x3C3C3C3C, 0x5EEDF00D


@pytest.fixture(scope="module")
def nrm(ctx):
    w = abi.MeshNormals(ctx)
    yield w
    w.close()


def _device(ctx, nrm, v, tri):
    """kt_mesh_normals_device on uploads with canaries behind every buffer -> (status, n_zero, output as left, inputs as left)"""
    n, m = len(v), len(tri)
    dv = ctx.upload(np.concatenate([v.view(np.uint32).reshape(-1), np.full(4 * GUARD, CV, np.uint32)]))
    dt = ctx.upload(np.concatenate([tri.reshape(-1), np.full(3 * GUARD, CT, np.uint32)]))
    on = ctx.upload(np.full(3 * (n + GUARD), CN, np.uint32))
    s, n_zero = nrm.normals_device(dv, n, dt, m, on)
    out = ctx.download(on, np.uint32, (3 * (n + GUARD),))
    ins = (ctx.download(dv, np.uint32, (4 * (n + GUARD),)), ctx.download(dt, np.uint32, (3 * (m + GUARD),)))
    for b in (dv, dt, on):
        b.free()
    return s, n_zero, out, ins


def _check_device(ctx, nrm, v, tri, want=None):
    n, m = len(v), len(tri)
    wn, wz = ref.normals(v, tri) if want is None else want
    s, n_zero, out, (iv, it) = _device(ctx, nrm, v, tri)
    assert s == abi.KT_OK and n_zero == wz
    assert np.array_equal(out[:3 * n], wn.view(np.uint32).reshape(-1))
    assert (out[3 * n:] == CN).all()                                                                  # nothing behind the output
    assert np.array_equal(iv[:4 * n], v.view(np.uint32).reshape(-1)) and (iv[4 * n:] == CV).all()     # the inputs are read only
    assert np.array_equal(it[:3 * m], tri.reshape(-1)) and (it[3 * m:] == CT).all()
    return (wn, wz), out


def _check_both(ctx, nrm, v, tri):
    want, got = _check_device(ctx, nrm, v, tri)
    _, again = _check_device(ctx, nrm, v, tri, want)                       # a second call: the same bytes
    assert np.array_equal(got, again)
    s, hn, hz = nrm.normals_host(v, tri)
    assert s == abi.KT_OK and hz == want[1] and len(hn) == len(v)
    assert np.array_equal(cases.as_bytes(hn), cases.as_bytes(want[0]))
    return want


@pytest.mark.parametrize("m", cases.TRIANGLE_COUNTS)
def test_lists_device_and_host_forms(ctx, nrm, m):
    for k, offset in enumerate(cases.OFFSETS):
        v, tri = cases.random_case(100 * m + k, m, offset)
        wn, wz = _check_both(ctx, nrm, v, tri)
        if m >= 63:
            assert 4 <= wz < len(v)


@pytest.mark.parametrize("k", cases.FAN_SIZES)
def test_contention_on_one_hub(ctx, nrm, k):
    v, tri = cases.fan_case(k)
    wn, wz = _check_both(ctx, nrm, v, tri)
    assert wz == 0 and wn[0].any()


def test_cancellation_and_a_sliver(ctx, nrm):
    v, tri = cases.cancelling_case()
    wn, wz = _check_both(ctx, nrm, v, tri)
    assert wz == len(v) and not wn.any()
    v, tri = cases.sphere_mesh()
    _check_both(ctx, nrm, v, tri)


def test_large_after_small_equals_a_fresh_object(ctx):
    small, large = cases.random_case(1, 65), cases.random_case(2, 70001, cases.OFFSETS[1])
    a, b = abi.MeshNormals(ctx), abi.MeshNormals(ctx)
    try:
        _check_device(ctx, a, *small)
        want, got = _check_device(ctx, a, *large)
        _, fresh = _check_device(ctx, b, *large, want)
        assert np.array_equal(got, fresh)
        _check_device(ctx, a, *small)                                       # ... and a small one after it
        for case in (small, large):
            x, y = a.normals(*case), b.normals(*case)
            assert x[1] == y[1] == ref.normals(*case)[1] and np.array_equal(cases.as_bytes(x[0]), cases.as_bytes(y[0]))
    finally:
        a.close()
        b.close()


def test_errors_leave_everything_intact(ctx, nrm):
    v, tri = cases.random_case(9, 4099)
    n, m = len(v), len(tri)
    want = ref.normals(v, tri)

    def refused(vb, tb):
        with pytest.raises(ValueError):
            ref.normals(vb, tb)
        s, n_zero, out, (iv, it) = _device(ctx, nrm, vb, tb)
        assert s == abi.KT_ERR_ARG and n_zero == 0 and (out == CN).all()             # the output keeps its pattern in full
        assert np.array_equal(iv[:4 * len(vb)], vb.view(np.uint32).reshape(-1)) and np.array_equal(it[:3 * len(tb)], tb.reshape(-1))
        keep = np.full(len(vb), 7.0, np.float32).repeat(3).view(abi.MESH_NORMAL_DTYPE)
        s, hn, hz = nrm.normals_host(vb, tb, keep)
        assert s == abi.KT_ERR_ARG and hz == 0 and (hn["normal"] == 7.0).all()       # ... and so does the host form's
        _check_device(ctx, nrm, v, tri, want)                                        # the same object's next valid call is correct

    for row, col in ((0, 0), (m // 2, 1), (m - 1, 2)):                               # an index out of range
        tb = tri.copy()
        tb[row, col] = n if row else 0xffffffff
        refused(v, tb)
    live = np.flatnonzero((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2]))
    for k, (axis, val) in enumerate(((0, float("nan")), (1, float("inf")), (2, 8192.0), (0, -8192.0), (1, float("-inf")))):
        vb = v.copy()                                                                # an invalid vertex that a triangle references
        vb["xyz"][tri[live[17 * k], k % 3], axis] = val
        refused(vb, tri)
        vu = v.copy()                                                                # ... and the same one unreferenced: accepted
        vu["xyz"][n - 3, axis] = val
        _check_device(ctx, nrm, vu, tri)
    one = np.array([[0, 1, 2]], np.uint32)                                           # legs 1 and 1: a cross component of exactly 1.0
    big = np.zeros(3, V)
    big["xyz"] = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]
    refused(big, one)
    refused(np.concatenate([v, big]), np.concatenate([tri, one + np.uint32(n)]))
    big["xyz"][2, 1] = np.nextafter(np.float32(1.0), np.float32(0.0))                # legs 1 and nextafter(1, 0): accepted
    _check_both(ctx, nrm, big, one)
    # sizes over 2^29 with dummy pointers: refused before anything is allocated
    start = abi.live_allocations()
    for nn, mm in (((1 << 29) + 1, 1), (3, (1 << 29) + 1)):
        assert nrm.normals_device(0x10000, nn, 0x20000, mm, 0x30000) == (abi.KT_ERR_ARG, 0)
    assert abi.live_allocations() == start
    # null pointers with n > 0, misaligned vertices, an output that overlaps an input
    dv, dt = ctx.upload(v), ctx.upload(tri)
    on = ctx.upload(np.full(3 * n, CN, np.uint32))
    good = dict(vertices=dv, n=n, triangles=dt, m=m, normals_out=on)
    for change in (dict(vertices=None), dict(triangles=None), dict(normals_out=None), dict(vertices=dv.ptr + 8), dict(normals_out=dv), dict(normals_out=dv.ptr + 16 * n - 4),
                   dict(normals_out=dt), dict(normals_out=dt.ptr + 12 * m - 4), dict(vertices=on.ptr, n=1, m=0, normals_out=on.ptr + 4)):
        assert nrm.normals_device(**{**good, **change}) == (abi.KT_ERR_ARG, 0), change
    assert (ctx.download(on, np.uint32, (3 * n,)) == CN).all()
    assert np.array_equal(ctx.download(dt, np.uint32, (m, 3)), tri) and np.array_equal(ctx.download(dv, V, (n,)).view(np.uint8), v.view(np.uint8))
    assert nrm.normals_device(**good) == (abi.KT_OK, want[1])                            # the object is still usable
    assert np.array_equal(ctx.download(on, np.float32, (n, 3)).view(np.uint8), want[0].view(np.uint8))
    # n = 0 and m = 0: KT_OK, all normals zero
    assert nrm.normals_device(None, 0, None, 0, None) == (abi.KT_OK, 0)
    assert nrm.normals_device(None, 0, dt, m, None) == (abi.KT_OK, 0)                    # (the triangles are not looked at: the restatement's rule)
    assert ref.normals(v[:0], tri)[0].shape == (0, 3) and ref.normals(v[:0], tri)[1] == 0
    assert nrm.normals_device(dv, n, None, 0, on) == (abi.KT_OK, n)
    assert not ctx.download(on, np.uint32, (3 * n,)).any()
    for b in (dv, dt, on):
        b.free()


def test_allocations_return(ctx):
    ctx.sync()
    start = abi.live_allocations()
    w = abi.MeshNormals(ctx)
    created = abi.live_allocations()[0]
    assert created > start[0]
    _check_device(ctx, w, *cases.random_case(4, 257))
    device_form = abi.live_allocations()[0]
    assert device_form == created + 1                                 # the sums are the object's
    w.normals(*cases.random_case(4, 257))
    assert abi.live_allocations()[0] == device_form + 3               # ... and so is the host form's staging
    w.normals(*cases.random_case(5, 65))                              # a smaller call takes nothing
    assert abi.live_allocations()[0] == device_form + 3
    w.normals(*cases.random_case(6, 4099))                            # a larger one releases and takes again
    assert abi.live_allocations()[0] == device_form + 3
    w.close()
    assert abi.live_allocations() == start


# ---- mesh, weld, simplify, normals, deform, normals: all on the device --------------------------------------------------------------------
def test_pipeline_on_the_device(ctx, nrm):
    """kt_extract_mesh_keyed on the N = 32 sphere's split boxes, kt_mesh_weld_device, kt_mesh_simplify_device at 2 voxels,
    kt_mesh_normals_device: the restatement's normals of the downloaded arrays; then kt_deform_apply_mesh_device with the 20-node graph of
    deform_cases in place and the normals again, of the moved vertices"""
    import deform_cases as dc
    import deform_mesh_cases as mc
    import mesh_simplify_cases as sc
    N, gname = 32, "m20_n64_c7"
    vol, col = wc.sphere_volume(N)
    dvol, dcol = ctx.upload(vol), ctx.upload(col)
    welder, simp, g = abi.MeshWeld(ctx), abi.MeshSimplify(ctx), abi.DeformationGraph(ctx, 20, 8)
    bufs = [dvol, dcol]
    try:
        gc = dc.case(gname)
        g.set_graph(gc["node_pos"], gc["node_time"])
        g.set_state(dc.restated(gname)[0])
        times = np.array([mc.span_times(20)[2], mc.span_times(20)[7]], np.uint64)
        for axis, cut in ((0, 15), (2, 15)):
            parts = [ctx.mesh_keyed(dvol, (3.0, 3.0, 3.0), (0, 0, 0), dcol, lo, hi, (0, 0, 0), N) for lo, hi in wc.split_boxes(N, axis, cut)[1:]]
            v, k, t, first, _ = wc.concat(*[(p[0], p[1], p[2]) for p in parts])
            n, m = len(v), len(t)
            dv, dk, dt = ctx.upload(v), ctx.upload(k), ctx.upload(t)
            wv, wk, sv, st, on = ctx.empty(16 * n), ctx.empty(8 * n), ctx.empty(16 * n), ctx.empty(12 * m), ctx.empty(12 * n)
            bufs += [dv, dk, dt, wv, wk, sv, st, on]
            s, nw, wf = welder.weld_device(dv, dk, n, dt, m, first, times, wc.NO_GATE, wv, wk, n)
            assert s == abi.KT_OK and 0 < nw < n
            s, ns, ms, sf = simp.simplify_device(wv, nw, dt, m, wf, 2 * sc.VOXEL, sv, n, st, m)
            assert s == abi.KT_OK and 0 < ns < nw and 0 < ms < m
            s, n_zero = nrm.normals_device(sv, ns, st, ms, on)
            hv, ht = ctx.download(sv, V, (ns,)), ctx.download(st, np.uint32, (ms, 3))
            want = ref.normals(hv, ht)
            assert s == abi.KT_OK and n_zero == want[1]
            assert np.array_equal(ctx.download(on, np.float32, (ns, 3)).view(np.uint8), want[0].view(np.uint8))
            out = hv["xyz"].astype(np.float64) - cases.SPHERE_CENTRE                     # ... and they still point away from the centre
            assert ((want[0] * out).sum(axis=1)[want[0].any(axis=1)] > 0).all()
            g.apply_mesh_device(sv, ns, sf, times)
            s, n_zero = nrm.normals_device(sv, ns, st, ms, on)
            moved = ctx.download(sv, V, (ns,))
            assert np.abs(moved["xyz"] - hv["xyz"]).max() > 0
            want2 = ref.normals(moved, ht)
            assert s == abi.KT_OK and n_zero == want2[1]
            got2 = ctx.download(on, np.float32, (ns, 3))
            assert np.array_equal(got2.view(np.uint8), want2[0].view(np.uint8)) and not np.array_equal(got2, want[0])
    finally:
        g.close()
        simp.close()
        welder.close()
        for b in bufs:
            b.free()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def _driver_files_carry_normals(tmp_path, p0, p1, plys):
    """p0: the run without -mn, p1: the run with it.  Every .ply of p1 has 27-byte rows whose positions, colours and faces are p0's file's
    and whose normals are the restatement's of that file's own arrays; <p1>.normals has one line per .ply with its counts; p0 wrote no
    .normals; everything else is byte-identical"""
    import deform_mesh_cases as mc
    rd = lambda p: open(p, "rb").read()
    exts0, exts1 = drv.outputs(tmp_path, p0), drv.outputs(tmp_path, p1)
    assert exts1 == sorted(exts0 + [".normals"]) and ".normals" not in exts0
    assert sorted(e for e in exts1 if e.endswith(".ply")) == sorted(plys)
    lines = [l.split() for l in open(p1 + ".normals").read().splitlines()]
    assert sorted(l[0] for l in lines) == sorted(os.path.basename(p1) + e for e in plys) and all(len(l) == 4 for l in lines)
    listed = {l[0]: tuple(int(x) for x in l[1:]) for l in lines}
    for ext in exts0:
        if not ext.endswith(".ply"):
            assert rd(p0 + ext) == rd(p1 + ext), ext
            continue
        v0, f0 = mc.read_ply(p0 + ext)
        v1, f1 = cases.read_ply_normals(p1 + ext)
        assert len(v0) == len(v1) > 0 and len(f0) > 0
        assert v0["xyz"].tobytes() == v1["xyz"].tobytes() and v0["rgb"].tobytes() == v1["rgb"].tobytes() and np.array_equal(f0, f1)
        full = np.zeros(len(v1), V)
        full["xyz"] = v1["xyz"]
        want, n_zero = ref.normals(full, f1.astype(np.uint32))
        assert np.ascontiguousarray(v1["normal"]).tobytes() == want.tobytes()
        assert listed[os.path.basename(p1) + ext] == (len(v1), len(f1), n_zero)
        print("%s: %d vertices, %d triangles, %d zero normals" % (ext, len(v1), len(f1), n_zero))


def test_driver_mn_on_the_welded_crab_walk(tmp_path):
    """kintinuous_hip -m -mw -ms 0.15 on the out-and-back crab-walk of tests/test_gpu_mesh_weld.py, with and without -mn; -mn without -m is
    ignored with a message"""
    run = drv.crab_walk_driver(tmp_path)

    _, p0 = run("plain", "-m", "-mw", "-ms", "0.15")
    _, p1 = run("nrm", "-m", "-mw", "-ms", "0.15", "-mn")
    nomesh, p2 = run("nomesh", "-mn")
    _driver_files_carry_normals(tmp_path, p0, p1, [".ply", "_weld.ply", "_simp.ply"])
    assert "-mn ignored without -m" in nomesh.stderr and not [e for e in drv.outputs(tmp_path, p2) if "normals" in e or e.endswith(".ply")]


def test_driver_mn_with_df_on_the_loop_log(tmp_path):
    """kintinuous_hip ... -lc -pg -pcd -df -m -mw -ms 0.05 on the ten-frame walk of tests/test_gpu_deform_mesh.py's driver test, with and
    without -mn: all six .ply files carry the normals of their own arrays, the deformed ones after the deformation"""
    run = drv.loop_log_driver(tmp_path)

    _, p0 = run("plain", "-m", "-mw", "-ms", "0.05")
    _, p1 = run("nrm", "-m", "-mw", "-ms", "0.05", "-mn")
    _driver_files_carry_normals(tmp_path, p0, p1, [".ply", "_weld.ply", "_simp.ply", "_def.ply", "_weld_def.ply", "_simp_def.ply"])
    import deform_mesh_cases as mc
    assert np.abs(mc.read_ply(p0 + "_def.ply")[0]["xyz"] - mc.read_ply(p0 + ".ply")[0]["xyz"]).max() > 0      # ... and it was deformed
    a, b = cases.read_ply_normals(p1 + ".ply")[0]["normal"], cases.read_ply_normals(p1 + "_def.ply")[0]["normal"]
    assert not np.array_equal(a, b)
