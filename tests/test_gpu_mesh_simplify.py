"""GPU: the simplification of the -m mesh by vertex clustering (kt_mesh_simplify.hip) -- kt_mesh_simplify_device and kt_mesh_simplify byte
for byte against kintinuous_amd/mesh_simplify_ref.py on synthetic lists, clusters that cross a wave, a workgroup and the head pass's
chunk, the sphere's split boxes meshed, welded and simplified on the device, the simplified mesh through kt_deform_apply_mesh, and the
driver's -ms."""
import numpy as np
import pytest

import mesh_driver_cases as drv
import mesh_simplify_cases as cases
import mesh_weld_cases as wc
from kintinuous_amd import abi, mesh_simplify_ref as ref

pytestmark = pytest.mark.gpu

V = abi.MESH_VERTEX_DTYPE
GUARD = 5
CV, CT = 0xA5A5A5A5, 0x3C3C3C3C


@pytest.fixture(scope="module")
def simp(ctx):
    w = abi.MeshSimplify(ctx)
    yield w
    w.close()


def _device(ctx, simp, case, vcap=None, tcap=None):
    """kt_mesh_simplify_device on uploads with canaries behind every buffer -> (status, n_out, m_out, span_first_out, outputs as left,
    inputs as left)"""
    v, tri, first, cell = case
    n, m = len(v), len(tri)
    vcap = n if vcap is None else vcap
    tcap = m if tcap is None else tcap
    dv = ctx.upload(np.concatenate([v.view(np.uint32).reshape(-1), np.full(4 * GUARD, CV, np.uint32)]))
    dt = ctx.upload(np.concatenate([tri.reshape(-1), np.full(3 * GUARD, CT, np.uint32)]))
    ov = ctx.upload(np.full(4 * (vcap + GUARD), CV, np.uint32))
    ot = ctx.upload(np.full(3 * (tcap + GUARD), CT, np.uint32))
    s, n_out, m_out, fo = simp.simplify_device(dv, n, dt, m, first, cell, ov, vcap, ot, tcap)
    out = (ctx.download(ov, np.uint32, (4 * (vcap + GUARD),)), ctx.download(ot, np.uint32, (3 * (tcap + GUARD),)))
    ins = (ctx.download(dv, np.uint32, (4 * (n + GUARD),)), ctx.download(dt, np.uint32, (3 * (m + GUARD),)))
    for b in (dv, dt, ov, ot):
        b.free()
    return s, n_out, m_out, fo, out, ins


def _check_device(ctx, simp, case, want=None):
    v, tri, first, cell = case
    n, m = len(v), len(tri)
    wv, wt, wf = ref.simplify(*case) if want is None else want
    s, n_out, m_out, fo, (ov, ot), (iv, it) = _device(ctx, simp, case)
    assert s == abi.KT_OK and (n_out, m_out) == (len(wv), len(wt))
    assert np.array_equal(ov[:4 * n_out], wv.view(np.uint32).reshape(-1)) and np.array_equal(ot[:3 * m_out], wt.reshape(-1)) and np.array_equal(fo, wf)
    assert (ov[4 * n_out:] == CV).all() and (ot[3 * m_out:] == CT).all()                              # nothing behind the outputs
    assert np.array_equal(iv[:4 * n], v.view(np.uint32).reshape(-1)) and (iv[4 * n:] == CV).all()     # the inputs are read only
    assert np.array_equal(it[:3 * m], tri.reshape(-1)) and (it[3 * m:] == CT).all()
    return (wv, wt, wf), (ov, ot, fo)


def _check_both(ctx, simp, case):
    want, got = _check_device(ctx, simp, case)
    _, again = _check_device(ctx, simp, case, want)                       # a second call: the same bytes
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    s, hv, ht, hf, n_out, m_out = simp.simplify_host(*case)
    assert s == abi.KT_OK and (n_out, m_out) == (len(want[0]), len(want[1]))
    cases.same((hv, ht, hf), want)
    return want


@pytest.mark.parametrize("n", cases.SIZES)
def test_lists_device_and_host_forms(ctx, simp, n):
    for seed, spans, cell, per in ((n, 6, 0.25, 3.0), (n + 1, 9, 0.5, 1.0), (n + 2, 1, 0.25, 20.0), (n + 3, 40, 0.125, 4.0)):
        want = _check_both(ctx, simp, cases.random_case(seed, n, spans, cell, per))
        if n >= 257:
            assert 0 < len(want[0]) < n and 0 < len(want[1]) < 2 * n


def test_cluster_sizes_one_cluster_and_a_table_beyond_lds(ctx, simp):
    """clusters of 1, 2, 63, 64, 65, 257 and 2049 members (across a wave, a workgroup and the head pass's 2048 entries); all 70001 vertices
    in one cluster; a table of 3000 spans, searched in global memory"""
    case = cases.sized_clusters_case()
    sizes = np.bincount(ref.cluster_of(case[0]["xyz"], case[2], case[3]))
    assert sorted(sizes.tolist()) == sorted(list(cases.CLUSTER_SIZES) * 3)
    _check_both(ctx, simp, case)
    want = _check_both(ctx, simp, cases.one_cluster_case())
    assert len(want[0]) == 1 and len(want[1]) == 0
    case = cases.many_spans_case()
    want = _check_both(ctx, simp, case)
    assert len(want[0]) > len(np.unique(ref.cell_keys(case[0]["xyz"], case[3])))


def test_p1_small_cell_returns_the_input(ctx, simp):
    v, t = cases.sphere_mesh()
    out = simp.simplify(v, t, [0, len(v)], 1e-4)
    cases.same(out, (v, t, np.array([0, len(v)], np.int64)))


def test_large_after_small_equals_a_fresh_object(ctx):
    small, large = cases.random_case(1, 65), cases.random_case(2, 70001, 40, 0.125, 4.0)
    a, b = abi.MeshSimplify(ctx), abi.MeshSimplify(ctx)
    try:
        _check_device(ctx, a, small)
        want, got = _check_device(ctx, a, large)
        _, fresh = _check_device(ctx, b, large, want)
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh))
        cases.same(a.simplify(*small), ref.simplify(*small))               # ... and a small one after it
        cases.same(a.simplify(*large), b.simplify(*large))
    finally:
        a.close()
        b.close()


def test_errors_leave_everything_intact(ctx, simp):
    case = cases.random_case(9, 4099, 6, 0.25, 3.0)
    v, tri, first, cell = case
    n, m = len(v), len(tri)
    want = ref.simplify(*case)
    n_keep, m_keep = len(want[0]), len(want[1])
    assert 0 < n_keep < n and 0 < m_keep < m

    def intact(res):
        _, _, _, fo, (ov, ot), (iv, it) = res
        assert (ov == CV).all() and (ot == CT).all()
        assert np.array_equal(iv[:4 * n], v.view(np.uint32).reshape(-1)) and np.array_equal(it[:3 * m], tri.reshape(-1))
        assert (fo == -1).all()                                                        # span_first_out untouched as well

    for vcap, tcap in ((n_keep - 1, m), (n, m_keep - 1), (n_keep - 1, m_keep - 1), (0, 0)):
        res = _device(ctx, simp, case, vcap=vcap, tcap=tcap)
        assert res[0] == abi.KT_ERR_CAPACITY and res[1:3] == (n_keep, m_keep)          # both true counts
        intact(res)
    res = _device(ctx, simp, case, vcap=n_keep, tcap=m_keep)                           # the smallest that fit
    assert res[0] == abi.KT_OK and res[1:3] == (n_keep, m_keep)
    for f in (np.array([1] + first[1:].tolist()), np.array(first[:-1].tolist() + [n - 1]), np.array([0, 9, 5] + first[3:].tolist())):
        res = _device(ctx, simp, (v, tri, f, cell))
        assert res[0] == abi.KT_ERR_ARG
        intact(res)
    for bad in (0.0, -0.25, float("inf"), float("-inf"), float("nan")):
        res = _device(ctx, simp, (v, tri, first, bad))
        assert res[0] == abi.KT_ERR_ARG
        intact(res)
        s, hv, ht, hf, _, _ = simp.simplify_host(v, tri, first, bad)
        assert s == abi.KT_ERR_ARG and not hv.view(np.uint32).any() and not ht.any() and (hf == -1).all()
    # an invalid vertex: found on the device
    for pos, axis, val in ((0, 0, float("nan")), (n // 2, 1, float("inf")), (n - 1, 2, 8192.0), (7, 0, -8192.0), (n - 2, 1, float("-inf"))):
        vb = v.copy()
        vb["xyz"][pos, axis] = val
        with pytest.raises(ValueError):
            ref.simplify(vb, tri, first, cell)
        res = _device(ctx, simp, (vb, tri, first, cell))
        assert res[0] == abi.KT_ERR_ARG
        _, _, _, fo, (ov, ot), _ = res
        assert (ov == CV).all() and (ot == CT).all() and (fo == -1).all()
        s, hv, ht, hf, _, _ = simp.simplify_host(vb, tri, first, cell)
        assert s == abi.KT_ERR_ARG and not hv.view(np.uint32).any() and not ht.any() and (hf == -1).all()
    # a cell index at 2^19 (and the last that fit, 2^19 - 1 and -2^19)
    small = np.zeros(3, V)
    small["xyz"][:, 0] = (1.0 - 2.0 ** -20, -1.0, 0.5)
    one = np.array([[0, 1, 2]], np.uint32)
    _check_device(ctx, simp, (small, one, [0, 3], 2.0 ** -19))
    for val in (1.0, -1.0 - 2.0 ** -20):
        sb = small.copy()
        sb["xyz"][2, 2] = val
        res = _device(ctx, simp, (sb, one, [0, 3], 2.0 ** -19))
        assert res[0] == abi.KT_ERR_ARG and (res[4][0] == CV).all() and (res[4][1] == CT).all()
    # the host form at too small a capacity: the true counts, nothing written
    for kw in (dict(vertex_capacity=n_keep - 1), dict(triangle_capacity=m_keep - 1)):
        s, hv, ht, hf, n_out, m_out = simp.simplify_host(v, tri, first, cell, **kw)
        assert s == abi.KT_ERR_CAPACITY and (n_out, m_out) == (n_keep, m_keep) and not hv.view(np.uint32).any() and not ht.any() and (hf == -1).all()
    # null pointers with n > 0, misaligned vertices, an output that is an input, n > 2^29
    dv, dt = ctx.upload(v), ctx.upload(tri)
    ov, ot = ctx.empty(16 * n + 16), ctx.empty(12 * m)
    good = dict(vertices=dv, n=n, triangles=dt, m=m, span_first=first, cell=cell, vertices_out=ov, vertex_capacity=n, triangles_out=ot, triangle_capacity=m)
    for change in (dict(vertices=None), dict(triangles=None), dict(vertices_out=None), dict(triangles_out=None), dict(vertices=dv.ptr + 8),
                   dict(vertices_out=ov.ptr + 4), dict(vertices_out=dv), dict(triangles_out=dt), dict(n=(1 << 29) + 1, span_first=[0, (1 << 29) + 1])):
        assert simp.simplify_device(**{**good, **change})[0] == abi.KT_ERR_ARG, change
    assert np.array_equal(ctx.download(dt, np.uint32, (m, 3)), tri) and np.array_equal(ctx.download(dv, V, (n,)).view(np.uint8), v.view(np.uint8))
    s, n_out, m_out, fo = simp.simplify_device(**good)                                   # the object is still usable
    assert s == abi.KT_OK and (n_out, m_out) == (n_keep, m_keep) and np.array_equal(fo, want[2])
    assert np.array_equal(ctx.download(ot, np.uint32, (m_keep, 3)), want[1])
    # n = 0: KT_OK with any valid table, null pointers included
    assert simp.simplify_device(None, 0, None, 0, [0, 0, 0], cell, None, 0, None, 0)[:3] == (abi.KT_OK, 0, 0)
    s, n_out, m_out, fo = simp.simplify_device(None, 0, None, 0, [0], cell, None, 0, None, 0)
    assert (s, n_out, m_out, fo.tolist()) == (abi.KT_OK, 0, 0, [0])
    for b in (dv, dt, ov, ot):
        b.free()


def test_allocations_return(ctx):
    ctx.sync()
    start = abi.live_allocations()
    w = abi.MeshSimplify(ctx)
    created = abi.live_allocations()[0]
    assert created > start[0]
    case = cases.random_case(4, 257)
    _check_device(ctx, w, case)
    device_form = abi.live_allocations()[0]
    assert device_form > created                                      # the per-vertex arrays, the triangle counts and the span table are the object's
    w.simplify(*case)
    assert abi.live_allocations()[0] == device_form + 4               # ... and so is the host form's staging
    w.simplify(*cases.random_case(5, 65))                             # a smaller call takes nothing
    assert abi.live_allocations()[0] == device_form + 4
    w.simplify(*cases.random_case(6, 4099))                           # a larger one releases and takes again
    assert abi.live_allocations()[0] == device_form + 4
    w.close()
    assert abi.live_allocations() == start


# ---- mesh, weld, simplify on the device -----------------------------------------------------------------------------------------------------
def test_split_boxes_meshed_welded_simplified(ctx, simp):
    """ctx.mesh_keyed of the N = 32 sphere's split boxes, welded on the device, simplified at 3 voxels: the restatement's bytes, and every
    directed edge of the result balanced (P2)"""
    N = 32
    vol, col = wc.sphere_volume(N)
    dv, dc = ctx.upload(vol), ctx.upload(col)
    welder = abi.MeshWeld(ctx)
    try:
        for axis, cut in wc.SPLITS:
            parts = [ctx.mesh_keyed(dv, (3.0, 3.0, 3.0), (0, 0, 0), dc, lo, hi, (0, 0, 0), N) for lo, hi in wc.split_boxes(N, axis, cut)[1:]]
            v, k, t, first, times = wc.concat(*[(p[0], p[1], p[2]) for p in parts])
            wv, _, wt, wf = welder.weld(v, k, t, first, times)
            rv, rt, rf = cases.welded_split(axis, cut)
            cases.same((wv, wt, wf), (rv, rt, rf))
            assert wc.closed(wt)
            for voxels in (3, 8):
                cell = voxels * cases.VOXEL
                got = simp.simplify(wv, wt, wf, cell)
                cases.same(got, ref.simplify(wv, wt, wf, cell))
                assert cases.balanced(got[1]) and 0 < len(got[0]) < len(wv)
                cases.check_distances(wv, wf, cell, got[0])
    finally:
        welder.close()
        dv.free()
        dc.free()


def test_simplified_mesh_through_the_deformation(ctx, simp):
    """The two-span mesh of mesh_simplify_cases.deform_case, simplified, goes into kt_deform_apply_mesh with span_first_out: every byte
    equals deform_ref.apply_mesh on the restatement's arrays."""
    import deform_cases as dc
    from kintinuous_amd import deform_ref
    v, tri, first, times, cell, gname = cases.deform_case()
    want = ref.simplify(v, tri, first, cell)
    got = simp.simplify(v, tri, first, cell)
    cases.same(got, want)
    sv, st, sf = got
    assert 0 < len(sv) < len(v) and 0 < sf[1] < len(sv)
    gc = dc.case(gname)
    g = abi.DeformationGraph(ctx, 20, 8)
    try:
        g.set_graph(gc["node_pos"], gc["node_time"])
        g.set_state(dc.restated(gname)[0])
        moved = g.apply_mesh(sv, sf, times)
    finally:
        g.close()
    ref_moved = deform_ref.apply_mesh(dc.graph(gname), dc.restated(gname)[0], want[0], want[2], times)
    assert moved.tobytes() == ref_moved.tobytes()
    assert np.abs(moved["xyz"] - sv["xyz"]).max() > 0


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def _rgb24(v):
    return v["rgb"][:, 0].astype(np.uint32) << 16 | v["rgb"][:, 1].astype(np.uint32) << 8 | v["rgb"][:, 2].astype(np.uint32)


def _driver_simp_is_the_restatements(prefix, source, cell):
    """<prefix>_simp.ply and <prefix>.simp against the restatement's simplification of what <prefix><source>.ply holds, with the first_in
    column of .simp as the span table (the .ply keeps three colour bytes of the vertex's four; the bytes are averaged one by one) ->
    (n_in, n_out, m_in, m_out, spans)"""
    import deform_mesh_cases as mc
    v, tri = mc.read_ply(prefix + source + ".ply")
    lines = [l.split() for l in open(prefix + ".simp").read().splitlines()]
    spans = [(int(a), int(b), int(c)) for tag, a, b, c in lines[:-1] if tag == "span"]
    assert len(spans) == len(lines) - 1 and lines[-1][0] == "result"
    n_in, n_out, m_in, m_out = (int(x) for x in lines[-1][1:5])
    assert float.fromhex(lines[-1][5]) == float(np.float32(cell))
    assert n_in == len(v) and m_in == len(tri)
    first = np.array([s[1] for s in spans] + [n_in], np.int64)
    full = np.zeros(n_in, V)
    full["xyz"], full["rgb"] = v["xyz"], _rgb24(v)
    rv, rt, rf = ref.simplify(full, tri.astype(np.uint32), first, cell)
    sv, stri = mc.read_ply(prefix + "_simp.ply")
    assert len(rv) == n_out == len(sv) and len(rt) == m_out == len(stri)
    assert np.ascontiguousarray(rv["xyz"]).tobytes() == np.ascontiguousarray(sv["xyz"]).tobytes() and np.array_equal(rv["rgb"], _rgb24(sv))
    assert np.array_equal(rt.astype(np.int32), stri)
    assert [s[2] for s in spans] == rf[:-1].tolist() and rf[-1] == n_out
    return n_in, n_out, m_in, m_out, len(spans)


def test_driver_ms_on_the_welded_crab_walk(tmp_path):
    """kintinuous_hip -m -mw -ms 0.15 on the out-and-back crab-walk of tests/test_gpu_mesh_weld.py (N = 96, 160 x 120, a 5.2 m volume):
    _simp.ply and .simp are the restatement's simplification of the run's own _weld.ply; .ply, _weld.ply and .weld are byte-identical to
    the run without -ms; -ms without -m is ignored with a message.
    Measured on an MI355X: see profiles/mesh_simplify.md."""
    run = drv.crab_walk_driver(tmp_path)

    _, p0 = run("plain", "-m", "-mw")
    _, p1 = run("simp", "-m", "-mw", "-ms", "0.15")
    nomesh, p2 = run("nomesh", "-ms", "0.15")
    rd = lambda p: open(p, "rb").read()
    assert drv.outputs(tmp_path, p1) == sorted(drv.outputs(tmp_path, p0) + [".simp", "_simp.ply"])
    assert {".ply", "_weld.ply", ".weld"} <= set(drv.outputs(tmp_path, p0))
    for ext in drv.outputs(tmp_path, p0):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    assert "-ms ignored without -m" in nomesh.stderr and not [e for e in drv.outputs(tmp_path, p2) if "simp" in e or e.endswith(".ply")]
    got = _driver_simp_is_the_restatements(p1, "_weld", 0.15)
    print("crab-walk: vertices %d -> %d, triangles %d -> %d in %d spans" % got)
    n_in, n_out, m_in, m_out, n_spans = got
    assert n_spans > 1 and 0 < n_out < n_in and 0 < m_out < m_in


def test_driver_ms_with_df_on_the_loop_log(tmp_path):
    """kintinuous_hip ... -lc -pg -pcd -df -m -ms 0.05 on the ten-frame walk of tests/test_gpu_deform_mesh.py's driver test: _simp.ply and
    .simp are the restatement's simplification of the run's own .ply; _simp_def.ply has _simp.ply's faces and colours and moved
    vertices; every file of the run without -ms is byte-identical."""
    import deform_mesh_cases as mc
    run = drv.loop_log_driver(tmp_path)

    _, p0 = run("plain", "-m")
    _, p1 = run("simp", "-m", "-ms", "0.05")
    rd = lambda p: open(p, "rb").read()
    assert drv.outputs(tmp_path, p1) == sorted(drv.outputs(tmp_path, p0) + [".simp", "_simp.ply", "_simp_def.ply"])
    for ext in drv.outputs(tmp_path, p0):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    got = _driver_simp_is_the_restatements(p1, "", 0.05)
    print("loop log: vertices %d -> %d, triangles %d -> %d in %d spans" % got)
    assert 0 < got[1] < got[0] and 0 < got[3] < got[2]
    sv, stri = mc.read_ply(p1 + "_simp.ply")
    dv, dtri = mc.read_ply(p1 + "_simp_def.ply")
    assert np.array_equal(stri, dtri) and len(sv) == len(dv) and sv["rgb"].tobytes() == dv["rgb"].tobytes()
    assert np.abs(dv["xyz"] - sv["xyz"]).max() > 0                                          # ... and it was deformed
