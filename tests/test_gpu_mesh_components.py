"""GPU: the connected-component filter of the -m mesh (kt_mesh_components.hip) -- kt_mesh_components_device and kt_mesh_components byte
for byte against kintinuous_amd/mesh_components_ref.py on every case of mesh_components_cases.py (random meshes under a permutation,
strips, hubs, exact sizes around the threshold, the connectivity and counting rules), a large call after a small one, the errors with
canaries, the sphere's split boxes meshed, filtered, simplified, given normals and deformed on the device, and the driver's -mc."""
import os

import numpy as np
import pytest

import mesh_driver_cases as drv
import mesh_components_cases as cases
import mesh_weld_cases as wc
from kintinuous_amd import abi, mesh_components_ref as ref

pytestmark = pytest.mark.gpu

V = abi.MESH_VERTEX_DTYPE
GUARD = 5
CV, CT, CL = 0xA5A5A5A5, 0x3C3C3C3C, 0x5EEDF00D


def _last_error():
    return abi.lib().kt_last_error().decode(errors="replace")


@pytest.fixture(scope="module")
def comp(ctx):
    w = abi.MeshComponents(ctx)
    yield w
    w.close()


def _device(ctx, comp, case, k, vcap=None, tcap=None, labels=True):
    """kt_mesh_components_device on uploads with canaries behind every buffer -> (status, n_out, m_out, span_first_out, stats, outputs as
    left (vertices, triangles, labels), inputs as left)"""
    v, tri, first = case
    n, m = len(v), len(tri)
    vcap = n if vcap is None else vcap
    tcap = m if tcap is None else tcap
    dv = ctx.upload(np.concatenate([v.view(np.uint32).reshape(-1), np.full(4 * GUARD, CV, np.uint32)]))
    dt = ctx.upload(np.concatenate([tri.reshape(-1), np.full(3 * GUARD, CT, np.uint32)]))
    ov = ctx.upload(np.full(4 * (vcap + GUARD), CV, np.uint32))
    ot = ctx.upload(np.full(3 * (tcap + GUARD), CT, np.uint32))
    ol = ctx.upload(np.full(n + GUARD, CL, np.uint32))
    s, n_out, m_out, fo, stats = comp.components_device(dv, n, dt, m, first, k, ov, vcap, ot, tcap, ol if labels else None)
    out = (ctx.download(ov, np.uint32, (4 * (vcap + GUARD),)), ctx.download(ot, np.uint32, (3 * (tcap + GUARD),)), ctx.download(ol, np.uint32, (n + GUARD,)))
    ins = (ctx.download(dv, np.uint32, (4 * (n + GUARD),)), ctx.download(dt, np.uint32, (3 * (m + GUARD),)))
    for b in (dv, dt, ov, ot, ol):
        b.free()
    return s, n_out, m_out, fo, stats, out, ins


def _check_device(ctx, comp, case, k, want=None):
    v, tri, first = case
    n, m = len(v), len(tri)
    wv, wt, wf, wl, ws = ref.components(*case, k) if want is None else want
    s, n_out, m_out, fo, stats, (ov, ot, ol), (iv, it) = _device(ctx, comp, case, k)
    assert s == abi.KT_OK and (n_out, m_out) == (len(wv), len(wt)) and stats == ws
    assert np.array_equal(ov[:4 * n_out], wv.view(np.uint32).reshape(-1)) and np.array_equal(ot[:3 * m_out], wt.reshape(-1)) and np.array_equal(fo, wf)
    assert np.array_equal(ol[:n], wl)
    assert (ov[4 * n_out:] == CV).all() and (ot[3 * m_out:] == CT).all() and (ol[n:] == CL).all()     # nothing behind the outputs
    assert np.array_equal(iv[:4 * n], v.view(np.uint32).reshape(-1)) and (iv[4 * n:] == CV).all()     # the inputs are read only
    assert np.array_equal(it[:3 * m], tri.reshape(-1)) and (it[3 * m:] == CT).all()
    return (wv, wt, wf, wl, ws), (ov, ot, ol, fo)


def _check_both(ctx, comp, case, k):
    want, got = _check_device(ctx, comp, case, k)
    _, again = _check_device(ctx, comp, case, k, want)                    # a second call: the same bytes
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    s, hv, ht, hf, hl, hs, n_out, m_out = comp.components_host(*case, k)
    assert s == abi.KT_OK and (n_out, m_out) == (len(want[0]), len(want[1]))
    cases.same_result((hv, ht, hf, hl, hs), want)
    return want


@pytest.fixture(scope="module")
def every_case():
    return cases.every_case()


@pytest.mark.parametrize("m", cases.SIZES)
def test_swept_cases_device_and_host_forms(ctx, comp, every_case, m):
    """the random meshes, the chains (descending and random) and the hubs (last and first) of m triangles"""
    mine = [c for c in every_case if c[0].endswith(" %d" % m)]
    assert len(mine) == 5
    for name, case, thresholds in mine:
        for k in thresholds:
            want = _check_both(ctx, comp, case, k)
        if name.startswith("random") and m >= 257:
            assert 0 < want[4][1] < want[4][0] and 0 < len(want[0]) < len(case[0])        # (at 40: something dropped, something kept)


def test_thresholds_and_the_rules(ctx, comp, every_case):
    rest = [c for c in every_case if not c[0][-1].isdigit()]
    assert len(rest) == 1 + len(cases.touching_case())
    for name, case, thresholds in rest:
        for k in thresholds:
            _check_both(ctx, comp, case, k)
    for name, case, k, stats, n_out in cases.touching_case():
        assert comp.components(*case, k)[4] == stats, name


def test_everything_dropped_everything_kept_and_no_labels(ctx, comp):
    case = cases.random_case(11, 4099)
    v, tri, first = case
    n, m = len(v), len(tri)
    s, n_out, m_out, fo, stats, (ov, ot, ol), _ = _device(ctx, comp, case, 301)            # above the largest component: everything goes
    assert (s, n_out, m_out) == (abi.KT_OK, 0, 0) and stats[1] == 0 and stats[2] <= 300 and not fo.any()
    assert (ov == CV).all() and (ot == CT).all() and np.array_equal(ol[:n], ref.components(*case, 301)[3])
    s, n_out, m_out, fo, stats, (ov, ot, ol), _ = _device(ctx, comp, case, 301, vcap=0, tcap=0)   # ... which fits into nothing
    assert (s, n_out, m_out) == (abi.KT_OK, 0, 0) and (ov == CV).all() and (ot == CT).all()
    s, n_out, m_out, fo, stats, (ov, ot, ol), _ = _device(ctx, comp, case, 0)              # everything kept: the input
    assert (s, n_out, m_out) == (abi.KT_OK, n, m) and stats[0] == stats[1] and np.array_equal(fo, first)
    assert np.array_equal(ov[:4 * n], v.view(np.uint32).reshape(-1)) and np.array_equal(ot[:3 * m], tri.reshape(-1))
    want = ref.components(*case, 40)
    s, n_out, m_out, fo, stats, (ov, ot, ol), _ = _device(ctx, comp, case, 40, labels=False)      # a null labels_out_dev
    assert s == abi.KT_OK and stats == want[4] and np.array_equal(fo, want[2]) and (ol == CL).all()
    assert np.array_equal(ov[:4 * n_out], want[0].view(np.uint32).reshape(-1)) and np.array_equal(ot[:3 * m_out], want[1].reshape(-1))
    s, hv, ht, hf, hl, hs, _, _ = comp.components_host(*case, 40, labels=False)
    assert s == abi.KT_OK and hl is None
    cases.same((hv, ht, hf), want[:3])
    # m = 0: n components of size 0
    s, n_out, m_out, fo, stats, _, _ = _device(ctx, comp, (v, tri[:0], first), 1)
    assert (s, n_out, m_out, stats) == (abi.KT_OK, 0, 0, (n, 0, 0))
    s, n_out, m_out, fo, stats, (ov, _, ol), _ = _device(ctx, comp, (v, tri[:0], first), 0)
    assert (s, n_out, m_out, stats) == (abi.KT_OK, n, 0, (n, n, 0)) and np.array_equal(ol[:n], np.arange(n)) and np.array_equal(ov[:4 * n], v.view(np.uint32).reshape(-1))


def test_large_after_small_equals_a_fresh_object(ctx):
    small, large = cases.random_case(1, 65), cases.random_case(2, 70001)
    a, b = abi.MeshComponents(ctx), abi.MeshComponents(ctx)
    try:
        _check_device(ctx, a, small, 4)
        want, got = _check_device(ctx, a, large, 40)
        _, fresh = _check_device(ctx, b, large, 40, want)
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh))
        cases.same_result(a.components(*small, 4), ref.components(*small, 4))          # ... and a small one after it
        cases.same_result(a.components(*large, 40), b.components(*large, 40))
    finally:
        a.close()
        b.close()


def test_errors_leave_everything_intact(ctx, comp):
    case = cases.random_case(9, 4099)
    v, tri, first = case
    n, m = len(v), len(tri)
    k = 40
    want = ref.components(*case, k)
    n_keep, m_keep = len(want[0]), len(want[1])
    assert 0 < n_keep < n and 0 < m_keep < m

    def intact(res, vb=v, tb=tri):
        _, _, _, fo, stats, (ov, ot, ol), (iv, it) = res
        assert (ov == CV).all() and (ot == CT).all() and (ol == CL).all()
        assert np.array_equal(iv[:4 * len(vb)], vb.view(np.uint32).reshape(-1)) and np.array_equal(it[:3 * len(tb)], tb.reshape(-1))
        assert (fo == -1).all() and stats == (-1, -1, -1)                              # span_first_out and the stats untouched as well

    for vcap, tcap in ((n_keep - 1, m), (n, m_keep - 1), (n_keep - 1, m_keep - 1), (0, 0)):
        res = _device(ctx, comp, case, k, vcap=vcap, tcap=tcap)
        assert res[0] == abi.KT_ERR_CAPACITY and res[1:3] == (n_keep, m_keep)          # both true counts
        assert "do not fit" in _last_error()
        intact(res)
    res = _device(ctx, comp, case, k, vcap=n_keep, tcap=m_keep)                        # the smallest that fit
    assert res[0] == abi.KT_OK and res[1:3] == (n_keep, m_keep)
    for f in (np.array([1] + first[1:].tolist()), np.array(first[:-1].tolist() + [n - 1]), np.array([0, 9, 5] + first[3:].tolist())):
        res = _device(ctx, comp, (v, tri, f), k)
        assert res[0] == abi.KT_ERR_ARG and "bad argument" in _last_error()
        intact(res)
    for row, col, val in ((0, 0, 0xffffffff), (m // 2, 1, n), (m - 1, 2, n), (5, 0, n + 7)):      # an index out of range: found on the device
        tb = tri.copy()
        tb[row, col] = val
        with pytest.raises(ValueError):
            ref.components(v, tb, first, k)
        res = _device(ctx, comp, (v, tb, first), k)
        assert res[0] == abi.KT_ERR_ARG and "index out of range" in _last_error()
        intact(res, tb=tb)
        s, hv, ht, hf, hl, hs, _, _ = comp.components_host(v, tb, first, k)
        assert s == abi.KT_ERR_ARG and not hv.view(np.uint32).any() and not ht.any() and (hf == -1).all() and (hl == 0xffffffff).all() and hs == (-1, -1, -1)
    _check_device(ctx, comp, case, k, want)                                            # the same object's next valid call is correct
    # the host form at too small a capacity: the true counts, nothing written
    for kw in (dict(vertex_capacity=n_keep - 1), dict(triangle_capacity=m_keep - 1)):
        s, hv, ht, hf, hl, hs, n_out, m_out = comp.components_host(v, tri, first, k, **kw)
        assert s == abi.KT_ERR_CAPACITY and (n_out, m_out) == (n_keep, m_keep) and not hv.view(np.uint32).any() and not ht.any() and (hf == -1).all()
        assert (hl == 0xffffffff).all() and hs == (-1, -1, -1)
    # sizes over 2^29 with dummy pointers: refused before anything is allocated
    start = abi.live_allocations()
    for nn, mm in (((1 << 29) + 1, 1), (3, (1 << 29) + 1)):
        assert comp.components_device(0x10000, nn, 0x20000, mm, [0, nn], 1, 0x30000, nn, 0x40000, mm)[0] == abi.KT_ERR_ARG
    assert abi.live_allocations() == start
    # null pointers with n > 0, misaligned vertices, an output that is or overlaps an input or another output
    dv, dt = ctx.upload(v), ctx.upload(tri)
    ov, ot, ol = ctx.upload(np.full(4 * n + 4, CV, np.uint32)), ctx.upload(np.full(3 * m, CT, np.uint32)), ctx.upload(np.full(n, CL, np.uint32))
    good = dict(vertices=dv, n=n, triangles=dt, m=m, span_first=first, min_triangles=k, vertices_out=ov, vertex_capacity=n, triangles_out=ot, triangle_capacity=m,
                labels_out=ol)
    for change in (dict(vertices=None), dict(triangles=None), dict(vertices_out=None), dict(triangles_out=None), dict(vertices=dv.ptr + 8),
                   dict(vertices_out=ov.ptr + 4), dict(vertices_out=dv), dict(triangles_out=dt), dict(labels_out=dv), dict(labels_out=dt),
                   dict(labels_out=dt.ptr + 12 * m - 4), dict(triangles_out=dv.ptr + 16 * n - 4), dict(vertices_out=dt.ptr + 16), dict(labels_out=ot),
                   dict(labels_out=ov.ptr + 16 * n - 4), dict(span_first=[])):
        assert comp.components_device(**{**good, **change})[0] == abi.KT_ERR_ARG, change
    assert (ctx.download(ov, np.uint32, (4 * n + 4,)) == CV).all() and (ctx.download(ot, np.uint32, (3 * m,)) == CT).all() and (ctx.download(ol, np.uint32, (n,)) == CL).all()
    assert np.array_equal(ctx.download(dt, np.uint32, (m, 3)), tri) and np.array_equal(ctx.download(dv, V, (n,)).view(np.uint8), v.view(np.uint8))
    s, n_out, m_out, fo, stats = comp.components_device(**good)                          # the object is still usable
    assert s == abi.KT_OK and (n_out, m_out) == (n_keep, m_keep) and np.array_equal(fo, want[2]) and stats == want[4]
    assert np.array_equal(ctx.download(ot, np.uint32, (m_keep, 3)), want[1]) and np.array_equal(ctx.download(ol, np.uint32, (n,)), want[3])
    # n = 0: KT_OK and zeros with any valid table, null pointers included
    assert comp.components_device(None, 0, None, 0, [0, 0, 0], k, None, 0, None, 0)[:3] == (abi.KT_OK, 0, 0)
    s, n_out, m_out, fo, stats = comp.components_device(None, 0, dt, m, [0], k, None, 0, None, 0)   # (the triangles are not looked at: the restatement's rule)
    assert (s, n_out, m_out, fo.tolist(), stats) == (abi.KT_OK, 0, 0, [0], (0, 0, 0))
    for b in (dv, dt, ov, ot, ol):
        b.free()


def test_allocations_return(ctx):
    ctx.sync()
    start = abi.live_allocations()
    w = abi.MeshComponents(ctx)
    created = abi.live_allocations()[0]
    assert created > start[0]
    case = cases.random_case(4, 257)
    _check_device(ctx, w, case, 4)
    device_form = abi.live_allocations()[0]
    assert device_form == created + 5 + 1 + 2                         # the per-vertex arrays, the triangle counts and the span table are the object's
    w.components(*case, 4)
    assert abi.live_allocations()[0] == device_form + 5               # ... and so is the host form's staging
    w.components(*cases.random_case(5, 65), 4)                        # a smaller call takes nothing
    assert abi.live_allocations()[0] == device_form + 5
    w.components(*cases.random_case(6, 4099), 4)                      # a larger one releases and takes again
    assert abi.live_allocations()[0] == device_form + 5
    w.close()
    assert abi.live_allocations() == start


# ---- mesh, weld, components, simplify, normals, deform: all on the device -----------------------------------------------------------------
def test_pipeline_on_the_device(ctx, comp):
    """kt_extract_mesh_keyed on the N = 32 sphere's split boxes; the concatenation filtered unwelded (two open halves: the smaller goes at
    a threshold between them) and welded (one piece: all of it stays); the filtered mesh through kt_mesh_simplify_device,
    kt_mesh_normals_device and kt_deform_apply_mesh_device with the pass's span table, each equal to its restatement"""
    import deform_cases as dc
    import deform_mesh_cases as mc
    import mesh_simplify_cases as sc
    from kintinuous_amd import deform_ref, mesh_normals_ref, mesh_simplify_ref
    N, gname = 32, "m20_n64_c7"
    vol, col = wc.sphere_volume(N)
    dvol, dcol = ctx.upload(vol), ctx.upload(col)
    welder, simp, nrm, g = abi.MeshWeld(ctx), abi.MeshSimplify(ctx), abi.MeshNormals(ctx), abi.DeformationGraph(ctx, 20, 8)
    bufs = [dvol, dcol]
    try:
        gc = dc.case(gname)
        g.set_graph(gc["node_pos"], gc["node_time"])
        g.set_state(dc.restated(gname)[0])
        times = np.array([mc.span_times(20)[2], mc.span_times(20)[7]], np.uint64)
        for axis, cut in ((0, 15), (1, 15), (2, 15)):
            parts = [ctx.mesh_keyed(dvol, (3.0, 3.0, 3.0), (0, 0, 0), dcol, lo, hi, (0, 0, 0), N) for lo, hi in wc.split_boxes(N, axis, cut)[1:]]
            v, k, t, first, _ = wc.concat(*[(p[0], p[1], p[2]) for p in parts])
            cases.same((v, k, t, first), cases.unwelded_split(axis, cut)[:4])
            n, m = len(v), len(t)
            dv, dk, dt = ctx.upload(v), ctx.upload(k), ctx.upload(t)
            cv, ct, cl = ctx.empty(16 * n), ctx.empty(12 * m), ctx.empty(4 * n)
            wv, wk, sv, st, on = ctx.empty(16 * n), ctx.empty(8 * n), ctx.empty(16 * n), ctx.empty(12 * m), ctx.empty(12 * n)
            bufs += [dv, dk, dt, cv, ct, cl, wv, wk, sv, st, on]
            # unwelded: two components, the sizes of the two halves; a threshold between them keeps the larger half alone
            halves = sorted([len(parts[0][1]), len(parts[1][1])])
            want = ref.components(v, t, first, halves[0] + 1)
            assert want[4] == (2, 1, halves[1])
            s, nc, mcnt, cf, stats = comp.components_device(dv, n, dt, m, first, halves[0] + 1, cv, n, ct, m, cl)
            assert s == abi.KT_OK and stats == want[4] and (nc, mcnt) == (len(want[0]), halves[1])
            cases.same((ctx.download(cv, V, (nc,)), ctx.download(ct, np.uint32, (mcnt, 3)), cf, ctx.download(cl, np.uint32, (n,))), want[:4])
            assert cf[1] in (0, nc) and wc.open_edges(want[1]) > 0                          # one span lost every vertex; a half is open
            # welded: one component, which a threshold of all its triangles keeps whole
            s, nw, wf = welder.weld_device(dv, dk, n, dt, m, first, times, wc.NO_GATE, wv, wk, n)
            assert s == abi.KT_OK and 0 < nw < n
            s, nc, mcnt, cf, stats = comp.components_device(wv, nw, dt, m, wf, m, cv, n, ct, m, cl)
            assert s == abi.KT_OK and stats == (1, 1, m) and (nc, mcnt) == (nw, m) and np.array_equal(cf, wf)
            fv, ft = ctx.download(cv, V, (nc,)), ctx.download(ct, np.uint32, (mcnt, 3))
            cases.same((fv, ft, cf), sc.welded_split(axis, cut))
            assert wc.closed(ft) and not ctx.download(cl, np.uint32, (nw,)).any()
            # the filtered mesh and the pass's table through the three passes that follow it
            cell = 2 * sc.VOXEL
            s, ns, ms, sf = simp.simplify_device(cv, nc, ct, mcnt, cf, cell, sv, n, st, m)
            assert s == abi.KT_OK and 0 < ns < nc and 0 < ms < mcnt
            cases.same((ctx.download(sv, V, (ns,)), ctx.download(st, np.uint32, (ms, 3)), sf), mesh_simplify_ref.simplify(fv, ft, cf, cell))
            s, n_zero = nrm.normals_device(cv, nc, ct, mcnt, on)
            wn, wz = mesh_normals_ref.normals(fv, ft)
            assert s == abi.KT_OK and n_zero == wz and np.array_equal(ctx.download(on, np.float32, (nc, 3)).view(np.uint8), wn.view(np.uint8))
            g.apply_mesh_device(cv, nc, cf, times)
            moved = ctx.download(cv, V, (nc,))
            assert moved.tobytes() == deform_ref.apply_mesh(dc.graph(gname), dc.restated(gname)[0], fv, cf, times).tobytes()
            assert np.abs(moved["xyz"] - fv["xyz"]).max() > 0
    finally:
        g.close()
        nrm.close()
        simp.close()
        welder.close()
        for b in bufs:
            b.free()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def _rgb24(v):
    return v["rgb"][:, 0].astype(np.uint32) << 16 | v["rgb"][:, 1].astype(np.uint32) << 8 | v["rgb"][:, 2].astype(np.uint32)


def _comp_file(prefix):
    """<prefix>.comp -> (spans [(utime, first_in, first_out)], (n_in, n_out, m_in, m_out, components, kept, largest))"""
    lines = [l.split() for l in open(prefix + ".comp").read().splitlines()]
    spans = [(int(a), int(b), int(c)) for tag, a, b, c in lines[:-1] if tag == "span"]
    assert len(spans) == len(lines) - 1 and lines[-1][0] == "result" and len(lines[-1]) == 8
    return spans, tuple(int(x) for x in lines[-1][1:])


def _driver_comp_is_the_restatements(prefix, source, k):
    """<prefix>_comp.ply and <prefix>.comp against the restatement's filter of what <prefix><source>.ply holds, with the first_in column of
    .comp as the span table -> the result line"""
    import deform_mesh_cases as mc
    v, tri = mc.read_ply(prefix + source + ".ply")
    spans, result = _comp_file(prefix)
    n_in, n_out, m_in, m_out = result[:4]
    assert n_in == len(v) and m_in == len(tri)
    first = np.array([s[1] for s in spans] + [n_in], np.int64)
    full = np.zeros(n_in, V)
    full["xyz"], full["rgb"] = v["xyz"], _rgb24(v)
    rv, rt, rf, _, stats = ref.components(full, tri.astype(np.uint32), first, k)
    cv, ctri = mc.read_ply(prefix + "_comp.ply")
    assert len(rv) == n_out == len(cv) and len(rt) == m_out == len(ctri) and stats == result[4:]
    assert np.ascontiguousarray(rv["xyz"]).tobytes() == np.ascontiguousarray(cv["xyz"]).tobytes() and np.array_equal(rv["rgb"], _rgb24(cv))
    assert np.array_equal(rt.astype(np.int32), ctri)
    assert [s[2] for s in spans] == rf[:-1].tolist() and rf[-1] == n_out
    return result


def test_driver_mc_on_the_welded_crab_walk(tmp_path):
    """kintinuous_hip -m -mw -mc <k> on the out-and-back crab-walk of tests/test_gpu_mesh_simplify.py's driver test (N = 96, 160 x 120, a
    5.2 m volume).  A first run at k = 1 gives the component sizes of the run's own welded mesh (its labels by the restatement); k is then
    put between the smallest and the largest, so that at least one component is dropped and at least one is kept.  _comp.ply and .comp
    are the restatement's filter of _weld.ply; every file of the run without -mc is byte-identical; -mc -ms feeds the filtered mesh;
    -mc without -m, and -mc 0, are ignored with a message."""
    import deform_mesh_cases as mc
    run = drv.crab_walk_driver(tmp_path)

    _, p0 = run("plain", "-m", "-mw")
    _, p1 = run("one", "-m", "-mw", "-mc", "1")
    spans, (n_in, n_out, m_in, m_out, comps, kept, largest) = _comp_file(p1)
    wv, wt = mc.read_ply(p1 + "_weld.ply")
    labels = ref.components(np.zeros(len(wv), V), wt.astype(np.uint32), [0, len(wv)], 0)[3]
    sizes = np.bincount(labels[wt[:, 0]])
    sizes = np.sort(sizes[sizes > 0])
    print("crab-walk: %d vertices, %d triangles, %d components (%d referenced), sizes %s ... %s" % (n_in, m_in, comps, kept, sizes[:5].tolist(), sizes[-3:].tolist()))
    assert largest == sizes[-1] and kept == len(sizes) and m_out == m_in
    assert sizes[0] < sizes[-1], "the welded crab-walk mesh has components of one size only: no threshold separates them"
    k = int(sizes[0]) + 1
    out, p2 = run("comp", "-m", "-mw", "-mc", str(k))
    rd = lambda p: open(p, "rb").read()
    assert drv.outputs(tmp_path, p2) == sorted(drv.outputs(tmp_path, p0) + [".comp", "_comp.ply"])
    for ext in drv.outputs(tmp_path, p0):
        assert rd(p0 + ext) == rd(p2 + ext), ext
    result = _driver_comp_is_the_restatements(p2, "_weld", k)
    print("-mc %d: vertices %d -> %d, triangles %d -> %d, %d components, %d kept, the largest of %d" % ((k,) + result))
    assert 0 < result[5] < result[4] and 0 < result[1] < result[0] and 0 < result[3] < result[2]      # at least one dropped, at least one kept
    assert len([l for l in out.stdout.splitlines() if l.startswith("mesh ") and "_comp.ply:" in l]) == 1
    # -mc -ms: the simplification takes the filtered mesh
    _, p3 = run("both", "-m", "-mw", "-mc", str(k), "-ms", "0.15")
    assert drv.outputs(tmp_path, p3) == sorted(drv.outputs(tmp_path, p2) + [".simp", "_simp.ply"])
    for ext in drv.outputs(tmp_path, p2):
        assert rd(p2 + ext) == rd(p3 + ext), ext
    simp_result = open(p3 + ".simp").read().splitlines()[-1].split()
    assert simp_result[0] == "result" and (int(simp_result[1]), int(simp_result[3])) == (result[1], result[3])
    # -mn: the filtered file gets normals and a .normals line without further work
    _, p4 = run("nrm", "-m", "-mw", "-mc", str(k), "-mn")
    assert os.path.basename(p4) + "_comp.ply" in [l.split()[0] for l in open(p4 + ".normals").read().splitlines()]
    # ignored with a message
    nomesh, p5 = run("nomesh", "-mc", str(k))
    assert "-mc ignored without -m" in nomesh.stderr and not [e for e in drv.outputs(tmp_path, p5) if "comp" in e or e.endswith(".ply")]
    zero, p6 = run("zero", "-m", "-mw", "-mc", "0")
    assert "-mc ignored" in zero.stderr and drv.outputs(tmp_path, p6) == drv.outputs(tmp_path, p0)


def test_driver_mc_with_df_on_the_loop_log(tmp_path):
    """kintinuous_hip ... -lc -pg -pcd -df -m -mc 1 on the ten-frame walk of tests/test_gpu_deform_mesh.py's driver test: _comp.ply is
    the restatement's filter of .ply; _comp_def.ply has _comp.ply's faces and colours and its vertices where the deformation's restatement
    puts them, from the run's own .deform and the pass's span table in .comp (the rule of test_gpu_deform_mesh.py: every float the
    restatement's or its neighbour); every file of the run without -mc is byte-identical."""
    import deform_cases as dc
    import deform_mesh_cases as mc
    from kintinuous_amd import deform_ref
    run = drv.loop_log_driver(tmp_path)

    _, p0 = run("plain", "-m")
    _, p1 = run("comp", "-m", "-mc", "1")
    rd = lambda p: open(p, "rb").read()
    assert drv.outputs(tmp_path, p1) == sorted(drv.outputs(tmp_path, p0) + [".comp", "_comp.ply", "_comp_def.ply"])
    for ext in drv.outputs(tmp_path, p0):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    result = _driver_comp_is_the_restatements(p1, "", 1)
    print("loop log: vertices %d -> %d, triangles %d -> %d, %d components, %d kept, the largest of %d" % result)
    before, faces = mc.read_ply(p1 + "_comp.ply")
    after, faces_after = mc.read_ply(p1 + "_comp_def.ply")
    assert np.array_equal(faces, faces_after) and len(faces) > 0 and len(before) == len(after) and before["rgb"].tobytes() == after["rgb"].tobytes()
    d = mc.deform_file(open(p1 + ".deform").read())
    pose_t = [p[0] for p in d["pose"]]
    orig = np.array([p[1:4] for p in d["pose"]], np.float32)
    keep = deform_ref.sample_nodes(orig, 0.02)
    graph = deform_ref.Graph(orig[keep], np.array([pose_t[k] for k in keep], np.uint64))
    src = np.array([c[1:4] for c in d["con"]], np.float32)
    x, _, _, _, _, status, _ = deform_ref.optimise(graph, src, np.array([c[0] for c in d["con"]], np.uint64), np.array([c[4:7] for c in d["con"]]), {"significant_error": 1e-9})
    assert status in (deform_ref.CONVERGED, deform_ref.MAX_STEPS)
    spans, _ = _comp_file(p1)
    v = np.zeros(len(before), V)
    v["xyz"] = before["xyz"]
    want = deform_ref.apply_mesh(graph, x, v, [s[2] for s in spans] + [len(before)], [s[0] for s in spans])
    got, wanted = after["xyz"].reshape(-1), want["xyz"].reshape(-1)
    near = (got == wanted) | (got == np.nextafter(wanted, np.float32(np.inf))) | (got == np.nextafter(wanted, np.float32(-np.inf)))
    near |= np.abs(got.astype(np.float64) - wanted.astype(np.float64)) <= 10 * dc.BOUND * (1.0 + float(np.abs(before["xyz"]).max()))
    assert near.all() and np.abs(after["xyz"] - before["xyz"]).max() > 0                   # ... and it was deformed
