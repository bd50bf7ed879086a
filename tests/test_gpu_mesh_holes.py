"""GPU: the boundary report and small-hole fill of the -m mesh (kt_mesh_holes.hip) -- kt_mesh_holes_device and kt_mesh_holes byte for byte
against kintinuous_amd/mesh_holes_ref.py on every case of mesh_holes_cases.py, a large call after a small one, the errors with canaries,
the filled sphere filtered, simplified, given normals and deformed on the device, and the driver's -mh."""
import os

import numpy as np
import pytest

import mesh_driver_cases as drv
import mesh_holes_cases as cases
from kintinuous_amd import abi, mesh_holes_ref as ref

pytestmark = pytest.mark.gpu

V = abi.MESH_VERTEX_DTYPE
GUARD = 5
CV, CT, CL = 0xA5A5A5A5, 0x3C3C3C3C, 0x5EEDF00D
UNTOUCHED = (-1,) * 9


def _last_error():
    return abi.lib().kt_last_error().decode(errors="replace")


@pytest.fixture(scope="module")
def holes(ctx):
    w = abi.MeshHoles(ctx)
    yield w
    w.close()


@pytest.fixture(scope="module")
def every_case():
    return cases.every_case()


@pytest.fixture(scope="module")
def wanted(every_case):
    """the restatement of every case at every threshold, computed once"""
    return {(name, k): ref.holes(*case, k) for name, case, thresholds in every_case for k in thresholds}


def _device(ctx, holes, case, k, vcap=None, tcap=None, loops=True):
    """kt_mesh_holes_device on uploads with canaries behind every buffer -> (status, n_out, m_out, span_first_out, stats, outputs as left
    (vertices, triangles, loop_out), inputs as left)"""
    v, tri, first = case
    n, m = len(v), len(tri)
    most = abi.MeshHoles.most(n, m)
    vcap = most[0] if vcap is None else vcap
    tcap = most[1] if tcap is None else tcap
    dv = ctx.upload(np.concatenate([v.view(np.uint32).reshape(-1), np.full(4 * GUARD, CV, np.uint32)]))
    dt = ctx.upload(np.concatenate([tri.reshape(-1), np.full(3 * GUARD, CT, np.uint32)]))
    ov = ctx.upload(np.full(4 * (vcap + GUARD), CV, np.uint32))
    ot = ctx.upload(np.full(3 * (tcap + GUARD), CT, np.uint32))
    ol = ctx.upload(np.full(n + GUARD, CL, np.uint32))
    s, n_out, m_out, fo, stats = holes.holes_device(dv, n, dt, m, first, k, ov, vcap, ot, tcap, ol if loops else None)
    out = (ctx.download(ov, np.uint32, (4 * (vcap + GUARD),)), ctx.download(ot, np.uint32, (3 * (tcap + GUARD),)), ctx.download(ol, np.uint32, (n + GUARD,)))
    ins = (ctx.download(dv, np.uint32, (4 * (n + GUARD),)), ctx.download(dt, np.uint32, (3 * (m + GUARD),)))
    for b in (dv, dt, ov, ot, ol):
        b.free()
    return s, n_out, m_out, fo, stats, out, ins


def _check_device(ctx, holes, case, k, want=None, **kw):
    v, tri, first = case
    n, m = len(v), len(tri)
    wv, wt, wf, wl, ws = ref.holes(*case, k) if want is None else want
    s, n_out, m_out, fo, stats, (ov, ot, ol), (iv, it) = _device(ctx, holes, case, k, **kw)
    assert s == abi.KT_OK and (n_out, m_out) == (len(wv), len(wt)) and stats == ws, (stats, ws)
    assert np.array_equal(ov[:4 * n_out], wv.view(np.uint32).reshape(-1)) and np.array_equal(ot[:3 * m_out], wt.reshape(-1)) and np.array_equal(fo, wf)
    assert np.array_equal(ol[:n], wl)
    assert (ov[4 * n_out:] == CV).all() and (ot[3 * m_out:] == CT).all() and (ol[n:] == CL).all()     # nothing behind the outputs
    assert np.array_equal(iv[:4 * n], v.view(np.uint32).reshape(-1)) and (iv[4 * n:] == CV).all()     # the inputs are read only
    assert np.array_equal(it[:3 * m], tri.reshape(-1)) and (it[3 * m:] == CT).all()
    return (wv, wt, wf, wl, ws), (ov, ot, ol, fo)


def _check_both(ctx, holes, case, k, want):
    _, got = _check_device(ctx, holes, case, k, want)
    _, again = _check_device(ctx, holes, case, k, want)                   # a second call: the same bytes
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    s, hv, ht, hf, hl, hs, n_out, m_out = holes.holes_host(*case, k)
    assert s == abi.KT_OK and (n_out, m_out) == (len(want[0]), len(want[1]))
    cases.same_result((hv, ht, hf, hl, hs), want)


GROUPS = ("tetra", "disc", "sphere", "shared vertex", "fin", "duplicate", "flipped", "degenerate", "spans", "invalid", "random")


@pytest.mark.parametrize("group", GROUPS)
def test_device_and_host_forms_equal_the_restatement(ctx, holes, every_case, wanted, group):
    mine = [c for c in every_case if c[0].split(" ")[0] == group.split(" ")[0]]
    assert mine
    for name, case, thresholds in mine:
        for k in thresholds:
            _check_both(ctx, holes, case, k, wanted[(name, k)])


def test_all_groups_are_run(every_case):
    assert {c[0].split(" ")[0] for c in every_case} == {g.split(" ")[0] for g in GROUPS}


def test_large_after_small_equals_a_fresh_object(ctx):
    small, large = cases.random_case(1, 65), cases.random_case(2, 70000)
    a, b = abi.MeshHoles(ctx), abi.MeshHoles(ctx)
    try:
        _check_device(ctx, a, small, 8)
        want, got = _check_device(ctx, a, large, 8)
        assert want[4][5] > 100 and want[4][4] > 0 and want[4][1] > 0
        _, fresh = _check_device(ctx, b, large, 8, want)
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh))
        cases.same_result(a.holes(*small, 8), ref.holes(*small, 8))                    # ... and a small one after it
        cases.same_result(a.holes(*large, 8), want)
    finally:
        a.close()
        b.close()


def test_null_loop_out_and_the_empty_inputs(ctx, holes, wanted, every_case):
    case = [c for n, c, _ in every_case if n == "random 4099"][0]
    v, tri, first = case
    n, m = len(v), len(tri)
    want = wanted[("random 4099", 4)]
    s, n_out, m_out, fo, stats, (ov, ot, ol), _ = _device(ctx, holes, case, 4, loops=False)
    assert s == abi.KT_OK and stats == want[4] and np.array_equal(fo, want[2]) and (ol == CL).all()
    assert np.array_equal(ov[:4 * n_out], want[0].view(np.uint32).reshape(-1)) and np.array_equal(ot[:3 * m_out], want[1].reshape(-1))
    s, hv, ht, hf, hl, hs, _, _ = holes.holes_host(*case, 4, loops=False)
    assert s == abi.KT_OK and hl is None
    cases.same((hv, ht, hf), want[:3])
    # m = 0: the output is the input
    s, n_out, m_out, fo, stats, (ov, ot, ol), _ = _device(ctx, holes, (v, tri[:0], first), 256)
    assert (s, n_out, m_out, stats) == (abi.KT_OK, n, 0, (0,) * 9) and np.array_equal(fo, first)
    assert np.array_equal(ov[:4 * n], v.view(np.uint32).reshape(-1)) and (ov[4 * n:] == CV).all() and (ol[:n] == 0xffffffff).all()
    # the smallest capacities that fit
    res = _device(ctx, holes, case, 4, vcap=len(want[0]), tcap=len(want[1]))
    assert res[0] == abi.KT_OK and res[1:3] == (len(want[0]), len(want[1]))


def test_errors_leave_everything_intact(ctx, holes, every_case, wanted):
    case = [c for n, c, _ in every_case if n == "random 4099"][0]
    v, tri, first = case
    n, m = len(v), len(tri)
    k = 4
    want = wanted[("random 4099", k)]
    n_true, m_true = len(want[0]), len(want[1])
    assert n_true > n and m_true > m

    def intact(res, vb=v, tb=tri):
        _, _, _, fo, stats, (ov, ot, ol), (iv, it) = res
        assert (ov == CV).all() and (ot == CT).all() and (ol == CL).all()
        assert np.array_equal(iv[:4 * len(vb)], vb.view(np.uint32).reshape(-1)) and np.array_equal(it[:3 * len(tb)], tb.reshape(-1))
        assert (fo == -1).all() and stats == UNTOUCHED                                 # span_first_out and the stats untouched as well

    for vcap, tcap in ((n_true - 1, m_true), (n_true, m_true - 1), (n_true - 1, m_true - 1), (0, 0), (n, m)):
        res = _device(ctx, holes, case, k, vcap=vcap, tcap=tcap)
        assert res[0] == abi.KT_ERR_CAPACITY and res[1:3] == (n_true, m_true)          # both true counts
        assert "do not fit" in _last_error()
        intact(res)
    for f in (np.array([1] + first[1:].tolist()), np.array(first[:-1].tolist() + [n - 1]), np.array([0, 9, 5] + first[3:].tolist())):
        res = _device(ctx, holes, (v, tri, f), k)
        assert res[0] == abi.KT_ERR_ARG and "bad argument" in _last_error()
        intact(res)
    for bad_k in (257, 1 << 20):
        res = _device(ctx, holes, case, bad_k)
        assert res[0] == abi.KT_ERR_ARG and "max_edges" in _last_error()
        intact(res)
    for row, col, val in ((0, 0, 0xffffffff), (m // 2, 1, n), (m - 1, 2, n), (5, 0, n + 7)):      # an index out of range: found on the device
        tb = tri.copy()
        tb[row, col] = val
        with pytest.raises(ValueError):
            ref.holes(v, tb, first, k)
        res = _device(ctx, holes, (v, tb, first), k)
        assert res[0] == abi.KT_ERR_ARG and "index out of range" in _last_error()
        intact(res, tb=tb)
        s, hv, ht, hf, hl, hs, _, _ = holes.holes_host(v, tb, first, k)
        assert s == abi.KT_ERR_ARG and not hv.view(np.uint32).any() and not ht.any() and (hf == -1).all() and (hl == CL).all() and hs == UNTOUCHED
    _check_device(ctx, holes, case, k, want)                                           # the same object's next valid call is correct
    # the host form at too small a capacity: the true counts, nothing written
    for kw in (dict(vertex_capacity=n_true - 1), dict(triangle_capacity=m_true - 1)):
        s, hv, ht, hf, hl, hs, n_out, m_out = holes.holes_host(v, tri, first, k, **kw)
        assert s == abi.KT_ERR_CAPACITY and (n_out, m_out) == (n_true, m_true) and not hv.view(np.uint32).any() and not ht.any() and (hf == -1).all()
        assert (hl == CL).all() and hs == UNTOUCHED
    # sizes over 2^29 with dummy pointers: refused before anything is allocated
    start = abi.live_allocations()
    for nn, mm in (((1 << 29) + 1, 1), (3, (1 << 29) + 1)):
        assert holes.holes_device(0x10000, nn, 0x20000, mm, [0, nn], 1, 0x30000, nn, 0x40000, mm)[0] == abi.KT_ERR_ARG
    assert abi.live_allocations() == start
    # null pointers with n > 0, misaligned vertices, an output that is or overlaps an input or another output
    vcap, tcap = abi.MeshHoles.most(n, m)
    dv, dt = ctx.upload(v), ctx.upload(tri)
    ov, ot, ol = ctx.upload(np.full(4 * vcap + 4, CV, np.uint32)), ctx.upload(np.full(3 * tcap, CT, np.uint32)), ctx.upload(np.full(n, CL, np.uint32))
    good = dict(vertices=dv, n=n, triangles=dt, m=m, span_first=first, max_edges=k, vertices_out=ov, vertex_capacity=vcap, triangles_out=ot, triangle_capacity=tcap,
                loop_out=ol)
    for change in (dict(vertices=None), dict(triangles=None), dict(vertices_out=None), dict(triangles_out=None), dict(vertices=dv.ptr + 8),
                   dict(vertices_out=ov.ptr + 4), dict(vertices_out=dv), dict(triangles_out=dt), dict(loop_out=dv), dict(loop_out=dt),
                   dict(loop_out=dt.ptr + 12 * m - 4), dict(triangles_out=dv.ptr + 16 * n - 4), dict(vertices_out=dt.ptr + 16), dict(loop_out=ot),
                   dict(loop_out=ov.ptr + 16 * vcap - 4), dict(triangles_out=ov.ptr + 16 * n + 16), dict(span_first=[])):
        assert holes.holes_device(**{**good, **change})[0] == abi.KT_ERR_ARG, change
        assert "bad argument" in _last_error()
    assert (ctx.download(ov, np.uint32, (4 * vcap + 4,)) == CV).all() and (ctx.download(ot, np.uint32, (3 * tcap,)) == CT).all() and (ctx.download(ol, np.uint32, (n,)) == CL).all()
    assert np.array_equal(ctx.download(dt, np.uint32, (m, 3)), tri) and np.array_equal(ctx.download(dv, V, (n,)).view(np.uint8), v.view(np.uint8))
    s, n_out, m_out, fo, stats = holes.holes_device(**good)                            # the object is still usable
    assert s == abi.KT_OK and (n_out, m_out) == (n_true, m_true) and np.array_equal(fo, want[2]) and stats == want[4]
    assert np.array_equal(ctx.download(ot, np.uint32, (m_true, 3)), want[1]) and np.array_equal(ctx.download(ol, np.uint32, (n,)), want[3])
    # n = 0: KT_OK and zeros with any valid table, null pointers included
    assert holes.holes_device(None, 0, None, 0, [0, 0, 0], k, None, 0, None, 0)[:3] == (abi.KT_OK, 0, 0)
    s, n_out, m_out, fo, stats = holes.holes_device(None, 0, dt, m, [0], k, None, 0, None, 0)   # (the triangles are not looked at: the restatement's rule)
    assert (s, n_out, m_out, fo.tolist(), stats) == (abi.KT_OK, 0, 0, [0], (0,) * 9)
    for b in (dv, dt, ov, ot, ol):
        b.free()


def test_allocations_return(ctx):
    ctx.sync()
    start = abi.live_allocations()
    w = abi.MeshHoles(ctx)
    created = abi.live_allocations()[0]
    assert created > start[0]
    case = cases.random_case(4, 257)
    _check_device(ctx, w, case, 8)
    device_form = abi.live_allocations()[0]
    assert device_form == created + 11 + 6 + 2                        # the per-vertex arrays, the per-half-edge arrays and the span table are the object's
    w.holes(*case, 8)
    assert abi.live_allocations()[0] == device_form + 5               # ... and so is the host form's staging
    w.holes(*cases.random_case(5, 65), 8)                             # a smaller call takes nothing
    assert abi.live_allocations()[0] == device_form + 5
    w.holes(*cases.random_case(6, 4099), 8)                           # a larger one releases and takes again
    assert abi.live_allocations()[0] == device_form + 5
    w.close()
    assert abi.live_allocations() == start


# ---- holes, components, simplify, normals, deform: all on the device ----------------------------------------------------------------------
def test_pipeline_on_the_device(ctx, holes, wanted, every_case):
    """the holed sphere under its table of empty and cut spans, filled on the device; the filled mesh and the pass's span table through
    kt_mesh_components_device, kt_mesh_simplify_device, kt_mesh_normals_device and kt_deform_apply_mesh_device, each equal to its
    restatement"""
    import deform_cases as dc
    import deform_mesh_cases as mc
    import mesh_simplify_cases as sc
    import mesh_weld_cases as wc
    from kintinuous_amd import deform_ref, mesh_components_ref, mesh_normals_ref, mesh_simplify_ref
    gname = "m20_n64_c7"
    v, tri, first = [c for n, c, _ in every_case if n == "spans"][0]
    want = wanted[("spans", 256)]
    n, m = len(v), len(tri)
    vcap, tcap = abi.MeshHoles.most(n, m)
    comp, simp, nrm, g = abi.MeshComponents(ctx), abi.MeshSimplify(ctx), abi.MeshNormals(ctx), abi.DeformationGraph(ctx, 20, 8)
    dv, dt = ctx.upload(v), ctx.upload(tri)
    fv, ft, fl = ctx.empty(16 * vcap), ctx.empty(12 * tcap), ctx.empty(4 * n)
    cv, ct, sv, st, on = ctx.empty(16 * vcap), ctx.empty(12 * tcap), ctx.empty(16 * vcap), ctx.empty(12 * tcap), ctx.empty(12 * vcap)
    try:
        gc = dc.case(gname)
        g.set_graph(gc["node_pos"], gc["node_time"])
        g.set_state(dc.restated(gname)[0])
        times = np.array([mc.span_times(20)[s % 9] for s in range(len(first) - 1)], np.uint64)
        s, nf, mf, ff, stats = holes.holes_device(dv, n, dt, m, first, 256, fv, vcap, ft, tcap, fl)
        assert s == abi.KT_OK and stats == want[4] and stats[5] == 7
        hv, ht = ctx.download(fv, V, (nf,)), ctx.download(ft, np.uint32, (mf, 3))
        cases.same((hv, ht, ff, ctx.download(fl, np.uint32, (n,))), want[:4])
        assert cases.edge_counts(ht) == (0, 2) and wc.closed(ht)                            # closed: V - E + F = 2 over the referenced vertices
        # components: one piece and the seven unreferenced ring centres and the loose vertices, which a threshold of 1 drops
        wc_ = mesh_components_ref.components(hv, ht, ff, 1)
        s, nc, mcnt, cf, cstats = comp.components_device(fv, nf, ft, mf, ff, 1, cv, vcap, ct, tcap)
        assert s == abi.KT_OK and cstats == wc_[4] and cstats[1] == 1 and (nc, mcnt) == (len(wc_[0]), mf)
        cases.same((ctx.download(cv, V, (nc,)), ctx.download(ct, np.uint32, (mcnt, 3)), cf), wc_[:3])
        cell = 2 * sc.VOXEL
        s, ns, ms, sf = simp.simplify_device(fv, nf, ft, mf, ff, cell, sv, vcap, st, tcap)
        assert s == abi.KT_OK and 0 < ns < nf and 0 < ms < mf
        cases.same((ctx.download(sv, V, (ns,)), ctx.download(st, np.uint32, (ms, 3)), sf), mesh_simplify_ref.simplify(hv, ht, ff, cell))
        s, n_zero = nrm.normals_device(fv, nf, ft, mf, on)
        wn, wz = mesh_normals_ref.normals(hv, ht)
        assert s == abi.KT_OK and n_zero == wz and np.array_equal(ctx.download(on, np.float32, (nf, 3)).view(np.uint8), wn.view(np.uint8))
        g.apply_mesh_device(fv, nf, ff, times)
        moved = ctx.download(fv, V, (nf,))
        assert moved.tobytes() == deform_ref.apply_mesh(dc.graph(gname), dc.restated(gname)[0], hv, ff, times).tobytes()
        assert np.abs(moved["xyz"] - hv["xyz"]).max() > 0
    finally:
        g.close()
        nrm.close()
        simp.close()
        comp.close()
        for b in (dv, dt, fv, ft, fl, cv, ct, sv, st, on):
            b.free()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def _rgb24(v):
    return v["rgb"][:, 0].astype(np.uint32) << 16 | v["rgb"][:, 1].astype(np.uint32) << 8 | v["rgb"][:, 2].astype(np.uint32)


def _holes_file(prefix):
    """<prefix>.holes -> (spans [(utime, first_in, first_out)], loops [(label, edges, filled)], (n_in, n_out, m_in, m_out) + the nine stats)"""
    lines = [l.split() for l in open(prefix + ".holes").read().splitlines()]
    spans = [(int(a), int(b), int(c)) for tag, a, b, c in (l for l in lines[:-1] if l[0] == "span")]
    loops = [(int(a), int(b), int(c)) for tag, a, b, c in (l for l in lines[:-1] if l[0] == "loop")]
    assert len(spans) + len(loops) == len(lines) - 1 and lines[-1][0] == "result" and len(lines[-1]) == 14
    assert [l[0] for l in lines[:-1]] == ["span"] * len(spans) + ["loop"] * len(loops)
    return spans, loops, tuple(int(x) for x in lines[-1][1:])


def _driver_holes_are_the_restatements(prefix, source, k):
    """<prefix>_fill.ply (k > 0) and <prefix>.holes against the restatement on what <prefix><source>.ply holds, with the first_in column of
    .holes as the span table -> (loops, result line).  The .ply keeps three colour bytes of four: the fourth of every vertex is compared as
    zero on both sides"""
    import deform_mesh_cases as mc
    v, tri = mc.read_ply(prefix + source + ".ply")
    spans, loops, result = _holes_file(prefix)
    n_in, n_out, m_in, m_out = result[:4]
    assert n_in == len(v) and m_in == len(tri)
    first = np.array([s[1] for s in spans] + [n_in], np.int64)
    full = np.zeros(n_in, V)
    full["xyz"], full["rgb"] = v["xyz"], _rgb24(v)
    rv, rt, rf, rl, stats = ref.holes(full, tri.astype(np.uint32), first, k)
    assert stats == result[4:] and (len(rv), len(rt)) == (n_out, m_out)
    assert [s[2] for s in spans] == rf[:-1].tolist() and rf[-1] == n_out
    labels = np.unique(rl[rl < ref.OPEN])
    counts = [int((rl == l).sum()) for l in labels]
    want_loops = [(int(l), c, int(3 <= c <= k)) for l, c in zip(labels, counts)]            # (the vertices of a mesh stage are all valid)
    assert loops == want_loops and sum(f for _, _, f in loops) == stats[5]
    if k > 0:
        fv, ftri = mc.read_ply(prefix + "_fill.ply")
        assert len(fv) == n_out and len(ftri) == m_out
        assert np.ascontiguousarray(rv["xyz"]).tobytes() == np.ascontiguousarray(fv["xyz"]).tobytes() and np.array_equal(rv["rgb"] & 0xffffff, _rgb24(fv))
        assert np.array_equal(rt.astype(np.int32), ftri)
    return loops, result


def test_driver_mh_on_the_welded_crab_walk(tmp_path):
    """kintinuous_hip -m -mw -mh <k> on the out-and-back crab-walk of tests/test_gpu_mesh_components.py's driver test (N = 96, 160 x 120, a
    5.2 m volume).  A first run at -mh 0 reports the simple loops of the run's own welded mesh and writes .holes only; k is then the
    smallest length when the loops have two lengths or more (some loop filled, some left), else that one length (all filled).  _fill.ply
    and .holes are the restatement applied to _weld.ply; every file of the run without -mh is byte-identical; -mh -ms feeds the filled
    mesh; -mh without -m and -mh 300 are ignored with a message."""
    run = drv.crab_walk_driver(tmp_path)

    rd = lambda p: open(p, "rb").read()
    _, p0 = run("plain", "-m", "-mw")
    _, p1 = run("report", "-m", "-mw", "-mh", "0")
    assert drv.outputs(tmp_path, p1) == sorted(drv.outputs(tmp_path, p0) + [".holes"])             # -mh 0 writes .holes only
    for ext in drv.outputs(tmp_path, p0):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    loops, result = _driver_holes_are_the_restatements(p1, "_weld", 0)
    lengths = sorted({edges for _, edges, _ in loops})
    print("crab-walk -mh 0: vertices %d, triangles %d; boundary %d, non-manifold %d, degenerate %d, loops %d, open %d, longest %d; lengths %s"
          % (result[0], result[2], result[4], result[5], result[6], result[7], result[8], result[10], [e for _, e, _ in loops]))
    if not loops:
        _, p2 = run("fill", "-m", "-mw", "-mh", "8")
        assert rd(p2 + "_fill.ply") == rd(p2 + "_weld.ply")                                   # no simple loop at all: nothing to fill
        return
    k = lengths[0]
    assert 3 <= k <= 256, "the shortest simple loop of the welded crab-walk is longer than the limit"
    out, p2 = run("fill", "-m", "-mw", "-mh", str(k))
    assert drv.outputs(tmp_path, p2) == sorted(drv.outputs(tmp_path, p0) + [".holes", "_fill.ply"])
    for ext in drv.outputs(tmp_path, p0):
        assert rd(p0 + ext) == rd(p2 + ext), ext
    loops2, result2 = _driver_holes_are_the_restatements(p2, "_weld", k)
    print("-mh %d: vertices %d -> %d, triangles %d -> %d, filled %d of %d loops" % (k, result2[0], result2[1], result2[2], result2[3], result2[9], result2[7]))
    filled = [f for _, _, f in loops2]
    if len(lengths) >= 2:
        assert 0 < sum(filled) < len(filled)                                                   # some loop is filled and some is left
    else:
        assert all(filled)
    assert result2[1] == result2[0] + sum(filled) and result2[3] == result2[2] + sum(e for _, e, f in loops2 if f)
    assert len([l for l in out.stdout.splitlines() if l.startswith("mesh ") and "_fill.ply:" in l]) == 1
    # -mh -ms: the simplification takes the filled mesh
    _, p3 = run("both", "-m", "-mw", "-mh", str(k), "-ms", "0.15")
    assert drv.outputs(tmp_path, p3) == sorted(drv.outputs(tmp_path, p2) + [".simp", "_simp.ply"])
    for ext in drv.outputs(tmp_path, p2):
        assert rd(p2 + ext) == rd(p3 + ext), ext
    simp_result = open(p3 + ".simp").read().splitlines()[-1].split()
    assert simp_result[0] == "result" and (int(simp_result[1]), int(simp_result[3])) == (result2[1], result2[3])
    # -mn: the filled file gets normals and a .normals line without further work
    _, p4 = run("nrm", "-m", "-mw", "-mh", str(k), "-mn")
    assert os.path.basename(p4) + "_fill.ply" in [l.split()[0] for l in open(p4 + ".normals").read().splitlines()]
    # ignored with a message
    nomesh, p5 = run("nomesh", "-mh", str(k))
    assert "-mh ignored without -m" in nomesh.stderr and not [e for e in drv.outputs(tmp_path, p5) if "fill" in e or "holes" in e or e.endswith(".ply")]
    big, p6 = run("big", "-m", "-mw", "-mh", "300")
    assert "-mh ignored" in big.stderr and drv.outputs(tmp_path, p6) == drv.outputs(tmp_path, p0)
    unwelded, p7 = run("unwelded", "-m", "-mh", "0")
    assert "every slab seam will show as a boundary" in unwelded.stderr and ".holes" in drv.outputs(tmp_path, p7)


def test_driver_mh_with_df_on_the_loop_log(tmp_path):
    """kintinuous_hip ... -lc -pg -pcd -df -m -mh 256 on the ten-frame walk of tests/test_gpu_deform_mesh.py's driver test: _fill.ply is
    the restatement's fill of .ply; _fill_def.ply has _fill.ply's faces and colours and its vertices where the deformation's restatement
    puts them, from the run's own .deform and the pass's span table in .holes (the rule of test_gpu_deform_mesh.py: every float the
    restatement's or its neighbour); every file of the run without -mh is byte-identical."""
    import deform_cases as dc
    import deform_mesh_cases as mc
    from kintinuous_amd import deform_ref
    run = drv.loop_log_driver(tmp_path)

    _, p0 = run("plain", "-m")
    _, p1 = run("fill", "-m", "-mh", "256")
    rd = lambda p: open(p, "rb").read()
    assert drv.outputs(tmp_path, p1) == sorted(drv.outputs(tmp_path, p0) + [".holes", "_fill.ply", "_fill_def.ply"])
    for ext in drv.outputs(tmp_path, p0):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    loops, result = _driver_holes_are_the_restatements(p1, "", 256)
    print("loop log -mh 256: vertices %d -> %d, triangles %d -> %d, boundary %d, loops %d, open %d, filled %d, longest %d"
          % (result[0], result[1], result[2], result[3], result[4], result[7], result[8], result[9], result[10]))
    before, faces = mc.read_ply(p1 + "_fill.ply")
    after, faces_after = mc.read_ply(p1 + "_fill_def.ply")
    assert np.array_equal(faces, faces_after) and len(faces) > 0 and len(before) == len(after) and before["rgb"].tobytes() == after["rgb"].tobytes()
    d = mc.deform_file(open(p1 + ".deform").read())
    pose_t = [p[0] for p in d["pose"]]
    orig = np.array([p[1:4] for p in d["pose"]], np.float32)
    keep = deform_ref.sample_nodes(orig, 0.02)
    graph = deform_ref.Graph(orig[keep], np.array([pose_t[k] for k in keep], np.uint64))
    src = np.array([c[1:4] for c in d["con"]], np.float32)
    x, _, _, _, _, status, _ = deform_ref.optimise(graph, src, np.array([c[0] for c in d["con"]], np.uint64), np.array([c[4:7] for c in d["con"]]), {"significant_error": 1e-9})
    assert status in (deform_ref.CONVERGED, deform_ref.MAX_STEPS)
    spans, _, _ = _holes_file(p1)
    v = np.zeros(len(before), V)
    v["xyz"] = before["xyz"]
    want = deform_ref.apply_mesh(graph, x, v, [s[2] for s in spans] + [len(before)], [s[0] for s in spans])
    got, wanted_xyz = after["xyz"].reshape(-1), want["xyz"].reshape(-1)
    near = (got == wanted_xyz) | (got == np.nextafter(wanted_xyz, np.float32(np.inf))) | (got == np.nextafter(wanted_xyz, np.float32(-np.inf)))
    near |= np.abs(got.astype(np.float64) - wanted_xyz.astype(np.float64)) <= 10 * dc.BOUND * (1.0 + float(np.abs(before["xyz"]).max()))
    assert near.all() and np.abs(after["xyz"] - before["xyz"]).max() > 0                   # ... and it was deformed
