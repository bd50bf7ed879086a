"""GPU: the quadric form of the mesh simplification (kt_mesh_simplify.hip) -- kt_mesh_simplify_quadric_device and kt_mesh_simplify_quadric
byte for byte against mesh_simplify_ref.simplify_quadric on synthetic lists, clusters that cross a wave, a workgroup and the head pass's
chunk, one cluster that takes every triangle's terms, the two forms in either order on one object, the errors, and the driver's -msq."""
import numpy as np
import pytest

import mesh_driver_cases as drv
import mesh_simplify_cases as mean_cases
import mesh_simplify_quadric_cases as cases
from kintinuous_amd import abi, mesh_simplify_ref as ref

pytestmark = pytest.mark.gpu

V = abi.MESH_VERTEX_DTYPE
GUARD = 5
CV, CT = 0xA5A5A5A5, 0x3C3C3C3C
BIAS = cases.DEFAULT_BIAS


@pytest.fixture(scope="module")
def simp(ctx):
    w = abi.MeshSimplify(ctx)
    yield w
    w.close()


def _device(ctx, simp, case, bias, vcap=None, tcap=None):
    """kt_mesh_simplify_quadric_device (bias None: kt_mesh_simplify_device) on uploads with canaries behind every buffer -> (status,
    n_out, m_out, span_first_out, n_placed, outputs as left, inputs as left)"""
    v, tri, first, cell = case
    n, m = len(v), len(tri)
    vcap = n if vcap is None else vcap
    tcap = m if tcap is None else tcap
    dv = ctx.upload(np.concatenate([v.view(np.uint32).reshape(-1), np.full(4 * GUARD, CV, np.uint32)]))
    dt = ctx.upload(np.concatenate([tri.reshape(-1), np.full(3 * GUARD, CT, np.uint32)]))
    ov = ctx.upload(np.full(4 * (vcap + GUARD), CV, np.uint32))
    ot = ctx.upload(np.full(3 * (tcap + GUARD), CT, np.uint32))
    if bias is None:
        s, n_out, m_out, fo = simp.simplify_device(dv, n, dt, m, first, cell, ov, vcap, ot, tcap)
        placed = 0
    else:
        s, n_out, m_out, fo, placed = simp.simplify_quadric_device(dv, n, dt, m, first, cell, bias, ov, vcap, ot, tcap)
    out = (ctx.download(ov, np.uint32, (4 * (vcap + GUARD),)), ctx.download(ot, np.uint32, (3 * (tcap + GUARD),)))
    ins = (ctx.download(dv, np.uint32, (4 * (n + GUARD),)), ctx.download(dt, np.uint32, (3 * (m + GUARD),)))
    for b in (dv, dt, ov, ot):
        b.free()
    return s, n_out, m_out, fo, placed, out, ins


def _want(case, bias):
    return (*ref.simplify(*case), 0) if bias is None else ref.simplify_quadric(*case, bias)


def _check_device(ctx, simp, case, bias, want=None):
    v, tri, first, cell = case
    n, m = len(v), len(tri)
    wv, wt, wf, wp = _want(case, bias) if want is None else want
    s, n_out, m_out, fo, placed, (ov, ot), (iv, it) = _device(ctx, simp, case, bias)
    assert s == abi.KT_OK and (n_out, m_out, placed) == (len(wv), len(wt), wp)
    assert np.array_equal(ov[:4 * n_out], wv.view(np.uint32).reshape(-1)) and np.array_equal(ot[:3 * m_out], wt.reshape(-1)) and np.array_equal(fo, wf)
    assert (ov[4 * n_out:] == CV).all() and (ot[3 * m_out:] == CT).all()                              # nothing behind the outputs
    assert np.array_equal(iv[:4 * n], v.view(np.uint32).reshape(-1)) and (iv[4 * n:] == CV).all()     # the inputs are read only
    assert np.array_equal(it[:3 * m], tri.reshape(-1)) and (it[3 * m:] == CT).all()
    return (wv, wt, wf, wp), (ov, ot, fo)


def _check_both(ctx, simp, case, bias=BIAS):
    want, got = _check_device(ctx, simp, case, bias)
    _, again = _check_device(ctx, simp, case, bias, want)                 # a second call: the same bytes
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    s, hv, ht, hf, n_out, m_out, placed = simp.simplify_quadric_host(*case, bias)
    assert s == abi.KT_OK and (n_out, m_out) == (len(want[0]), len(want[1]))
    cases.same4((hv, ht, hf, placed), want)
    return want


@pytest.mark.parametrize("n", cases.SIZES)
def test_lists_device_and_host_forms(ctx, simp, n):
    for seed, spans, per, bias in ((n, 6, 3.0, 2.0 ** -6), (n + 1, 9, 1.0, 2.0 ** -10), (n + 2, 1, 20.0, 1.0), (n + 3, 40, 4.0, 2.0 ** -20)):
        want = _check_both(ctx, simp, cases.random_case(seed, n, spans, per), bias)
        if n >= 257:
            assert 0 < len(want[0]) < n and 0 < len(want[1]) and want[3] > 0
    # no triangles: m = 0, every cluster keeps the mean (t = 0)
    v, _, first, cell = cases.random_case(n, n, 6, 3.0)
    want = _check_both(ctx, simp, (v, np.zeros((0, 3), np.uint32), first, cell))
    assert want[3] == 0


def test_cluster_sizes_one_cluster_and_a_table_beyond_lds(ctx, simp):
    """clusters of 1, 2, 63, 64, 65, 257 and 2049 members; 4099 vertices in one cluster with 8000 triangles, every atomic on the same nine
    words; a table of 3000 spans, searched in global memory"""
    case = cases.sized_clusters_case()
    sizes = np.bincount(ref.cluster_of(case[0]["xyz"], case[2], case[3]))
    assert sorted(sizes.tolist()) == sorted(list(cases.CLUSTER_SIZES) * 3)
    want = _check_both(ctx, simp, case)
    assert want[3] > 0
    case = cases.one_cluster_case()
    assert len(case[0]) == 4099 and len(case[1]) == 8000
    want = _check_both(ctx, simp, case)
    assert len(want[0]) == 1 and len(want[1]) == 0
    want = _check_both(ctx, simp, cases.many_spans_case(), 2.0 ** -10)
    assert want[3] > 0


def test_small_cell_returns_the_input_and_the_cube_is_the_restatements(ctx, simp):
    v, t = mean_cases.sphere_mesh()
    out = simp.simplify_quadric(v, t, [0, len(v)], 1e-4, BIAS)
    cases.same4(out, (v, t, np.array([0, len(v)], np.int64), 0))
    v, t = cases.cube_mesh()
    for cell in (0.11, 0.33):
        for bias in (2.0 ** -6, 2.0 ** -10):
            cases.same4(simp.simplify_quadric(v, t, [0, len(v)], cell, bias), ref.simplify_quadric(v, t, [0, len(v)], cell, bias))


def test_the_two_forms_in_either_order_equal_a_fresh_object(ctx):
    small, large = cases.random_case(1, 65), cases.random_case(2, 4099, 40, 4.0)
    a, b, c = abi.MeshSimplify(ctx), abi.MeshSimplify(ctx), abi.MeshSimplify(ctx)
    try:
        _check_device(ctx, a, small, None)                                   # mean, then quadric (small, then large)
        want, got = _check_device(ctx, a, large, BIAS)
        _, fresh = _check_device(ctx, b, large, BIAS, want)
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh))
        want, got = _check_device(ctx, a, large, None)                       # quadric, then mean: simplify()'s bytes
        _, fresh = _check_device(ctx, c, large, None, want)
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh))
        mean_cases.same(a.simplify(*large), ref.simplify(*large))
        cases.same4(a.simplify_quadric(*small, BIAS), ref.simplify_quadric(*small, BIAS))
        cases.same4(c.simplify_quadric(*large, 2.0 ** -10), ref.simplify_quadric(*large, 2.0 ** -10))   # the first quadric call after mean calls
    finally:
        for w in (a, b, c):
            w.close()


def test_errors_leave_everything_intact(ctx, simp):
    case = cases.random_case(9, 4099, 6, 3.0)
    v, tri, first, cell = case
    n, m = len(v), len(tri)
    want = ref.simplify_quadric(*case, BIAS)
    n_keep, m_keep = len(want[0]), len(want[1])
    assert 0 < n_keep < n and 0 < m_keep < m

    def intact(res):
        _, _, _, fo, placed, (ov, ot), (iv, it) = res
        assert (ov == CV).all() and (ot == CT).all() and placed == 0
        assert np.array_equal(iv[:4 * n], v.view(np.uint32).reshape(-1)) and np.array_equal(it[:3 * m], tri.reshape(-1))
        assert (fo == -1).all()                                                        # span_first_out untouched as well

    for vcap, tcap in ((n_keep - 1, m), (n, m_keep - 1), (n_keep - 1, m_keep - 1), (0, 0)):
        res = _device(ctx, simp, case, BIAS, vcap=vcap, tcap=tcap)
        assert res[0] == abi.KT_ERR_CAPACITY and res[1:3] == (n_keep, m_keep)          # both true counts
        intact(res)
    res = _device(ctx, simp, case, BIAS, vcap=n_keep, tcap=m_keep)                     # the smallest that fit
    assert res[0] == abi.KT_OK and res[1:3] == (n_keep, m_keep) and res[4] == want[3]
    for kw in (dict(vertex_capacity=n_keep - 1), dict(triangle_capacity=m_keep - 1)):
        s, hv, ht, hf, n_out, m_out, placed = simp.simplify_quadric_host(v, tri, first, cell, BIAS, **kw)
        assert s == abi.KT_ERR_CAPACITY and (n_out, m_out, placed) == (n_keep, m_keep, 0) and not hv.view(np.uint32).any() and not ht.any() and (hf == -1).all()

    def refused(bad_case, bias=BIAS, restated=True):
        if restated:
            with pytest.raises(ValueError):
                ref.simplify_quadric(*bad_case, bias)
        res = _device(ctx, simp, bad_case, bias)
        assert res[0] == abi.KT_ERR_ARG and res[1:3] == (0, 0) and res[4] == 0
        _, _, _, fo, _, (ov, ot), (iv, it) = res
        assert (ov == CV).all() and (ot == CT).all() and (fo == -1).all()
        assert np.array_equal(iv[:4 * len(bad_case[0])], bad_case[0].view(np.uint32).reshape(-1)) and np.array_equal(it[:3 * len(bad_case[1])], bad_case[1].reshape(-1))
        s, hv, ht, hf, _, _, placed = simp.simplify_quadric_host(*bad_case, bias)
        assert s == abi.KT_ERR_ARG and not hv.view(np.uint32).any() and not ht.any() and (hf == -1).all() and placed == 0

    for bias in (0.0, 2.0 ** -21, float(np.nextafter(np.float32(2.0 ** -20), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2))), 2.0, -0.5,
                 float("nan"), float("inf"), float("-inf")):
        refused(case, bias)
    _check_device(ctx, simp, case, 2.0 ** -20)                                         # the ends of the range are in it
    _check_device(ctx, simp, case, 1.0)
    for bad in (n, n + 7, 0xffffffff):                                                 # an index >= n: found on the device
        tb = tri.copy()
        tb[m // 2, 1] = bad
        refused((v, tb, first, cell))
    big = np.zeros(3, V)                                                               # a term of 1 or more: one 2 m triangle
    big["xyz"][1, 0], big["xyz"][2, 1] = 2.0, 2.0
    one = np.array([[0, 1, 2]], np.uint32)
    refused((big, one, np.array([0, 3]), 0.25))
    big["xyz"] *= 0.25
    _check_device(ctx, simp, (big, one, np.array([0, 3]), 0.25), BIAS)
    for pos, axis, val in ((0, 0, float("nan")), (n // 2, 1, float("inf")), (n - 1, 2, 8192.0), (7, 0, -8192.0)):   # invalid vertices
        vb = v.copy()
        vb["xyz"][pos, axis] = val
        refused((vb, tri, first, cell))
    for f in (np.array([1] + first[1:].tolist()), np.array(first[:-1].tolist() + [n - 1]), np.array([0, 9, 5] + first[3:].tolist())):   # bad tables
        refused((v, tri, f, cell))
    for bad in (0.0, -0.25, float("inf"), float("nan")):
        refused((v, tri, first, bad))
    # null pointers with n > 0, misaligned vertices, an output that is an input, a null n_placed is the binding's own, m > 2^29
    dv, dt = ctx.upload(v), ctx.upload(tri)
    ov, ot = ctx.empty(16 * n + 16), ctx.empty(12 * m)
    good = dict(vertices=dv, n=n, triangles=dt, m=m, span_first=first, cell=cell, bias=BIAS, vertices_out=ov, vertex_capacity=n, triangles_out=ot, triangle_capacity=m)
    for change in (dict(vertices=None), dict(triangles=None), dict(vertices_out=None), dict(triangles_out=None), dict(vertices=dv.ptr + 8),
                   dict(vertices_out=ov.ptr + 4), dict(vertices_out=dv), dict(triangles_out=dt), dict(m=(1 << 29) + 1)):
        assert simp.simplify_quadric_device(**{**good, **change})[0] == abi.KT_ERR_ARG, change
    s, n_out, m_out, fo, placed = simp.simplify_quadric_device(**good)                  # the object is still usable
    assert s == abi.KT_OK and (n_out, m_out, placed) == (n_keep, m_keep, want[3]) and np.array_equal(fo, want[2])
    assert np.array_equal(ctx.download(ot, np.uint32, (m_keep, 3)), want[1])
    assert ctx.download(ov, V, (n_keep,)).tobytes() == want[0].tobytes()
    # n = 0: KT_OK with any valid table, null pointers included, whatever the triangle count says
    assert simp.simplify_quadric_device(None, 0, None, 0, [0, 0, 0], cell, BIAS, None, 0, None, 0)[:3] == (abi.KT_OK, 0, 0)
    s, n_out, m_out, fo, placed = simp.simplify_quadric_device(None, 0, None, 0, [0], cell, BIAS, None, 0, None, 0)
    assert (s, n_out, m_out, fo.tolist(), placed) == (abi.KT_OK, 0, 0, [0], 0)
    for b in (dv, dt, ov, ot):
        b.free()


def test_allocations_return_and_the_mean_form_takes_no_more(ctx):
    ctx.sync()
    start = abi.live_allocations()
    w, plain = abi.MeshSimplify(ctx), abi.MeshSimplify(ctx)
    created = abi.live_allocations()[0]
    assert created > start[0]
    case = cases.random_case(4, 257)
    _check_device(ctx, plain, case, None)
    mean_only = abi.live_allocations()[0]
    per_object = mean_only - created
    _check_device(ctx, w, case, None)
    assert abi.live_allocations()[0] == mean_only + per_object > mean_only           # two objects, the same allocations each
    _check_device(ctx, w, case, BIAS)
    assert abi.live_allocations()[0] == mean_only + per_object + 1                   # the nine sums: one buffer, on the first quadric call
    _check_device(ctx, w, cases.random_case(5, 65), BIAS)                            # a smaller call takes nothing
    _check_device(ctx, w, case, None)
    assert abi.live_allocations()[0] == mean_only + per_object + 1
    w.simplify_quadric(*cases.random_case(6, 4099), BIAS)                            # a larger one releases and takes again (and the staging)
    assert abi.live_allocations()[0] == mean_only + per_object + 1 + 4
    w.close()
    plain.close()
    assert abi.live_allocations() == start


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def _rgb24(v):
    return v["rgb"][:, 0].astype(np.uint32) << 16 | v["rgb"][:, 1].astype(np.uint32) << 8 | v["rgb"][:, 2].astype(np.uint32)


def _driver_simp_is_the_restatements(prefix, source, cell, bias):
    """<prefix>_simp.ply and <prefix>.simp against the restatement's quadric simplification of what <prefix><source>.ply holds, with the
    first_in column of .simp as the span table -> (n_in, n_out, m_in, m_out, spans, placed, multi-member clusters)"""
    import deform_mesh_cases as mc
    v, tri = mc.read_ply(prefix + source + ".ply")
    lines = [l.split() for l in open(prefix + ".simp").read().splitlines()]
    spans = [(int(a), int(b), int(c)) for tag, a, b, c in lines[:-2] if tag == "span"]
    assert len(spans) == len(lines) - 2 and lines[-2][0] == "result" and lines[-1][0] == "quadric" and len(lines[-1]) == 4
    n_in, n_out, m_in, m_out = (int(x) for x in lines[-2][1:5])
    assert float.fromhex(lines[-2][5]) == float(np.float32(cell)) and float.fromhex(lines[-1][1]) == float(np.float32(bias))
    assert n_in == len(v) and m_in == len(tri)
    first = np.array([s[1] for s in spans] + [n_in], np.int64)
    full = np.zeros(n_in, V)
    full["xyz"], full["rgb"] = v["xyz"], _rgb24(v)
    rv, rt, rf, placed = ref.simplify_quadric(full, tri.astype(np.uint32), first, cell, bias)
    many = int(cases.multi_member(full, first, cell).sum())
    assert (int(lines[-1][2]), int(lines[-1][3])) == (placed, many)
    sv, stri = mc.read_ply(prefix + "_simp.ply")
    assert len(rv) == n_out == len(sv) and len(rt) == m_out == len(stri)
    assert np.ascontiguousarray(rv["xyz"]).tobytes() == np.ascontiguousarray(sv["xyz"]).tobytes() and np.array_equal(rv["rgb"], _rgb24(sv))
    assert np.array_equal(rt.astype(np.int32), stri)
    assert [s[2] for s in spans] == rf[:-1].tolist() and rf[-1] == n_out
    mean = ref.simplify(full, tri.astype(np.uint32), first, cell)[0]
    assert mean["xyz"].tobytes() != rv["xyz"].tobytes()                                   # ... and it is not the mean form's
    return n_in, n_out, m_in, m_out, len(spans), placed, many


def _same_but_simp(tmp_path, p0, p1):
    """every file of the run without -msq is there with it, byte-identical but for _simp*.ply and .simp"""
    rd = lambda p: open(p, "rb").read()
    assert drv.outputs(tmp_path, p1) == drv.outputs(tmp_path, p0)
    changed = [ext for ext in drv.outputs(tmp_path, p0) if rd(p0 + ext) != rd(p1 + ext)]
    assert set(changed) <= {".simp", "_simp.ply", "_simp_def.ply"} and {".simp", "_simp.ply"} <= set(changed), changed
    return changed


def test_driver_msq_on_the_welded_crab_walk(tmp_path):
    """kintinuous_hip -m -mw -ms 0.15 -msq on the out-and-back crab-walk of tests/test_gpu_mesh_simplify.py: _simp.ply and .simp are the
    restatement's quadric simplification of the run's own _weld.ply at the default bias; every other file is byte-identical to the run
    with -ms alone; -msq and -msb without -ms are ignored with a message."""
    run = drv.crab_walk_driver(tmp_path)

    _, p0 = run("mean", "-m", "-mw", "-ms", "0.15")
    _, p1 = run("quad", "-m", "-mw", "-ms", "0.15", "-msq")
    alone, p2 = run("alone", "-m", "-mw", "-msq", "-msb", "0.25")
    _same_but_simp(tmp_path, p0, p1)
    assert "-msq ignored without -ms" in alone.stderr and "-msb ignored without -ms" in alone.stderr
    assert not [e for e in drv.outputs(tmp_path, p2) if "simp" in e] and "_weld.ply" in drv.outputs(tmp_path, p2)
    got = _driver_simp_is_the_restatements(p1, "_weld", 0.15, 2.0 ** -6)
    print("crab-walk: vertices %d -> %d, triangles %d -> %d in %d spans, %d of %d clusters placed" % got)
    n_in, n_out, m_in, m_out, n_spans, placed, many = got
    assert n_spans > 1 and 0 < n_out < n_in and 0 < m_out < m_in and 0 < placed <= many
    # the mean form's file is what it was: the restatement's simplify() of the same _weld.ply
    import deform_mesh_cases as mc
    v, tri = mc.read_ply(p0 + "_weld.ply")
    lines = [l.split() for l in open(p0 + ".simp").read().splitlines()]
    assert lines[-1][0] == "result"
    full = np.zeros(len(v), V)
    full["xyz"], full["rgb"] = v["xyz"], _rgb24(v)
    first = np.array([int(l[2]) for l in lines[:-1]] + [len(v)], np.int64)
    rv = ref.simplify(full, tri.astype(np.uint32), first, 0.15)[0]
    assert np.ascontiguousarray(rv["xyz"]).tobytes() == np.ascontiguousarray(mc.read_ply(p0 + "_simp.ply")[0]["xyz"]).tobytes()


def test_driver_msq_with_df_on_the_loop_log(tmp_path):
    """kintinuous_hip ... -lc -pg -pcd -df -m -ms 0.05 -msq -msb 0.001 on the ten-frame walk of tests/test_gpu_mesh_simplify.py's driver
    test: _simp.ply and .simp are the restatement's quadric simplification of the run's own .ply; _simp_def.ply has _simp.ply's faces and
    colours and moved vertices; every other file is byte-identical to the run with -ms alone."""
    import deform_mesh_cases as mc
    run = drv.loop_log_driver(tmp_path)

    _, p0 = run("mean", "-m", "-ms", "0.05")
    _, p1 = run("quad", "-m", "-ms", "0.05", "-msq", "-msb", "0.001")
    changed = _same_but_simp(tmp_path, p0, p1)
    assert "_simp_def.ply" in changed
    got = _driver_simp_is_the_restatements(p1, "", 0.05, 0.001)
    print("loop log: vertices %d -> %d, triangles %d -> %d in %d spans, %d of %d clusters placed" % got)
    assert 0 < got[1] < got[0] and 0 < got[3] < got[2] and 0 < got[5] <= got[6]
    sv, stri = mc.read_ply(p1 + "_simp.ply")
    dv, dtri = mc.read_ply(p1 + "_simp_def.ply")
    assert np.array_equal(stri, dtri) and len(sv) == len(dv) and sv["rgb"].tobytes() == dv["rgb"].tobytes()
    assert np.abs(dv["xyz"] - sv["xyz"]).max() > 0                                          # ... and it was deformed
