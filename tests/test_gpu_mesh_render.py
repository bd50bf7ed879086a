"""GPU: the rasteriser of the -m mesh (kt_mesh_render.hip) -- kt_mesh_render_device and kt_mesh_render byte for byte against
kintinuous_amd/mesh_render_ref.py on every case of mesh_render_cases, every subset of the output pointers, a large call after a small
one, the errors with canaries, the chain from the volume to the image on the device against the ray cast's depth image, and the driver's
-mv, -mvf, -mvb and, with -df, the deformed twin."""
import itertools
import os

import numpy as np
import pytest

import mesh_driver_cases as drv
import mesh_render_cases as cases
from kintinuous_amd import abi, mesh_render_ref as ref

pytestmark = pytest.mark.gpu

V = abi.MESH_VERTEX_DTYPE
GUARD = 5
CV, CT = 0xA5A5A5A5, 0x3C3C3C3C
CANARY = {"index": 0x5EEDF00D, "depth": 0xBEEF, "color": 0xC3, "model": 0x7E}
DTYPE = {"index": np.uint32, "depth": np.uint16, "color": np.uint8, "model": np.uint8}
WIDTH = {"index": 1, "depth": 1, "color": 3, "model": 3}
PLANES = cases.PLANES
NONE = (-1, -1, -1, -1)                               # the stats of a call that left them alone


@pytest.fixture(scope="module")
def ren(ctx):
    w = abi.MeshRender(ctx)
    yield w
    w.close()


def _device(ctx, ren, s, planes=PLANES, **change):
    """kt_mesh_render_device on uploads with canaries behind every buffer -> (status, stats, {plane: buffer as left}, inputs as left)"""
    v, tri = s["v"], s["tri"]
    n, m, pixels = len(v), len(tri), s["cols"] * s["rows"]
    dv = ctx.upload(np.concatenate([v.view(np.uint32).reshape(-1), np.full(4 * GUARD, CV, np.uint32)]))
    dt = ctx.upload(np.concatenate([tri.reshape(-1), np.full(3 * GUARD, CT, np.uint32)]))
    outs = {p: ctx.upload(np.full(WIDTH[p] * (pixels + GUARD), CANARY[p], DTYPE[p])) for p in planes}
    kw = dict(vertices=dv, n=n, triangles=dt, m=m, intr=s["intr"], cols=s["cols"], rows=s["rows"], R=s["R"], t=s["t"], near=s["near"])
    kw.update({p: outs.get(p) for p in PLANES})
    kw.update(change)
    status, stats = ren.render_device(**kw)
    got = {p: ctx.download(outs[p], DTYPE[p], (WIDTH[p] * (pixels + GUARD),)) for p in planes}
    ins = (ctx.download(dv, np.uint32, (4 * (n + GUARD),)), ctx.download(dt, np.uint32, (3 * (m + GUARD),)))
    for b in [dv, dt] + list(outs.values()):
        b.free()
    return status, stats, got, ins


def _inputs_intact(s, ins):
    n, m = len(s["v"]), len(s["tri"])
    assert np.array_equal(ins[0][:4 * n], s["v"].view(np.uint32).reshape(-1)) and (ins[0][4 * n:] == CV).all()      # the inputs are read only
    assert np.array_equal(ins[1][:3 * m], s["tri"].reshape(-1)) and (ins[1][3 * m:] == CT).all()


def _check_device(ctx, ren, s, want, planes=PLANES):
    pixels = s["cols"] * s["rows"]
    status, stats, got, ins = _device(ctx, ren, s, planes)
    assert status == abi.KT_OK and stats == want[4]
    for p in planes:
        k = WIDTH[p] * pixels
        assert np.array_equal(got[p][:k], want[PLANES.index(p)].reshape(-1)), p
        assert (got[p][k:] == CANARY[p]).all(), p                                                                     # nothing behind the output
    _inputs_intact(s, ins)
    return got


def _check_both(ctx, ren, s, want):
    got = _check_device(ctx, ren, s, want)
    again = _check_device(ctx, ren, s, want)                                                                          # a second call: the same bytes
    assert all(np.array_equal(got[p], again[p]) for p in PLANES)
    status, res, stats = ren.render_host(*cases.args(s))
    assert status == abi.KT_OK and stats == want[4]
    for k, p in enumerate(PLANES):
        assert res[p].shape == want[k].shape and np.array_equal(res[p], want[k]), p


@pytest.mark.parametrize("name", cases.names())
def test_every_case_device_and_host_forms(ctx, ren, name):
    """(the shuffled soup among them: the bytes of the restatement of the shuffled list)"""
    _check_both(ctx, ren, cases.case(name), cases.want(name))


def test_every_subset_of_the_outputs(ctx, ren):
    s, want = cases.case("sweep"), cases.want("sweep")
    for k in range(len(PLANES) + 1):
        for planes in itertools.combinations(PLANES, k):
            _check_device(ctx, ren, s, want, planes)
            status, res, stats = ren.render_host(*cases.args(s), planes=planes)
            assert status == abi.KT_OK and stats == want[4] and set(res) == set(planes)
            assert all(np.array_equal(res[p], want[PLANES.index(p)]) for p in planes)


def test_large_after_small_equals_a_fresh_object(ctx):
    small, large = "centres 7x5", "sphere outside"
    a, b = abi.MeshRender(ctx), abi.MeshRender(ctx)
    try:
        _check_device(ctx, a, cases.case(small), cases.want(small))
        got = _check_device(ctx, a, cases.case(large), cases.want(large))
        fresh = _check_device(ctx, b, cases.case(large), cases.want(large))
        assert all(np.array_equal(got[p], fresh[p]) for p in PLANES)
        _check_device(ctx, a, cases.case(small), cases.want(small))                  # ... and a small one after it
        for name in (small, large, "fill 160x120"):
            x, y = a.render(*cases.args(cases.case(name))), b.render(*cases.args(cases.case(name)))
            assert x[4] == y[4] == cases.want(name)[4] and all(np.array_equal(p, q) for p, q in zip(x[:4], y[:4]))
    finally:
        a.close()
        b.close()


def test_allocations_return(ctx):
    ctx.sync()
    start = abi.live_allocations()
    w = abi.MeshRender(ctx)
    created = abi.live_allocations()[0]
    assert created > start[0]
    _check_device(ctx, w, cases.case("fan"), cases.want("fan"))
    device_form = abi.live_allocations()[0]
    assert device_form == created + 3                                 # the records, the pixel words and the list are the object's
    w.render(*cases.args(cases.case("fan")))
    assert abi.live_allocations()[0] == device_form + 6               # ... and so is the host form's staging
    w.render(*cases.args(cases.case("centres 7x5")))                  # a smaller call takes nothing
    assert abi.live_allocations()[0] == device_form + 6
    w.render(*cases.args(cases.case("sphere inside")))                # a larger one releases and takes again
    assert abi.live_allocations()[0] == device_form + 6
    w.close()
    assert abi.live_allocations() == start


def test_errors_leave_everything_intact(ctx, ren):
    name = "fan"
    s, want = cases.case(name), cases.want(name)
    v, tri = s["v"], s["tri"]
    n, m, pixels = len(v), len(tri), s["cols"] * s["rows"]

    def refused(bad, cause):
        with pytest.raises(ValueError, match=cause):
            ref.render(*cases.args(bad))
        status, stats, got, ins = _device(ctx, ren, bad)
        assert status == abi.KT_ERR_ARG and stats == NONE
        assert all((got[p] == CANARY[p]).all() for p in PLANES)                      # every output keeps its pattern in full
        _inputs_intact(bad, ins)
        keep = {p: np.full((bad["rows"], bad["cols"]) + ((3,) if WIDTH[p] == 3 else ()), CANARY[p], DTYPE[p]) for p in PLANES}
        status, res, stats = ren.render_host(*cases.args(bad), out=keep)
        assert status == abi.KT_ERR_ARG and stats == NONE and all((res[p] == CANARY[p]).all() for p in PLANES)       # ... and so does the host form's
        _check_device(ctx, ren, s, want)                                             # the same object's next valid call is correct

    for row, col in ((0, 0), (m // 2, 1), (m - 1, 2)):                               # an index out of range
        tb = tri.copy()
        tb[row, col] = n if row else 0xffffffff
        refused({**s, "tri": tb}, "index out of range")
    for k, (axis, val) in enumerate(((0, float("nan")), (1, float("inf")), (2, 8192.0), (0, -8192.0), (1, float("-inf")))):
        vb = v.copy()                                                                # an invalid vertex that a triangle references
        vb["xyz"][1 + k, axis] = val
        refused({**s, "v": vb}, "not finite or has a coordinate")
        vu = np.concatenate([v, vb[1 + k:2 + k]])                                    # ... and the same one unreferenced: accepted
        _check_device(ctx, ren, {**s, "v": vu}, want)
    eq = np.concatenate([tri, [[1, 1, n - 1]]]).astype(np.uint32)                    # a triangle with two equal indices still references its vertices
    vb = v.copy()
    vb["xyz"][1, 0] = np.nan
    refused({**s, "v": vb, "tri": eq}, "not finite or has a coordinate")
    # sizes over 2^29 with dummy pointers: refused before anything is allocated
    start = abi.live_allocations()
    for nn, mm in (((1 << 29) + 1, 1), (3, (1 << 29) + 1)):
        assert ren.render_device(0x10000, nn, 0x20000, mm, s["intr"], 4, 4, s["R"], s["t"], 0.05, None, None, None, None) == (abi.KT_ERR_ARG, NONE)
    assert abi.live_allocations() == start
    # every argument bound, null and misaligned pointers, outputs that are or overlap an input or another output
    dv, dt = ctx.upload(v), ctx.upload(tri)
    outs = {p: ctx.upload(np.full(WIDTH[p] * pixels, CANARY[p], DTYPE[p])) for p in PLANES}
    good = dict(vertices=dv, n=n, triangles=dt, m=m, intr=s["intr"], cols=s["cols"], rows=s["rows"], R=s["R"], t=s["t"], near=s["near"], **outs)
    nan, inf = float("nan"), float("inf")
    bad_R = s["R"].copy()
    bad_R[1, 2] = nan
    for change in (dict(vertices=None), dict(triangles=None), dict(vertices=dv.ptr + 8), dict(intr=None), dict(R=None), dict(t=None),
                   dict(cols=0), dict(rows=0), dict(cols=-3), dict(cols=8193, rows=1), dict(cols=1, rows=8193),
                   dict(intr=(0.0, 64.0, 33.0, 21.0)), dict(intr=(64.0, -64.0, 33.0, 21.0)), dict(intr=(nan, 64.0, 33.0, 21.0)), dict(intr=(64.0, 64.0, inf, 21.0)),
                   dict(intr=(64.0, 64.0, 33.0, nan)), dict(R=bad_R), dict(t=(0.0, nan, 0.0)), dict(t=(8192.0, 0.0, 0.0)), dict(t=(0.0, 0.0, -8192.0)), dict(t=(inf, 0.0, 0.0)),
                   dict(near=0.0), dict(near=0.00099), dict(near=8192.0), dict(near=-1.0), dict(near=nan),
                   dict(index=dv), dict(color=dt), dict(depth=outs["index"]), dict(model=outs["color"].ptr + 3 * pixels - 1), dict(depth=dv.ptr + 16 * (n - 1)),
                   dict(index=outs["depth"].ptr + 2 * pixels - 4, depth=outs["depth"])):
        assert ren.render_device(**{**good, **change}) == (abi.KT_ERR_ARG, NONE), change
    for p in PLANES:
        assert (ctx.download(outs[p], DTYPE[p], (WIDTH[p] * pixels,)) == CANARY[p]).all(), p
    assert np.array_equal(ctx.download(dt, np.uint32, (m, 3)), tri) and np.array_equal(ctx.download(dv, V, (n,)).view(np.uint8), v.view(np.uint8))
    assert ren.render_device(**good) == (abi.KT_OK, want[4])                         # the object is still usable
    for k, p in enumerate(PLANES):
        assert np.array_equal(ctx.download(outs[p], DTYPE[p], (WIDTH[p] * pixels,)), want[k].reshape(-1)), p
    for change in (dict(near=0.001), dict(t=(8191.0, 0.0, 0.0)), dict(cols=8192, rows=1, index=None, depth=None, color=None, model=None)):
        kw = {**good, **change}                                                      # the bounds themselves are allowed
        wanted = ref.render(v, tri, kw["intr"], kw["cols"], kw["rows"], kw["R"], kw["t"], kw["near"])[4]
        assert ren.render_device(**kw) == (abi.KT_OK, wanted), change
    # n = 0 or m = 0: an empty image
    for kw in (dict(vertices=None, n=0, triangles=None, m=0), dict(vertices=None, n=0), dict(triangles=None, m=0)):
        assert ren.render_device(**{**good, **kw}) == (abi.KT_OK, (0, 0, 0, 0)), kw
        assert (ctx.download(outs["index"], np.uint32, (pixels,)) == ref.NO_TRIANGLE).all()
        assert not any(ctx.download(outs[p], DTYPE[p], (WIDTH[p] * pixels,)).any() for p in PLANES[1:])
        assert ren.render_device(**good) == (abi.KT_OK, want[4])
    empty = ren.render(v[:0], tri[:0], s["intr"], 7, 5, s["R"], s["t"])
    assert empty[4] == (0, 0, 0, 0) and (empty[0] == ref.NO_TRIANGLE).all() and not empty[1].any() and not empty[2].any() and not empty[3].any()
    for b in [dv, dt] + list(outs.values()):
        b.free()


# ---- volume -> mesh -> image against volume -> ray cast -> depth image: all on the device -------------------------------------------------
# Measured on the CPU (profiles/mesh_render.md) with mesh_ref.extract_mesh + the restatement against the oracle's ray cast and depth image
# on the same volume and pose: over the 6597 pixels valid in both, the median |depth difference| is 3.0 mm and the maximum 219 mm (at
# the silhouette, where the ray cast's trilinear zero crossing and the mesh's linear one along voxel edges part); 2.29 % of the pixels
# are valid in exactly one.  The voxels are 93.75 mm.  The two sides interpolate the same TSDF differently: the gap is a property of
# the pair, asserted at twice the measurement.
CHAIN_MEDIAN_MM, CHAIN_MAX_MM, CHAIN_ONE_ONLY = 3.0, 219, 0.0229


def test_chain_on_the_device(ctx, ren):
    import mesh_weld_cases as wc
    from kintinuous_amd import mesh_ref
    N, size, cols, rows = 32, 3.0, 160, 120
    intr = (50.0, 50.0, 79.5, 59.5)
    R, t_vol = np.eye(3, dtype=np.float32), np.array([1.5, 1.6, 0.1], np.float32)
    t_mesh = (t_vol.astype(np.float64) - size / 2).astype(np.float32)               # the mesh is centred on the volume's middle (mesh_ref)
    vol, col = wc.sphere_volume(N)
    dvol, dcol = ctx.upload(vol), ctx.upload(col)
    bufs = [dvol, dcol]
    try:
        s, nv, nt = ctx.extract_mesh(dvol, (size,) * 3, (0, 0, 0), dcol, (0, 0, 0), (N - 1,) * 3, (0, 0, 0), N)
        dv, dt = ctx.empty(16 * nv), ctx.empty(12 * nt)
        bufs += [dv, dt]
        s, nv2, nt2 = ctx.extract_mesh(dvol, (size,) * 3, (0, 0, 0), dcol, (0, 0, 0), (N - 1,) * 3, (0, 0, 0), N, dv, nv, dt, nt)
        assert s == abi.KT_OK and (nv2, nt2) == (nv, nt) and nt > 3000
        outs = {p: ctx.empty(WIDTH[p] * cols * rows * np.dtype(DTYPE[p]).itemsize) for p in PLANES}
        bufs += list(outs.values())
        status, stats = ren.render_device(dv, nv, dt, nt, intr, cols, rows, R, t_mesh, 0.05, **outs)
        rv, rt = mesh_ref.extract_mesh(vol, col, (size,) * 3, (0, 0, 0), (0, 0, 0), (N - 1,) * 3, (0, 0, 0), N)
        want = ref.render(rv, rt, intr, cols, rows, R, t_mesh, 0.05)
        assert status == abi.KT_OK and stats == want[4]
        for k, p in enumerate(PLANES):
            assert np.array_equal(ctx.download(outs[p], DTYPE[p], want[k].shape), want[k]), p
        mesh_depth = want[1]
        vm, nm, cm, dd = ctx.zeros(12 * cols * rows), ctx.zeros(12 * cols * rows), ctx.zeros(4 * cols * rows), ctx.zeros(2 * cols * rows)
        bufs += [vm, nm, cm, dd]
        ctx.raycast(abi.Intr(*intr), R, t_vol, 3 * size / N, [size] * 3, dvol, vm, nm, cols, rows, [0, 0, 0], cm, dcol, N)
        ctx.generate_depth(R.T, t_vol, vm, nm, cols, rows, dd)
        ray_depth = ctx.download(dd, np.uint16, (rows, cols))
        a, b = ray_depth > 0, mesh_depth > 0
        both = a & b
        diff = np.abs(ray_depth[both].astype(np.int64) - mesh_depth[both].astype(np.int64))
        print("chain: %d pixels valid in both, median %.1f mm, max %d mm, %.2f %% valid in exactly one" % (both.sum(), np.median(diff), diff.max(), 100 * (a ^ b).mean()))
        assert both.sum() > 6000
        assert np.median(diff) <= 2 * CHAIN_MEDIAN_MM and diff.max() <= 2 * CHAIN_MAX_MM and (a ^ b).mean() <= 2 * CHAIN_ONE_ONLY
    finally:
        for b in bufs:
            b.free()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def _view_file(path):
    """<prefix>.view -> {name: value string}"""
    out = {}
    for line in open(path).read().splitlines():
        name, value = line.split(None, 1)
        assert name not in out
        out[name] = value
    return out


def _pose_of(view):
    return (np.array([float.fromhex(x) for x in view["R"].split()], np.float32).reshape(3, 3), np.array([float.fromhex(x) for x in view["t"].split()], np.float32))


def _read_pnm(path, magic, dtype, channels):
    raw = open(path, "rb").read()
    head = raw.split(b"\n", 3)
    assert head[0] == magic
    cols, rows = (int(x) for x in head[1].split())
    assert int(head[2]) == (65535 if dtype == ">u2" else 255)
    a = np.frombuffer(head[3], dtype)
    return a.reshape((rows, cols) + ((channels,) if channels > 1 else ()))


def _driver_view_is_the_restatements(prefix, stem, source, cam):
    """<prefix><stem>_view_{depth.pgm,color.ppm,model.ppm} against the restatement's rendering of <prefix><source>.ply at the pose of the
    .view file -> (view, stats)"""
    import deform_mesh_cases as mc
    view = _view_file(prefix + ".view")
    assert view["file"] == os.path.basename(prefix) + source + ".ply"
    v, tri = mc.read_ply(prefix + source + ".ply")
    full = np.zeros(len(v), V)
    full["xyz"] = v["xyz"]
    full["rgb"] = v["rgb"][:, 0].astype(np.uint32) << 16 | v["rgb"][:, 1].astype(np.uint32) << 8 | v["rgb"][:, 2].astype(np.uint32)
    R, t = _pose_of(view)
    index, depth, color, model, stats = ref.render(full, tri.astype(np.uint32), (cam.fx, cam.fy, cam.cx, cam.cy), cam.cols, cam.rows, R, t, float.fromhex(view["near"]))
    assert tuple(int(view[name]) for name in ref.STAT_NAMES) == stats and stats[0] > 0 and stats[3] > 0
    assert np.array_equal(_read_pnm(prefix + stem + "_view_depth.pgm", b"P5", ">u2", 1), depth)
    assert np.array_equal(_read_pnm(prefix + stem + "_view_color.ppm", b"P6", np.uint8, 3), color)
    assert np.array_equal(_read_pnm(prefix + stem + "_view_model.ppm", b"P6", np.uint8, 3), model)
    return view, stats


def test_driver_mv_on_the_smoothed_crab_walk(tmp_path):
    """kintinuous_hip -m -mw -mt 5 -mv on the out-and-back crab-walk of tests/test_gpu_mesh_smooth.py's driver test: the three images are the
    restatement's rendering of the _smooth.ply the run wrote, at the pose in .view, which is the last dense pose; every file of the run
    without -mv is byte-identical; -mvb 1.0 moves the camera back by exactly that along its viewing axis; -mvf takes another pose and
    refuses one out of range with nothing written; -mv without -m is ignored with a message"""
    run = drv.crab_walk_driver(tmp_path)
    cam = run.cam

    rd = lambda p: open(p, "rb").read()
    views = [".view", "_smooth_view_color.ppm", "_smooth_view_depth.pgm", "_smooth_view_model.ppm"]
    _, p0 = run("plain", "-m", "-mw", "-mt", "5")
    out, p1 = run("view", "-m", "-mw", "-mt", "5", "-mv")
    assert drv.outputs(tmp_path, p1) == sorted(drv.outputs(tmp_path, p0) + views)
    for ext in drv.outputs(tmp_path, p0):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    view, stats = _driver_view_is_the_restatements(p1, "_smooth", "_smooth", cam)
    last = [float(x) for x in open(p1 + ".poses").read().splitlines()[-1].split()[1:4]]                # (.poses leaves the first frame out; six digits)
    assert int(view["frame"]) == int(view["poses"]) - 1 > 10 and float.fromhex(view["back"]) == 0.0
    assert np.allclose(_pose_of(view)[1], last, rtol=0, atol=1e-4)
    print("crab-walk -mv: drawn %d, clipped %d, degenerate %d triangles, %d covered pixels" % stats)
    assert stats[3] > cam.cols * cam.rows // 2                                       # the wall fills most of the view
    # -mvb 1.0: the same axes, the centre one metre back along the viewing axis (float arithmetic: t - 1.0f * R's third column)
    _, p2 = run("back", "-m", "-mw", "-mt", "5", "-mv", "-mvb", "1.0")
    view_b, stats_b = _driver_view_is_the_restatements(p2, "_smooth", "_smooth", cam)
    (R0, t0), (R1, t1) = _pose_of(view), _pose_of(view_b)
    assert np.array_equal(R0, R1) and float.fromhex(view_b["back"]) == 1.0
    assert np.array_equal(t1, t0 - np.float32(1.0) * R0[:, 2])
    # -mvf: another pose; without -mt the welded mesh is viewed
    _, p3 = run("first", "-m", "-mw", "-mv", "-mvf", "3")
    view_f, _ = _driver_view_is_the_restatements(p3, "_weld", "_weld", cam)
    assert int(view_f["frame"]) == 3 and not np.array_equal(_pose_of(view_f)[1], t0)
    bad, p4 = run("range", "-m", "-mw", "-mv", "-mvf", "4000", ok=False)
    assert "-mvf" in bad.stderr and not [e for e in drv.outputs(tmp_path, p4) if "view" in e]
    # ignored with a message
    nomesh, p5 = run("nomesh", "-mv")
    assert "-mv ignored without -m" in nomesh.stderr and not [e for e in drv.outputs(tmp_path, p5) if "view" in e]


def test_driver_mv_with_df_on_the_loop_log(tmp_path):
    """kintinuous_hip ... -lc -pg -pcd -df -m -mv on the ten-frame walk of tests/test_gpu_deform_mesh.py's driver test: <prefix>_view_* is the
    restatement's rendering of .ply from the last dense pose, <prefix>_def_view_* that of _def.ply from the pose _opt.poses holds for the
    same frame (_def.view); every file of the run without -mv is byte-identical."""
    run = drv.loop_log_driver(tmp_path)
    cam = run.cam

    _, p0 = run("plain", "-m")
    _, p1 = run("view", "-m", "-mv")
    rd = lambda p: open(p, "rb").read()
    views = [".view", "_def.view"] + [stem + "_view_" + name for stem in ("", "_def") for name in ("color.ppm", "depth.pgm", "model.ppm")]
    assert drv.outputs(tmp_path, p1) == sorted(drv.outputs(tmp_path, p0) + views)
    for ext in drv.outputs(tmp_path, p0):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    view, _ = _driver_view_is_the_restatements(p1, "", "", cam)
    os.replace(p1 + "_def.view", p1 + ".view")                                      # (the helper reads <prefix>.view)
    view_d, _ = _driver_view_is_the_restatements(p1, "_def", "_def", cam)
    assert view_d["frame"] == view["frame"] and view_d["poses"] == view["poses"]
    opt = np.array([[float(x) for x in l.split()[1:4]] for l in open(p1 + "_opt.poses").read().splitlines()])
    assert (np.abs(opt - _pose_of(view_d)[1]).max(axis=1) < 1e-4).any()              # the camera centre is a node of the optimised graph (six digits)
