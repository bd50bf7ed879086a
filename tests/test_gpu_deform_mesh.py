"""GPU.  The fused mesh pass of the deformation graph (csrc/kt_deform.hip: df_apply_mesh behind kt_deform_apply_mesh[_device]; DESIGN.md
4.11) on the meshes of tests/deform_mesh_cases.py: every byte of the vertex array against deform_ref.apply_mesh and against the two-call
route through kt_deform_weights_device + kt_deform_apply_device on the same positions as 48-byte points -- the kernel shares the bodies
of df_weigh and df_position with that route, so the two must agree bit for bit on the device --, a canary vertex behind the array, the host
form, the same call twice, a large case after a small one, the argument errors with canaries, the allocations, and the driver's
-m -df run: <prefix>_def.ply against the restatement run on <prefix>.ply from the run's own <prefix>.deform."""
import ctypes as C

import numpy as np
import pytest

import deform_cases as dc
import deform_mesh_cases as mc

pytestmark = pytest.mark.gpu

CANARY = np.array([((1.5, -2.5, 3.5), 0xdeadbeef)], dtype=[("xyz", np.float32, 3), ("rgb", np.uint32)])


@pytest.fixture(scope="module")
def dg(ctx):
    from kintinuous_amd import abi
    g = abi.DeformationGraph(ctx, 257, 300)
    yield g
    g.close()


def _set(g, name):
    """the case's graph with the restatement's optimised state loaded"""
    c = mc.case(name)
    gc = dc.case(c["graph"])
    g.set_graph(gc["node_pos"], gc["node_time"])
    g.set_state(dc.restated(c["graph"])[0])
    return c


def _device_form(g, ctx, c):
    """kt_deform_apply_mesh_device on an upload of the vertices with a canary vertex behind them -> (vertices, canary)"""
    n = len(c["vertices"])
    buf = ctx.upload(np.concatenate([c["vertices"], CANARY.astype(c["vertices"].dtype)]))
    g.apply_mesh_device(buf, n, c["span_first"], c["span_time"])
    ctx.sync()
    got = ctx.download(buf, c["vertices"].dtype, (n + 1,))
    buf.free()
    return got[:n], got[n:]


@pytest.mark.parametrize("name", mc.NAMES)
def test_device_form_bit_equal(dg, ctx, name):
    c = _set(dg, name)
    want = mc.restated(name)
    got, canary = _device_form(dg, ctx, c)
    print(name, "largest displacement %.3f m" % np.abs(got["xyz"] - c["vertices"]["xyz"]).max(), "differing vertices",
          int((got["xyz"].view(np.uint32) != want["xyz"].view(np.uint32)).any(axis=1).sum()))
    assert got.tobytes() == want.tobytes()
    assert got["rgb"].tobytes() == c["vertices"]["rgb"].tobytes()
    assert canary.tobytes() == CANARY.tobytes()
    again, _ = _device_form(dg, ctx, c)                                # the same call from the same input: the same bytes
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("name", mc.NAMES)
def test_host_form_same_bytes(dg, name):
    c = _set(dg, name)
    got = dg.apply_mesh(c["vertices"], c["span_first"], c["span_time"])
    assert got.tobytes() == mc.restated(name).tobytes()


@pytest.mark.parametrize("name", mc.NAMES)
def test_fused_equals_two_call_route(dg, ctx, name):
    """the positions of kt_deform_weights_device + kt_deform_apply_device on the expanded points: the refactored bodies on the old path"""
    c = _set(dg, name)
    n = len(c["vertices"])
    fused, _ = _device_form(dg, ctx, c)
    dp, dt, di, dw = ctx.upload(mc.as_points(c["vertices"])), ctx.upload(mc.expanded_times(c)), ctx.empty(16 * n), ctx.empty(32 * n)
    dg.weights_device(dp, dt, n, di, dw)
    dg.apply_device(dp, di, dw, n)
    ctx.sync()
    from kintinuous_amd import abi
    pts = ctx.download(dp, abi.NPOINT_DTYPE, (n,))
    for b in (dp, dt, di, dw):
        b.free()
    assert fused["xyz"].tobytes() == pts["xyz"].tobytes()


def test_no_state_survives_a_call(ctx):
    """a large mesh after a small one on the same object (the span table and the staging grow): the bytes of a fresh object, and back"""
    from kintinuous_amd import abi
    g = abi.DeformationGraph(ctx, 257, 300)
    for name in (mc.SMALL, mc.LARGE, mc.SMALL):
        c = _set(g, name)
        assert g.apply_mesh(c["vertices"], c["span_first"], c["span_time"]).tobytes() == mc.restated(name).tobytes()
        assert _device_form(g, ctx, c)[0].tobytes() == mc.restated(name).tobytes()
    g.close()
    fresh = abi.DeformationGraph(ctx, 257, 300)
    c = _set(fresh, mc.LARGE)
    assert fresh.apply_mesh(c["vertices"], c["span_first"], c["span_time"]).tobytes() == mc.restated(mc.LARGE).tobytes()
    fresh.close()


def test_bad_arguments_leave_the_vertices_alone(ctx):
    from kintinuous_amd import abi
    ktlib = abi.lib()
    OK, ARG, STATE = 0, 2, 4
    c = mc.case("m21_n65_c300-mixed")
    gc = dc.case(c["graph"])
    n, S = len(c["vertices"]), len(c["span_time"])
    first, times = np.array(c["span_first"], dtype=np.uintp), np.array(c["span_time"], dtype=np.uint64)
    host = np.array(c["vertices"])
    dev = ctx.upload(host)
    p = lambda a: None if a is None else a.ctypes.data

    def both(vdev, vhost, nn, f, t, s, h=True):
        """the status of the device form and of the host form, which must agree"""
        g_h = g.h if h else None
        a = ktlib.kt_deform_apply_mesh_device(g_h, vdev, nn, p(f), p(t), s)
        b = ktlib.kt_deform_apply_mesh(g_h, vhost, nn, p(f), p(t), s)
        assert a == b, (a, b)
        return a

    g = abi.DeformationGraph(ctx, 21, 300)
    assert both(dev.ptr, p(host), n, first, times, S) == STATE                      # no graph yet
    assert both(None, None, 0, np.zeros(1, np.uintp), None, 0) == STATE             # ... for an empty mesh too
    g.set_graph(gc["node_pos"], gc["node_time"])
    g.set_state(dc.restated(c["graph"])[0])
    f = first.copy(); f[0] = 1
    assert both(dev.ptr, p(host), n, f, times, S) == ARG                            # does not start at 0
    f = first.copy(); f[4], f[5] = first[5], first[4]
    assert first[4] < first[5] and both(dev.ptr, p(host), n, f, times, S) == ARG    # decreases
    f = first.copy(); f[-1] = n - 1; f[-2] = n - 1
    assert both(dev.ptr, p(host), n, f, times, S) == ARG                            # does not end at n
    assert both(dev.ptr, p(host), n - 1, first, times, S) == ARG
    assert both(None, None, n, first, times, S) == ARG                              # null pointers with n > 0
    assert both(dev.ptr, p(host), n, None, times, S) == ARG
    assert both(dev.ptr, p(host), n, first, None, S) == ARG
    assert both(dev.ptr + 4, p(host) + 4, n - 1, np.array([0, n - 1], np.uintp), times, 1) == ARG     # not 16-byte aligned
    big = (1 << 29) + 1
    assert both(dev.ptr, p(host), big, np.array([0, big], np.uintp), times, 1) == ARG                 # above the mesh stage's bound
    assert both(dev.ptr, p(host), n, first, times, 0) == ARG                        # vertices without a span
    assert both(dev.ptr, p(host), n, first, times, -1) == ARG
    assert both(dev.ptr, p(host), n, first, times, S, h=False) == ARG
    # nothing to do: KT_OK
    assert both(None, None, 0, None, None, 0) == OK
    assert both(None, None, 0, np.zeros(1, np.uintp), None, 0) == OK
    assert both(dev.ptr, p(host), 0, np.zeros(3, np.uintp), times, 2) == OK
    ctx.sync()
    assert host.tobytes() == c["vertices"].tobytes()
    assert ctx.download(dev, host.dtype, (n,)).tobytes() == c["vertices"].tobytes()
    dev.free()
    assert g.apply_mesh(c["vertices"], first, times).tobytes() == mc.restated("m21_n65_c300-mixed").tobytes()   # still usable
    assert len(g.apply_mesh(host[:0], [0], [])) == 0
    g.close()


def test_allocations_return(ctx):
    from kintinuous_amd import abi
    ctx.sync()
    start = abi.live_allocations()
    g = abi.DeformationGraph(ctx, 21, 300)
    c = _set(g, "m21_n65_c300-one4099")
    held = abi.live_allocations()[0]
    buf = ctx.upload(c["vertices"])
    mine = abi.live_allocations()[0] - held
    g.apply_mesh_device(buf, len(c["vertices"]), c["span_first"], c["span_time"])    # the span table is the object's
    table = abi.live_allocations()[0]
    assert table > held + mine
    g.apply_mesh(c["vertices"], c["span_first"], c["span_time"])                     # ... and so is the host form's staging: one more buffer
    assert abi.live_allocations()[0] == table + 1
    c2 = mc.case("m21_n65_c300-mixed")                                               # more spans, fewer vertices: released and taken again
    g.apply_mesh(c2["vertices"], c2["span_first"], c2["span_time"])
    assert abi.live_allocations()[0] == table + 1
    ctx.sync()
    buf.free()
    g.close()
    assert abi.live_allocations() == start


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------
def _ulp_close(got, want, extent):
    """the end-to-end rule of tests/test_gpu_deform.py, restated: every float equals the restatement's or its neighbour; near zero
    max(1 ulp, 10 BOUND (1 + extent)) absolute"""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    both_nan = np.isnan(got) & np.isnan(want)
    up, down = np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))
    near = (got == want) | (got == up) | (got == down) | both_nan
    near |= np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 10 * dc.BOUND * (1.0 + extent)
    return bool(near.all())


def test_driver_df_mesh(ctx, tmp_path):
    """kintinuous_hip ... -lc -pg -pcd -m -df on the ten-frame walk of tests/test_gpu_deform.py's driver test: _def.ply has the faces of .ply
    and its vertices where the restatement puts the .ply's, from the run's own .deform (nodes, constraints, `mesh` spans); .ply and every
    other file are byte-identical to a run without -df; with no kept loop (-it 0) nothing moves and _def.ply equals .ply."""
    import os
    import subprocess
    import loop_db_cases as lc
    from kintinuous_amd import abi, build, klg, synth, deform_ref as ref
    build.build_host()
    frames = [lc.frames()[k] for k in range(10)]
    log = str(tmp_path / "ten.klg")
    klg.write_klg(log, frames + [frames[-1]], timestamps=[1000 * (k + 1) for k in range(10)] + [99000], cols=lc.COLS, rows=lc.ROWS)
    cam = lc.camera()
    calib = tmp_path / "calib.txt"
    calib.write_text(f"{cam.fx!r} {cam.fy!r} {cam.cx!r} {cam.cy!r}\n")
    tfile = str(tmp_path / "traj.csv")
    synth.write_trajectory_file(tfile, [1000 * (k + 1) for k in range(10)], synth.ground_truth_rows([(T[:3, :3], T[:3, 3]) for T in lc.poses()]))

    def run(name, *extra):
        prefix = str(tmp_path / name)
        r = subprocess.run([build.HOST_BIN, "-l", log, "-c", str(calib), "-n", "96", "-w", str(lc.COLS), "-h", str(lc.ROWS), "-s", "6", "-p", tfile, "-o", prefix,
                            "-v", "vocab.yml.gz", "-lc", "-dl", "3", "-pcd", "-m", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (extra, r.returncode, r.stdout, r.stderr[-2000:])
        print(r.stdout, r.stderr)
        return r, prefix

    plain, p0 = run("pg", "-pg")
    df, p1 = run("df", "-pg", "-df", "-dg", "0.02", "-ds", "1e-9")
    none, p2 = run("none", "-pg", "-it", "0", "-df", "-dg", "0.02")
    rd = lambda p: open(p, "rb").read()
    for ext in (".ply", ".pcd", ".poses", ".loops", ".graph", "_opt.poses"):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    assert not os.path.exists(p0 + "_def.ply") and not os.path.exists(p0 + ".deform")
    # no kept loop: insignificant, nothing moved
    d2 = mc.deform_file(open(p2 + ".deform").read())
    assert d2["result"][2] == "insignificant" and d2["mesh"]
    assert rd(p2 + "_def.ply") == rd(p2 + ".ply")
    # the kept loop
    d = mc.deform_file(open(p1 + ".deform").read())
    assert len([l for l in df.stdout.splitlines() if l.startswith("deformation ")]) == 1
    assert open(p1 + ".deform").read().splitlines()[-1].startswith("result ")              # the mesh lines come before it
    before, faces = mc.read_ply(p1 + ".ply")
    after, faces_after = mc.read_ply(p1 + "_def.ply")
    assert np.array_equal(faces, faces_after) and len(faces) > 0
    assert len(d["mesh"]) >= 1 and sum(c for _, c in d["mesh"]) == len(before) == len(after) and len(before) > 0
    assert after["rgb"].tobytes() == before["rgb"].tobytes()
    pose_t = [p[0] for p in d["pose"]]
    orig = np.array([p[1:4] for p in d["pose"]], np.float32)
    keep = ref.sample_nodes(orig, 0.02)
    g = ref.Graph(orig[keep], np.array([pose_t[k] for k in keep], np.uint64))
    assert np.array_equal(np.array([n[1:4] for n in d["node"]], np.float32), g.gf) and [n[0] for n in d["node"]] == g.gt.tolist()
    src = np.array([c[1:4] for c in d["con"]], np.float32)
    x, e0, e1, ce, steps, status, _ = ref.optimise(g, src, np.array([c[0] for c in d["con"]], np.uint64), np.array([c[4:7] for c in d["con"]]), {"significant_error": 1e-9})
    names = {ref.CONVERGED: "converged", ref.MAX_STEPS: "max-steps", ref.INSIGNIFICANT: "insignificant", ref.SINGULAR: "singular"}
    assert (names[status], steps) == d["result"][2:4] and status in (ref.CONVERGED, ref.MAX_STEPS)
    v = np.zeros(len(before), abi.MESH_VERTEX_DTYPE)
    v["xyz"] = before["xyz"]
    first = np.concatenate([[0], np.cumsum([c for _, c in d["mesh"]])])
    want = ref.apply_mesh(g, x, v, first, [t for t, _ in d["mesh"]])
    extent = float(np.abs(before["xyz"]).max())
    moved = float(np.abs(after["xyz"] - before["xyz"]).max())
    print("mesh", len(before), "vertices", len(faces), "faces", len(d["mesh"]), "spans; largest displacement", moved, "differing floats",
          int((after["xyz"] != want["xyz"]).sum()))
    assert moved > 0.0
    assert _ulp_close(after["xyz"], want["xyz"], extent)
