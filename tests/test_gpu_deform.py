"""GPU.  The deformation-graph stage (csrc/kt_deform.hip: kt_deform_*) against its numpy restatement
(kintinuous_amd/deform_ref.py), which tests/test_deform_ref.py ties to an independent Gauss-Newton, to a central difference, to
least_squares and to a brute-force weighting.  The stage uses + - * / and sqrt alone: the weights and the apply pass are held bit for bit,
the optimised state to the bound of tests/deform_cases.py with equal step counts and status, the same call to the same bytes.
Measured on an MI355X: the largest state difference is 0 on every case (profiles/deformation.md)."""
import ctypes as C

import numpy as np
import pytest

import deform_cases as dc

pytestmark = pytest.mark.gpu


def _bytes(out):
    state, r = out
    return state.tobytes() + bytes(r)


@pytest.fixture(scope="module")
def dg(ctx):
    from kintinuous_amd import abi
    g = abi.DeformationGraph(ctx, 257, 300)
    yield g
    g.close()


def _set(g, name):
    c = dc.case(name)
    g.set_graph(c["node_pos"], c["node_time"])
    return c


def _optimise(g, c, params=None):
    return g.optimise(c["src"], c["src_time"], c["target"], params)


@pytest.mark.parametrize("name", dc.NAMES)
def test_weights_bit_equal(dg, name):
    c = _set(dg, name)
    want_idx, want_w = dc.restated_weights(name)
    idx, w = dg.weights(c["points"], c["times"])
    assert np.array_equal(idx, want_idx)
    assert w.tobytes() == want_w.tobytes()


@pytest.mark.parametrize("name", dc.NAMES)
def test_apply_after_set_state_bit_equal(dg, ctx, name):
    """the restatement's state loaded, then the device pass on device arrays: every byte of the point array"""
    c = _set(dg, name)
    n = len(c["points"])
    dg.set_state(dc.restated(name)[0])
    want = dc.restated_apply(name)
    if n == 0:
        from kintinuous_amd import abi
        assert abi.lib().kt_deform_apply_device(dg.h, None, None, None, 0) == 0
        return
    idx, w = dc.restated_weights(name)
    dp, di, dw = ctx.upload(c["points"]), ctx.upload(idx), ctx.upload(w)
    dg.apply_device(dp, di, dw, n)
    ctx.sync()
    got = ctx.download(dp, c["points"].dtype, (n,))
    for b in (dp, di, dw):
        b.free()
    moved = np.abs(got["xyz"] - c["points"]["xyz"]).max()
    print(name, "largest displacement %.3f m" % moved)
    assert got.tobytes() == want.tobytes()
    for f in ("one", "zero", "bgra", "curvature", "pad"):
        assert got[f].tobytes() == c["points"][f].tobytes()


@pytest.mark.parametrize("name", dc.NAMES)
def test_optimise_matches_restatement(dg, name):
    c = _set(dg, name)
    want, e0, e1, ce, steps, status, trace = dc.restated(name)
    state, r = _optimise(dg, c)
    diff = float(np.abs(state - want).max())
    print(name, "largest state difference %.3e" % diff, "errors", r.error_start, r.error_end, r.constraint_error, "restated", e0, e1, ce, "steps", r.steps, steps,
          "status", r.status, status)
    assert diff <= dc.BOUND
    assert (r.steps, r.status) == (steps, status)
    assert abs(r.error_start - e0) <= dc.rel_bound(e0) and abs(r.error_end - e1) <= dc.rel_bound(e1) and abs(r.constraint_error - ce) <= dc.rel_bound(ce)
    assert _bytes(_optimise(dg, c)) == _bytes((state, r))             # the same call, the same bytes


def _ulp_close(got, want, extent):
    """every float equals the restatement's or its neighbour; near zero max(1 ulp, 10 BOUND (1 + extent)) absolute"""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    both_nan = np.isnan(got) & np.isnan(want)
    up, down = np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))
    near = (got == want) | (got == up) | (got == down) | both_nan
    near |= np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 10 * dc.BOUND * (1.0 + extent)
    return bool(near.all())


@pytest.mark.parametrize("name", dc.NAMES)
def test_end_to_end(dg, name):
    """kt_deform_apply after kt_deform_optimise on host arrays"""
    c = _set(dg, name)
    _optimise(dg, c)
    got = dg.apply(c["points"], c["times"])
    want = dc.restated_apply(name)
    assert _ulp_close(got["xyz"], want["xyz"], c["extent"]) and _ulp_close(got["normal"], want["normal"], 1.0)
    for f in ("one", "zero", "bgra", "curvature", "pad"):
        assert got[f].tobytes() == c["points"][f].tobytes()


def test_no_state_survives_a_call(ctx):
    """a large case after a small one on the same object: the bytes of a fresh object, and back"""
    from kintinuous_amd import abi
    fresh = abi.DeformationGraph(ctx, 65, 300)
    big = _set(fresh, dc.LARGE)
    want = _bytes(_optimise(fresh, big))
    fresh.close()
    g = abi.DeformationGraph(ctx, 65, 300)
    small = _set(g, dc.SMALL)
    first = _bytes(_optimise(g, small))
    _set(g, dc.LARGE)
    assert _bytes(_optimise(g, big)) == want
    _set(g, dc.SMALL)
    assert _bytes(_optimise(g, small)) == first
    g.close()


def test_tightened_params_and_step_limit(dg):
    """kt_deform_params: thresholds that never stop the loop end at max_steps with KT_DEFORM_MAX_STEPS, as the restatement does"""
    from kintinuous_amd import abi, deform_ref as ref
    name = "m19_n63_c7"
    c = _set(dg, name)
    p = {"delta_tol": 0.0, "error_tol": 0.0, "change_tol": 0.0, "max_steps": 5}
    want, e0, e1, ce, steps, status, _ = ref.optimise(dc.graph(name), c["src"], c["src_time"], c["target"], p)
    state, r = _optimise(dg, c, abi.DeformParams(delta_tol=0.0, error_tol=0.0, change_tol=0.0, max_steps=5))
    assert (r.steps, r.status) == (steps, status) == (5, abi.KT_DEFORM_MAX_STEPS)
    assert np.abs(state - want).max() <= dc.BOUND and abs(r.error_end - e1) <= dc.rel_bound(e1)


def _raw_optimise(g, n_con, src, tm, tgt, out, res, params=None):
    from kintinuous_amd import abi
    p = lambda a: None if a is None else a.ctypes.data
    return abi.lib().kt_deform_optimise(g.h if g is not None else None, n_con, p(src), p(tm), p(tgt), C.addressof(params) if params is not None else None, p(out),
                                        C.addressof(res) if res is not None else None)


def test_capacity_and_bad_arguments(ctx):
    from kintinuous_amd import abi
    ktlib = abi.lib()
    ARG, STATE = 2, 4
    c = dc.case("m21_n65_c300")
    g = abi.DeformationGraph(ctx, 21, 300)
    out = np.full((22, 12), -7.0)
    res = abi.DeformResult(-1.0, -2.0, -3.0, -4, -5)
    untouched = lambda: (out == -7.0).all() and (res.error_start, res.error_end, res.constraint_error, res.steps, res.status) == (-1.0, -2.0, -3.0, -4, -5)
    src, tm, tgt = np.ascontiguousarray(c["src"]), np.ascontiguousarray(c["src_time"]), np.ascontiguousarray(c["target"])
    assert _raw_optimise(g, 300, src, tm, tgt, out, res) == STATE and untouched()       # no graph yet
    pos, times = np.ascontiguousarray(c["node_pos"]), np.ascontiguousarray(c["node_time"])
    # four nodes: KT_ERR_ARG; one node too many: KT_ERR_CAPACITY; times that do not increase: KT_ERR_ARG
    assert ktlib.kt_deform_set_graph(g.h, 4, pos.ctypes.data, times.ctypes.data) == ARG
    pos22, times22 = np.concatenate([pos, pos[:1] + 9]), np.append(times, times[-1] + 5).astype(np.uint64)
    assert ktlib.kt_deform_set_graph(g.h, 22, pos22.ctypes.data, times22.ctypes.data) == abi.KT_ERR_CAPACITY
    bad = times.copy(); bad[7] = bad[6]
    assert ktlib.kt_deform_set_graph(g.h, 21, pos.ctypes.data, bad.ctypes.data) == ARG
    assert ktlib.kt_deform_set_graph(g.h, 21, None, times.ctypes.data) == ARG and ktlib.kt_deform_set_graph(None, 21, pos.ctypes.data, times.ctypes.data) == ARG
    assert _raw_optimise(g, 300, src, tm, tgt, out, res) == STATE and untouched()       # the refused calls set nothing
    g.set_graph(pos, times)
    before = _bytes(_optimise(g, c))
    # one constraint too many: KT_ERR_CAPACITY before any work, nothing written
    src301, tm301, tgt301 = np.concatenate([src, src[:1]]), np.append(tm, tm[:1]), np.concatenate([tgt, tgt[:1]])
    assert _raw_optimise(g, 301, src301, tm301, tgt301, out, res) == abi.KT_ERR_CAPACITY and untouched()
    assert _raw_optimise(None, 300, src, tm, tgt, out, res) == ARG
    assert _raw_optimise(g, 300, None, tm, tgt, out, res) == ARG
    assert _raw_optimise(g, 300, src, None, tgt, out, res) == ARG
    assert _raw_optimise(g, 300, src, tm, None, out, res) == ARG
    assert _raw_optimise(g, 300, src, tm, tgt, None, res) == ARG
    assert _raw_optimise(g, 300, src, tm, tgt, out, None) == ARG
    assert _raw_optimise(g, -1, src, tm, tgt, out, res) == ARG
    assert _raw_optimise(g, 300, src, tm, tgt, out, res, abi.DeformParams(max_steps=65)) == ARG
    assert _raw_optimise(g, 300, src, tm, tgt, out, res, abi.DeformParams(max_steps=-1)) == ARG
    assert untouched()
    # the device entries: null and misaligned arrays
    pts = ctx.upload(c["points"])
    assert ktlib.kt_deform_weights_device(g.h, pts.ptr, None, 65, None, None) == ARG
    assert ktlib.kt_deform_weights_device(g.h, pts.ptr + 4, pts.ptr, 1, pts.ptr, pts.ptr) == ARG
    assert ktlib.kt_deform_apply_device(g.h, pts.ptr, None, None, 65) == ARG
    assert ktlib.kt_deform_apply(g.h, None, None, 65) == ARG and ktlib.kt_deform_apply(None, None, None, 0) == ARG
    assert ktlib.kt_deform_set_state(g.h, None) == ARG
    ctx.sync()
    assert ctx.download(pts, c["points"].dtype, (65,)).tobytes() == c["points"].tobytes()
    pts.free()
    h = C.c_void_p()
    assert ktlib.kt_deform_create(ctx.h, 4, 4, None, C.byref(h)) == ARG
    assert ktlib.kt_deform_create(ctx.h, 4097, 4, None, C.byref(h)) == ARG
    assert ktlib.kt_deform_create(ctx.h, 16, -1, None, C.byref(h)) == ARG
    assert ktlib.kt_deform_create(None, 16, 4, None, C.byref(h)) == ARG
    assert ktlib.kt_deform_create(ctx.h, 16, 4, None, None) == ARG
    assert ktlib.kt_deform_destroy(None) == 0
    assert _bytes(_optimise(g, c)) == before                          # still usable, and unchanged by the refused calls
    g.close()


def test_no_constraint_is_insignificant(dg):
    from kintinuous_amd import abi, deform_ref as ref
    c = _set(dg, "m19_n63_c7")
    state, r = dg.optimise()
    _, e0, e1, _, _, _, _ = ref.optimise(dc.graph("m19_n63_c7"))     # (g_n - g_j) + g_j rounds: the identity's error is tiny, not zero
    assert (r.steps, r.status, r.constraint_error) == (0, abi.KT_DEFORM_INSIGNIFICANT, 0.0)
    assert abs(r.error_start - e0) <= dc.BOUND and abs(r.error_end - e1) <= dc.BOUND and e0 < 1e-25
    assert (state == ref.identity(19)).all()
    got = dg.apply(c["points"], c["times"])                           # the identity state moves nothing (normals are re-normalised)
    assert np.abs(got["xyz"] - c["points"]["xyz"]).max() <= 1e-6
    assert len(dg.apply(c["points"][:0], c["times"][:0])) == 0        # n = 0


def test_allocations_return(ctx):
    from kintinuous_amd import abi
    ctx.sync()
    start = abi.live_allocations()
    g = abi.DeformationGraph(ctx, 65, 300)
    assert abi.live_allocations()[0] > start[0]
    c = _set(g, dc.LARGE)
    _optimise(g, c)
    held = abi.live_allocations()[0]
    g.apply(c["points"], c["times"])                                  # the staging of kt_deform_apply is the object's too
    assert abi.live_allocations()[0] > held
    g.close()
    assert abi.live_allocations() == start


def test_singular_system_is_reported(ctx):
    """a straight line of nodes: KT_DEFORM_SINGULAR with KT_OK, the identity state and finite errors, not NaN after max_steps"""
    from kintinuous_amd import abi, deform_ref as ref
    from test_deform_ref import straight_line
    pos, times, src, src_time, target = straight_line()
    want, e0, e1, ce, steps, status, _ = ref.optimise(ref.Graph(pos, times), src, src_time, target)
    g = abi.DeformationGraph(ctx, 8, 3)
    g.set_graph(pos, times)
    state, r = g.optimise(src, src_time, target)
    g.close()
    assert (r.status, r.steps) == (abi.KT_DEFORM_SINGULAR, 0) == (status, steps)
    assert (state == want).all() and (r.error_start, r.error_end, r.constraint_error) == (e0, e1, ce)


# ---- the shell and the driver ------------------------------------------------------------------------------------------------------------
def _deform_file(path):
    out = {"pose": [], "node": [], "con": [], "slice": [], "result": None}
    for line in open(path).read().splitlines():
        f = line.split()
        if f[0] == "result":
            out["result"] = (int(f[1]), int(f[2]), f[3], int(f[4])) + tuple(float.fromhex(v) for v in f[5:8])
        elif f[0] == "slice":
            out["slice"].append((int(f[1]), int(f[2])))
        else:
            out[f[0]].append((int(f[1]),) + tuple(float.fromhex(v) for v in f[2:]))
    return out


def test_driver_df(ctx, tmp_path):
    """kintinuous_hip -v x -lc -pg -pcd -df -dg 0.02 on the ten-frame walk of tests/test_gpu_pose_graph.py's driver test: _def.pcd has the
    points of .pcd, moved as the shell's logic says when it is run through the restatement from the run's own .deform (the stage's inputs
    in hex, so nothing is lost to text): the nodes are the sampling of the original camera positions, the camera constraints are the
    pose lines, the loop constraints sit at the kept loops' times, and the restatement's optimise + apply on them gives the file's floats
    under the end-to-end rule.  Every other file is byte-identical to a run without -df; -df without -pg is ignored with a message; with
    no kept loop (-it 0) the status is insignificant and _def.pcd equals .pcd."""
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
                            "-v", "vocab.yml.gz", "-lc", "-dl", "3", "-pcd", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (extra, r.returncode, r.stdout, r.stderr[-2000:])
        print(r.stdout, r.stderr)
        return r, prefix

    plain, p0 = run("pg", "-pg")
    df, p1 = run("df", "-pg", "-df", "-dg", "0.02", "-ds", "1e-9")       # the walk follows its ground truth: the gate is lowered so that the loop deforms
    none, p2 = run("none", "-pg", "-it", "0", "-df", "-dg", "0.02")
    nopg, p3 = run("nopg", "-df")
    rd = lambda p: open(p, "rb").read()
    for ext in (".pcd", ".poses", ".loops", ".graph", "_opt.poses"):
        assert rd(p0 + ext) == rd(p1 + ext), ext
    assert not os.path.exists(p0 + "_def.pcd") and not os.path.exists(p0 + ".deform")
    assert "-df ignored" in nopg.stderr and not os.path.exists(p3 + "_def.pcd") and rd(p3 + ".pcd") == rd(p0 + ".pcd")
    # no kept loop: insignificant, nothing moved
    assert "rejected" in open(p2 + ".graph").read() and "kept" not in open(p2 + ".graph").read()
    d2 = _deform_file(p2 + ".deform")
    assert d2["result"][2] == "insignificant" and d2["result"][3] == 0 and len(d2["con"]) == len(d2["pose"])
    assert rd(p2 + "_def.pcd") == rd(p2 + ".pcd")
    # the kept loop
    d = _deform_file(p1 + ".deform")
    summary = [l for l in df.stdout.splitlines() if l.startswith("deformation ")]
    assert len(summary) == 1 and (" %d nodes" % d["result"][0]) in summary[0] and ("status " + d["result"][2]) in summary[0]
    pose_t = [p[0] for p in d["pose"]]
    assert pose_t == sorted(set(pose_t)) and len(pose_t) >= 10
    orig = np.array([p[1:4] for p in d["pose"]], np.float32)
    keep = ref.sample_nodes(orig, 0.02)
    assert [n[0] for n in d["node"]] == [pose_t[k] for k in keep] and len(keep) >= 5
    assert np.array_equal(np.array([n[1:4] for n in d["node"]], np.float32), orig[keep])
    assert d["con"][:len(d["pose"])] == d["pose"]                                          # the camera constraints, original -> optimised
    kept_times = set()
    for l in open(p1 + ".graph").read().splitlines():
        f = l.split()
        if f[3] == "kept":
            kept_times |= {int(f[0]), int(f[1])}
    loop_cons = d["con"][len(d["pose"]):]
    assert kept_times and loop_cons and {c[0] for c in loop_cons} == kept_times
    assert d["result"][:2] == (len(keep), len(d["con"]))
    g = ref.Graph(orig[keep], np.array([pose_t[k] for k in keep], np.uint64))
    src = np.array([c[1:4] for c in d["con"]], np.float32)
    x, e0, e1, ce, steps, status, _ = ref.optimise(g, src, np.array([c[0] for c in d["con"]], np.uint64), np.array([c[4:7] for c in d["con"]]), {"significant_error": 1e-9})
    print("restated", e0, e1, ce, steps, status, "driver", d["result"])
    names = {ref.CONVERGED: "converged", ref.MAX_STEPS: "max-steps", ref.INSIGNIFICANT: "insignificant", ref.SINGULAR: "singular"}
    assert (names[status], steps) == d["result"][2:4]
    assert abs(d["result"][4] - e0) <= dc.rel_bound(e0) and abs(d["result"][5] - e1) <= dc.rel_bound(e1) and abs(d["result"][6] - ce) <= dc.rel_bound(ce)
    before, after = klg.read_pcd(p1 + ".pcd"), klg.read_pcd(p1 + "_def.pcd")
    assert len(before) == len(after) == sum(c for _, c in d["slice"]) and len(before) > 0
    pts = np.zeros(len(before), abi.NPOINT_DTYPE)
    pts["xyz"], pts["normal"] = before["xyz"], before["normal"]
    times = np.concatenate([np.full(c, t, np.uint64) for t, c in d["slice"]])
    want = ref.apply(g, x, pts, times) if status in (ref.CONVERGED, ref.MAX_STEPS) else pts
    extent = float(np.abs(before["xyz"]).max())
    print("largest displacement", float(np.abs(after["xyz"] - before["xyz"]).max()))
    assert _ulp_close(after["xyz"], want["xyz"], extent) and _ulp_close(after["normal"], want["normal"], 1.0)
    assert after["bgra"].tobytes() == before["bgra"].tobytes() and after["curvature"].tobytes() == before["curvature"].tobytes()
