"""GPU.  The pose-graph stage (csrc/kt_posegraph.hip: kt_pose_graph_*) against its numpy restatement
(kintinuous_amd/pose_graph_ref.py), which tests/test_pose_graph_ref.py ties to an independent optimiser, to stationarity and to mpmath.
Poses and chi2 agree within the bound of tests/pose_graph_cases.py (equality is not asked: sin, cos, atan2 and sqrt in double differ in
the last bit between the device's library and numpy's); step counts and status are equal; the same call returns the same bytes.
Graphs WITHOUT loops are held to equality: their poses are products alone, none of those functions is on the path.  Above 65536 nodes
(pg_scan_carry's serial runs) and at the step limit the cases are pc.LARGE and pc.STEP_LIMIT, on a 131073-node object of their own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_graph_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(c):
    return c["T0"], c["chain_Z"], c["loop_a"], c["loop_b"], c["loop_Z"]


def _bytes(out):
    poses, r = out
    return poses.tobytes() + bytes(r)


@pytest.fixture(scope="module")
def graph(ctx):
    from kintinuous_amd import abi
    g = abi.PoseGraph(ctx, 4097, 64)
    yield g
    g.close()


@pytest.mark.parametrize("name", pc.NAMES)
def test_case_matches_restatement(graph, name):
    c = pc.case(name)
    want, chi2_start, chi2_end, steps, status, deltas = pc.restated(name)
    poses, r = graph.optimise(*_args(c))
    diff = float(np.abs(poses - want).max())
    print(name, "largest pose difference %.3e" % diff, "chi2", r.chi2_start, r.chi2_end, "restated", chi2_start, chi2_end, "steps", r.steps, steps, "status", r.status,
          "last delta", deltas[-1] if deltas else None)
    assert diff <= pc.BOUND
    assert abs(r.chi2_start - chi2_start) <= pc.chi2_bound(chi2_start) and abs(r.chi2_end - chi2_end) <= pc.chi2_bound(chi2_end)
    close = bool(deltas) and 0.5e-9 <= deltas[-1] <= 2e-9
    assert r.steps == steps or (close and abs(r.steps - steps) == 1)
    assert r.status == status
    assert (poses[:, 3] == [0.0, 0.0, 0.0, 1.0]).all() and np.array_equal(poses[0], c["T0"])       # node 0 stays where it was put
    again = graph.optimise(*_args(c))
    assert _bytes(again) == _bytes((poses, r))                        # the same call, the same bytes


def test_contradiction_ends_above_the_threshold(graph):
    _, r = graph.optimise(*_args(pc.case(pc.CONTRADICTION)))
    assert r.status == 0 and r.chi2_end >= 10.0


def test_no_state_survives_a_call(ctx):
    """64 loops after 1 loop (and after a converged call) on the same object: the bytes of a fresh object"""
    from kintinuous_amd import abi
    small, big = pc.case("n257_two"), pc.case("n257_l64")
    one = {**small, "loop_a": small["loop_a"][:1], "loop_b": small["loop_b"][:1], "loop_Z": small["loop_Z"][:1]}
    fresh = abi.PoseGraph(ctx, 300, 64)
    want = _bytes(fresh.optimise(*_args(big)))
    fresh.close()
    g = abi.PoseGraph(ctx, 300, 64)
    first = _bytes(g.optimise(*_args(one)))
    assert _bytes(g.optimise(*_args(big))) == want
    assert _bytes(g.optimise(*_args(one))) == first                  # and back: nothing of the 64 loops' S is left either
    g.close()


def _raw_call(g, n, T0, cz, L, la, lb, lz, out, res):
    from kintinuous_amd import abi
    p = lambda a: None if a is None else a.ctypes.data
    return abi.lib().kt_pose_graph_optimise(g.h if g is not None else None, n, p(T0), p(cz), L, p(la), p(lb), p(lz), p(out), C.byref(res) if res is not None else None)


def test_capacity_and_bad_arguments(ctx):
    from kintinuous_amd import abi
    ktlib = abi.lib()
    c = pc.case("n65_spans")
    T0, cz = np.ascontiguousarray(c["T0"]), np.ascontiguousarray(c["chain_Z"])
    la, lb, lz = np.ascontiguousarray(c["loop_a"]), np.ascontiguousarray(c["loop_b"]), np.ascontiguousarray(c["loop_Z"])
    g = abi.PoseGraph(ctx, 65, 7)
    before = _bytes(g.optimise(*_args(c)))
    out = np.full((66, 4, 4), -7.0)
    res = abi.PoseGraphResult(-1.0, -2.0, -3, -4)
    untouched = lambda: (out == -7.0).all() and (res.chi2_start, res.chi2_end, res.steps, res.status) == (-1.0, -2.0, -3, -4)
    # one node or one loop too many: KT_ERR_CAPACITY before any work, nothing written
    cz66 = np.concatenate([cz, cz[:1]])
    assert _raw_call(g, 66, T0, cz66, 7, la, lb, lz, out, res) == abi.KT_ERR_CAPACITY and untouched()
    la8, lb8, lz8 = np.append(la, 3).astype(np.int32), np.append(lb, 9).astype(np.int32), np.concatenate([lz, lz[:1]])
    assert _raw_call(g, 65, T0, cz, 8, la8, lb8, lz8, out, res) == abi.KT_ERR_CAPACITY and untouched()
    # null and out-of-range arguments: KT_ERR_ARG
    ARG = 2
    assert _raw_call(None, 65, T0, cz, 7, la, lb, lz, out, res) == ARG
    assert _raw_call(g, 65, None, cz, 7, la, lb, lz, out, res) == ARG
    assert _raw_call(g, 65, T0, None, 7, la, lb, lz, out, res) == ARG
    assert _raw_call(g, 65, T0, cz, 7, None, lb, lz, out, res) == ARG
    assert _raw_call(g, 65, T0, cz, 7, la, None, lz, out, res) == ARG
    assert _raw_call(g, 65, T0, cz, 7, la, lb, None, out, res) == ARG
    assert _raw_call(g, 65, T0, cz, 7, la, lb, lz, None, res) == ARG
    assert _raw_call(g, 65, T0, cz, 7, la, lb, lz, out, None) == ARG
    assert _raw_call(g, 0, T0, cz, 0, None, None, None, out, res) == ARG
    assert _raw_call(g, 65, T0, cz, -1, la, lb, lz, out, res) == ARG
    for bad_a, bad_b in ((65, 0), (-1, 3), (4, 65), (4, -2), (9, 9)):
        la2, lb2 = la.copy(), lb.copy()
        la2[6], lb2[6] = bad_a, bad_b
        assert _raw_call(g, 65, T0, cz, 7, la2, lb2, lz, out, res) == ARG
    assert untouched()
    h = C.c_void_p()
    assert ktlib.kt_pose_graph_create(ctx.h, 0, 4, None, C.byref(h)) == ARG
    assert ktlib.kt_pose_graph_create(ctx.h, 16, 65, None, C.byref(h)) == ARG
    assert ktlib.kt_pose_graph_create(ctx.h, 16, -1, None, C.byref(h)) == ARG
    assert ktlib.kt_pose_graph_create(None, 16, 4, None, C.byref(h)) == ARG
    assert ktlib.kt_pose_graph_create(ctx.h, 16, 4, None, None) == ARG
    assert ktlib.kt_pose_graph_destroy(None) == 0
    assert _bytes(g.optimise(*_args(c))) == before                    # still usable, and unchanged by the refused calls
    g.close()


def test_allocations_return(ctx):
    from kintinuous_amd import abi
    ctx.sync()
    start = abi.live_allocations()
    g = abi.PoseGraph(ctx, 1025, 64)
    assert abi.live_allocations()[0] > start[0]
    g.optimise(*_args(pc.case("n65_spans")))
    g.close()
    assert abi.live_allocations() == start
    g = abi.PoseGraph(ctx, 8, 0)                                      # no room for loops at all: a chain still composes
    c = pc.case("n2_chain")
    poses, r = g.optimise(*_args(c))
    assert (r.steps, r.status) == (0, 0) and np.abs(poses[1] - c["T0"] @ c["chain_Z"][0]).max() < 1e-14
    g.close()
    assert abi.live_allocations() == start


# ---- above 65536 nodes (pg_scan_carry's serial runs of per >= 2 block totals) and at the step limit -----------------------------------------
@pytest.fixture(scope="module")
def big_graph(ctx):
    """131073 nodes: 513 block totals, three per lane of the carry scan; about 155 MB on the device"""
    from kintinuous_amd import abi
    g = abi.PoseGraph(ctx, 131073, 64)
    yield g
    g.close()


def _first_difference(poses, want):
    k = int(np.nonzero((poses != want).reshape(len(poses), -1).any(1))[0][0])
    return "first node that differs: %d (block %d, element %d), by %.3e" % (k, k // 256, k % 256, np.abs(poses[k] - want[k]).max())


@pytest.mark.parametrize("name", ["n2_chain", "n257_chain"] + pc.LARGE_CHAINS)
def test_chain_only_poses_are_bit_equal(big_graph, name):
    """without loops the poses are products alone: + and * in double, uncontracted, in the scan tree's order on both sides -- neither sin, cos,
    atan2 nor sqrt is on the path, so the restatement's bytes are the device's (chi2 does pass through Log_SO3 and keeps its bound)"""
    c = pc.case(name)
    want, chi2_start, chi2_end, steps, status, deltas = pc.restated(name)
    poses, r = big_graph.optimise(*_args(c))
    equal = poses.tobytes() == want.tobytes()
    print(name, "bit-equal" if equal else _first_difference(poses, want), "chi2", r.chi2_start, r.chi2_end, "restated", chi2_start, chi2_end)
    assert equal, _first_difference(poses, want)
    assert abs(r.chi2_start - chi2_start) <= pc.chi2_bound(chi2_start) and abs(r.chi2_end - chi2_end) <= pc.chi2_bound(chi2_end)
    assert (r.steps, r.status) == (steps, status) == (0, 0)
    assert (poses[:, 3] == [0.0, 0.0, 0.0, 1.0]).all() and np.array_equal(poses[0], c["T0"])
    assert _bytes(big_graph.optimise(*_args(c))) == _bytes((poses, r))


def test_large_case_with_loops_matches_restatement(big_graph):
    """n65537_l7 (per = 2 in the carry scan, seven loops).  Measured on an MI355X: largest pose difference 1.4e-14, chi2 551.7561495627116 ->
    0.1663282742223818 (restated ...8230), 4 steps on both sides"""
    c = pc.case(pc.LARGE_LOOPS)
    want, chi2_start, chi2_end, steps, status, deltas = pc.restated(pc.LARGE_LOOPS)
    poses, r = big_graph.optimise(*_args(c))
    diff = float(np.abs(poses - want).max())
    print(pc.LARGE_LOOPS, "largest pose difference %.3e" % diff, "chi2", r.chi2_start, r.chi2_end, "restated", chi2_start, chi2_end, "steps", r.steps, steps, "status",
          r.status, "deltas", deltas)
    assert diff <= pc.BOUND
    assert abs(r.chi2_start - chi2_start) <= pc.chi2_bound(chi2_start) and abs(r.chi2_end - chi2_end) <= pc.chi2_bound(chi2_end)
    assert (r.steps, r.status) == (steps, status)                     # no allowance: the case's seed keeps every delta away from 1e-9
    assert (poses[:, 3] == [0.0, 0.0, 0.0, 1.0]).all() and np.array_equal(poses[0], c["T0"])
    assert _bytes(big_graph.optimise(*_args(c))) == _bytes((poses, r))


def test_large_case_with_exact_measurements_gives_the_truth(big_graph):
    c = pc.noise_free(pc.LARGE_LOOPS)
    poses, r = big_graph.optimise(*_args(c))
    diff = float(np.abs(poses - c["truth"]).max())
    print(pc.LARGE_LOOPS, "exact measurements: largest difference to the truth %.3e" % diff, "chi2", r.chi2_start, r.chi2_end, "steps", r.steps)
    assert r.status == 0 and r.steps <= 2
    assert diff <= pc.EXACT_BOUND_LARGE


def test_step_limit(ctx, big_graph):
    """20 steps without convergence: KT_POSE_GRAPH_MAX_STEPS, the unconverged state exported, and none of it (done, steps, maxdelta_bits)
    left for the next call on the object.  Measured on an MI355X: largest pose difference 6.7e-15, chi2_end 5752.812034588508 (restated ...514)"""
    from kintinuous_amd import abi, pose_graph_ref as ref
    c, other = pc.case(pc.STEP_LIMIT), pc.case("n65_spans")
    want, chi2_start, chi2_end, steps, status, deltas = pc.restated(pc.STEP_LIMIT)
    poses, r = big_graph.optimise(*_args(c))
    diff = float(np.abs(poses - want).max())
    print(pc.STEP_LIMIT, "largest pose difference %.3e" % diff, "chi2", r.chi2_start, r.chi2_end, "restated", chi2_start, chi2_end, "steps", r.steps, "status", r.status)
    assert (r.steps, r.status) == (20, abi.KT_POSE_GRAPH_MAX_STEPS) and (steps, status) == (20, ref.MAX_STEPS)
    assert diff <= pc.BOUND
    assert abs(r.chi2_start - chi2_start) <= pc.chi2_bound(chi2_start) and abs(r.chi2_end - chi2_end) <= pc.chi2_bound(chi2_end)
    assert (poses[:, 3] == [0.0, 0.0, 0.0, 1.0]).all() and np.array_equal(poses[0], c["T0"])
    first = _bytes((poses, r))
    assert _bytes(big_graph.optimise(*_args(c))) == first
    fresh = abi.PoseGraph(ctx, 65, 7)
    fresh_other = _bytes(fresh.optimise(*_args(other)))
    assert _bytes(fresh.optimise(*_args(c))) == first                # a fresh object's first call ends the same way
    fresh.close()
    assert _bytes(big_graph.optimise(*_args(other))) == fresh_other   # a converging call right after the unfinished one
    assert _bytes(big_graph.optimise(*_args(c))) == first


def test_capacity_of_the_large_object(ctx, big_graph):
    from kintinuous_amd import abi
    c = pc.case("n2_chain")
    before = _bytes(big_graph.optimise(*_args(c)))
    T0, cz = np.ascontiguousarray(c["T0"]), np.ascontiguousarray(c["chain_Z"])
    out = np.full((2, 4, 4), -7.0)                                    # dummy-sized: a refused call reads and writes nothing
    res = abi.PoseGraphResult(-1.0, -2.0, -3, -4)
    assert _raw_call(big_graph, 131074, T0, cz, 0, None, None, None, out, res) == abi.KT_ERR_CAPACITY
    assert (out == -7.0).all() and (res.chi2_start, res.chi2_end, res.steps, res.status) == (-1.0, -2.0, -3, -4)
    assert _bytes(big_graph.optimise(*_args(c))) == before
    ctx.sync()
    start = abi.live_allocations()
    g = abi.PoseGraph(ctx, 131073, 64)
    assert abi.live_allocations()[0] > start[0]
    g.optimise(*_args(pc.case("n65_spans")))
    g.close()
    assert abi.live_allocations() == start


# ---- the shell and the driver ------------------------------------------------------------------------------------------------------------
def _read_poses(path):
    """a .poses file: [(utime, 4x4 float32)] from `seconds x y z qx qy qz qw`"""
    from scipy.spatial.transform import Rotation
    out = []
    for line in open(path).read().splitlines():
        v = [float(x) for x in line.split()]
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = Rotation.from_quat(v[4:8]).as_matrix()
        T[:3, 3] = v[1:4]
        out.append((int(round(v[0] * 1e6)), T))
    return out


def _shell_through_restatement(dense, loops, thresh):
    """iSAMInterface + the driver's -pg walk, with pose_graph_ref in the place of the device: (graph lines, poses by time)"""
    from kintinuous_amd import pose_graph_ref as ref
    eye = np.eye(4, dtype=np.float32)
    times, chain, seen = [], [], set()
    for (t1, P), (t2, Q) in zip(dense[:-1], dense[1:]):
        if t1 >= t2 or (t1, t2) in seen:
            continue
        if not times:
            times.append(t1)
            T0 = ref.measurement(eye, P)
        assert times[-1] == t1 and t2 not in times
        seen.add((t1, t2))
        chain.append(ref.measurement(P, Q))
        times.append(t2)
    kept, lines = [], []
    run = lambda ls: ref.optimise(T0, chain, [times.index(l[0]) for l in ls], [times.index(l[1]) for l in ls], [l[2] for l in ls])
    for t1, t2, icp in loops:
        cand = (t1, t2, ref.measurement(eye, icp))
        _, _, chi2, steps, _, _ = run(kept + [cand])
        stays = chi2 < thresh
        if stays:
            kept.append(cand)
        lines.append((t1, t2, chi2, "kept" if stays else "rejected", steps))
    poses = run(kept)[0]
    return lines, sorted(zip(times, poses), key=lambda p: p[0])


def test_driver_pg(ctx, tmp_path):
    """kintinuous_hip -v x -lc -pg on the ten-frame walk of tests/test_gpu_loop_db.py: .graph and _opt.poses agree with the shell's logic
    driven through the restatement from the run's own dense poses and .loops; without -pg neither file exists and nothing else changes.
    The .poses format keeps six significant digits, so the Python side starts from inputs that are 1e-6 off the driver's: poses are compared
    to 1e-4 (the chain's 9 edges and a loop spread such errors, they do not amplify them), chi2 to 2 % + 1e-3, flags and times exactly."""
    import loop_db_cases as dc
    from kintinuous_amd import build, klg, synth
    build.build_host()
    frames = [dc.frames()[k] for k in range(10)]
    log = str(tmp_path / "ten.klg")
    klg.write_klg(log, frames + [frames[-1]], timestamps=[1000 * (k + 1) for k in range(10)] + [99000], cols=dc.COLS, rows=dc.ROWS)
    cam = dc.camera()
    calib = tmp_path / "calib.txt"
    calib.write_text(f"{cam.fx!r} {cam.fy!r} {cam.cx!r} {cam.cy!r}\n")
    tfile = str(tmp_path / "traj.csv")
    synth.write_trajectory_file(tfile, [1000 * (k + 1) for k in range(10)], synth.ground_truth_rows([(T[:3, :3], T[:3, 3]) for T in dc.poses()]))

    def run(name, *extra):
        prefix = str(tmp_path / name)
        r = subprocess.run([build.HOST_BIN, "-l", log, "-c", str(calib), "-n", "96", "-w", str(dc.COLS), "-h", str(dc.ROWS), "-s", "6", "-p", tfile, "-o", prefix,
                            "-v", "vocab.yml.gz", "-lc", "-dl", "3", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (extra, r.returncode, r.stdout, r.stderr[-2000:])
        print(r.stdout, r.stderr)
        return r, prefix

    plain, p0 = run("lc")
    pg, p1 = run("pg", "-pg")
    none, p2 = run("none", "-pg", "-it", "0")
    # without -pg: neither file, and -pg changes nothing else
    assert not os.path.exists(p0 + ".graph") and not os.path.exists(p0 + "_opt.poses")
    for ext in (".poses", ".loops"):
        assert open(p0 + ext, "rb").read() == open(p1 + ext, "rb").read() == open(p2 + ext, "rb").read()
    strip = lambda out: [l for l in out.splitlines() if not l.startswith(("pose graph", "frames ", "loops "))]
    assert strip(plain.stdout) == strip(pg.stdout)
    # the driver's dense poses: .poses leaves the first frame out, _opt.poses holds every node -- and with every loop rejected (-it 0) it
    # is the chain's composition, i.e. the dense poses themselves, which the last lines of this test check against .poses
    dense = _read_poses(p2 + "_opt.poses")
    assert len(dense) == len(_read_poses(p1 + ".poses")) + 1
    loops = []
    for line in open(p1 + ".loops").read().splitlines():
        f = line.split()
        loops.append((int(f[0]), int(f[1]), np.array([float.fromhex(v) for v in f[5:21]], np.float32).reshape(4, 4)))
    assert len(loops) >= 1
    for prefix, thresh in ((p1, 10.0), (p2, 0.0)):
        want_lines, want_poses = _shell_through_restatement(dense, loops, thresh)
        got_lines = [l.split() for l in open(prefix + ".graph").read().splitlines()]
        print(got_lines, want_lines)
        assert len(got_lines) == len(want_lines) == len(loops)
        for g, w in zip(got_lines, want_lines):
            assert (int(g[0]), int(g[1]), g[3]) == (w[0], w[1], w[3])
            assert abs(float.fromhex(g[2]) - w[2]) <= 0.02 * w[2] + 1e-3 and abs(int(g[4]) - w[4]) <= 1
        got_poses = _read_poses(prefix + "_opt.poses")
        assert [t for t, _ in got_poses] == [t for t, _ in want_poses]
        worst = max(float(np.abs(g.astype(np.float64) - w).max()) for (_, g), (_, w) in zip(got_poses, want_poses))
        print("threshold", thresh, "largest difference to the restatement's poses %.3e" % worst)
        assert worst <= 1e-4
    # every loop rejected: the optimised trajectory is the chain's composition, i.e. the input poses (node order = time order here)
    assert all(l.split()[3] == "rejected" for l in open(p2 + ".graph").read().splitlines())
    by_time = dict(dense)
    assert max(float(np.abs(g - by_time[t]).max()) for t, g in _read_poses(p2 + ".poses")) <= 3e-5   # two roundings to six digits of coordinates up to 6 m
    assert "kept" in open(p1 + ".graph").read()                      # the walk's own loop agrees with its ground-truth chain
