"""GPU.  The loop-closure candidate source (csrc/kt_loopdb.hip: kt_loop_db_*) against its numpy restatement
(kintinuous_amd/loop_db_ref.py), which tests/test_loop_db_ref.py ties to an independent matcher and to hand-made selections.  Everything is
integer: results are compared for equality."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import loop_db_cases as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_SIZES = (0, 1, 63, 64, 65, 511, 512, 513, 2048)     # the tile and wave edges
QUERY_SIZES = (1, 64, 65, 257, 2048)


@functools.lru_cache(maxsize=None)
def _score_case():
    """(queries by size, the nine entries, the restatement's scores [query size][entry]), computed once"""
    from kintinuous_amd import loop_db_ref as ref
    rng = np.random.default_rng(17)
    queries = {n: dc.random_descriptors(rng, n) for n in QUERY_SIZES}
    planted = queries[257]
    queries[2048][:257] = planted           # the largest query carries the planted descriptors too
    queries[65][:65] = planted[:65]
    queries[64][:64] = planted[:64]
    queries[1][:1] = planted[:1]
    entries = []
    for n in ENTRY_SIZES:                   # half of an entry: descriptors of the largest query, 5 bits off, from all over its index range
        base = dc.random_descriptors(rng, n)
        for j, i in zip(rng.permutation(n)[: n // 2], rng.permutation(2048)):
            base[j] = dc.flip(queries[2048][i], rng, 5)
        entries.append(dc.planted_entry(rng, planted, n, base=base) if n else base)
    want = {n: ref.scores(q, entries) for n, q in queries.items()}
    return queries, entries, want


def _filled(ctx, entries, max_entries=12):
    from kintinuous_amd import abi
    db = abi.LoopDb(ctx, max_entries)
    for k, e in enumerate(entries):
        assert db.add_descriptors(e) == k
    return db


def test_scores_whole_and_sub_ranges(ctx):
    queries, entries, want = _score_case()
    db = _filled(ctx, entries)
    assert db.size == len(entries)
    E = len(entries)
    for n in QUERY_SIZES:
        got = db.scores(queries[n], 0, E - 1)
        print("query", n, "scores", got.tolist(), "restated", want[n].tolist())
        assert got.tolist() == want[n].tolist()
    assert want[2048][0] == 0 and want[2048][8] > 900 and want[257][8] > 50      # the scores are not all trivial
    q = queries[2048]
    for first, last in ((0, 0), (8, 8), (3, 5), (1, 8), (0, 4)):
        assert db.scores(q, first, last).tolist() == want[2048][first:last + 1].tolist()
    assert db.scores(np.zeros((0, 8), np.uint32), 0, E - 1).tolist() == [0] * E          # an empty query
    assert db.scores(entries[8], 8, 8).tolist() == [_self_score(entries[8])]      # 2048 against themselves, four tiles on both sides
    db.destroy()


def _self_score(e):
    from kintinuous_amd import loop_db_ref as ref
    return ref.score(e, e)


def test_round_trip_and_determinism(ctx):
    queries, entries, want = _score_case()
    runs = []
    for _ in range(2):
        db = _filled(ctx, entries)
        for k, e in enumerate(entries):
            back = db.entry(k)
            assert back.shape == e.shape and back.tobytes() == e.tobytes()
        runs.append([db.scores(queries[n], 0, len(entries) - 1).tobytes() for n in QUERY_SIZES])
        runs[-1].append(db.scores(queries[2048], 0, len(entries) - 1).tobytes())       # the same call again on the same database
        db.destroy()
    assert runs[0] == runs[1] and runs[0][-1] == runs[0][-2]


_SCENARIO = []


def _scenario_gpu_runs(ctx):
    """the ten-frame scenario through kt_loop_db_detect, twice on fresh databases, computed once: [[fields]], the entries read back
    after the first run"""
    from kintinuous_amd import abi
    if _SCENARIO:
        return _SCENARIO[0]
    prm = abi.loop_db_detect_params(**dc.DETECT)
    runs, entries = [], None
    for _ in range(2):
        db = abi.LoopDb(ctx, 12)
        runs.append([db.detect(rgb, depth, prm).fields() for depth, rgb in dc.frames()])
        if entries is None:
            entries = [db.entry(k) for k in range(db.size)]
        db.destroy()
    _SCENARIO.append((runs, entries))
    return runs, entries


def test_scenario_equals_restatement(ctx):
    runs, _ = _scenario_gpu_runs(ctx)
    want = [r.fields() for r in dc.restated()]
    for g, w in zip(runs[0], want):
        print(g, w)
    assert runs[0] == want
    assert runs[0] == runs[1]               # determinism


def test_detect_stores_frame_keypoints(ctx):
    """an entry added by kt_loop_db_detect holds kt_frame_keypoints' descriptors of that frame"""
    _, entries = _scenario_gpu_runs(ctx)
    for k, (depth, rgb) in enumerate(dc.frames()):
        s, out, n = ctx.frame_keypoints(rgb, depth)
        assert s == 0 and n == dc.KEYPOINTS[k]
        assert entries[k].shape == out[2].shape and entries[k].tobytes() == out[2].tobytes()


def test_reset_forgets_entries_and_island(ctx):
    from kintinuous_amd import abi, loop_db_ref as ref
    frames = dc.frames()
    want = [r.fields() for r in dc.restated()]
    prm = abi.loop_db_detect_params(**dc.DETECT)
    db = abi.LoopDb(ctx, 12)
    assert [db.detect(rgb, depth, prm).fields() for depth, rgb in frames[:7]] == want[:7]      # ends DETECTED: an island is remembered
    db.reset()
    assert db.size == 0
    assert [db.detect(rgb, depth, prm).fields() for depth, rgb in frames] == want              # as new
    # the remembered island does not survive a reset: frames 0, 1, 2 and 8 again (by descriptor), then frame 9 as the FIRST detect call --
    # its island {0} would be consistent with the island 0..2 that the run above left behind
    db.reset()
    desc = dc.descriptors()
    stored = [desc[0], desc[1], desc[2], desc[8]]
    for d in stored:
        db.add_descriptors(d)
    r = db.detect(frames[9][1], frames[9][0], prm)
    w = ref.select(ref.scores(desc[9], stored), None, ref.DetectParams(**dc.DETECT))
    w.n_keypoints = dc.KEYPOINTS[9]
    assert r.fields() == w.fields() and r.status == ref.NOT_CONSISTENT and (r.island_first, r.island_last) == (0, 0)
    db.destroy()


def test_capacity(ctx):
    from kintinuous_amd import abi
    queries, entries, want = _score_case()
    twelve = (entries + entries)[:12]
    db = _filled(ctx, twelve)
    before = db.scores(queries[257], 0, 11).tolist()
    e = C.c_int(-5)
    d = np.ascontiguousarray(entries[3])
    ktlib = abi.lib()
    assert ktlib.kt_loop_db_add_descriptors(db.h, d.ctypes.data, len(d), C.byref(e)) == abi.KT_ERR_CAPACITY and e.value == -5
    depth, rgb = dc.frames()[0]
    res = abi.LoopDbResult()
    prm = abi.loop_db_detect_params()
    assert ktlib.kt_loop_db_detect(db.h, np.ascontiguousarray(rgb).ctypes.data, np.ascontiguousarray(depth).ctypes.data, dc.COLS, dc.ROWS, C.byref(prm),
                                   C.byref(res)) == abi.KT_ERR_CAPACITY
    assert db.size == 12
    for k, ent in enumerate(twelve):
        assert db.entry(k).tobytes() == ent.tobytes()
    assert db.scores(queries[257], 0, 11).tolist() == before == (want[257].tolist() * 2)[:12]   # still usable
    db.destroy()


def test_bad_arguments(ctx):
    from kintinuous_amd import abi
    ktlib = abi.lib()
    queries, entries, _ = _score_case()
    db = _filled(ctx, entries[:3])
    q = np.ascontiguousarray(queries[64])
    out = np.full(4, -7, np.int32)
    sc = lambda n, first, last, o=out.ctypes.data: ktlib.kt_loop_db_scores(db.h, q.ctypes.data, n, first, last, o)
    assert sc(64, 1, 0) == 2 and sc(64, 0, 3) == 2 and sc(64, -1, 1) == 2 and sc(64, 0, 2, None) == 2
    big = np.zeros((2049, 8), np.uint32)
    assert ktlib.kt_loop_db_scores(db.h, big.ctypes.data, 2049, 0, 2, out.ctypes.data) == 2
    assert (out == -7).all()                # nothing was written
    e = C.c_int(-5)
    assert ktlib.kt_loop_db_add_descriptors(db.h, big.ctypes.data, 2049, C.byref(e)) == 2 and db.size == 3
    n = C.c_size_t(0)
    assert ktlib.kt_loop_db_entry(db.h, 3, big.ctypes.data, 2049, C.byref(n)) == 2
    assert ktlib.kt_loop_db_entry(db.h, 2, big.ctypes.data, 1, C.byref(n)) == abi.KT_ERR_CAPACITY and n.value == len(entries[2]) and not big.any()
    assert sc(64, 0, 2) == 0 and (out[:3] >= 0).all()
    h = C.c_void_p()
    p = abi.loop_match_params()
    assert ktlib.kt_loop_db_create(ctx.h, 0, C.byref(p), None, C.byref(h)) == 2
    assert ktlib.kt_loop_db_create(ctx.h, 4, C.byref(abi.loop_match_params(max_keypoints=5000)), None, C.byref(h)) == 2
    assert ktlib.kt_loop_db_size(None) == -1 and ktlib.kt_loop_db_destroy(None) == 0
    db.destroy()


# ---- the tools ---------------------------------------------------------------------------------------------------------------------
def _write_log(tmp_path, name, which):
    """a .klg of the scenario's frames `which` (the reader never returns a log's last frame: it is written twice), times 1000 (k + 1)"""
    from kintinuous_amd import klg
    frames = [dc.frames()[k] for k in which]
    log = str(tmp_path / name)
    klg.write_klg(log, frames + [frames[-1]], timestamps=[1000 * (k + 1) for k in which] + [99000], cols=dc.COLS, rows=dc.ROWS)
    cam = dc.camera()
    calib = tmp_path / "calib.txt"
    calib.write_text(f"{cam.fx!r} {cam.fy!r} {cam.cx!r} {cam.cy!r}\n")
    return log, str(calib)


def _fields(text):
    """'key value; key value' -> [(key, value)] in order (`score` appears twice on an accepted -all line)"""
    return [tuple(part.split(" ", 1)) for part in text.strip().split("; ")]


def _loop_tool_all(log, calib, *extra):
    from kintinuous_amd import build
    r = subprocess.run([build.LOOP_TOOL, "-l", log, "-all", "-w", str(dc.COLS), "-h", str(dc.ROWS), "-c", calib, *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    print(r.stdout)
    return [_fields(l) for l in r.stdout.strip().splitlines()]


def test_loop_tool_all(ctx, tmp_path):
    from kintinuous_amd import abi, build, loop_db_ref as ref
    build.build_host()
    log, calib = _write_log(tmp_path, "ten.klg", range(10))
    lines = _loop_tool_all(log, calib, "-dl", "3", "-k", "1")
    want = dc.restated()
    assert len(lines) == 10
    for i, (f, w) in enumerate(zip(lines, want)):
        head = dict(f[:6])
        assert (int(head["sample"]), head["status"], int(head["candidate"]), int(head["score"]), int(head["reference"]), head["island"].split()) == \
            (i, ref.STATUS_NAMES[w.status], w.candidate, w.candidate_score, w.reference_score, [str(w.island_first), str(w.island_last)])
        assert (len(f) > 6) == (w.status == ref.DETECTED)
    # sample 9's pair is (0, 9): the same fields as loop_tool -a 0 -b 9, which in turn prints what the C-ABI calls give (test_gpu_loop_match.test_shell)
    r = subprocess.run([build.LOOP_TOOL, "-l", log, "-a", "0", "-b", "9", "-w", str(dc.COLS), "-h", str(dc.ROWS), "-c", calib], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    print(r.stdout)
    pair = _fields(r.stdout)
    assert [k for k, _ in pair] == ["matches", "inliers", "share", "score", "verdict", "times", "projected", "constraint"]
    assert lines[9][6:] == pair and dict(pair)["verdict"] == "accepted" and dict(pair)["times"] == "10000 1000"
    (d0, rgb0), (d9, rgb9) = dc.frames()[0], dc.frames()[9]
    cam = dc.camera()
    intr = abi.Intr(cam.fx, cam.fy, cam.cx, cam.cy)
    got = ctx.loop_match_frames(rgb0, d0, rgb9, d9, intr)
    f = dict(pair)
    assert int(f["matches"]) == got["info"]["n_matches"] and int(f["inliers"]) == got["info"]["n_inliers"]
    M, score, _ = ctx.loop_icp_depth_frames(d0, d9, intr, got["bootstrap"], float(np.float32(2.5) * (np.float32(6.0) / np.float32(512))))
    assert np.float32(float.fromhex(f["score"])).tobytes() == np.float32(score).tobytes()
    assert np.array([float.fromhex(v) for v in f["constraint"].split()], np.float32).tobytes() == M.tobytes()
    # every other frame: samples are frames 0, 2, 4, 6, 8
    every = _loop_tool_all(log, calib, "-every", "2", "-dl", "1", "-k", "0")
    db = ref.Database(max_entries=12)
    for i, f in enumerate(every):
        w = db.detect_descriptors(dc.descriptors()[2 * i], ref.DetectParams(dislocal=1, consistency=0))
        assert (dict(f[:6])["status"], int(dict(f[:6])["candidate"])) == (ref.STATUS_NAMES[w.status], w.candidate)
    assert len(every) == 5


def test_driver_lc(ctx, tmp_path):
    """kintinuous_hip -v x -lc: .poses as without -lc, and .loops = the constraints PlaceRecognition yields on the tap's samples"""
    from kintinuous_amd import build, synth
    build.build_host()
    log, calib = _write_log(tmp_path, "ten.klg", range(10))
    stamps = [1000 * (k + 1) for k in range(10)]
    rows = synth.ground_truth_rows([(T[:3, :3], T[:3, 3]) for T in dc.poses()])
    tfile = str(tmp_path / "traj.csv")
    synth.write_trajectory_file(tfile, stamps, rows)

    def run(name, *extra):
        prefix = str(tmp_path / name)
        r = subprocess.run([build.HOST_BIN, "-l", log, "-c", calib, "-n", "96", "-w", str(dc.COLS), "-h", str(dc.ROWS), "-s", "6", "-p", tfile, "-o", prefix, *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (extra, r.returncode, r.stdout, r.stderr[-2000:])
        print(r.stdout, r.stderr)
        return r, prefix

    plain, p0 = run("plain", "-v", "vocab.yml.gz")
    lc, p1 = run("lc", "-v", "vocab.yml.gz", "-lc", "-dl", "3")
    assert open(p0 + ".poses", "rb").read() == open(p1 + ".poses", "rb").read()
    assert not os.path.exists(p0 + ".loops")
    strip = lambda out: [l for l in out.splitlines() if not l.startswith(("loop", "frames "))]
    assert strip(plain.stdout) == strip(lc.stdout)
    # the tap's samples: the first frame, every frame that moved 0.15 or more since the last sample, and the last pose once more
    times = [int(dict(_fields(l))["time"]) for l in lc.stdout.splitlines() if l.startswith("loop sample")]
    print("sampled times", times)
    sampled = [t // 1000 - 1 for t in times]
    assert sampled == TAP_SAMPLES
    assert f"place recognition samples {len(TAP_SAMPLES)} " in lc.stdout
    # the same samples as a log of their own through loop_tool -all (PlaceRecognition, the same class)
    log2, _ = _write_log(tmp_path, "sampled.klg", sampled)
    want = []
    for f in _loop_tool_all(log2, calib, "-dl", "3", "-n", "96", "-s", "6"):     # the driver's volume: the registration's leaf is 2.5 voxel edges
        if len(f) > 6 and dict(f[6:])["verdict"] == "accepted":
            pair = dict(f[6:])
            want.append(" ".join([*pair["times"].split(), pair["matches"], pair["inliers"], pair["score"], pair["constraint"]]))
    got = open(p1 + ".loops").read().splitlines()
    print(got, want)
    assert got == want and len(got) >= 1
    assert f"{len(got)} accepted constraints" in lc.stdout
    # -lc without -v: said so, nothing written
    r, p2 = run("nov", "-lc")
    assert "-lc ignored without -v" in r.stderr and not os.path.exists(p2 + ".loops")


# The tap does not sample every frame of this log: its movement measure (rotation angle + translation) / 2 against the last SAMPLE must reach
# 0.15.  From the ten poses (kt_host_place_recognition_movement): 0.175 for frame 1, 0.189 for frames 2 - 7, 0.119 for frame 8 against 7 (not
# sampled), 0.227 for frame 9 against 7; the first frame is always sampled and the FINAL slice carries the last pose once more.
TAP_SAMPLES = [0, 1, 2, 3, 4, 5, 6, 7, 9, 9]
