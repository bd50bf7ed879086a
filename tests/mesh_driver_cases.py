"""The two logs the driver tests of the -m mesh passes run kintinuous_hip on, and what they list afterwards.  Each driver returns
run(name, *extra, ok=True) -> (completed process, prefix): one run of the driver with the log's fixed options, the outputs under
<tmp_path>/<name>*, its exit status asserted to be 0 (ok) or not 0 (not ok).  run.cam is the camera of the log."""
import os
import subprocess


def outputs(tmp_path, prefix):
    """what a run wrote, as the endings behind its prefix, sorted"""
    base = os.path.basename(prefix)
    return sorted(f[len(base):] for f in os.listdir(tmp_path) if f.startswith(base + ".") or f.startswith(base + "_"))


def _driver(tmp_path, cam, log, options, **how):
    from kintinuous_amd import build
    build.build_host()
    calib = tmp_path / "calib.txt"
    calib.write_text(f"{cam.fx!r} {cam.fy!r} {cam.cx!r} {cam.cy!r}\n")

    def run(name, *extra, ok=True):
        prefix = str(tmp_path / name)
        r = subprocess.run([build.HOST_BIN, "-l", log, "-c", str(calib), "-n", "96", "-w", str(cam.cols), "-h", str(cam.rows), *options, "-o", prefix, *extra],
                           capture_output=True, text=True, timeout=120, **how)
        assert (r.returncode == 0) == ok, (extra, r.returncode, r.stdout, r.stderr[-2000:])
        return r, prefix

    run.cam = cam
    return run


def crab_walk_driver(tmp_path):
    """the out-and-back crab-walk along the wall: 40 frames at 160 x 120, N = 96, a 5.2 m volume shifting every 3 voxels"""
    from kintinuous_amd import klg, synth
    cam = synth.Camera.small(160, 120)
    traj = synth.crabwalk_trajectory(420)
    frames = [synth.render(synth.Scene("wall"), cam, *traj[i]) for i in list(range(0, 40, 2)) + list(range(40, 0, -2))]
    log = str(tmp_path / "crab.klg")
    klg.write_klg(log, list(frames) + [frames[-1]], cols=cam.cols, rows=cam.rows)
    return _driver(tmp_path, cam, log, ["-s", "5.2", "-t", "3"], cwd=str(tmp_path))


def loop_log_driver(tmp_path):
    """the ten-frame walk of loop_db_cases.py with its ground-truth trajectory, through loop closure, pose graph and deformation (-df)"""
    import loop_db_cases as lc
    from kintinuous_amd import klg, synth
    frames = [lc.frames()[k] for k in range(10)]
    stamps = [1000 * (k + 1) for k in range(10)]
    log = str(tmp_path / "ten.klg")
    klg.write_klg(log, frames + [frames[-1]], timestamps=stamps + [99000], cols=lc.COLS, rows=lc.ROWS)
    tfile = str(tmp_path / "traj.csv")
    synth.write_trajectory_file(tfile, stamps, synth.ground_truth_rows([(T[:3, :3], T[:3, 3]) for T in lc.poses()]))
    return _driver(tmp_path, lc.camera(), log, ["-s", "6", "-p", tfile, "-v", "vocab.yml.gz", "-lc", "-dl", "3", "-pcd", "-pg", "-df", "-dg", "0.02", "-ds", "1e-9"])
