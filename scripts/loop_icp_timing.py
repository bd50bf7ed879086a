#!/usr/bin/env python3
"""Time of the loop-closure registration stage (kt_loop_icp_depth_frames) on a 640x480 pair of the room scene at the
512^3 / 6 m leaf (2.5 voxel edges): the mean wall-clock time of repeated synchronous calls after a warm-up (the call uploads both frames,
runs the stage and returns the transform: what a backend thread would wait for), with the spread, the cloud sizes and the iteration
count.  Also the time of a float64 scipy (cKDTree) run of the same iterations on the same pair: "what a CPU does" with a kd-tree -- it
is NOT PCL's time, PCL is not on this machine.

    python scripts/loop_icp_timing.py [--calls 20] [--warmup 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import loop_icp_cases as lc
    from kintinuous_amd import abi
    cam, d1 = lc.render(640, 480, "A")
    _, d2 = lc.render(640, 480, "B")
    intr = abi.Intr(cam.fx, cam.fy, cam.cx, cam.cy)
    ctx = abi.Ctx(0)
    for _ in range(a.warmup):
        M, score, info = ctx.loop_icp_depth_frames(d1, d2, intr, lc.bootstrap(), lc.LEAF)
    ts = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        ctx.loop_icp_depth_frames(d1, d2, intr, lc.bootstrap(), lc.LEAF)
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    print(f"kt_loop_icp_depth_frames 640x480, leaf {lc.LEAF:.5f} m: mean {ts.mean():.3f} ms  (min {ts.min():.3f}, median {np.median(ts):.3f}, max {ts.max():.3f}; "
          f"{a.calls} calls after {a.warmup})")
    print(f"  clouds {info['n_source']} -> {info['n_target']} points, {info['iterations']} iterations, converged {info['converged']}, score {score:.6f}")
    t0 = time.perf_counter()
    M64, s64, its, sec_icp = lc.icp64(d1, d2, cam, lc.bootstrap(), lc.LEAF)
    print(f"float64 scipy cKDTree run of the same stage on the CPU (not PCL): {1e3 * (time.perf_counter() - t0):.1f} ms in all, "
          f"{1e3 * sec_icp:.1f} ms in its {its} iterations; score {s64:.6f}")
    ctx.close()


if __name__ == "__main__":
    main()
