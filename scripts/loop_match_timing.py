#!/usr/bin/env python3
"""Time of the loop-closure bootstrap stage (kt_loop_match_frames) on the 640x480 pair (A, B) of the room scene with the
blocky scene texture of tests/loop_match_cases.py: the wall-clock time of repeated synchronous calls after a warm-up (the call uploads
both frames, runs keypoints, matching and RANSAC, refits on the host and returns the bootstrap: what a backend thread would wait for),
with the spread and the counts.  Also the time of the numpy restatement (kintinuous_amd/loop_match_ref.py) on this machine's CPU: the
RESTATEMENT's time, not SURF's and not OpenCV's -- neither is on this machine.

    python scripts/loop_match_timing.py [--calls 20] [--warmup 3]
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
    import loop_match_cases as mc
    from kintinuous_amd import abi, loop_match_ref as ref
    cam, d_old, rgb_old = mc.frame(640, 480, "A")
    _, d_new, rgb_new = mc.frame(640, 480, "B")
    intr = abi.Intr(cam.fx, cam.fy, cam.cx, cam.cy)
    ctx = abi.Ctx(0)
    for _ in range(a.warmup):
        got = ctx.loop_match_frames(rgb_old, d_old, rgb_new, d_new, intr)
    ts = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        ctx.loop_match_frames(rgb_old, d_old, rgb_new, d_new, intr)
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    print(f"kt_loop_match_frames 640x480: min {ts.min():.3f} ms, median {np.median(ts):.3f} ms, max {ts.max():.3f} ms ({a.calls} calls after {a.warmup}; "
          f"the time includes the binding's array set-up)")
    print(f"  {got['info']}")
    t0 = time.perf_counter()
    want = ref.loop_match_frames(rgb_old, d_old, rgb_new, d_new, cam.fx, cam.fy, cam.cx, cam.cy, ref.Params())
    print(f"the numpy restatement of the same stage on the CPU (not SURF, not OpenCV): {1e3 * (time.perf_counter() - t0):.1f} ms; {want['info']}")
    ctx.close()


if __name__ == "__main__":
    main()
