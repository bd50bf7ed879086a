#!/usr/bin/env python3
"""Time of the pose-graph stage (kt_pose_graph_optimise): the wall clock around the synchronous call (upload, every
Gauss-Newton step enqueued at once, one wait, one download), repeated after a warm-up, on the closed-curve graphs of
tests/pose_graph_cases.py at N = 1 000, 10 000, 100 000 nodes with L = 1, 8, 64 loops.  Beside each, where it finishes within a minute, the
time of the numpy restatement (kintinuous_amd/pose_graph_ref.py) on the same graph, and the largest difference of the two results.

    python scripts/pose_graph_timing.py [--calls 20] [--warmup 3] [--nodes 1000 10000 100000] [--loops 1 8 64] [--ref-limit 60]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def graph(N, L, seed=1):
    """the ground truth and noise of tests/pose_graph_cases.py at any size: loop 0 closes the curve, the others span random pairs"""
    import pose_graph_cases as pc
    rng = np.random.default_rng(seed)
    T = pc.truth(N)
    Ti = np.linalg.inv(T)
    chain = np.einsum("kij,kjl->kil", Ti[:-1], T[1:])
    for k in range(N - 1):
        chain[k] = chain[k] @ pc.exp(0.5e-3 * rng.standard_normal(3), 0.2e-3 * rng.standard_normal(3))
    pairs = [(N - 1, 0)]
    while len(pairs) < L:
        a, b = (int(v) for v in rng.integers(0, N, 2))
        if a != b:
            pairs.append((a, b))
    loop_Z = np.array([Ti[a] @ T[b] @ pc.exp(pc._bounded(rng, 0.02), pc._bounded(rng, np.deg2rad(2.0))) for a, b in pairs])
    return T[0], chain, np.array([a for a, _ in pairs], np.int32), np.array([b for _, b in pairs], np.int32), loop_Z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nodes", type=int, nargs="+", default=[1000, 10000, 100000])
    ap.add_argument("--loops", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--ref-limit", type=float, default=60.0, help="skip the restatement where its estimated time exceeds this many seconds")
    a = ap.parse_args()
    from kintinuous_amd import abi, pose_graph_ref as ref
    ctx = abi.Ctx(0)
    pg = abi.PoseGraph(ctx, max(a.nodes), max(a.loops))
    ref_rate = None           # seconds per (node x step) of the restatement, from the last run: the estimate that decides whether to run it
    for N in a.nodes:
        for L in a.loops:
            args = graph(N, L)
            for _ in range(a.warmup):
                poses, r = pg.optimise(*args)
            ts = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                poses, r = pg.optimise(*args)
                ts.append(time.perf_counter() - t0)
            ts = np.array(ts) * 1e3
            line = (f"N {N} L {L}: kt_pose_graph_optimise min {ts.min():.3f} ms, median {np.median(ts):.3f} ms, max {ts.max():.3f} ms ({a.calls} calls after {a.warmup}); "
                    f"steps {r.steps} status {r.status} chi2 {r.chi2_start:.6g} -> {r.chi2_end:.6g}")
            pairs = L * (L + 1) // 2
            estimate = None if ref_rate is None else ref_rate * N * (1 + pairs / 40.0) * max(r.steps, 1)
            if estimate is None or estimate <= a.ref_limit:
                t0 = time.perf_counter()
                want = ref.optimise(*args)
                sec = time.perf_counter() - t0
                ref_rate = sec / (N * (1 + pairs / 40.0) * max(want[3], 1))
                line += f"; restatement {sec:.2f} s, steps {want[3]}, largest pose difference {np.abs(poses - want[0]).max():.3e}"
            else:
                line += f"; restatement not run (estimated {estimate:.0f} s)"
            print(line, flush=True)
    pg.close()
    ctx.close()


if __name__ == "__main__":
    main()
