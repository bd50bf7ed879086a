#!/usr/bin/env python3
"""Time of the loop-closure candidate source's scoring (kt_loop_db_scores): a 2048-descriptor query against 64, 256 and
1000 entries of 2048 random descriptors each, as the wall-clock time of repeated synchronous calls after a warm-up (the call uploads the
query, scores every entry in one launch and downloads the scores).  Beside each, the only way to get the same numbers without the
database: one kt_descriptor_match call per entry on the same data (it uploads both descriptor sets every time), counted on the host.

    python scripts/loop_db_timing.py [--calls 20] [--warmup 3] [--baseline-calls 5] [--sizes 64 256 1000]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, calls, warmup):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return np.array(ts) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-calls", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 1000])
    a = ap.parse_args()
    from kintinuous_amd import abi
    K = 2048
    rng = np.random.default_rng(1)
    ctx = abi.Ctx(0)
    query = rng.integers(0, 2 ** 32, size=(K, 8), dtype=np.uint64).astype(np.uint32)
    for E in a.sizes:
        entries = [rng.integers(0, 2 ** 32, size=(K, 8), dtype=np.uint64).astype(np.uint32) for _ in range(E)]
        for e in entries[:: max(E // 16, 1)]:            # some entries share descriptors with the query: scores are not all zero
            e[: K // 4] = query[rng.permutation(K)[: K // 4]]
        db = abi.LoopDb(ctx, E)
        for e in entries:
            db.add_descriptors(e)
        ts, scores = _timed(lambda: db.scores(query, 0, E - 1), a.calls, a.warmup)
        tb, base = _timed(lambda: np.array([int((ctx.descriptor_match(query, e)[0] >= 0).sum()) for e in entries], np.int32), a.baseline_calls, 1)
        same = scores.tolist() == base.tolist()
        dist = E * K * K
        print(f"{E} entries x {K}: kt_loop_db_scores min {ts.min():.3f} ms, median {np.median(ts):.3f} ms, max {ts.max():.3f} ms ({a.calls} calls after {a.warmup}); "
              f"{E} kt_descriptor_match calls min {tb.min():.1f} ms, median {np.median(tb):.1f} ms ({a.baseline_calls} after 1); "
              f"ratio of medians {np.median(tb) / np.median(ts):.1f}; {dist / (np.median(ts) * 1e-3) / 1e12:.2f} T distances/s by the wall clock; "
              f"scores equal: {same}; non-zero scores {int((scores > 0).sum())}")
        if not same or np.median(ts) > np.median(tb):
            print("FAILED: the database is slower than the per-entry calls, or the numbers differ")
            sys.exit(1)
        db.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
