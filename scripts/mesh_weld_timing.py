#!/usr/bin/env python3
"""Time of the seam weld (kt_mesh_weld_device): the wall clock around the synchronous call, the median of --calls after
--warmup, on a mesh of --spans slabs of equal size whose keys rise inside a slab (as the mesh stage emits them) and of which --seam of
each slab's vertices share their key with a vertex of the slab before; 2 triangles per vertex, each over vertices within 4096 of each other.
The bytes the pass must move: 24 B in and 24 B out per vertex (16 of vertex, 8 of key) and 12 B per triangle read and written; the HBM
time that implies stands beside the measurement.  The triangles are remapped in place, so every call after the first remaps the indices
the call before left (they stay below n): the same loads and stores at other addresses.

    python scripts/mesh_weld_timing.py [--calls 20] [--warmup 3] [--vertices 100000 1000000 4000000] [--spans 8] [--seam 0.03] [--gap-us -1] [--hbm-gbs 8000]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOCAL = 4096


def slabs(n, spans, seam, seed=1):
    from kintinuous_amd import abi
    rng = np.random.default_rng(seed)
    first = np.linspace(0, n, spans + 1).astype(np.int64)
    keys = np.zeros(n, np.uint64)
    tri = []
    for s in range(spans):
        lo, hi = int(first[s]), int(first[s + 1])
        k = (np.uint64(s) << np.uint64(40)) + np.sort(rng.choice(1 << 36, hi - lo, replace=False).astype(np.uint64)) * np.uint64(4)
        if s > 0 and hi > lo:       # the first of this slab's vertices lie on the plane the slab before left behind: its last keys again
            share = min(int(seam * (hi - lo)), lo - int(first[s - 1]))
            k[:share] = keys[lo - share:lo]
        keys[lo:hi] = k
        # a triangle's vertices lie within LOCAL vertices of each other, as marching cubes leaves them (the rows around one cell)
        base = rng.integers(0, max(hi - lo, 1), (2 * (hi - lo), 1))
        tri.append(lo + (base + rng.integers(0, LOCAL, (2 * (hi - lo), 3))) % max(hi - lo, 1))
    v = np.zeros(n, abi.MESH_VERTEX_DTYPE)
    v["xyz"] = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    v["rgb"] = 0x00c08040
    times = (1_000_000 + 400_000 * np.arange(spans)).astype(np.uint64)
    return v, keys, np.concatenate(tri).astype(np.uint32), first, times


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vertices", type=int, nargs="+", default=[100000, 1000000, 4000000])
    ap.add_argument("--spans", type=int, default=8)
    ap.add_argument("--seam", type=float, default=0.03, help="the share of a slab's vertices that repeat a key of the slab before")
    ap.add_argument("--gap-us", type=int, default=-1, help="max_gap in microseconds (the slabs are 400000 apart); -1: no gate")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the bound is computed from, GB/s")
    a = ap.parse_args()
    from kintinuous_amd import abi
    ctx = abi.Ctx(0)
    w = abi.MeshWeld(ctx)
    gap = abi.NO_GATE if a.gap_us < 0 else a.gap_us
    for n in a.vertices:
        v, keys, tri, first, times = slabs(n, a.spans, a.seam)
        m = len(tri)
        dv, dk, dt, ov, ok = ctx.upload(v), ctx.upload(keys), ctx.upload(tri), ctx.empty(16 * n), ctx.empty(8 * n)
        out = {}

        def call():
            out["r"] = w.weld_device(dv, dk, n, dt, m, first, times, gap, ov, ok, n)      # synchronises once, for n_out
        med, lo, hi = timed(call, a.calls, a.warmup)
        s, n_out, _ = out["r"]
        assert s == abi.KT_OK
        nbytes = 24 * n + 24 * n_out + 2 * 12 * m
        bound = nbytes / (a.hbm_gbs * 1e9) * 1e3
        print(f"vertices {n} spans {a.spans} triangles {m} gate {'none' if a.gap_us < 0 else a.gap_us}: kt_mesh_weld_device median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}; "
              f"{a.calls} calls after {a.warmup}); kept {n_out}; {nbytes / 1e6:.1f} MB to move, HBM bound {bound:.4f} ms at {a.hbm_gbs:.0f} GB/s: {med / bound:.0f} x the bound", flush=True)
        for b in (dv, dk, dt, ov, ok):
            b.free()
    w.close()
    ctx.close()


if __name__ == "__main__":
    main()
