#!/usr/bin/env python3
"""Time of the deformation-graph stage (kt_deform_*): the wall clock around the synchronous calls, the median of --calls
after --warmup, on the spiral maps of tests/deform_cases.py at any size.
  optimise  kt_deform_optimise (upload, weights of the sources, lists, every Gauss-Newton step enqueued at once, one wait, one download)
            at 100 / 1000 nodes with 1e3 / 1e4 constraints, with the 0.1 gate taken away (see main)
  weights   kt_deform_weights_device + a wait, against the HBM bound of its bytes: 48 + 8 read and 48 written per point
  apply     kt_deform_apply_device + a wait: 48 + 48 read and 28 written per point
at 1e5 / 1e6 / 4e6 points.
  mesh      kt_deform_apply_mesh_device + a wait on as many 16-byte vertices in --spans spans (12 read and 12 written per vertex, the span
            table and the window's nodes aside; the bound is taken for 28: a 16-byte read, a 12-byte write), and beside it, in the same
            process, the route such a mesh had to take before: the same positions as 48-byte points with a time each through
            kt_deform_weights_device + kt_deform_apply_device and ONE wait (104 + 124 bytes per vertex)

    python scripts/deform_timing.py [--calls 20] [--warmup 3] [--nodes 100 1000] [--constraints 1000 10000] [--points 100000 1000000 4000000] [--hbm-gbs 8000]
                                    [--spans 8] [--only optimise passes mesh]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def world(M, n, L, seed=1):
    import deform_cases as dc
    from kintinuous_amd import abi
    rng = np.random.default_rng(seed)
    node_pos = dc.curve(np.arange(M)).astype(np.float32)
    node_time = (dc.T0 + dc.DT * np.arange(M)).astype(np.uint64)
    u = rng.uniform(-0.5, M - 0.5, n)
    pts = np.zeros(n, dtype=abi.NPOINT_DTYPE)
    pts["xyz"] = (dc.curve(u) + rng.uniform(-1.0, 1.0, (n, 3))).astype(np.float32)
    pts["normal"] = [0.0, 0.0, 1.0]
    times = np.round(dc.T0 + dc.DT * u).astype(np.uint64)
    su = np.sort(rng.uniform(0.0, M - 1.0, L))
    src = dc.curve(su).astype(np.float32)
    return node_pos, node_time, pts, times, src, np.round(dc.T0 + dc.DT * su).astype(np.uint64), dc.corrected(src.astype(np.float64), su / (M - 1.0))


def mesh_state(M, seed=2):
    """a state near the identity, as an optimise leaves it: the apply passes then do work that moves something"""
    rng = np.random.default_rng(seed)
    x = np.zeros((M, 12))
    x[:, [0, 4, 8]] = 1.0
    return x + 0.01 * rng.standard_normal((M, 12))


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
    ap.add_argument("--nodes", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--constraints", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--points", type=int, nargs="+", default=[100000, 1000000, 4000000])
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the bound is computed from, GB/s")
    ap.add_argument("--spans", type=int, default=8, help="the spans of the mesh rows")
    ap.add_argument("--only", nargs="+", default=["optimise", "passes", "mesh"], choices=["optimise", "passes", "mesh"])
    a = ap.parse_args()
    from kintinuous_amd import abi
    ctx = abi.Ctx(0)
    dg = abi.DeformationGraph(ctx, max(a.nodes), max(a.constraints))
    # |r_con| / n_con falls with the number of constraints (a drift of 0.3 m is below the 0.1 gate from about 1000 of them on), and a call
    # that stops at the gate times nothing but the start: the gate is taken away so that the steps run
    gate_off = abi.DeformParams(significant_error=0.0)
    for M in a.nodes:
        for L in a.constraints if "optimise" in a.only else []:
            node_pos, node_time, _, _, src, src_time, target = world(M, 0, L)
            dg.set_graph(node_pos, node_time)
            out = {}

            def call():
                out["r"] = dg.optimise(src, src_time, target, gate_off)[1]
            med, lo, hi = timed(call, a.calls, a.warmup)
            r = out["r"]
            print(f"nodes {M} constraints {L}: kt_deform_optimise median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}; {a.calls} calls after {a.warmup}); steps {r.steps} "
                  f"status {r.status} error {r.error_start:.6g} -> {r.error_end:.6g}", flush=True)
        for n in a.points if "passes" in a.only else []:
            _, _, pts, times, _, _, _ = world(M, n, 1)
            dp, dt, di, dw = ctx.upload(pts), ctx.upload(times), ctx.empty(16 * n), ctx.empty(32 * n)

            def weights():
                dg.weights_device(dp, dt, n, di, dw)
                ctx.sync()

            def apply():
                dg.apply_device(dp, di, dw, n)
                ctx.sync()
            for name, fn, nbytes in (("weights", weights, (48 + 8 + 48) * n), ("apply", apply, (48 + 48 + 28) * n)):
                med, lo, hi = timed(fn, a.calls, a.warmup)
                bound = nbytes / (a.hbm_gbs * 1e9) * 1e3
                print(f"nodes {M} points {n}: {name} median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {nbytes / 1e6:.1f} MB, HBM bound {bound:.3f} ms at "
                      f"{a.hbm_gbs:.0f} GB/s: {med / bound:.1f} x the bound, {nbytes / med / 1e6:.0f} GB/s", flush=True)
            for b in (dp, dt, di, dw):
                b.free()
        for n in a.points if "mesh" in a.only else []:
            node_pos, node_time, pts, _, _, _, _ = world(M, n, 1)
            dg.set_graph(node_pos, node_time)
            dg.set_state(mesh_state(M))
            first = np.linspace(0, n, a.spans + 1).astype(np.uintp)          # spans of equal size, like the slabs of a steady walk
            span_time = np.round(node_time[0] + (node_time[-1] - node_time[0]) * (np.arange(a.spans) + 0.5) / a.spans).astype(np.uint64)
            v = np.zeros(n, dtype=abi.MESH_VERTEX_DTYPE)
            v["xyz"], v["rgb"] = pts["xyz"], 0x00c08040
            times = np.repeat(span_time, np.diff(first.astype(np.int64)))
            dv, dp, dt, di, dw = ctx.upload(v), ctx.upload(pts), ctx.upload(times), ctx.empty(16 * n), ctx.empty(32 * n)

            def fused():
                dg.apply_mesh_device(dv, n, first, span_time)
                ctx.sync()

            def two_calls():
                dg.weights_device(dp, dt, n, di, dw)
                dg.apply_device(dp, di, dw, n)
                ctx.sync()
            # the passes run in place: a call deforms what the call before left, which changes no time (finite positions, the same windows)
            fm, flo, fhi = timed(fused, a.calls, a.warmup)
            tm, tlo, thi = timed(two_calls, a.calls, a.warmup)
            bound = 28 * n / (a.hbm_gbs * 1e9) * 1e3
            print(f"nodes {M} vertices {n} spans {a.spans}: fused mesh median {fm:.3f} ms (min {flo:.3f}, max {fhi:.3f}); 24 B per vertex moved, HBM bound for 28 B "
                  f"{bound:.4f} ms at {a.hbm_gbs:.0f} GB/s: {bound / fm:.3f} of the bound's rate; two-call route median {tm:.3f} ms (min {tlo:.3f}, max {thi:.3f}), "
                  f"228 B per vertex; fused / two-call {fm / tm:.2f}", flush=True)
            for b in (dv, dp, dt, di, dw):
                b.free()
    dg.close()
    ctx.close()


if __name__ == "__main__":
    main()
