#!/usr/bin/env python3
"""Time of the mesh simplification (kt_mesh_simplify_device) beside the seam weld's at the same size in the same run: the
wall clock around the synchronous call, the median of --calls after --warmup.  The mesh: --spans slabs of equal size side by side along
x, each a whole number of cells thick, each slab's vertices uniform in its box and sorted by position (z, y, x) as a mesher leaves them;
2 triangles per vertex, each over vertices within 4096 of each other in the list.  The cell is 0.02 m and the boxes are sized so that a
cell holds about --members vertices; the measured mean (n / n_out) is printed.  The bytes the pass must move: 16 B per vertex in, 16 B
per vertex out, 12 B per triangle read and 12 B per surviving triangle written; the HBM time that implies stands beside the measurement.
The weld runs on mesh_weld_timing.py's input of the same n and spans.

The quadric form (kt_mesh_simplify_quadric_device) is timed beside the mean form in the same run on a mesh of its own at the same sizes:
the same vertices, but 2 triangles per vertex over vertices within --quadric-local (64) of each other in the list, in the order of their
first vertex -- a mesher's triangles are small and come in cell order, and the form refuses a triangle of about a square metre.  Its ratio
to kt_mesh_simplify_device on that mesh is printed.  Last, --single vertices in ONE cell of half a metre with 2 triangles per vertex: every
term of every triangle goes to the same nine sums.

    python scripts/mesh_simplify_timing.py [--calls 20] [--warmup 3] [--vertices 100000 1000000 4000000] [--spans 8] [--members 4 20] [--hbm-gbs 8000]
                                           [--bias 0.015625] [--quadric-local 64] [--single 1000000] [--no-weld] [--no-mean] [--no-quadric]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
LOCAL = 4096
CELL = 0.02


def slab_mesh(n, spans, members, seed=1, local=LOCAL, in_order=False):
    from kintinuous_amd import abi
    rng = np.random.default_rng(seed)
    cells = max(n / members, 1.0)
    wx = max(round(cells ** (1 / 3) / spans), 1)                 # a slab is a whole number of cells thick: no cell is cut by a span
    yz = max((cells / (spans * wx)) ** 0.5, 1.0)
    first = np.linspace(0, n, spans + 1).astype(np.int64)
    v = np.zeros(n, abi.MESH_VERTEX_DTYPE)
    tri = []
    for s in range(spans):
        lo, hi = int(first[s]), int(first[s + 1])
        p = rng.uniform(0, 1, (hi - lo, 3)) * np.array([wx, yz, yz]) * CELL
        p[:, 0] += (s - spans // 2) * wx * CELL
        p[:, 1:] -= round(yz / 2) * CELL
        c = np.floor(p / CELL).astype(np.int64)
        p = p[np.lexsort((c[:, 0], c[:, 1], c[:, 2]))]
        v["xyz"][lo:hi] = p.astype(np.float32)
        base = rng.integers(0, max(hi - lo, 1), (2 * (hi - lo), 1))
        if in_order:
            base = np.sort(base, axis=0)
        tri.append(lo + (base + rng.integers(0, local, (2 * (hi - lo), 3))) % max(hi - lo, 1))
    v["rgb"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return v, np.concatenate(tri).astype(np.uint32), first


def single_cluster(n, seed=2):
    """n vertices in one cell of half a metre, 2 n triangles between any three of them"""
    from kintinuous_amd import abi
    rng = np.random.default_rng(seed)
    v = np.zeros(n, abi.MESH_VERTEX_DTYPE)
    v["xyz"] = (-0.5 + rng.uniform(0.001, 0.499, (n, 3))).astype(np.float32)
    v["rgb"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return v, rng.integers(0, n, (2 * n, 3)).astype(np.uint32), np.array([0, n], np.int64)


def both_forms(ctx, ws, timed, a, v, tri, first, cell, what):
    """the mean and the quadric form on one mesh: both medians and their ratio"""
    from kintinuous_amd import abi
    n, m = len(v), len(tri)
    dv, dt, ov, ot = ctx.upload(v), ctx.upload(tri), ctx.empty(16 * n), ctx.empty(12 * m)
    out = {}

    def mean():
        out["m"] = ws.simplify_device(dv, n, dt, m, first, cell, ov, n, ot, m)

    def quadric():
        out["q"] = ws.simplify_quadric_device(dv, n, dt, m, first, cell, a.bias, ov, n, ot, m)
    mm, mlo, mhi = timed(mean, a.calls, a.warmup)
    qm, qlo, qhi = timed(quadric, a.calls, a.warmup)
    assert out["m"][0] == abi.KT_OK and out["q"][0] == abi.KT_OK, (out["m"][0], out["q"][0])
    _, n_out, m_out, _, placed = out["q"]
    print(f"{what}: vertices {n} triangles {m} cell {cell} m bias {a.bias}: kt_mesh_simplify_device median {mm:.3f} ms (min {mlo:.3f}, max {mhi:.3f}), "
          f"kt_mesh_simplify_quadric_device median {qm:.3f} ms (min {qlo:.3f}, max {qhi:.3f}): {qm / mm:.2f} x the mean form; out {n_out} vertices "
          f"({n / max(n_out, 1):.1f} per cluster, {placed} placed), {m_out} triangles", flush=True)
    for b in (dv, dt, ov, ot):
        b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vertices", type=int, nargs="+", default=[100000, 1000000, 4000000])
    ap.add_argument("--spans", type=int, default=8)
    ap.add_argument("--members", type=float, nargs="+", default=[4.0, 20.0], help="vertices per cell the boxes are sized for")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the bound is computed from, GB/s")
    ap.add_argument("--no-weld", action="store_true", help="leave the weld out (for a kernel trace of the simplification alone)")
    ap.add_argument("--no-mean", action="store_true", help="leave the mean form's table out (for a kernel trace of the quadric form's runs)")
    ap.add_argument("--no-quadric", action="store_true", help="leave the quadric form out")
    ap.add_argument("--bias", type=float, default=0.015625, help="of the quadric form")
    ap.add_argument("--quadric-local", type=int, default=64, help="the list distance of a triangle's vertices on the quadric form's mesh")
    ap.add_argument("--single", type=int, default=1000000, help="vertices of the single-cluster case (0: none)")
    a = ap.parse_args()
    from kintinuous_amd import abi
    from mesh_weld_timing import slabs, timed
    ctx = abi.Ctx(0)
    w, ws = abi.MeshWeld(ctx), abi.MeshSimplify(ctx)
    for n in a.vertices:
        weld_med = None
        if not a.no_weld:
            v, keys, tri, first, times = slabs(n, a.spans, 0.03)
            m = len(tri)
            dv, dk, dt, ov, ok = ctx.upload(v), ctx.upload(keys), ctx.upload(tri), ctx.empty(16 * n), ctx.empty(8 * n)
            weld_med, lo, hi = timed(lambda: w.weld_device(dv, dk, n, dt, m, first, times, abi.NO_GATE, ov, ok, n), a.calls, a.warmup)
            print(f"vertices {n} spans {a.spans} triangles {m}: kt_mesh_weld_device median {weld_med:.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
            for b in (dv, dk, dt, ov, ok):
                b.free()
        for members in ([] if a.no_mean else a.members):
            v, tri, first = slab_mesh(n, a.spans, members)
            m = len(tri)
            dv, dt, ov, ot = ctx.upload(v), ctx.upload(tri), ctx.empty(16 * n), ctx.empty(12 * m)
            out = {}

            def call():
                out["r"] = ws.simplify_device(dv, n, dt, m, first, CELL, ov, n, ot, m)      # synchronises once, for the two counts
            med, lo, hi = timed(call, a.calls, a.warmup)
            s, n_out, m_out, _ = out["r"]
            assert s == abi.KT_OK
            nbytes = 16 * n + 16 * n_out + 12 * m + 12 * m_out
            bound = nbytes / (a.hbm_gbs * 1e9) * 1e3
            ratio = "" if weld_med is None else f"; {med / weld_med:.2f} x the weld"
            print(f"vertices {n} spans {a.spans} triangles {m} cell {CELL} m: kt_mesh_simplify_device median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}; {a.calls} calls "
                  f"after {a.warmup}); out {n_out} vertices ({n / max(n_out, 1):.1f} per cluster), {m_out} triangles; {nbytes / 1e6:.1f} MB to move, HBM bound "
                  f"{bound:.4f} ms at {a.hbm_gbs:.0f} GB/s: {med / bound:.0f} x the bound{ratio}", flush=True)
            for b in (dv, dt, ov, ot):
                b.free()
        for members in ([] if a.no_quadric else a.members):
            v, tri, first = slab_mesh(n, a.spans, members, local=a.quadric_local, in_order=True)
            both_forms(ctx, ws, timed, a, v, tri, first, CELL, f"spans {a.spans}, about {members:g} per cell")
    if a.single and not a.no_quadric:
        both_forms(ctx, ws, timed, a, *single_cluster(a.single), 0.5, "one cluster")
    w.close()
    ws.close()
    ctx.close()


if __name__ == "__main__":
    main()
