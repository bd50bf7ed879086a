#!/usr/bin/env python3
"""Time of the smoothing pass (kt_mesh_smooth_device) beside the vertex normals' and the seam weld's at the same vertex count
in the same run: the wall clock around the synchronous call, the median of --calls after --warmup.  The meshes are
mesh_normals_timing.py's: extracted on the device (kt_extract_mesh) from a 512^3 volume of spheres of radius 58 voxels on a lattice of
period 128, the meshed box grown until it holds about the wanted number of vertices; every size is timed with the triangles as the mesher
leaves them (cell order) and with the triangle list shuffled.  The call is timed at steps = 0 (the adjacency build, the init and the finish
pass) and at steps = --steps; the difference over 2 * steps is one half-step.  The bytes a half-step must move: 24 B per vertex read and
24 B written, 8 B per vertex of degree and row offset, 4 B per neighbour entry; the gathered 24 B per neighbour entry come on top where the
caches do not hold them.  The HBM times of both sums stand beside the measurement.  The weld runs on mesh_weld_timing.py's input of the
same n.

    python scripts/mesh_smooth_timing.py [--calls 20] [--warmup 3] [--steps 10] [--vertices 100000 1000000 4000000] [--spans 8] [--hbm-gbs 8000]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--vertices", type=int, nargs="+", default=[100000, 1000000, 4000000])
    ap.add_argument("--spans", type=int, default=8, help="of the weld's input")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the bounds are computed from, GB/s")
    ap.add_argument("--no-others", action="store_true", help="leave the weld and the normals out (for a kernel trace of the smoothing alone)")
    a = ap.parse_args()
    from kintinuous_amd import abi
    from mesh_normals_timing import N, VOXEL, box_for, spheres_volume
    from mesh_weld_timing import slabs, timed
    ctx = abi.Ctx(0)
    w, wn, ws = abi.MeshWeld(ctx), abi.MeshNormals(ctx), abi.MeshSmooth(ctx)
    dvol = ctx.upload(spheres_volume())
    dcol = ctx.empty(4 * N ** 3)
    abi._chk(abi.lib().kt_memset(ctx.h, dcol.ptr, 1, 4 * N ** 3))      # every voxel observed (weight 1), one grey
    size = (N * VOXEL,) * 3
    rng = np.random.default_rng(1)
    lam, mu = abi.MeshSmooth.LAMBDA, abi.MeshSmooth.MU
    for want in a.vertices:
        lo, hi = box_for(want)
        s, n, m = ctx.extract_mesh(dvol, size, (0, 0, 0), dcol, lo, hi, (0, 0, 0), N)
        dv, dt, on, do = ctx.empty(16 * n), ctx.empty(12 * m), ctx.empty(12 * n), ctx.empty(16 * n)
        s, n2, m2 = ctx.extract_mesh(dvol, size, (0, 0, 0), dcol, lo, hi, (0, 0, 0), N, dv, n, dt, m)
        assert s == abi.KT_OK and (n2, m2) == (n, m)
        if not a.no_others:
            v, keys, tri, first, times = slabs(n, a.spans, 0.03)
            bufs = [ctx.upload(v), ctx.upload(keys), ctx.upload(tri), ctx.empty(16 * n), ctx.empty(8 * n)]
            weld_med, wlo, whi = timed(lambda: w.weld_device(bufs[0], bufs[1], n, bufs[2], len(tri), first, times, abi.NO_GATE, bufs[3], bufs[4], n), a.calls, a.warmup)
            print(f"vertices {n} spans {a.spans} triangles {len(tri)}: kt_mesh_weld_device median {weld_med:.3f} ms (min {wlo:.3f}, max {whi:.3f})", flush=True)
            for b in bufs:
                b.free()
        for order in ("cell order", "shuffled"):
            if order == "shuffled":
                tri = ctx.download(dt, np.uint32, (m, 3))
                ctx.upload(tri[rng.permutation(m)], dt)
            if not a.no_others:
                med, tlo, thi = timed(lambda: wn.normals_device(dv, n, dt, m, on), a.calls, a.warmup)
                print(f"vertices {n} triangles {m} ({order}): kt_mesh_normals_device median {med:.3f} ms (min {tlo:.3f}, max {thi:.3f})", flush=True)
            out = {}
            t = {}
            for steps in (0, a.steps):
                def call():
                    out["r"] = ws.smooth_device(dv, n, dt, m, steps, lam, mu, 0, do)     # synchronises once, for the four result words
                t[steps] = timed(call, a.calls, a.warmup)
                assert out["r"][0] == abi.KT_OK
            rim, moved, edges = out["r"][1]
            got = ctx.download(do, np.uint32, (n, 4))
            entries = 2 * edges                                                         # at most: a pinned rim vertex has none
            must = 24 * n + 24 * n + 8 * n + 4 * entries
            gathered = must + 24 * entries
            half = (t[a.steps][0] - t[0][0]) / (2 * a.steps)
            b0, b1 = must / (a.hbm_gbs * 1e9) * 1e3, gathered / (a.hbm_gbs * 1e9) * 1e3
            print(f"vertices {n} triangles {m} ({order}): kt_mesh_smooth_device steps 0 median {t[0][0]:.3f} ms (min {t[0][1]:.3f}, max {t[0][2]:.3f}), steps {a.steps} median "
                  f"{t[a.steps][0]:.3f} ms (min {t[a.steps][1]:.3f}, max {t[a.steps][2]:.3f}; {a.calls} calls after {a.warmup}); a half-step {half:.4f} ms; {rim} rim vertices, "
                  f"{moved} moved, {edges} edges, checksum {int(got.astype(np.uint64).sum()) & 0xffffffff:08x}; a half-step must move {must / 1e6:.1f} MB, HBM bound "
                  f"{b0:.4f} ms at {a.hbm_gbs:.0f} GB/s: {half / b0:.1f} x; with every gather from memory {gathered / 1e6:.1f} MB, {b1:.4f} ms: {half / b1:.1f} x", flush=True)
        for b in (dv, dt, on, do):
            b.free()
    w.close()
    wn.close()
    ws.close()
    dvol.free()
    dcol.free()
    ctx.close()


if __name__ == "__main__":
    main()
