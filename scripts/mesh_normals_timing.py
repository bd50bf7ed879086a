#!/usr/bin/env python3
"""Time of the vertex normals (kt_mesh_normals_device) beside the seam weld's at the same vertex count in the same run: the
wall clock around the synchronous call, the median of --calls after --warmup.  The mesh is extracted on the device (kt_extract_mesh) from a
512^3 volume of spheres of radius 58 voxels on a lattice of period 128 (about 63000 vertices a sphere, two triangles per vertex; a voxel of
1 cm); the box that is meshed is grown along z, then y, then x until it holds about the wanted number of vertices.  Every size is timed
twice: with the triangles as the mesher leaves them (cell order) and with the triangle list shuffled, the worst case for locality and the
best for contention.  The bytes the pass must move: 16 B per vertex and 12 B per triangle in, 12 B per vertex out, 24 B per vertex of sums
zeroed and 24 B read back; the HBM time that implies stands beside the measurement (the atomics come on top: up to 72 B of added words per
triangle).  The weld runs on mesh_weld_timing.py's input of the same n.

    python scripts/mesh_normals_timing.py [--calls 20] [--warmup 3] [--vertices 100000 1000000 4000000] [--spans 8] [--hbm-gbs 8000] [--dump DIR]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
N, PERIOD, RADIUS, VOXEL = 512, 128, 58.0, 0.01


def spheres_volume():
    """int16 [N, N, N]: the distance to the nearest lattice centre minus the radius, in voxels, truncated at 8 voxels"""
    z, y, x = np.mgrid[0:PERIOD, 0:PERIOD, 0:PERIOD].astype(np.float32)
    c = np.float32(PERIOD / 2 - 0.3)
    r = np.sqrt((x - c) ** 2 + (y - c - np.float32(0.2)) ** 2 + (z - c + np.float32(0.15)) ** 2) - np.float32(RADIUS)
    tile = np.clip(np.round(r / 8.0 * 32767), -32767, 32767).astype(np.int16)
    k = N // PERIOD
    return np.ascontiguousarray(np.tile(tile, (k, k, k)))


def box_for(n):
    """the cells [0, hi) that hold about n vertices: whole spheres first, the last layer cut"""
    per = 6.0 * np.pi * RADIUS ** 2                       # vertices of one sphere, about
    want, k = n / per, N // PERIOD
    hi = [N - 1, N - 1, N - 1]
    if want < k:
        hi = [PERIOD, PERIOD, int(min(max(want, 0.25) * PERIOD, N - 1))]
    elif want < k * k:
        hi = [PERIOD, int(min(want / k * PERIOD, N - 1)), N - 1]
    elif want < k * k * k:
        hi = [int(min(want / (k * k) * PERIOD, N - 1)), N - 1, N - 1]
    return (0, 0, 0), tuple(hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vertices", type=int, nargs="+", default=[100000, 1000000, 4000000])
    ap.add_argument("--spans", type=int, default=8, help="of the weld's input")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the bound is computed from, GB/s")
    ap.add_argument("--no-weld", action="store_true", help="leave the weld out (for a kernel trace of the normals alone)")
    ap.add_argument("--dump", default="", help="a directory: the normals of every timed mesh go there as .npy, for comparing two builds")
    a = ap.parse_args()
    from kintinuous_amd import abi
    from mesh_weld_timing import slabs, timed
    ctx = abi.Ctx(0)
    w, wn = abi.MeshWeld(ctx), abi.MeshNormals(ctx)
    dvol = ctx.upload(spheres_volume())
    dcol = ctx.empty(4 * N ** 3)
    abi._chk(abi.lib().kt_memset(ctx.h, dcol.ptr, 1, 4 * N ** 3))      # every voxel observed (weight 1), one grey
    size = (N * VOXEL,) * 3
    rng = np.random.default_rng(1)
    for want in a.vertices:
        lo, hi = box_for(want)
        s, n, m = ctx.extract_mesh(dvol, size, (0, 0, 0), dcol, lo, hi, (0, 0, 0), N)
        dv, dt, on = ctx.empty(16 * n), ctx.empty(12 * m), ctx.empty(12 * n)
        s, n2, m2 = ctx.extract_mesh(dvol, size, (0, 0, 0), dcol, lo, hi, (0, 0, 0), N, dv, n, dt, m)
        assert s == abi.KT_OK and (n2, m2) == (n, m)
        weld_med = None
        if not a.no_weld:
            v, keys, tri, first, times = slabs(n, a.spans, 0.03)
            bufs = [ctx.upload(v), ctx.upload(keys), ctx.upload(tri), ctx.empty(16 * n), ctx.empty(8 * n)]
            weld_med, wlo, whi = timed(lambda: w.weld_device(bufs[0], bufs[1], n, bufs[2], len(tri), first, times, abi.NO_GATE, bufs[3], bufs[4], n), a.calls, a.warmup)
            print(f"vertices {n} spans {a.spans} triangles {len(tri)}: kt_mesh_weld_device median {weld_med:.3f} ms (min {wlo:.3f}, max {whi:.3f})", flush=True)
            for b in bufs:
                b.free()
        nbytes = 16 * n + 12 * m + 12 * n + 24 * n + 24 * n
        bound = nbytes / (a.hbm_gbs * 1e9) * 1e3
        for order in ("cell order", "shuffled"):
            if order == "shuffled":
                tri = ctx.download(dt, np.uint32, (m, 3))
                ctx.upload(tri[rng.permutation(m)], dt)
            out = {}

            def call():
                out["r"] = wn.normals_device(dv, n, dt, m, on)          # synchronises once, for the status and the zero normals
            med, tlo, thi = timed(call, a.calls, a.warmup)
            s, n_zero = out["r"]
            assert s == abi.KT_OK
            got = ctx.download(on, np.uint32, (n, 3))
            if a.dump:
                os.makedirs(a.dump, exist_ok=True)
                np.save(os.path.join(a.dump, "normals_%d_%s.npy" % (want, order.split()[0])), got)
            ratio = "" if weld_med is None else f"; {med / weld_med:.2f} x the weld"
            print(f"vertices {n} triangles {m} ({order}): kt_mesh_normals_device median {med:.3f} ms (min {tlo:.3f}, max {thi:.3f}; {a.calls} calls after "
                  f"{a.warmup}); {n_zero} zero normals, checksum {int(got.astype(np.uint64).sum()) & 0xffffffff:08x}; {nbytes / 1e6:.1f} MB to move, HBM bound "
                  f"{bound:.4f} ms at {a.hbm_gbs:.0f} GB/s: {med / bound:.0f} x the bound{ratio}", flush=True)
        for b in (dv, dt, on):
            b.free()
    w.close()
    wn.close()
    dvol.free()
    dcol.free()
    ctx.close()


if __name__ == "__main__":
    main()
