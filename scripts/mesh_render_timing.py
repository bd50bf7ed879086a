#!/usr/bin/env python3
"""Time of the rasteriser (kt_mesh_render_device) beside the ray cast's view of the same scene in the same run: the wall
clock around the synchronous call, the median of --calls after --warmup.  The meshes are mesh_normals_timing.py's: extracted on the device
(kt_extract_mesh) from a 512^3 volume of spheres of radius 58 voxels on a lattice of period 128 (a voxel of 1 cm), the meshed box grown
until it holds about the wanted number of vertices (along z first, then y, then x, from the corner of the volume).  The camera stands
inside the lattice, 11 cm inside the volume's z = 0 face at the corner the box grows from, midway between the first four columns of spheres,
and looks along +z down the channel between them, so that every size has something in view.  Every mesh is drawn at 640 x 480 and at
1280 x 960, all four planes wanted, as it is and with one triangle more that fills the image half a metre in front of the camera --
which ONE wave draws, in blocks of 8 x 8 pixels.  The yardstick is
kt_raycast followed by kt_generate_image of the volume the mesh came from, at the same pose, intrinsics and image size, waited for once.
The shares of the passes come from a kernel trace of this script (--no-others leaves the yardstick out).

    python scripts/mesh_render_timing.py [--calls 20] [--warmup 3] [--vertices 100000 1000000 4000000] [--no-others]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

IMAGES = ((640, 480), (1280, 960))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vertices", type=int, nargs="+", default=[100000, 1000000, 4000000])
    ap.add_argument("--no-others", action="store_true", help="leave the ray cast out (for a kernel trace of the rasteriser alone)")
    a = ap.parse_args()
    from kintinuous_amd import abi
    from mesh_normals_timing import N, VOXEL, box_for, spheres_volume
    from mesh_weld_timing import timed
    ctx = abi.Ctx(0)
    ren = abi.MeshRender(ctx)
    dvol = ctx.upload(spheres_volume())
    dcol = ctx.empty(4 * N ** 3)
    abi._chk(abi.lib().kt_memset(ctx.h, dcol.ptr, 1, 4 * N ** 3))      # every voxel observed (weight 1), one grey
    size = (N * VOXEL,) * 3
    R = np.eye(3, dtype=np.float32)
    t_mesh = np.array([-1.278, -1.278, -2.45], np.float32)              # the mesh is centred on the middle of the volume ...
    t_vol = (t_mesh.astype(np.float64) + N * VOXEL / 2).astype(np.float32)   # ... which the ray cast calls (size / 2,) * 3
    for cols, rows in IMAGES:
        intr = (cols * 0.82, cols * 0.82, cols / 2 - 0.5, rows / 2 - 0.5)
        pixels = cols * rows
        index, depth, color, model = ctx.empty(4 * pixels), ctx.empty(2 * pixels), ctx.empty(3 * pixels), ctx.empty(3 * pixels)
        if not a.no_others:
            vm, nm, cm, img, cimg = ctx.zeros(12 * pixels), ctx.zeros(12 * pixels), ctx.zeros(4 * pixels), ctx.zeros(3 * pixels), ctx.zeros(3 * pixels)

            def cast():
                ctx.raycast(abi.Intr(*intr), R, t_vol, 8 * VOXEL, size, dvol, vm, nm, cols, rows, [0, 0, 0], cm, dcol, N)
                ctx.generate_image(vm, nm, cm, cols, rows, t_vol, 1, img, cimg)
                ctx.sync()
            med, lo, hi = timed(cast, a.calls, a.warmup)
            hit = int((ctx.download(img, np.uint8, (rows, cols, 3)).max(axis=2) > 0).sum())
            print(f"{cols} x {rows}: kt_raycast + kt_generate_image median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {hit} of {pixels} pixels lit", flush=True)
            for b in (vm, nm, cm, img, cimg):
                b.free()
        for want in a.vertices:
            blo, bhi = box_for(want)
            s, n, m = ctx.extract_mesh(dvol, size, (0, 0, 0), dcol, blo, bhi, (0, 0, 0), N)
            dv, dt = ctx.empty(16 * (n + 3)), ctx.empty(12 * (m + 1))
            s, n2, m2 = ctx.extract_mesh(dvol, size, (0, 0, 0), dcol, blo, bhi, (0, 0, 0), N, dv, n, dt, m)
            assert s == abi.KT_OK and (n2, m2) == (n, m)
            # one triangle more, behind the mesh's own arrays: it covers the image 0.5 m in front of the camera
            big = np.zeros(3, abi.MESH_VERTEX_DTYPE)
            big["xyz"] = t_mesh + np.array([(-2.0, -1.5, 0.5), (4.0, -1.5, 0.5), (-2.0, 4.0, 0.5)], np.float32)
            big["rgb"] = (0xFF0000, 0x00FF00, 0x0000FF)
            abi._chk(abi.lib().kt_upload(ctx.h, dv.ptr + 16 * n, big.ctypes.data, 48))
            last = np.array([n, n + 1, n + 2], np.uint32)
            abi._chk(abi.lib().kt_upload(ctx.h, dt.ptr + 12 * m, last.ctypes.data, 12))
            out, t = {}, {}
            for extra in (0, 1):
                def call():
                    out[extra] = ren.render_device(dv, n + 3 * extra, dt, m + extra, intr, cols, rows, R, t_mesh, abi.MeshRender.NEAR, index, depth, color, model)
                t[extra] = timed(call, a.calls, a.warmup)
                assert out[extra][0] == abi.KT_OK
            checksum = int(ctx.download(depth, np.uint16, (pixels,)).astype(np.uint64).sum()) & 0xffffffff
            st0, st1 = out[0][1], out[1][1]
            print(f"{cols} x {rows}, vertices {n} triangles {m}: kt_mesh_render_device median {t[0][0]:.3f} ms (min {t[0][1]:.3f}, max {t[0][2]:.3f}; {a.calls} calls after "
                  f"{a.warmup}); drawn {st0[0]}, clipped {st0[1]}, degenerate {st0[2]}, covered {st0[3]} of {pixels}; with the image-filling triangle median {t[1][0]:.3f} ms "
                  f"(min {t[1][1]:.3f}, max {t[1][2]:.3f}), covered {st1[3]}: the triangle costs {t[1][0] - t[0][0]:.3f} ms; depth checksum {checksum:08x}", flush=True)
            for b in (dv, dt):
                b.free()
        for b in (index, depth, color, model):
            b.free()
    ren.close()
    dvol.free()
    dcol.free()
    ctx.close()


if __name__ == "__main__":
    main()
