#!/usr/bin/env python3
"""Time of the connected-component filter (kt_mesh_components_device) beside the seam weld's and the normals' on the same
mesh in the same run: the wall clock around the synchronous call (each enqueues its passes and waits once), the median of --calls after
--warmup.  Two meshes: the welded mesh of the suite's out-and-back crab-walk (N = 96, 160 x 120, 40 frames, a 5.2 m volume, shift
threshold 3), tracked and meshed here with the tracker's mesh stage and keys, and tests/mesh_components_cases.random_case(2, 70001).  The
weld is timed on the crab-walk's collected mesh (what it is given in the driver), the filter and the normals on the welded one.  The CPU
column is the suite's independent check (scipy's connected components, np.minimum.at, np.bincount, masks) and the numpy restatement.

    python scripts/mesh_components_timing.py [--calls 200] [--warmup 20] [--min-triangles 40] [--mesh both|crab|random]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def crab_walk(ctx):
    """(vertices, keys, triangles, span_first, span_time) of the crab-walk's collected mesh"""
    from kintinuous_amd import abi, synth
    cam = synth.Camera.small(160, 120)
    traj = synth.crabwalk_trajectory(420)
    frames = [synth.render(synth.Scene("wall"), cam, *traj[i]) for i in list(range(0, 40, 2)) + list(range(40, 0, -2))]
    cfg = abi.TrackerConfig(cam.cols, cam.rows, 96, cam.fx, cam.fy, cam.cx, cam.cy, 5.2, 3, 2, 0, 0, 0, 0, 0, 0)
    trk = abi.Tracker(ctx, cfg)
    try:
        trk.enable_mesh_keys(True)
        trk.enable_mesh_stage(True)
        for k, (d, rgb) in enumerate(frames):
            trk.process_frame_host(d, rgb, 33333 * k)
        trk.finalise()
        ns = trk.num_slices()
        meshes = [trk.slice_mesh(i) for i in range(ns)]
        keys = [trk.slice_mesh_keys(i) for i in range(ns)]
        times = [trk.slice_pose(i)[2] for i in range(ns)]
    finally:
        trk.close()
    first = np.concatenate([[0], np.cumsum([len(m[0]) for m in meshes])]).astype(np.int64)
    tri = np.concatenate([m[1] + np.uint32(first[i]) for i, m in enumerate(meshes)]).astype(np.uint32)
    return np.concatenate([m[0] for m in meshes]), np.concatenate(keys), tri, first, np.array(times, np.uint64)


def cpu_timed(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--min-triangles", type=int, default=40)
    ap.add_argument("--mesh", choices=("both", "crab", "random"), default="both", help="one mesh alone: for a kernel trace")
    a = ap.parse_args()
    import mesh_components_cases as cases
    from kintinuous_amd import abi, mesh_components_ref as ref
    from mesh_weld_timing import timed
    ctx = abi.Ctx(0)
    welder, comp, nrm = abi.MeshWeld(ctx), abi.MeshComponents(ctx), abi.MeshNormals(ctx)
    k = a.min_triangles
    v, keys, tri, first, times = crab_walk(ctx)
    wv, _, wt, wf = welder.weld(v, keys, tri, first, times)
    meshes = [("crab-walk, welded", wv, wt, wf, (v, keys, tri, first, times)), ("random_case(2, 70001)",) + cases.random_case(2, 70001) + (None,)]
    meshes = [x for x, tag in zip(meshes, ("crab", "random")) if a.mesh in ("both", tag)]
    for name, mv, mt, mf, unwelded in meshes:
        n, m = len(mv), len(mt)
        want = ref.components(mv, mt, mf, k)
        dv, dt = ctx.upload(mv), ctx.upload(mt)
        ov, ot, ol, on = ctx.empty(16 * n), ctx.empty(12 * max(m, 1)), ctx.empty(4 * n), ctx.empty(12 * n)
        out = {}

        def call():
            out["r"] = comp.components_device(dv, n, dt, m, mf, k, ov, n, ot, m, ol)
        med, lo, hi = timed(call, a.calls, a.warmup)
        s, n_out, m_out, fo, stats = out["r"]
        assert s == abi.KT_OK and stats == want[4] and (n_out, m_out) == (len(want[0]), len(want[1])) and np.array_equal(ctx.download(ol, np.uint32, (n,)), want[3])
        print(f"{name}: {n} vertices, {m} triangles, {len(mf) - 1} spans; min_triangles {k}: {stats[0]} components, {stats[1]} kept, the largest of {stats[2]}; "
              f"{n_out} vertices and {m_out} triangles kept", flush=True)
        print(f"  kt_mesh_components_device median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}; {a.calls} calls after {a.warmup})", flush=True)
        if nrm.normals_device(dv, n, dt, m, on)[0] == abi.KT_OK:   # (the random case's vertices are any 16 bytes: no positions to take normals of)
            nmed, nlo, nhi = timed(lambda: nrm.normals_device(dv, n, dt, m, on), a.calls, a.warmup)
            print(f"  kt_mesh_normals_device median {nmed:.4f} ms (min {nlo:.4f}, max {nhi:.4f}) on the same mesh: the filter takes {med / nmed:.2f} x", flush=True)
        if unwelded is not None:
            uv, uk, ut, uf, utm = unwelded
            bufs = [ctx.upload(uv), ctx.upload(uk), ctx.upload(ut), ctx.empty(16 * len(uv)), ctx.empty(8 * len(uv))]

            def weld_call():
                ctx.upload(ut, bufs[2])                     # the weld remaps the triangles in place: every call starts from the collected list
                return welder.weld_device(bufs[0], bufs[1], len(uv), bufs[2], len(ut), uf, utm, abi.NO_GATE, bufs[3], bufs[4], len(uv))
            upl, _, _ = timed(lambda: ctx.upload(ut, bufs[2]), a.calls, a.warmup)
            wmed, wlo, whi = timed(weld_call, a.calls, a.warmup)
            print(f"  kt_mesh_weld_device on the collected mesh ({len(uv)} vertices) median {wmed - upl:.4f} ms (min {wlo - upl:.4f}, max {whi - upl:.4f}; the "
                  f"{upl:.4f} ms upload of the triangles taken off): the filter takes {med / (wmed - upl):.2f} x", flush=True)
            for b in bufs:
                b.free()
        chk = cpu_timed(lambda: cases.check(mv, mt, mf, k), 10)
        rst = cpu_timed(lambda: ref.components(mv, mt, mf, k), 10)
        print(f"  on the CPU: the scipy check median {chk:.3f} ms, the numpy restatement {rst:.3f} ms (10 calls each)", flush=True)
        for b in (dv, dt, ov, ot, ol, on):
            b.free()
    welder.close()
    comp.close()
    nrm.close()
    ctx.close()


if __name__ == "__main__":
    main()
