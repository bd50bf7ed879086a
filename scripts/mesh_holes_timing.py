#!/usr/bin/env python3
"""Time of the boundary report and small-hole fill (kt_mesh_holes_device) beside the seam weld's and the component
filter's on the same mesh in the same run: the wall clock around the synchronous call (each enqueues its passes and waits once), the median
of --calls after --warmup.  Two meshes: the welded mesh of the suite's out-and-back crab-walk (mesh_components_timing.crab_walk), and
tests/mesh_holes_cases.random_case(2, 70000), the suite's 4099-triangle random patch at about 70000 triangles.  The weld is timed on the
crab-walk's collected mesh (what it is given in the driver), the other two on the welded one.  The CPU column is the numpy restatement.

    python scripts/mesh_holes_timing.py [--calls 200] [--warmup 20] [--max-edges 8] [--mesh both|crab|random]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--max-edges", type=int, default=8)
    ap.add_argument("--mesh", choices=("both", "crab", "random"), default="both", help="one mesh alone: for a kernel trace")
    a = ap.parse_args()
    import mesh_holes_cases as cases
    from kintinuous_amd import abi, mesh_holes_ref as ref
    from mesh_components_timing import cpu_timed, crab_walk
    from mesh_weld_timing import timed
    ctx = abi.Ctx(0)
    welder, comp, holes = abi.MeshWeld(ctx), abi.MeshComponents(ctx), abi.MeshHoles(ctx)
    k = a.max_edges
    v, keys, tri, first, times = crab_walk(ctx)
    wv, _, wt, wf = welder.weld(v, keys, tri, first, times)
    meshes = [("crab-walk, welded", wv, wt, wf, (v, keys, tri, first, times)), ("random_case(2, 70000)",) + cases.random_case(2, 70000) + (None,)]
    meshes = [x for x, tag in zip(meshes, ("crab", "random")) if a.mesh in ("both", tag)]
    for name, mv, mt, mf, unwelded in meshes:
        n, m = len(mv), len(mt)
        want = ref.holes(mv, mt, mf, k)
        vcap, tcap = abi.MeshHoles.most(n, m)
        dv, dt = ctx.upload(mv), ctx.upload(mt)
        ov, ot, ol = ctx.empty(16 * vcap), ctx.empty(12 * max(tcap, 1)), ctx.empty(4 * n)
        out = {}

        def call():
            out["r"] = holes.holes_device(dv, n, dt, m, mf, k, ov, vcap, ot, tcap, ol)
        med, lo, hi = timed(call, a.calls, a.warmup)
        s, n_out, m_out, fo, stats = out["r"]
        assert s == abi.KT_OK and stats == want[4] and (n_out, m_out) == (len(want[0]), len(want[1])) and np.array_equal(ctx.download(ol, np.uint32, (n,)), want[3])
        assert np.array_equal(ctx.download(ot, np.uint32, (m_out, 3)), want[1]) and ctx.download(ov, abi.MESH_VERTEX_DTYPE, (n_out,)).tobytes() == want[0].tobytes()
        loops = want[3][want[3] < ref.OPEN]
        lengths = np.sort(np.bincount(loops)[np.unique(loops)]) if len(loops) else np.zeros(0, np.int64)
        print(f"{name}: {n} vertices, {m} triangles, {len(mf) - 1} spans; max_edges {k}: " + ", ".join(f"{nm} {x}" for nm, x in zip(ref.STAT_NAMES, stats)), flush=True)
        print(f"  the simple loops' lengths: {lengths[:12].tolist()}{' ...' if len(lengths) > 12 else ''} {lengths[-3:].tolist() if len(lengths) > 12 else ''}", flush=True)
        print(f"  kt_mesh_holes_device median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}; {a.calls} calls after {a.warmup})", flush=True)
        cv, ct, cl = ctx.empty(16 * n), ctx.empty(12 * max(m, 1)), ctx.empty(4 * n)
        cmed, clo, chi = timed(lambda: comp.components_device(dv, n, dt, m, mf, 40, cv, n, ct, m, cl), a.calls, a.warmup)
        print(f"  kt_mesh_components_device (min_triangles 40) median {cmed:.4f} ms (min {clo:.4f}, max {chi:.4f}) on the same mesh: the hole pass takes {med / cmed:.2f} x", flush=True)
        if unwelded is not None:
            uv, uk, ut, uf, utm = unwelded
            bufs = [ctx.upload(uv), ctx.upload(uk), ctx.upload(ut), ctx.empty(16 * len(uv)), ctx.empty(8 * len(uv))]

            def weld_call():
                ctx.upload(ut, bufs[2])                     # the weld remaps the triangles in place: every call starts from the collected list
                return welder.weld_device(bufs[0], bufs[1], len(uv), bufs[2], len(ut), uf, utm, abi.NO_GATE, bufs[3], bufs[4], len(uv))
            upl, _, _ = timed(lambda: ctx.upload(ut, bufs[2]), a.calls, a.warmup)
            wmed, wlo, whi = timed(weld_call, a.calls, a.warmup)
            print(f"  kt_mesh_weld_device on the collected mesh ({len(uv)} vertices) median {wmed - upl:.4f} ms (min {wlo - upl:.4f}, max {whi - upl:.4f}; the "
                  f"{upl:.4f} ms upload of the triangles taken off): the hole pass takes {med / (wmed - upl):.2f} x", flush=True)
            for b in bufs:
                b.free()
        rst = cpu_timed(lambda: ref.holes(mv, mt, mf, k), 10)
        print(f"  on the CPU: the numpy restatement median {rst:.3f} ms (10 calls)", flush=True)
        for b in (dv, dt, ov, ot, ol, cv, ct, cl):
            b.free()
    welder.close()
    comp.close()
    holes.close()
    ctx.close()


if __name__ == "__main__":
    main()
