"""Meshes in spans for the fused mesh pass of the deformation graph (kt_deform_apply_mesh[_device], df_apply_mesh):
tests/test_deform_mesh_ref.py, tests/test_gpu_deform_mesh.py.

The graphs and the restated optimised states are deform_cases': M = 5 (the window is all nodes, the fifth nearest is the farthest), 20, 21
(the first size at which the window cuts a node off), 257, and `octa` (M = 6: five nodes at distance 1 from the origin, pairs of nodes at
equal float distance).  Two span tables per graph:
  mixed     spans of 0, 1, 255, 256 and 257 vertices -- below, at and above the workgroup's 256 lanes -- with empty spans first, in the middle
            and last.  The nine spans that hold vertices carry the nine times of span_times(): before the first node, after the last, on a
            node, exactly midway between two nodes (the tie goes to the lower index), and times whose nearest node is within 19 of either
            end, where the window is clipped (found = 18, 19, 20 from the front, M - 19 and M - 2 from the back).
  one4099   ONE span of 4099 vertices (17 workgroups, the last with three lanes at work) at a midway time.
Vertices are random finite positions within 1.5 m of the path; the first vertex of every span of three or more sits on the span's nearest
node (d = 0); on `octa` the second sits at the origin (five equidistant nodes: every weight 0.25); the rgb words start with 0, 0xffffffff,
0x7fc00001 (a quiet NaN with a payload) and 0xff800000 (-inf) and go on at random: any float a uint32 may look like.
"""
from __future__ import annotations

import functools

import numpy as np

import deform_cases as dc

GRAPHS = ["m5_n1_c3", "m20_n64_c7", "m21_n65_c300", "m257_n4099_c300", "octa"]
TABLES = ["mixed", "one4099"]
NAMES = [g + "-" + t for g in GRAPHS for t in TABLES]
SMALL, LARGE = "m5_n1_c3-mixed", "m257_n4099_c300-one4099"      # a large call after a small one on the same object
MIXED_SIZES = [0, 0, 1, 255, 256, 0, 257, 1, 255, 256, 257, 1, 0]
RGB_EDGES = [0x00000000, 0xffffffff, 0x7fc00001, 0xff800000]


def span_times(M):
    """nine times for a graph of M nodes at T0 + DT i (clipped to the graph where it is shorter than the edge asks)"""
    T0, DT, k = dc.T0, dc.DT, M // 2
    return [T0 - 5000,                               # before the first node
            T0 + DT * (M - 1) + 7000,                # after the last
            T0 + DT * k,                             # a node's time
            T0 + DT * k + DT // 2,                   # the exact midpoint of nodes k and k + 1: node k
            T0 + DT * min(18, M - 1) + 3,            # found = 18: the window starts at node 0 with a node to spare
            T0 + DT * min(19, M - 1),                # found = 19: the last size of window that starts at node 0
            T0 + DT * min(20, M - 1) - 1,            # found = 20: node 0 is cut off
            T0 + DT * max(M - 19, 0) + 5,            # within 19 of the end
            T0 + DT * max(M - 2, 0)]


def nearest_node(node_time, t):
    """the restated `found` of a time, written apart from deform_ref.weights: Python integers, a tie to the lower index"""
    return min(range(len(node_time)), key=lambda i: (abs(int(node_time[i]) - int(t)), i))


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: graph (a deform_cases name), vertices (n,) MESH_VERTEX_DTYPE, span_first (S + 1,) uintp, span_time (S,) uint64, extent --
    read-only arrays"""
    from kintinuous_amd import abi
    gname, table = name.split("-")
    c = dc.case(gname)
    M = len(c["node_time"])
    rng = np.random.default_rng(7000 + NAMES.index(name))
    if table == "mixed":
        sizes, pool = MIXED_SIZES, iter(span_times(M))
        times = [next(pool) if s else dc.T0 for s in sizes]
    else:
        sizes, times = [4099], [dc.T0 + dc.DT * (M // 2) + dc.DT // 2]
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uintp)
    n = int(first[-1])
    v = np.zeros(n, dtype=abi.MESH_VERTEX_DTYPE)
    v["rgb"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for s, (size, t) in enumerate(zip(sizes, times)):
        lo = int(first[s])
        k = nearest_node(c["node_time"], t)
        if gname == "octa":
            xyz = rng.uniform(-2.0, 2.0, (size, 3))
        else:
            off = rng.standard_normal((size, 3))
            off *= (rng.uniform(0.05, 1.5, size) / np.linalg.norm(off, axis=1))[:, None]
            xyz = dc.curve(k + rng.uniform(-3.0, 3.0, size)) + off
        v["xyz"][lo:lo + size] = xyz.astype(np.float32)
        if size >= 3:
            v["xyz"][lo] = c["node_pos"][k]                         # on a node
            if gname == "octa":
                v["xyz"][lo + 1] = 0.0                              # five nodes at distance 1
        if size >= 255:
            v["rgb"][lo + 2:lo + 2 + len(RGB_EDGES)] = RGB_EDGES
    out = {"graph": gname, "vertices": v, "span_first": first, "span_time": np.array(times, dtype=np.uint64), "extent": c["extent"]}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def expanded_times(c):
    return np.repeat(c["span_time"], np.diff(c["span_first"].astype(np.int64)))


def as_points(vertices):
    """the vertices as 48-byte points: today's route through kt_deform_weights_device + kt_deform_apply_device"""
    from kintinuous_amd import abi
    pts = np.zeros(len(vertices), dtype=abi.NPOINT_DTYPE)
    pts["xyz"] = vertices["xyz"]
    pts["one"] = 1.0
    pts["normal"] = [0.0, 0.0, 1.0]
    return pts


@functools.lru_cache(maxsize=None)
def restated(name):
    """deform_ref.apply_mesh of a case with the graph's restated optimised state, computed once per process"""
    from kintinuous_amd import deform_ref as ref
    c = case(name)
    out = ref.apply_mesh(dc.graph(c["graph"]), dc.restated(c["graph"])[0], c["vertices"], c["span_first"], c["span_time"])
    out.setflags(write=False)
    return out


# ---- the driver's files ------------------------------------------------------------------------------------------------------------------
def mesh_line(utime, vertices):
    """a `mesh` line of <prefix>.deform as the driver prints it"""
    return "mesh %d %d" % (utime, vertices)


def deform_file(text):
    """<prefix>.deform: pose / node / con lines (a time, then hex floats), slice and mesh lines (a time and a count), the result line"""
    out = {"pose": [], "node": [], "con": [], "slice": [], "mesh": [], "result": None}
    for line in text.splitlines():
        f = line.split()
        if f[0] == "result":
            out["result"] = (int(f[1]), int(f[2]), f[3], int(f[4])) + tuple(float.fromhex(v) for v in f[5:8])
        elif f[0] in ("slice", "mesh"):
            assert len(f) == 3
            out[f[0]].append((int(f[1]), int(f[2])))
        else:
            out[f[0]].append((int(f[1]),) + tuple(float.fromhex(v) for v in f[2:]))
    return out


PLY_VERTEX = np.dtype([("xyz", "<f4", 3), ("rgb", np.uint8, 3)])
PLY_FACE = np.dtype([("n", np.uint8), ("idx", "<i4", 3)])


def read_ply(path):
    """the binary PLY of kt_host_save_ply: (vertices PLY_VERTEX, faces (n, 3) int32)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int([l for l in head if l.startswith("element vertex ")][0].split()[2])
    nf = int([l for l in head if l.startswith("element face ")][0].split()[2])
    assert [l for l in head if l.startswith("property ")] == ["property float x", "property float y", "property float z", "property uchar red",
                                                              "property uchar green", "property uchar blue", "property list uchar int vertex_indices"]
    assert len(raw) == end + PLY_VERTEX.itemsize * nv + PLY_FACE.itemsize * nf
    v = np.frombuffer(raw, PLY_VERTEX, nv, end)
    f = np.frombuffer(raw, PLY_FACE, nf, end + PLY_VERTEX.itemsize * nv)
    assert (f["n"] == 3).all()
    return v, f["idx"]
