"""Synthetic maps for the deformation-graph stage (tests/test_deform_ref.py, tests/test_gpu_deform.py).

A case is a drifting trajectory (a slowly widening spiral with a vertical wobble, nodes about 0.8 m apart, 0.4 s between them), the corrected
one (a rotation about z and a shift that both grow along the path, up to 0.1 rad and 0.4 m: what a pose graph hands back), a point cloud
within 1.5 m of the path with times, normals, colours and padding, and constraints original -> corrected on the path.  Everything comes from
a seeded generator.  The first points of a cloud carry the edges: a time before the first node, after the last, equal to a node's, at the
exact midpoint of two nodes; a point on a node; a zero and a NaN normal.  The case `octa` is a crafted graph: five nodes at distance 1 from
the origin (the 0.25 rule, and the tie rule on which four of them are taken) and pairs of nodes at equal float distance from a point.
"""
from __future__ import annotations

import functools

import numpy as np

T0, DT = 1_000_000, 400_000          # microseconds: midpoints of two nodes are whole numbers


def curve(u):
    """the drifting path at node parameter u (node i sits at u = i)"""
    th = 0.27 * np.asarray(u, dtype=np.float64)
    r = 3.0 + 0.05 * th
    return np.stack([r * np.cos(th), r * np.sin(th), 0.3 * np.sin(3.0 * th)], -1)


def corrected(p, s):
    """the point p of the drifted map at path fraction s in [0, 1] where the corrected trajectory puts it"""
    p, s = np.asarray(p, dtype=np.float64), np.asarray(s, dtype=np.float64)
    a = 0.1 * s
    c, sn = np.cos(a), np.sin(a)
    q = np.stack([c * p[..., 0] - sn * p[..., 1], sn * p[..., 0] + c * p[..., 1], p[..., 2]], -1)
    return q + s[..., None] * np.array([0.3, -0.2, 0.1])


# name, nodes, points, constraints
_SPECS = [
    ("m5_n0_c1", 5, 0, 1),          # one constraint: see case()
    ("m5_n1_c3", 5, 1, 3),          # the fewest constraints that determine a deformation
    ("m6_n1_c7", 6, 1, 7),
    ("m19_n63_c7", 19, 63, 7),
    ("m20_n64_c7", 20, 64, 7),
    ("m21_n65_c300", 21, 65, 300),
    ("m25_n4099_c300", 25, 4099, 300),
    ("m64_n65_c7", 64, 65, 7),
    ("m65_n63_c300", 65, 63, 300),
    ("m257_n4099_c300", 257, 4099, 300),
    ("octa", 6, 9, 7),
]
_SEEDS = {}
NAMES = [s[0] for s in _SPECS]
SMALL, LARGE = "m19_n63_c7", "m65_n63_c300"          # a large call after a small one on the same object


def _points(rng, n):
    from kintinuous_amd import abi
    pts = np.zeros(n, dtype=abi.NPOINT_DTYPE)
    nrm = rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True) if n else 1.0
    pts["one"] = 1.0
    pts["normal"] = nrm.astype(np.float32)
    pts["zero"] = rng.standard_normal(n).astype(np.float32)            # padding carries values: the stage must leave them alone
    pts["bgra"] = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    pts["curvature"] = rng.random(n, dtype=np.float32)
    pts["pad"] = rng.standard_normal((n, 2)).astype(np.float32)
    return pts


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: node_pos (M, 3) f32, node_time (M,) u64, points (n,) NPOINT_DTYPE, times (n,) u64, src (L, 3) f32, src_time (L,) u64,
    target (L, 3) f64, extent -- read-only arrays"""
    idx = NAMES.index(name)
    _, M, n, L = _SPECS[idx]
    rng = np.random.default_rng(_SEEDS.get(name, 4000 + idx))
    node_time = (T0 + DT * np.arange(M)).astype(np.uint64)
    pts = _points(rng, n)
    if name == "octa":
        node_pos = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, -3]], dtype=np.float32)
        pts["xyz"] = np.array([[0, 0, 0],            # five nodes at distance 1: every weight 0.25, nodes 0..3 by the tie rule
                               [0.5, 0.5, 0],        # nodes 0 and 1 at equal float distance, and 2 and 3
                               [0.5, -0.5, 0.25],
                               [1, 0, 0],            # on node 0
                               [0, 0, -3],           # on node 5
                               [0.25, 0, 0], [0, 0, 0.5], [-0.5, 0.5, -0.5], [2, 2, 2]], dtype=np.float32)
        times = np.array([T0 + 2 * DT, T0, T0 + 5 * DT, T0 - 1, T0 + 9 * DT, T0 + DT // 2, T0 + 3 * DT + DT // 2, T0 + 4 * DT + 1, T0 + 2 * DT - 1], dtype=np.uint64)
        su = rng.uniform(0.0, M - 1.0, L)
        src = (node_pos[np.round(su).astype(int)] + 0.3 * rng.standard_normal((L, 3))).astype(np.float32)
        src_time = np.round(T0 + DT * su).astype(np.uint64)
        target = corrected(src.astype(np.float64), su / (M - 1.0))
    else:
        node_pos = curve(np.arange(M)).astype(np.float32)
        u = rng.uniform(-0.5, M - 0.5, n)
        off = rng.standard_normal((n, 3))
        off *= (rng.uniform(0.05, 1.5, n) / np.linalg.norm(off, axis=1))[:, None] if n else 1.0
        pts["xyz"] = (curve(u) + off).astype(np.float32)
        times = np.round(T0 + DT * u).astype(np.int64)
        k = M // 2
        if n == 1:
            times[0] = T0 + DT * k + DT // 2                               # the exact midpoint of nodes k and k + 1
        if n >= 63:
            times[0] = T0 - 5000                                           # before the first node
            times[1] = T0 + DT * (M - 1) + 7000                            # after the last
            times[2] = T0 + DT * k                                         # a node's time
            times[3] = T0 + DT * k + DT // 2                               # the exact midpoint
            pts["xyz"][4] = node_pos[k]; times[4] = T0 + DT * k            # on a node
            pts["normal"][5] = 0.0                                         # a zero normal stays
            pts["normal"][6] = [np.nan, 0.0, 1.0]                          # a NaN normal stays
        times = times.astype(np.uint64)
        # constraints on the path, the last one at its end, where the drift is largest
        su = np.sort(rng.uniform(0.0, M - 1.0, L))
        su[-1] = M - 1.0
        src = curve(su).astype(np.float32)
        src_time = np.round(T0 + DT * su).astype(np.uint64)
        target = corrected(src.astype(np.float64), su / (M - 1.0))
        if L == 1:
            # One point constraint leaves the three rotations about it free: the normal matrix is singular (the reference's CHOLMOD would
            # refuse it), so no optimum exists to compare.  The single constraint asks for 5 mm, below the 0.1 gate (10 x 0.005 / 1): the
            # defined result is "insignificant", after every per-constraint kernel has run with one constraint.
            target = src.astype(np.float64) + np.array([0.005, 0.0, 0.0])
    out = {"node_pos": node_pos, "node_time": node_time, "points": pts, "times": times, "src": src, "src_time": src_time, "target": target,
           "extent": float(np.abs(node_pos).max() + 1.5)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# THE BOUND of both test modules.  G = the largest state-entry difference between the restatement and the independent Gauss-Newton of
# tests/test_deform_ref.py over the cases (profiles/deformation.md lists it per case); the bound is 10 G with a floor of 1e-9: operation
# order is the only difference.
G_MEASURED = 1.5e-13
BOUND = max(10 * G_MEASURED, 1e-9)


def rel_bound(v):
    """errors are held to the same bound, relative to their size above 1"""
    return BOUND * max(1.0, abs(v))


@functools.lru_cache(maxsize=None)
def graph(name):
    from kintinuous_amd import deform_ref as ref
    c = case(name)
    return ref.Graph(c["node_pos"], c["node_time"])


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement's optimise for a case, computed once per process: (state, error_start, error_end, constraint_error, steps, status, trace)"""
    from kintinuous_amd import deform_ref as ref
    c = case(name)
    out = ref.optimise(graph(name), c["src"], c["src_time"], c["target"])
    out[0].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated_weights(name):
    from kintinuous_amd import deform_ref as ref
    c = case(name)
    idx, w = ref.weights(graph(name), c["points"]["xyz"], c["times"])
    idx.setflags(write=False); w.setflags(write=False)
    return idx, w


@functools.lru_cache(maxsize=None)
def restated_apply(name):
    """the points after the restatement's apply with the restatement's optimised state"""
    from kintinuous_amd import deform_ref as ref
    c = case(name)
    idx, w = restated_weights(name)
    out = ref.apply_points(graph(name), restated(name)[0], c["points"], idx, w)
    out.setflags(write=False)
    return out
