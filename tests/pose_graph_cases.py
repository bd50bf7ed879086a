"""Synthetic pose graphs for the pose-graph stage (tests/test_pose_graph_ref.py, tests/test_gpu_pose_graph.py).

Ground truth: N poses on a closed curve (a circle of 2 m with a vertical wobble), the camera looking inward.  Chain measurements are the true
increments times Exp of Gaussian noise (0.2 mrad / 0.5 mm per step); loop measurements the true relative poses times noise of at most
2 degrees / 2 cm, so the minimum is well conditioned and the residual small.  Everything comes from a seeded generator.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.spatial.transform import Rotation


def truth(N):
    th = 2.0 * np.pi * np.arange(N) / max(N, 1)
    p = np.stack([2.0 * np.cos(th), 2.0 * np.sin(th), 0.2 * np.sin(3.0 * th)], -1)
    T = np.tile(np.eye(4), (N, 1, 1))
    for k in range(N):
        z = -p[k] / np.linalg.norm(p[k])                     # towards the centre
        x = np.cross([0.0, 0.0, 1.0], z); x /= np.linalg.norm(x)
        T[k, :3, 0], T[k, :3, 1], T[k, :3, 2], T[k, :3, 3] = x, np.cross(z, x), z, p[k]
    return T


def inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def exp(v, w):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(w).as_matrix()
    T[:3, 3] = v
    return T


def _bounded(rng, bound):
    d = rng.standard_normal(3)
    return d / np.linalg.norm(d) * bound * rng.uniform(0.2, 1.0)


# name, N, loops (a, b), index of the loop that contradicts the others by 30 cm (or None)
_SPECS = [
    ("n1", 1, [], None),
    ("n2_chain", 2, [], None),
    ("n257_chain", 257, [], None),
    ("n2_neighbours", 2, [(1, 0)], None),                                  # parallel to the chain edge
    ("n3_same_pair_twice", 3, [(2, 0), (2, 0)], None),
    ("n63_full", 63, [(62, 0)], None),
    ("n64_a_below_b", 64, [(5, 60)], None),
    # over everything, nested twice, overlapping, two disjoint, neighbours
    ("n65_spans", 65, [(64, 0), (40, 10), (30, 20), (50, 35), (8, 2), (63, 58), (21, 20)], None),
    ("n65_contradiction", 65, [(64, 0), (60, 3), (62, 1), (63, 2)], 3),
    ("n257_two", 257, [(256, 0), (100, 200)], None),
    ("n257_l64", 257, "random64", None),
    ("n1025_l7", 1025, [(1024, 0), (900, 100), (300, 600), (1000, 500), (40, 2), (1023, 990), (513, 512)], None),
    ("n4097_full", 4097, [(4096, 0)], None),
    ("n4097_l64", 4097, "random64", None),
]
# the seeds are chosen so that at most one case in ten ends with max |delta| within a factor of two of the stopping bound 1e-9
_SEEDS = {"n1025_l7": 2001}
NAMES = [s[0] for s in _SPECS]
INDEPENDENT = [s[0] for s in _SPECS if s[1] <= 1025]        # the cases the independent optimiser runs on
CONTRADICTION = "n65_contradiction"


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: N, T0 (4, 4), chain_Z (N - 1, 4, 4), loop_a, loop_b (int32), loop_Z (L, 4, 4), truth (N, 4, 4) -- read-only arrays"""
    idx = NAMES.index(name)
    _, N, loops, bad = _SPECS[idx]
    rng = np.random.default_rng(_SEEDS.get(name, 1000 + idx))
    T = truth(N)
    chain = np.tile(np.eye(4), (max(N - 1, 0), 1, 1))
    for k in range(1, N):
        chain[k - 1] = inv(T[k - 1]) @ T[k] @ exp(0.5e-3 * rng.standard_normal(3), 0.2e-3 * rng.standard_normal(3))
    if loops == "random64":
        loops = [(N - 1, 0)]
        while len(loops) < 64:
            a, b = (int(v) for v in rng.integers(0, N, 2))
            if a != b:
                loops.append((a, b))
    L = len(loops)
    loop_Z = np.tile(np.eye(4), (L, 1, 1))
    for l, (a, b) in enumerate(loops):
        loop_Z[l] = inv(T[a]) @ T[b] @ exp(_bounded(rng, 0.02), _bounded(rng, np.deg2rad(2.0)))
        if bad == l:
            loop_Z[l, :3, 3] += np.array([0.3, 0.0, 0.0])
    out = {"N": N, "T0": T[0].copy(), "chain_Z": chain, "loop_a": np.array([a for a, _ in loops], dtype=np.int32),
           "loop_b": np.array([b for _, b in loops], dtype=np.int32), "loop_Z": loop_Z, "truth": T}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# THE BOUND of both test modules.  G = the largest pose-entry difference between the restatement and the independent optimiser of
# tests/test_pose_graph_ref.py (its docstring lists G per case); the bound is 10 G with a floor of 1e-9.
G_MEASURED = 5.3e-10
BOUND = max(10 * G_MEASURED, 1e-9)


def chi2_bound(chi2):
    """chi2 is held to the same bound as the pose entries, relative to its size above 1"""
    return BOUND * max(1.0, abs(chi2))


def noise_free(name):
    """the same graph with exact chain and loop measurements: the minimum is the ground truth"""
    c = dict(case(name))
    T = c["truth"]
    c["chain_Z"] = np.array([inv(T[k - 1]) @ T[k] for k in range(1, c["N"])]).reshape(-1, 4, 4)
    c["loop_Z"] = np.array([inv(T[a]) @ T[b] for a, b in zip(c["loop_a"], c["loop_b"])]).reshape(-1, 4, 4)
    return c


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement's result for a case, computed once per process: (poses, chi2_start, chi2_end, steps, status, deltas)"""
    from kintinuous_amd import pose_graph_ref as ref
    c = case(name)
    out = ref.optimise(c["T0"], c["chain_Z"], c["loop_a"], c["loop_b"], c["loop_Z"])
    out[0].setflags(write=False)
    return out
