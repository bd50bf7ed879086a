"""Synthetic pose graphs for the pose-graph stage (tests/test_pose_graph_ref.py, tests/test_gpu_pose_graph.py).

Ground truth: N poses on a closed curve (a circle of 2 m with a vertical wobble), the camera looking inward.  Chain measurements are the true
increments times Exp of Gaussian noise (0.2 mrad / 0.5 mm per step); loop measurements the true relative poses times noise of at most
2 degrees / 2 cm, so the minimum is well conditioned and the residual small.  Everything comes from a seeded generator.

NAMES are the cases every module runs (1 to 4097 nodes, drawn node by node); LARGE the ones above 65536 nodes (the same curve and noise
levels from array expressions), which only the tests written for them pick up; STEP_LIMIT the one graph that does not converge in 20 steps.
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


# ---- above 65536 nodes: the carry scan's serial runs (per = ceil(ceil(N / 256) / 256) >= 2) -----------------------------------------------
# These cases are NOT in NAMES: the modules that parametrise over NAMES (finite-difference Jacobians, the independent optimiser) would run for
# minutes on them.  They come from a vectorised generator of their own, so no existing case changes a byte.  name, N, loops, seed
_LARGE_SPECS = [
    ("n65536_chain", 65536, [], 3000),                                     # nb = 256, per = 1: every lane of the carry scan owns one total
    ("n65537_chain", 65537, [], 3001),                                     # nb = 257, per = 2: lanes 0..127 two totals, lane 128 one, the rest none
    ("n131073_chain", 131073, [], 3002),                                   # nb = 513, per = 3: lanes 0..170 three, the rest none; the last block one node
    # n1025_l7's loops times 64: end to start, nested twice, a < b, overlapping, neighbours; the adjacent pair sits across the boundary of
    # two scan blocks (127 | 128) that belong to two lanes' runs (63 | 64)
    ("n65537_l7", 65537, [(65536, 0), (57600, 6400), (19200, 38400), (64000, 32000), (2560, 128), (65472, 63360), (32768, 32767)], 3003),
]
LARGE = [s[0] for s in _LARGE_SPECS]
LARGE_CHAINS = [s[0] for s in _LARGE_SPECS if not s[2]]
LARGE_LOOPS = "n65537_l7"
# the seed of n65537_l7 is chosen so that in the restatement NO step's max |delta| lies within a factor of two of the stopping bound 1e-9
# (tests/test_pose_graph_ref.py asserts it), so the device takes the same number of steps
STEP_LIMIT = "n65_step_limit"       # n65_contradiction's graph with the contradicting loop 4 m off instead of 0.3 m: 20 steps do not converge
STEP_LIMIT_MOVE = 4.0
# exact measurements at 65537 nodes return the ground truth within: 65536 products, each adding at most 3 roundings of 1.1e-16 on entries
# below 4.3 (test_exact_measurements_give_the_truth's derivation at this size: 9e-11 at worst)
EXACT_BOUND_LARGE = 1e-10


def truth_large(N):
    """truth(N) from array expressions"""
    th = 2.0 * np.pi * np.arange(N) / N
    p = np.stack([2.0 * np.cos(th), 2.0 * np.sin(th), 0.2 * np.sin(3.0 * th)], -1)
    z = -p / np.linalg.norm(p, axis=1)[:, None]
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x, axis=1)[:, None]
    T = np.tile(np.eye(4), (N, 1, 1))
    T[:, :3, 0], T[:, :3, 1], T[:, :3, 2], T[:, :3, 3] = x, np.cross(z, x), z, p
    return T


def _mul(A, B):
    """(..., 4, 4) x (..., 4, 4), entry by entry (the same bits on every machine, which a library's matmul does not promise)"""
    return sum(A[..., :, c, None] * B[..., None, c, :] for c in range(4))


def _inv(T):
    out = np.tile(np.eye(4), T.shape[:-2] + (1, 1))
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -sum(Rt[..., :, c] * T[..., None, c, 3] for c in range(3))
    return out


def increments(T):
    """T_{k-1}^-1 T_k for k = 1 .. N - 1, in one batched product"""
    return _mul(_inv(T[:-1]), T[1:])


def _large_case(name):
    _, N, loops, seed = _LARGE_SPECS[LARGE.index(name)]
    rng = np.random.default_rng(seed)
    T = truth_large(N)
    noise = np.tile(np.eye(4), (N - 1, 1, 1))
    noise[:, :3, 3] = 0.5e-3 * rng.standard_normal((N - 1, 3))
    noise[:, :3, :3] = Rotation.from_rotvec(0.2e-3 * rng.standard_normal((N - 1, 3))).as_matrix()
    chain = _mul(increments(T), noise)
    loop_Z = np.tile(np.eye(4), (len(loops), 1, 1))
    for l, (a, b) in enumerate(loops):
        loop_Z[l] = inv(T[a]) @ T[b] @ exp(_bounded(rng, 0.02), _bounded(rng, np.deg2rad(2.0)))
    return {"N": N, "T0": T[0].copy(), "chain_Z": chain, "loop_a": np.array([a for a, _ in loops], dtype=np.int32),
            "loop_b": np.array([b for _, b in loops], dtype=np.int32), "loop_Z": loop_Z, "truth": T}


def _step_limit_case():
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case(CONTRADICTION).items()}
    bad = _SPECS[NAMES.index(CONTRADICTION)][3]
    c["loop_Z"][bad, 0, 3] += STEP_LIMIT_MOVE - 0.3
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: N, T0 (4, 4), chain_Z (N - 1, 4, 4), loop_a, loop_b (int32), loop_Z (L, 4, 4), truth (N, 4, 4) -- read-only arrays"""
    if name in LARGE or name == STEP_LIMIT:
        out = _large_case(name) if name in LARGE else _step_limit_case()
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        return out
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
    if name in LARGE:
        c["chain_Z"], c["loop_Z"] = increments(T), _mul(_inv(T[c["loop_a"]]), T[c["loop_b"]]).reshape(-1, 4, 4)
        return c
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
