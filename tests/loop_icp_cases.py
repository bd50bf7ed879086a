"""Shared by tests/test_loop_icp_ref.py (CPU) and tests/test_gpu_loop_icp.py: the frame pairs of the loop-closure registration tests, their
ground truth, and an INDEPENDENT float64 implementation of the stage (scipy cKDTree, double everywhere, numpy binning) that shares no
code with kintinuous_amd/loop_icp_ref.py -- the role tests/test_slice_independent.py plays for the slice stage."""
import functools

import numpy as np
from scipy.spatial import cKDTree

LEAF = 2.5 * 6.0 / 512          # 2.5 voxel edges of the 512^3 / 6 m volume (PlaceRecognition.cpp:250)


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _pose(R, c):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, c
    return T


# camera-to-scene poses of the "room" scene: A and B a few degrees and centimetres apart; C looks at the side wall (another part of the room)
POSE_A = _pose(np.eye(3), np.zeros(3))
POSE_B = _pose(_rot([0, 1, 0], np.radians(3.0)) @ _rot([1, 0, 0], np.radians(1.0)), np.array([0.05, 0.01, 0.03]))
POSE_C = _pose(_rot([0, 1, 0], np.radians(80.0)), np.array([0.4, 0.0, -0.3]))


@functools.lru_cache(maxsize=None)
def render(cols, rows, which):
    from kintinuous_amd import synth
    cam = synth.Camera.small(cols, rows)
    T = {"A": POSE_A, "B": POSE_B, "C": POSE_C}[which]
    depth, _ = synth.render(synth.Scene("room"), cam, T[:3, :3], T[:3, 3])
    return cam, depth


def truth(which_from="A", which_to="B"):
    """the transform that takes points of the first camera's frame into the second's"""
    P = {"A": POSE_A, "B": POSE_B, "C": POSE_C}
    return np.linalg.inv(P[which_to]) @ P[which_from]


def bootstrap(seed=7):
    """the truth of (A, B) perturbed by about 1 degree and 2 cm (float32 4x4, as a PnP bootstrap would arrive)"""
    rng = np.random.default_rng(seed)
    axis, direction = rng.normal(size=3), rng.normal(size=3)
    P = _pose(_rot(axis, np.radians(1.0)), 0.02 * direction / np.linalg.norm(direction))
    return (P @ truth()).astype(np.float32)


def pose_error(M, M_true):
    """(rotation angle in radians, translation distance in metres) between two rigid transforms"""
    D = np.asarray(M, np.float64) @ np.linalg.inv(M_true)
    R = D[:3, :3]                                           # atan2 of the skew part and the trace: well conditioned near zero, unlike arccos
    ang = np.arctan2(0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]), (np.trace(R) - 1) / 2)
    return float(ang), float(np.linalg.norm(D[:3, 3]))


def pose_distance(Ma, Mb):
    return pose_error(Ma, np.asarray(Mb, np.float64))


# ---- the independent float64 implementation --------------------------------------------------------------------------------------
def cloud64(depth, cam, max_dist):
    rows, cols = depth.shape
    pts = []
    for u in range(cols):                                   # column outer, as the reference walks the image
        d = depth[:, u].astype(np.float64)
        v = np.flatnonzero((d != 0) & (d < max_dist * 1000.0))
        z = d[v] / 1000.0
        pts.append(np.stack([(u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z], axis=1))
    return np.concatenate(pts) if pts else np.zeros((0, 3))


def grid64(p, leaf):
    if len(p) == 0:
        return p
    ijk = np.floor(p / leaf).astype(np.int64)
    ijk -= ijk.min(axis=0)
    div = ijk.max(axis=0) + 1
    key = ijk[:, 0] + div[0] * (ijk[:, 1] + div[1] * ijk[:, 2])
    uniq, inverse, counts = np.unique(key, return_inverse=True, return_counts=True)
    cen = np.zeros((len(uniq), 3))
    np.add.at(cen, inverse, p)
    return cen / counts[:, None]


def kabsch64(s, t):
    sm, tm = s.mean(axis=0), t.mean(axis=0)
    U, _, Vt = np.linalg.svd((s - sm).T @ (t - tm))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, tm - R @ sm
    return M


def icp64(depth1, depth2, cam, boot, leaf, max_dist=4.0, max_iterations=10):
    """(M float64, score, iterations, seconds spent in the registration itself)"""
    import time
    S, T = grid64(cloud64(depth1, cam, max_dist), leaf), grid64(cloud64(depth2, cam, max_dist), leaf)
    t0 = time.perf_counter()
    M = np.asarray(boot, np.float64).copy()
    tree = cKDTree(T)
    prev, its, dist = None, 0, None
    for _ in range(max_iterations):
        Sk = S @ M[:3, :3].T + M[:3, 3]
        dist, idx = tree.query(Sk)
        if prev is not None and np.array_equal(idx, prev):
            break
        M = kabsch64(Sk, T[idx]) @ M
        prev, dist, its = idx, None, its + 1
    if dist is None:
        dist, _ = tree.query(S @ M[:3, :3].T + M[:3, 3])
    return M, float(np.mean(dist ** 2)), its, time.perf_counter() - t0


@functools.lru_cache(maxsize=None)
def run64(cols, rows, to="B"):
    cam, d1 = render(cols, rows, "A")
    _, d2 = render(cols, rows, to)
    return icp64(d1, d2, cam, bootstrap(), LEAF)
