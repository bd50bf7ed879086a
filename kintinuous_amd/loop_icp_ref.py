"""The loop-closure registration stage (include/kt_abi.h: kt_loop_icp_depth_frames) restated in numpy: no GPU, no oracle.

It replaces PlaceRecognition::icpDepthFrames (backend/PlaceRecognition.cpp:238-276) and is a definition, not a port of PCL: float32 where
the definition says float32 (cloud, voxel grid, transformed points, squared distances), float64 sums, a float64 SVD for the closed-form
rigid fit.  csrc/kt_loop.hip computes the same thing on the GPU; the only difference the definition leaves open is the order of the
double sums (about 1e-13 on the transform).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

F = np.float32


def depth_to_cloud(frame: np.ndarray, fx, fy, cx, cy, max_dist: float = 4.0) -> np.ndarray:
    """DepthCamera::convertToXYZPointCloud (backend/DepthCamera.cpp:143-163) with float intrinsics: float32 [n, 3], column outer."""
    frame = np.asarray(frame, np.uint16)
    rows, cols = frame.shape
    d = frame.T.astype(F)                                     # [u, v]: C order of the transpose is the reference's point order
    keep = (frame.T != 0) & (d < F(max_dist) * F(1000.0))
    u = np.broadcast_to(np.arange(cols, dtype=F)[:, None], (cols, rows))
    v = np.broadcast_to(np.arange(rows, dtype=F)[None, :], (cols, rows))
    z = d * F(0.001)
    x = (u - F(cx)) * z * (F(1.0) / F(fx))
    y = (v - F(cy)) * z * (F(1.0) / F(fy))
    return np.stack([x[keep], y[keep], z[keep]], axis=1).astype(F)


def voxel_grid(points: np.ndarray, leaf: float) -> np.ndarray:
    """pcl::VoxelGrid<PointXYZ> at `leaf` as csrc/kt_slice.hip restates it: float leaf indices relative to the cloud's minimum, the points of
    a leaf summed in input order in float32, centroid = sum * (1 / count), leaves in key order.  float32 [n_leaves, 3]."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    if len(p) == 0:
        return p.copy()
    inv = F(1.0) / F(leaf)
    mn, mx = p.min(axis=0), p.max(axis=0)
    # "Leaf size is too small for the input dataset": PCL passes the cloud through
    cells = 1
    for a in range(3):
        cells *= int(np.trunc(np.float64((mx[a] - mn[a]) * inv))) + 1
    if cells > 2147483647:
        return p.copy()
    min_b = np.floor(mn * inv).astype(np.int64)
    div_b = np.floor(mx * inv).astype(np.int64) - min_b + 1
    ijk = (np.floor(p * inv) - min_b.astype(F)).astype(np.int64)      # float subtraction, then truncation (voxel_grid.hpp)
    key = (ijk[:, 0] + ijk[:, 1] * div_b[0] + ijk[:, 2] * (div_b[0] * div_b[1] & 0xFFFFFFFF)) & 0xFFFFFFFF
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    count = np.diff(np.r_[head, len(ks)])
    acc = np.zeros((len(head), 3), F)
    ps = p[order]
    for r in range(int(count.max())):                                  # the r-th point of every leaf that has one, in input order
        has = count > r
        acc[has] = acc[has] + ps[head[has] + r]
    return (acc * (F(1.0) / count.astype(F))[:, None]).astype(F)


def depth_to_cloud_grid(frame, fx, fy, cx, cy, leaf: float, max_dist: float = 4.0) -> np.ndarray:
    """steps a + b (kt_depth_to_cloud_grid)"""
    return voxel_grid(depth_to_cloud(frame, fx, fy, cx, cy, max_dist), leaf)


def nearest(src: np.ndarray, dst: np.ndarray, chunk_elems: int = 1 << 22) -> Tuple[np.ndarray, np.ndarray]:
    """kt_cloud_nearest: for every src point the LOWEST index of a nearest dst point under d2 = (dx * dx + dy * dy) + dz * dz in float32,
    and that d2.  Brute force, in chunks of src rows."""
    src = np.ascontiguousarray(src, F).reshape(-1, 3)
    dst = np.ascontiguousarray(dst, F).reshape(-1, 3)
    idx = np.zeros(len(src), np.uint32)
    d2 = np.zeros(len(src), F)
    step = max(1, chunk_elems // max(len(dst), 1))
    tx, ty, tz = dst[:, 0][None, :], dst[:, 1][None, :], dst[:, 2][None, :]
    for i0 in range(0, len(src), step):
        s = src[i0:i0 + step]
        dx, dy, dz = s[:, 0:1] - tx, s[:, 1:2] - ty, s[:, 2:3] - tz
        d = (dx * dx + dy * dy) + dz * dz
        j = np.argmin(d, axis=1)                                       # the first minimum: the lowest index
        idx[i0:i0 + step] = j
        d2[i0:i0 + step] = d[np.arange(len(s)), j]
    return idx, d2


def transform_points(M: np.ndarray, S: np.ndarray) -> np.ndarray:
    """float32(M . s): the product in double, ((m0 x + m1 y) + m2 z) + m3, rounded once per coordinate"""
    x, y, z = (S[:, k].astype(np.float64) for k in range(3))
    return np.stack([((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3] for a in range(3)], axis=1).astype(F)


def rigid_fit(s: np.ndarray, t: np.ndarray) -> np.ndarray:
    """the rigid dM (float64 4x4, det R = +1) minimising sum |dM s_i - t_i|^2: SVD of the centred cross-covariance"""
    s, t = s.astype(np.float64), t.astype(np.float64)
    sm, tm = s.mean(axis=0), t.mean(axis=0)
    H = (s - sm).T @ (t - tm)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    dM = np.eye(4)
    dM[:3, :3], dM[:3, 3] = R, tm - R @ sm
    return dM


def icp_clouds(S: np.ndarray, T: np.ndarray, bootstrap, max_iterations: int = 10):
    """steps c + d on the down-sampled clouds: (M float32 [4, 4], score float, info)"""
    M = np.asarray(bootstrap, F).reshape(4, 4).astype(np.float64)
    info = dict(n_source=len(S), n_target=len(T), iterations=0, converged=False)
    if len(S) == 0 or len(T) == 0:
        return M.astype(F), float("inf"), info
    prev, d2 = None, None
    for _ in range(int(max_iterations)):
        Sk = transform_points(M, S)
        idx, d2 = nearest(Sk, T)
        if prev is not None and np.array_equal(idx, prev):            # a fixed point: nothing to update, this pass's d2 are the score's
            info["converged"] = True
            break
        M = rigid_fit(Sk, T[idx]) @ M
        info["iterations"] += 1
        prev, d2 = idx, None
    if d2 is None:
        _, d2 = nearest(transform_points(M, S), T)
    score = float(F(d2.astype(np.float64).sum() / len(S)))
    return M.astype(F), score, info


def icp_depth_frames(frame1, frame2, fx, fy, cx, cy, bootstrap, leaf: float, max_dist: float = 4.0, max_iterations: int = 10):
    """kt_loop_icp_depth_frames: (M float32 [4, 4] = the reference's getFinalTransformation() * bootstrap, score, info)"""
    S = depth_to_cloud_grid(frame1, fx, fy, cx, cy, leaf, max_dist)
    T = depth_to_cloud_grid(frame2, fx, fy, cx, cy, leaf, max_dist)
    return icp_clouds(S, T, bootstrap, max_iterations)
