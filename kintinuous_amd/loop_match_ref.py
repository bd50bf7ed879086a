"""The loop-closure bootstrap stage (include/kt_abi.h: kt_frame_keypoints, kt_descriptor_match, kt_loop_match_frames)
restated in numpy: no GPU, no oracle.

It takes the place of the dense half of PlaceRecognition::processLoopClosureDetection before icpDepthFrames (SURF keypoints, surfMatch3D,
cv::solvePnPRansac) and is a definition, not a port of SURF or of OpenCV's PnP: FAST-9 corners, an upright BRIEF-256 on a 5x5 box sum, a
Hamming ratio test with a cross-check, and a three-point rigid RANSAC scored by reprojection.  Every step is integer arithmetic or float /
double arithmetic of a fixed order, so csrc/kt_match.hip computes the same bits; the one exception is the final refit (kt_host_rigid_fit
there, an SVD here: loop_icp_ref.rigid_fit), which agrees to rounding.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import brief_table
from .loop_icp_ref import rigid_fit

F = np.float32
# the 16-pixel Bresenham ring of radius 3 as (dx, dy), clockwise from the top
RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
MARGIN = brief_table.REACH + 2      # the descriptor's reach plus the radius of the 5x5 box
NO_SECOND = 257                     # d2 when there is no second neighbour: one more than any Hamming distance of 256 bits
DEGENERATE_EPS = 1e-3               # metres: |p1 - p0| and the distance of p2 from that line
MAX_KEYPOINTS_LIMIT = 4096


@dataclass
class Params:                       # kt_loop_match_params and kt_loop_match_params_default
    fast_threshold: int = 20
    max_keypoints: int = 2048
    max_hamming: int = 64
    ratio_num: int = 4
    ratio_den: int = 5
    n_hypotheses: int = 500
    reproj_px: float = 2.0
    max_dist: float = 4.0
    seed: int = 1


def intensity(rgb: np.ndarray) -> np.ndarray:
    """kt_bgr_to_intensity: trunc(fmaf(g, 0.587f, fmaf(r, 0.114f, b * 0.299f))) on bytes 0, 1, 2.  The fused steps are exact in double
    (8-bit x 24-bit products), so rounding the double result once to float32 is the fma."""
    rgb = np.asarray(rgb, np.uint8)
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    p = (rgb[..., 2].astype(F) * F(0.299)).astype(np.float64)
    q = (r * np.float64(F(0.114)) + p).astype(F).astype(np.float64)
    return (g * np.float64(F(0.587)) + q).astype(F).astype(np.int32).astype(np.uint8)


def fast_scores(I: np.ndarray, t: int) -> np.ndarray:
    """uint16 [rows, cols]: the FAST-9 score of every corner, 0 elsewhere (and within 3 pixels of a border)"""
    I = np.asarray(I, np.uint8).astype(np.int32)
    rows, cols = I.shape
    out = np.zeros((rows, cols), np.uint16)
    if rows < 7 or cols < 7:
        return out
    c = I[3:rows - 3, 3:cols - 3]
    ring = np.stack([I[3 + dy:rows - 3 + dy, 3 + dx:cols - 3 + dx] for dx, dy in RING])
    bright, dark = ring > c + t, ring < c - t
    corner = np.zeros(c.shape, bool)
    for s in range(16):
        run = [(s + k) % 16 for k in range(9)]
        corner |= bright[run].all(axis=0) | dark[run].all(axis=0)
    score = np.maximum(np.abs(ring - c) - t, 0).sum(axis=0)
    out[3:rows - 3, 3:cols - 3] = np.where(corner, score, 0)
    return out


def nms(score: np.ndarray) -> np.ndarray:
    """a corner survives when it beats the neighbours before it in raster order strictly and the ones after it weakly"""
    s = np.asarray(score, np.int32)
    rows, cols = s.shape
    p = np.zeros((rows + 2, cols + 2), np.int32)
    p[1:-1, 1:-1] = s
    keep = s > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            q = p[1 + dy:rows + 1 + dy, 1 + dx:cols + 1 + dx]
            keep &= (s > q) if (dy < 0 or (dy == 0 and dx < 0)) else (s >= q)
    return keep


def box5(I: np.ndarray) -> np.ndarray:
    """uint16 [rows, cols]: the sum of the 5x5 window around every pixel whose window lies inside the image, 0 elsewhere"""
    I = np.asarray(I, np.uint8).astype(np.int32)
    rows, cols = I.shape
    out = np.zeros((rows, cols), np.uint16)
    if rows < 5 or cols < 5:
        return out
    acc = np.zeros((rows - 4, cols - 4), np.int32)
    for dy in range(5):
        for dx in range(5):
            acc += I[dy:rows - 4 + dy, dx:cols - 4 + dx]
    out[2:rows - 2, 2:cols - 2] = acc
    return out


def describe(S: np.ndarray, uv: np.ndarray) -> np.ndarray:
    """uint32 [n, 8]: bit k = S(p + a_k) < S(p + b_k), in word k / 32 at position k % 32"""
    tab = brief_table.build_table().astype(np.int64)
    u, v = uv[:, 0].astype(np.int64)[:, None], uv[:, 1].astype(np.int64)[:, None]
    a = S[v + tab[None, :, 1], u + tab[None, :, 0]]
    b = S[v + tab[None, :, 3], u + tab[None, :, 2]]
    bits = (a < b).astype(np.uint64).reshape(len(uv), 8, 32)
    return (bits << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def frame_keypoints(rgb: np.ndarray, depth: np.ndarray, prm: Params = Params()):
    """kt_frame_keypoints (steps a-c): (uv int32 [n, 2], score int32 [n], desc uint32 [n, 8]), best first"""
    depth = np.asarray(depth, np.uint16)
    rows, cols = depth.shape
    I = intensity(np.asarray(rgb, np.uint8).reshape(rows, cols, 3))
    score = fast_scores(I, int(prm.fast_threshold))
    keep = nms(score)
    inside = np.zeros((rows, cols), bool)
    if rows > 2 * MARGIN and cols > 2 * MARGIN:
        inside[MARGIN:rows - MARGIN, MARGIN:cols - MARGIN] = True
    keep &= inside & (depth != 0) & (depth.astype(F) < F(prm.max_dist) * F(1000.0))
    idx = np.flatnonzero(keep)
    sc = score.reshape(-1)[idx].astype(np.int32)
    order = np.lexsort((idx, -sc))[:int(prm.max_keypoints)]
    idx, sc = idx[order], sc[order]
    uv = np.stack([idx % cols, idx // cols], axis=1).astype(np.int32)
    return uv, sc, describe(box5(I), uv)


def points3d(uv: np.ndarray, depth: np.ndarray, fx, fy, cx, cy) -> np.ndarray:
    """step d, float32 [n, 3]: z = d * 0.001f, x = ((float)u - cx) * z * (1.0f / fx), y likewise (kt_loop.hip's cloud step)"""
    d = np.asarray(depth, np.uint16)[uv[:, 1], uv[:, 0]].astype(F)
    z = d * F(0.001)
    x = (uv[:, 0].astype(F) - F(cx)) * z * (F(1.0) / F(fx))
    y = (uv[:, 1].astype(F) - F(cy)) * z * (F(1.0) / F(fy))
    return np.stack([x, y, z], axis=1).astype(F)


def _popcount64(x: np.ndarray) -> np.ndarray:
    x = x - ((x >> np.uint64(1)) & np.uint64(0x5555555555555555))
    x = (x & np.uint64(0x3333333333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return (x * np.uint64(0x0101010101010101)) >> np.uint64(56)


def hamming(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """int32 [len(a), len(b)]"""
    a64 = np.ascontiguousarray(a, np.uint32).reshape(-1, 8).view(np.uint64)
    b64 = np.ascontiguousarray(b, np.uint32).reshape(-1, 8).view(np.uint64)
    out = np.zeros((len(a64), len(b64)), np.int32)
    for k in range(4):
        out += _popcount64(a64[:, k][:, None] ^ b64[:, k][None, :]).astype(np.int32)
    return out


def descriptor_match(desc_new: np.ndarray, desc_old: np.ndarray, prm: Params = Params()):
    """kt_descriptor_match (step e without the cross-check): (old index or -1 int32 [n_new], d1, d2 int32 [n_new]).  d1 / d2 are the two
    smallest distances with duplicates counted, the index the lowest one at d1; d2 = NO_SECOND when there is one old descriptor."""
    n_new, n_old = len(desc_new), len(desc_old)
    idx, d1, d2 = np.zeros(n_new, np.int32), np.zeros(n_new, np.int32), np.full(n_new, NO_SECOND, np.int32)
    for i0 in range(0, n_new, 256):
        D = hamming(desc_new[i0:i0 + 256], desc_old)
        r = np.arange(len(D))
        j = np.argmin(D, axis=1)
        idx[i0:i0 + 256], d1[i0:i0 + 256] = j, D[r, j]
        if n_old > 1:
            D[r, j] = NO_SECOND
            d2[i0:i0 + 256] = D.min(axis=1)
    ok = (d1 <= int(prm.max_hamming)) & (int(prm.ratio_den) * d1 < int(prm.ratio_num) * d2)
    return np.where(ok, idx, -1).astype(np.int32), d1, d2


def match_keypoints(desc_new, desc_old, prm: Params = Params()) -> np.ndarray:
    """step e: int32 [n_matches, 2] = (new index, old index) in new-keypoint order, ratio-tested and cross-checked"""
    if len(desc_new) == 0 or len(desc_old) == 0:
        return np.zeros((0, 2), np.int32)
    fwd, _, _ = descriptor_match(desc_new, desc_old, prm)
    back = np.concatenate([np.argmin(hamming(desc_old[j0:j0 + 256], desc_new), axis=1) for j0 in range(0, len(desc_old), 256)])
    i = np.flatnonzero(fwd >= 0)
    i = i[back[fwd[i]] == i]
    return np.stack([i, fwd[i]], axis=1).astype(np.int32)


def draw_hash(seed: int, h: np.ndarray, k: int) -> np.ndarray:
    """the counter hash of (seed, hypothesis, draw): murmur3's 32-bit finaliser of seed + 0x9E3779B9 * (3 h + k + 1), all mod 2^32"""
    m = np.uint64(0xFFFFFFFF)
    x = (np.uint64(seed & 0xFFFFFFFF) + np.uint64(0x9E3779B9) * (np.uint64(3) * h.astype(np.uint64) + np.uint64(k + 1))) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x


def draw_triples(seed: int, n_hyp: int, n_matches: int) -> np.ndarray:
    """int64 [n_hyp, 3]: three distinct match indices per hypothesis, made distinct by skipping over the ones already drawn"""
    h = np.arange(n_hyp)
    M = np.uint64(n_matches)
    i0 = (draw_hash(seed, h, 0) % M).astype(np.int64)
    i1 = (draw_hash(seed, h, 1) % (M - np.uint64(1))).astype(np.int64)
    i1 += i1 >= i0
    i2 = (draw_hash(seed, h, 2) % (M - np.uint64(2))).astype(np.int64)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 += i2 >= lo
    i2 += i2 >= hi
    return np.stack([i0, i1, i2], axis=1)


def _triad(p0, p1, p2):
    """orthonormal triads of [n, 3] double triples: (e1, e2, e3, centroid, degenerate)"""
    a = p1 - p0
    n1 = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        e1 = a / n1[:, None]
        b = p2 - p0
        c = np.stack([e1[:, 1] * b[:, 2] - e1[:, 2] * b[:, 1], e1[:, 2] * b[:, 0] - e1[:, 0] * b[:, 2], e1[:, 0] * b[:, 1] - e1[:, 1] * b[:, 0]], axis=1)
        n3 = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        e3 = c / n3[:, None]
        e2 = np.stack([e3[:, 1] * e1[:, 2] - e3[:, 2] * e1[:, 1], e3[:, 2] * e1[:, 0] - e3[:, 0] * e1[:, 2], e3[:, 0] * e1[:, 1] - e3[:, 1] * e1[:, 0]], axis=1)
    cen = ((p0 + p1) + p2) / 3.0
    return e1, e2, e3, cen, ~((n1 >= DEGENERATE_EPS) & (n3 >= DEGENERATE_EPS))


def fit_triples(Pn: np.ndarray, Po: np.ndarray, tri: np.ndarray):
    """the rigid T (new camera -> old camera) through three pairs: (R [n, 3, 3], t [n, 3], degenerate [n]) in double"""
    Pn, Po = Pn.astype(np.float64), Po.astype(np.float64)
    n1, n2, n3, cn, dn = _triad(Pn[tri[:, 0]], Pn[tri[:, 1]], Pn[tri[:, 2]])
    o1, o2, o3, co, do = _triad(Po[tri[:, 0]], Po[tri[:, 1]], Po[tri[:, 2]])
    with np.errstate(invalid="ignore"):
        R = (o1[:, :, None] * n1[:, None, :] + o2[:, :, None] * n2[:, None, :]) + o3[:, :, None] * n3[:, None, :]
        t = co - ((R[:, :, 0] * cn[:, 0:1] + R[:, :, 1] * cn[:, 1:2]) + R[:, :, 2] * cn[:, 2:3])
    return R, t, dn | do


def reprojection_inliers(R, t, Pn, uv_old, fx, fy, cx, cy, reproj_px) -> np.ndarray:
    """bool [n_hyp, n_matches]: the new point moved by (R, t) has z > 0 and projects within reproj_px of the old keypoint.  Intrinsics are
    the kt_intr floats widened to double; u = (fx * X) / Z + cx."""
    x, y, z = (Pn[:, k].astype(np.float64)[None, :] for k in range(3))
    fx, fy, cx, cy = (np.float64(F(v)) for v in (fx, fy, cx, cy))
    with np.errstate(divide="ignore", invalid="ignore"):
        X, Y, Z = (((R[:, a, 0:1] * x + R[:, a, 1:2] * y) + R[:, a, 2:3] * z) + t[:, a:a + 1] for a in range(3))
        du = ((fx * X) / Z + cx) - uv_old[:, 0].astype(np.float64)[None, :]
        dv = ((fy * Y) / Z + cy) - uv_old[:, 1].astype(np.float64)[None, :]
        return (Z > 0.0) & ((du * du + dv * dv) <= np.float64(F(reproj_px)) * np.float64(F(reproj_px)))


def rigid_inverse(T: np.ndarray) -> np.ndarray:
    R, t = T[:3, :3], T[:3, 3]
    out = np.eye(4)
    out[:3, :3] = R.T
    out[:3, 3] = [-((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2]) for a in range(3)]
    return out


def ransac(Pn, Po, uv_old, fx, fy, cx, cy, prm: Params = Params()):
    """step f on the matched 3D points (new, old) and the old pixels: (pose float32 [4, 4], bootstrap float32 [4, 4], inlier bool
    [n_matches], best hypothesis index or -1, that hypothesis's score)"""
    M = len(Pn)
    eye = np.eye(4, dtype=F)
    none = (eye, eye.copy(), np.zeros(M, bool), -1, 0)
    if M < 3 or prm.n_hypotheses < 1:
        return none
    tri = draw_triples(prm.seed, int(prm.n_hypotheses), M)
    R, t, deg = fit_triples(Pn, Po, tri)
    score = np.where(deg, 0, reprojection_inliers(R, t, Pn, uv_old, fx, fy, cx, cy, prm.reproj_px).sum(axis=1))
    best = int(np.argmax(score))                                     # the first maximum: the lowest hypothesis index
    if score[best] < 3:
        return none
    inl = reprojection_inliers(R[best:best + 1], t[best:best + 1], Pn, uv_old, fx, fy, cx, cy, prm.reproj_px)[0]
    T = rigid_fit(Pn[inl], Po[inl])
    inl = reprojection_inliers(T[None, :3, :3], T[None, :3, 3], Pn, uv_old, fx, fy, cx, cy, prm.reproj_px)[0]
    return T.astype(F), rigid_inverse(T).astype(F), inl, best, int(score[best])


def loop_match_frames(rgb_old, depth_old, rgb_new, depth_new, fx, fy, cx, cy, prm: Params = Params()):
    """kt_loop_match_frames: dict(pose, bootstrap, matches int32 [n, 4] = (old u, old v, new u, new v), inlier bool [n], info, and the
    keypoints of both frames)"""
    ko, kn = frame_keypoints(rgb_old, depth_old, prm), frame_keypoints(rgb_new, depth_new, prm)
    m = match_keypoints(kn[2], ko[2], prm)
    uv_new, uv_old = kn[0][m[:, 0]], ko[0][m[:, 1]]
    Pn, Po = points3d(uv_new, depth_new, fx, fy, cx, cy), points3d(uv_old, depth_old, fx, fy, cx, cy)
    pose, boot, inl, best, best_score = ransac(Pn, Po, uv_old, fx, fy, cx, cy, prm)
    info = dict(n_kp_old=len(ko[0]), n_kp_new=len(kn[0]), n_matches=len(m), n_inliers=int(inl.sum()), best_hypothesis=best)
    return dict(pose=pose, bootstrap=boot, matches=np.concatenate([uv_old, uv_new], axis=1).astype(np.int32).reshape(-1, 4), inlier=inl, info=info,
                keypoints_old=ko, keypoints_new=kn, match_index=m, best_score=best_score)
