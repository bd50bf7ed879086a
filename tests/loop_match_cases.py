"""Shared by tests/test_loop_match_ref.py (CPU) and tests/test_gpu_loop_match.py: the frames of the loop-closure bootstrap tests and an
INDEPENDENT implementation of the two steps that decide the result -- a brute-force Hamming matcher over np.unpackbits and a float64
reprojection count for a given T -- that shares no code with kintinuous_amd/loop_match_ref.py.

The frames are loop_icp_cases' room poses A, B (a few degrees and centimetres from A) and C (another wall).  synth.render's colour is a
smooth sinusoid that gives a corner detector almost nothing, so the colour is replaced by a blocky texture fixed to the SCENE: the scene
point of every pixel (from its depth and the camera pose) falls into a cube of edge CELL, and the cube's integer coordinates are hashed
into a grey level.  Two views of the same surface see the same blocks."""
import functools

import numpy as np

import loop_icp_cases as lc

CELL = 0.11                        # metres; chosen on the CPU (tests/test_loop_match_ref.py) together with the default parameters
SHIFT = (0.031, 0.047, 0.023)      # keeps the room's walls (x = +-1.6, y = -1.1 / 1.0, z = -2.2 / 2.8) off the cube faces


def _camera(cols, rows):
    from kintinuous_amd import synth
    return synth.Camera(173, 97, 140.0, 141.0, 85.5, 50.25) if (cols, rows) == (173, 97) else synth.Camera.small(cols, rows)


def texture(depth, cam, pose, cell=CELL):
    """rgb24 [rows, cols, 3]: the grey level of the scene cube behind every pixel (0 depth: black)"""
    rows, cols = depth.shape
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    z = depth.astype(np.float64) / 1000.0
    p = np.stack([(u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z], axis=-1) @ pose[:3, :3].T + pose[:3, 3]
    q = np.floor((p + np.array(SHIFT)) / cell).astype(np.int64)
    h = (q[..., 0] * 73856093) ^ (q[..., 1] * 19349663) ^ (q[..., 2] * 83492791)
    h = (h ^ (h >> 13)) * 1274126177
    grey = (32 + ((h >> 7) & 0xFFFF) % 192).astype(np.uint8)
    grey[depth == 0] = 0
    return np.repeat(grey[..., None], 3, axis=2)


@functools.lru_cache(maxsize=None)
def frame(cols, rows, which):
    """(camera, depth uint16 [rows, cols], rgb24 [rows, cols, 3]) of pose A, B or C"""
    from kintinuous_amd import synth
    cam = _camera(cols, rows)
    T = {"A": lc.POSE_A, "B": lc.POSE_B, "C": lc.POSE_C}[which]
    depth, _ = synth.render(synth.Scene("room"), cam, T[:3, :3], T[:3, 3])
    return cam, depth, texture(depth, cam, T)


@functools.lru_cache(maxsize=None)
def restated(cols, rows, old="A", new="B"):
    """the restatement's result on a pair with the default parameters, computed once"""
    from kintinuous_amd import loop_match_ref as ref
    cam, d_old, rgb_old = frame(cols, rows, old)
    _, d_new, rgb_new = frame(cols, rows, new)
    return ref.loop_match_frames(rgb_old, d_old, rgb_new, d_new, cam.fx, cam.fy, cam.cx, cam.cy, ref.Params())


def checker(cols, rows, square=8, lo=60, hi=180):
    """a constant-contrast checkerboard: every inner crossing is a corner of the same score"""
    v, u = np.mgrid[0:rows, 0:cols]
    grey = np.where(((u // square) + (v // square)) % 2 == 0, lo, hi).astype(np.uint8)
    return np.repeat(grey[..., None], 3, axis=2)


def blob_frame(cols, rows, centres, size=6, lo=40, hi=220):
    """bright squares whose top-left corner pixel sits at the given (u, v): FAST fires at that pixel (among the square's corners)"""
    grey = np.full((rows, cols), lo, np.uint8)
    for u, v in centres:
        grey[max(v, 0):v + size, max(u, 0):u + size] = hi
    return np.repeat(grey[..., None], 3, axis=2)


# ---- the independent implementation ------------------------------------------------------------------------------------------------
def brute_match(desc_new, desc_old, max_hamming, ratio_num, ratio_den):
    """(old index or -1, d1, d2) per new descriptor: distances from unpacked bits, a stable sort for the lowest-index tie rule"""
    bn = np.unpackbits(np.ascontiguousarray(desc_new, np.uint32).view(np.uint8).reshape(len(desc_new), 32), axis=1)
    bo = np.unpackbits(np.ascontiguousarray(desc_old, np.uint32).view(np.uint8).reshape(len(desc_old), 32), axis=1)
    idx, d1, d2 = [], [], []
    for row in bn:
        dist = (row[None, :] != bo).sum(axis=1)
        order = np.argsort(dist, kind="stable")
        a = int(dist[order[0]])
        b = int(dist[order[1]]) if len(order) > 1 else 257
        idx.append(int(order[0]) if a <= max_hamming and ratio_den * a < ratio_num * b else -1)
        d1.append(a)
        d2.append(b)
    return np.array(idx, np.int32), np.array(d1, np.int32), np.array(d2, np.int32)


def count_inliers64(T, P_new, uv_old, cam_f32, reproj_px):
    """the matches whose new 3D point, moved by T (4x4) and projected with the float intrinsics, lands within reproj_px of the old pixel"""
    fx, fy, cx, cy = (float(np.float32(v)) for v in cam_f32)
    flags = []
    for p, (uo, vo) in zip(np.asarray(P_new, np.float64), np.asarray(uv_old, np.float64)):
        q = T[:3, :3] @ p + T[:3, 3]
        if q[2] <= 0:
            flags.append(False)
            continue
        e = np.hypot(fx * q[0] / q[2] + cx - uo, fy * q[1] / q[2] + cy - vo)
        flags.append(bool(e <= reproj_px))
    return np.array(flags, bool)
