"""The ray cast's voxel indexing (csrc/kt_rc_index.hpp, used by kt_raycast_kernel of csrc/kt_raycast.hip): floor-and-convert in one instruction
(v_cvt_flr_i32_f32), the guard band by v_fract_f32, the in-volume test by one compare, and -- for a power-of-two N -- the storage wrap as a mask
and the linear index as shifts.  Every one is an identity of the form it replaced; this module holds them in three ways.

1. `test_value_list` (no GPU): the list of floats the hook is fed, `index_values()`, against numpy -- it contains every class DESIGN.md 4.2 lists
   (every integer of [-4, N + 4] +- 1 ulp, the guard-band edges around them, -0.0, denormals, +-2^23, +-2^24, +-2^31, infinities, NaN of both
   signs, 10^5 random floats), the subtraction q - floor(q) and min(q - floor(q), 1 - 2^-24) (what v_fract_f32 returns) give the same guard
   decision on all of them, and mask / shift equal conditional subtraction / multiply for every (w, N) of the list.
2. `test_hook_old_equals_new` (GPU): the hook kt_debug_rc_index (csrc/kt_measure.h) runs the kernel's own helpers next to the former forms on
   that list for N in {64, 96, 256, 512, 768}: equal voxels, equal guard decisions, equal in-volume flags, elements, tap offsets, indices.  One
   class is not an identity and is pinned as such: a NaN converts to +-(2^31 - 1) in one instruction and to 0 through the pair, which is why
   the kernel's guards must -- and here do -- turn every NaN down (the former march guard let a NaN coordinate through; the present one does not).
3. `test_raycast_equals_oracle` (GPU): 40 x 24 images (ragged against the 16 x 16 tile) of volumes the voxel kernel filled, 64^3 (power-of-two
   path, 2^3 bricks) and 96^3 (general path, 3^3 bricks), under the storage wraps (N - 1, 0, N / 2 + 1) and (1, N - 1, N - 1) -- every axis wraps
   inside a trilinear cell and inside a brick --: vmap, nmap, colour image and S equal to the oracle's bit for bit, with and without hops, and
   the number of samples the hops replaced equal to what the kernel before this change counted (tests/golden/raycast_index_hops.json).
   `test_case_conditions` (no GPU) asserts with the oracle alone that the committed poses give every group of cases hits and misses, rays
   leaving through each of the six faces, and hits in the outermost voxel layers that get no normal (the `hx > 1 && ... < N - 2` edge); the
   GPU test asserts that every group hops.
"""
import functools
import json
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
f32 = np.float32
GUARD = f32(2e-4)
NS = [64, 96, 256, 512, 768]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOPS_GOLDEN = os.path.join(ROOT, "tests", "golden", "raycast_index_hops.json")


# ---- the value list ----------------------------------------------------------------------------------------------------------------------------
def _nan(bits):
    return np.array([bits], np.uint32).view(f32)[0]


@functools.lru_cache(maxsize=None)
def index_values():
    """float32 array: the classes of module docstring item 1, in that order; the last 10^5 are random"""
    up, dn = f32(np.inf), f32(-np.inf)
    ints = np.arange(-4, max(NS) + 5, dtype=f32)
    out = []
    for base in (ints, ints + GUARD, ints - GUARD, ints + (f32(1) - GUARD)):
        out += [base, np.nextafter(base, up), np.nextafter(base, dn)]
    tiny = f32(1.1754944e-38)
    special = [-0.0, 0.0, 1e-45, -1e-45, 1e-39, -1e-39, tiny, -tiny, -1e-30, 1e-30, -6e-8, -2.9e-8, -3.1e-8, 2.0 ** 23, -2.0 ** 23, 2.0 ** 23 + 1, -2.0 ** 23 - 1,
               2.0 ** 24, -2.0 ** 24, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 128, -2.0 ** 31 + 128, 2.0 ** 31 + 256, -2.0 ** 31 - 256, 3e38, -3e38, np.inf, -np.inf,
               1023.5, -1023.5, 1024.0, -1024.0, 1024.5, -1024.5]
    out.append(np.array(special, f32))
    out.append(np.array([_nan(0x7fc00000), _nan(0xffc00000), _nan(0x7fffffff), _nan(0xff800001), _nan(0x7f800001)], f32))
    rng = np.random.default_rng(20)
    bits = rng.integers(0, 2 ** 32, 30000, dtype=np.uint64).astype(np.uint32).view(f32)
    out += [rng.uniform(-8, max(NS) + 8, 50000).astype(f32), rng.uniform(-1, 1, 10000).astype(f32), rng.normal(0, 3e3, 10000).astype(f32), bits]
    v = np.concatenate(out)
    v.setflags(write=False)
    return v


def wn_pairs(N):
    return [(w, N) for w in (0, 1, 31, 33, N // 2 + 1, N - 1)]


def _cvt_i32(x):
    """v_cvt_i32_f32 of an integer-valued float: saturates, NaN -> 0"""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 0, np.clip(x, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def _guards(q):
    """(guard of one coordinate from the float32 subtraction, the same from v_fract_f32's value) -- numpy restatements"""
    with np.errstate(invalid="ignore"):
        fr = (q - np.floor(q)).astype(f32)
        fract = np.minimum(fr, np.nextafter(f32(1), f32(0)))
        lo, hi = GUARD, f32(1) - GUARD
        return (fr > lo) & (fr < hi) & (np.abs(q) < 1024), (fract > lo) & (fract < hi) & (np.abs(q) < 1024), fr


def _guard3(q, fract=True):
    """the march's guard of the coordinates (q[i], q[i + 1], q[i + 2]) as the kernel forms it: the largest |fraction - 0.5| against 0.5 - 2e-4,
    the largest |q| against 1024; a NaN coordinate fails it"""
    with np.errstate(invalid="ignore"):
        fr = (q - np.floor(q)).astype(f32)
        if fract:
            fr = np.minimum(fr, np.nextafter(f32(1), f32(0)))
        d = np.abs(fr - f32(0.5))
        d = np.where(np.isnan(q), 0, d)          # (a NaN fraction drops out of the first maximum ...)
        off = np.maximum(np.maximum(d, np.roll(d, -1)), np.roll(d, -2))
        big = np.maximum(np.maximum(np.abs(q), np.roll(np.abs(q), -1)), np.roll(np.abs(q), -2))   # (... and stays in the second)
        return (off < f32(0.5) - GUARD) & (big < 1024)


def test_value_list():
    q = index_values()
    assert q.dtype == f32 and q.size > 100000
    bits = q.view(np.uint32)
    with np.errstate(invalid="ignore"):
        fl = np.floor(q)
    # the classes
    for N in NS:
        k = np.arange(-4, N + 5, dtype=f32)
        for want in (k, np.nextafter(k, f32(np.inf)), np.nextafter(k, f32(-np.inf)), k + GUARD, k - GUARD, np.nextafter(k + GUARD, f32(np.inf)),
                     np.nextafter(k - GUARD, f32(-np.inf))):
            assert np.isin(want.view(np.uint32), bits).all(), N
    assert (bits == 0x80000000).any() and (bits == 0).any()
    den = (np.abs(q) > 0) & (np.abs(q) < f32(1.1754944e-38))
    assert (den & (q > 0)).any() and (den & (q < 0)).any()
    for v in (2.0 ** 23, 2.0 ** 24, 2.0 ** 31):
        assert (q == f32(v)).any() and (q == f32(-v)).any()
    assert np.isposinf(q).any() and np.isneginf(q).any()
    nan = np.isnan(q)
    assert (nan & (bits >> 31 == 0)).any() and (nan & (bits >> 31 == 1)).any()
    assert q.size - 100000 > 0 and np.isfinite(q[-100000:-30000]).all()
    # the guard: subtraction and v_fract_f32 decide alike; the list has members on both sides of both edges, and members whose subtraction rounds to 1.0
    old, new, fr = _guards(q)
    assert np.array_equal(old, new) and np.array_equal(_guard3(q, False), _guard3(q, True))
    assert (fr == 1).any() and old.sum() > 50000 and (~old).sum() > 10000
    near = np.abs(fr - GUARD) < 1e-6
    assert (near & old).any() and (near & ~old & np.isfinite(q)).any()
    near = np.abs(fr - (f32(1) - GUARD)) < 1e-6
    assert (near & old).any() and (near & ~old & np.isfinite(q)).any()
    # floor then truncating convert == floor-convert wherever floor(q) is representable: nothing to compute in numpy but the pair itself
    g = _cvt_i32(fl)
    assert g[np.flatnonzero(bits == 0x80000000)[0]] == 0 and (g[den & (q < 0)] == -1).all() and (g[np.isposinf(q)] == 2 ** 31 - 1).all()
    # the integer side: mask == conditional subtraction, shifts == multiplies, one compare == three, for u < N (and the one compare for any u)
    for N in NS:
        u = np.arange(N, dtype=np.int64)
        anyu = np.concatenate([np.arange(-8, N + 8), np.array([2 ** 31 - 1, -2 ** 31, 2 ** 24, -2 ** 24])]) & 0xffffffff
        for (w, _) in wn_pairs(N):
            X = u + w
            X = X - np.where(X >= N, N, 0)
            assert np.array_equal(X, (u + w) % N)
            if N & (N - 1) == 0:
                k = N.bit_length() - 1
                assert np.array_equal(X, (u + w) & (N - 1))
                assert np.array_equal((X[:, None] * N + X[None, :]) * N + X[0], (((X[:, None] << k) | X[None, :]) << k) | X[0])
        three = (anyu[:, None] < N) & (anyu[None, :] < N)
        if N & (N - 1) == 0:
            assert np.array_equal(three, (anyu[:, None] | anyu[None, :]) < N)
        assert np.array_equal(three, np.maximum(anyu[:, None], anyu[None, :]) < N)


# ---- the hook ----------------------------------------------------------------------------------------------------------------------------------
W_VOXEL, W_SAFE1, W_SAFE3, W_INSIDE, W_ELEM, W_INBOUNDS, W_TAP_Z, W_TAP_Y, W_INDEX, W_BRICK = range(10)


@gpu
@pytest.mark.parametrize("N", NS)
def test_hook_old_equals_new(ctx, N):
    q = index_values()
    pairs = wn_pairs(N)
    old, new = ctx.rc_index(q, pairs)
    n = q.size
    nan = np.isnan(q)
    nan3 = nan | np.roll(nan, -1) | np.roll(nan, -2)          # a NaN among the three coordinates of thread i
    with np.errstate(invalid="ignore"):
        g = _cvt_i32(np.floor(q))
    guard_old, guard_new, _ = _guards(q)
    for p, (w, _) in enumerate(pairs):
        o, e = old[p].astype(np.int64), new[p].astype(np.int64)
        msg = f"N={N} w={w}"
        # the voxel: the pair is numpy's floor, saturated; one instruction gives the same for everything but a NaN, which saturates by its sign
        assert np.array_equal(old[p][:, W_VOXEL].view(np.int32), g.astype(np.int32)), msg
        assert np.array_equal(o[~nan, W_VOXEL], e[~nan, W_VOXEL]), msg
        sign = q.view(np.uint32)[nan] >> 31
        assert np.array_equal(new[p][nan, W_VOXEL].view(np.int32), np.where(sign == 1, -2 ** 31, 2 ** 31 - 1).astype(np.int32)), msg
        # ... so no NaN may pass a guard
        assert not e[nan, W_SAFE1].any() and not e[nan3, W_SAFE3].any(), msg
        # the guards: equal decisions (and numpy's); the march's differs by design where a coordinate is a NaN, and only there
        assert np.array_equal(o[:, W_SAFE1], e[:, W_SAFE1]) and np.array_equal(o[:, W_SAFE1], guard_old.astype(np.int64)), msg
        assert np.array_equal(e[:, W_SAFE1], guard_new.astype(np.int64)), msg
        assert np.array_equal(o[~nan3, W_SAFE3], e[~nan3, W_SAFE3]), msg
        assert np.array_equal(e[:, W_SAFE3], _guard3(q).astype(np.int64)), msg
        assert e[:, W_SAFE3].sum() > 1000 and (e[:, W_SAFE3] == 0).sum() > 1000, msg
        # the integer side, wherever the voxels are equal (no NaN among the three)
        ok = ~nan3
        for word in (W_INSIDE, W_ELEM, W_TAP_Z, W_TAP_Y, W_INDEX, W_BRICK):
            bad = o[ok, word] != e[ok, word]
            assert not bad.any(), f"{msg} word {word}: {int(bad.sum())} differ, first at q = {q[ok][bad][:3]}"
        assert e[:, W_INBOUNDS].all(), msg     # the march's load stays inside the volume for ANY coordinates, NaN included
        # ... and numpy's own arithmetic for the in-volume flag and the element
        gx, gy, gz = g, np.roll(g, -1), np.roll(g, -2)
        inside = (gx >= 0) & (gx < N) & (gy >= 0) & (gy < N) & (gz >= 0) & (gz < N)
        wr = (w, N - 1 - w, (w + N // 2 + 1) % N)
        elem = (((gz + wr[2]) % N) * N + (gy + wr[1]) % N) * N + (gx + wr[0]) % N
        assert np.array_equal(e[ok, W_INSIDE], inside[ok].astype(np.int64)), msg
        assert np.array_equal(e[ok, W_ELEM], np.where(inside, elem, 0)[ok]), msg
        assert inside[ok].sum() > 1000, msg
    assert n == old.shape[1]


# ---- ray cast cases ----------------------------------------------------------------------------------------------------------------------------
SIZE = 6.0
COLS, ROWS = 40, 24


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


# camera-to-world rotations whose optical axis (camera +z) points along +x, -x, +y, -y, +z, -z
_DIRS = {"+x": _rot(1, np.pi / 2), "-x": _rot(1, -np.pi / 2), "+y": _rot(0, -np.pi / 2), "-y": _rot(0, np.pi / 2), "+z": np.eye(3), "-z": _rot(1, np.pi)}


def _trunc(N):
    return max(0.06, 2.1 * SIZE / N)


def wraps(N):
    return [[N - 1, 0, N // 2 + 1], [1, N - 1, N - 1]]


@functools.lru_cache(maxsize=None)
def _frames(kind, N):
    """[(cam, depth, rgb, R, t)] of the 160 x 120 frames a volume is fused from.
    'room': the synthetic room (far wall, sphere, cube) through a lens of half the field of view, twice, from poses that put everything it sees
    into the octant x, y, z > 3.4 m -- one brick of the 2^3 at 64^3 -- so that the other bricks stay unflagged and rays hop.  'edge': two flat walls square to yawed cameras of the same lens, 1.7 voxels inside the z = N and the x = 0 faces:
    zero crossings in the outermost two voxel layers."""
    from kintinuous_amd import synth
    cam = synth.Camera.small(160, 120)
    c = np.full(3, SIZE / 2)
    out = []
    if kind == "room":
        scene = synth.Scene("room")
        tele = synth.Camera(cam.cols, cam.rows, 2 * cam.fx, 2 * cam.fy, cam.cx, cam.cy)
        at = np.array([4.5, 4.6, 3.15])                   # where the scene's origin sits in the volume
        for R, pos in ((np.eye(3), np.zeros(3)), (_rot(1, 0.06), np.array([0.08, 0.03, 0.0]))):
            depth, rgb = synth.render(scene, tele, R, pos)
            out.append((tele, depth, rgb, R.astype(f32), (pos + at).astype(f32)))
    else:
        cell = SIZE / N
        rng = np.random.default_rng(9)
        rgb = rng.integers(0, 256, (cam.rows, cam.cols, 3)).astype(np.uint8)
        cam = synth.Camera(cam.cols, cam.rows, 2 * cam.fx, 2 * cam.fy, cam.cx, cam.cy)   # (narrow: each wall stays inside one octant)
        for d, yaw, pos in (("+z", 0.12, np.array([4.3, 4.3, 3.0])), ("-x", -0.1, np.array([3.0, 4.3, 4.4]))):
            R = _DIRS[d] @ _rot(1, yaw)
            axis = R[:, 2]                                # the wall is the plane through `anchor` square to the optical axis
            anchor = pos.copy()
            if d == "+z":
                anchor[2] = SIZE - 1.7 * cell
            else:
                anchor[0] = 1.7 * cell
            dist = float((anchor - pos) @ axis)
            depth = np.full((cam.rows, cam.cols), int(round(dist * 1000)), np.uint16)
            out.append((cam, depth, rgb, R.astype(f32), pos.astype(f32)))
    return out


def _nmap_of(oracle, cam, depth):
    from oracle.oracle import OIntr
    return oracle.create_nmap(oracle.create_vmap(OIntr(cam.fx, cam.fy, cam.cx, cam.cy), oracle.bilateral_filter(depth)))


_REF_VOL = {}


def _ref_volume(oracle, kind, N, wrap):
    """the volume of a case fused by the oracle (the device's must equal it)"""
    from oracle.oracle import OIntr
    key = (kind, N, tuple(wrap))
    if key not in _REF_VOL:
        vol, col = np.zeros((N, N, N), np.int16), np.zeros((N, N, N, 4), np.uint8)
        for (cam, depth, rgb, R, t) in _frames(kind, N):
            oracle.integrate_tsdf(depth, OIntr(cam.fx, cam.fy, cam.cx, cam.cy), [SIZE] * 3, oracle.mat33_inverse(R), t, _trunc(N), vol, wrap, col, rgb,
                                  _nmap_of(oracle, cam, depth), True)
        vol.setflags(write=False)
        col.setflags(write=False)
        _REF_VOL[key] = (vol, col)
    return _REF_VOL[key]


def _dev_volume(ctx, oracle, kind, N, wrap):
    """the same frames through the voxel kernel with the brick flags handed on: device buffers (volume, colour volume, flags) and host copies"""
    from kintinuous_amd.abi import Intr
    nb = N // 32
    dvol, dcol, dfl = ctx.upload(np.zeros((N, N, N), np.int16)), ctx.upload(np.zeros((N, N, N, 4), np.uint8)), ctx.upload(np.zeros(nb ** 3, np.uint8))
    for (cam, depth, rgb, R, t) in _frames(kind, N):
        ctx.integrate_tsdf_bricks(ctx.upload(depth), cam.cols, cam.rows, Intr(cam.fx, cam.fy, cam.cx, cam.cy), [SIZE] * 3, oracle.mat33_inverse(R), t, _trunc(N),
                                  dvol, ctx.empty(depth.size * 4), wrap, dcol, ctx.upload(rgb), ctx.upload(_nmap_of(oracle, cam, depth)), True, N, dfl)
    ctx.sync()
    return dvol, dcol, dfl, ctx.download(dvol, np.int16, (N, N, N)), ctx.download(dcol, np.uint8, (N, N, N, 4)), ctx.download(dfl, np.uint8, (nb, nb, nb))


def _look_at(eye, target):
    """camera-to-world rotation with the optical axis (camera +z) along target - eye"""
    fwd = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([0.0, 0.0, 1.0])
    right = np.cross(up, fwd)
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(fwd, right), fwd], 1)


def cases(kind):
    """[(group, name, R, t)]: cameras of the 40 x 24 casts"""
    out = []
    if kind == "room":
        eye = np.array([1.4, 1.6, 1.3])                   # in the low octant: its bricks hold nothing
        # towards +x and +y past the fused surfaces, towards +z into them; towards -x, -y, -z nothing but the low faces
        aims = {"+x": [6.0, 3.9, 3.6], "-x": [0.0, 1.2, 1.0], "+y": [3.8, 6.0, 3.7], "-y": [1.1, 0.0, 0.9], "+z": [4.5, 4.6, 5.9], "-z": [1.0, 1.3, 0.0]}
        for d, aim in aims.items():
            e = np.array([4.1, 4.2, 1.8]) if d == "+z" else eye   # (+z: from behind the fusing camera, through the unflagged brick under it)
            out.append(("faces", d, _look_at(e, np.array(aim)), e))
        for name, eye2, aim in (("through z = 0", [3.9, 4.0, -0.45], [4.5, 4.6, 5.6]), ("past the x = N, z = 0 edge", [6.4, 4.4, -0.3], [4.4, 4.6, 5.4])):
            out.append(("outside", name, _look_at(np.array(eye2), np.array(aim)), np.array(eye2)))
    else:
        for name, eye2, aim in (("z = N wall", [4.25, 4.35, 1.6], [4.4, 4.2, 6.0]), ("x = 0 wall", [4.0, 2.6, 4.4], [0.0, 4.4, 4.4])):
            out.append(("edge", name, _look_at(np.array(eye2), np.array(aim)), np.array(eye2)))
    return [(g, n, R.astype(f32), t.astype(f32)) for (g, n, R, t) in out]


def _intr():
    from kintinuous_amd import synth
    cam = synth.Camera.small(COLS, ROWS)
    return (cam.fx, cam.fy, cam.cx, cam.cy)


def _prefill():
    rng = np.random.default_rng(3)
    return (rng.uniform(-1, 1, (3 * ROWS, COLS)).astype(f32), rng.uniform(-1, 1, (3 * ROWS, COLS)).astype(f32), rng.integers(0, 255, (ROWS, COLS, 4)).astype(np.uint8))


_ORACLE_CAST = {}


def _oracle_cast(oracle, key, vol, col, N, wrap, R, t):
    from oracle.oracle import OIntr
    if key not in _ORACLE_CAST:
        v, n, c = (a.copy() for a in _prefill())
        S = oracle.raycast(OIntr(*_intr()), R, t, _trunc(N), [SIZE] * 3, np.ascontiguousarray(vol), v, n, wrap, c, np.ascontiguousarray(col))
        for a in (v, n, c):
            a.setflags(write=False)
        _ORACLE_CAST[key] = (v, n, c, S)
    return _ORACLE_CAST[key]


def _exit_faces(R, t):
    """per pixel: the face (0..5 = x lo, x hi, y lo, y hi, z lo, z hi) through which the pixel's ray leaves the volume (geometry only, float64)"""
    fx, fy, cx, cy = _intr()
    x, y = np.meshgrid(np.arange(COLS, dtype=np.float64), np.arange(ROWS, dtype=np.float64))
    d = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1) @ np.asarray(R, np.float64).T
    with np.errstate(divide="ignore"):
        tx = (np.where(d > 0, SIZE, 0.0) - np.asarray(t, np.float64)) / d
    ax = np.argmin(tx, -1)
    return 2 * ax + (np.take_along_axis(d, ax[..., None], -1)[..., 0] > 0)


ALL = [(kind, N) for N in (64, 96) for kind in ("room", "edge")]


def test_case_conditions(oracle_mod):
    """With the oracle alone: every group of cases has hits and misses (S > 0); the misses of the 'faces' group leave through all six faces; the
    'outside' cameras start outside the volume; the 'edge' group has hits without a normal (the crossing lies in the outermost two layers) and
    hits with one."""
    for kind, N in ALL:
        for wrap in wraps(N):
            vol, col = _ref_volume(oracle_mod, kind, N, wrap)
            assert (vol < 0).any()
            groups = {}
            for (group, name, R, t) in cases(kind):
                v, n, c, S = _oracle_cast(oracle_mod, (kind, N, tuple(wrap), name), vol, col, N, wrap, R, t)
                hit = np.isfinite(v[:ROWS])
                g = groups.setdefault(group, {"hits": 0, "misses": 0, "S": 0, "faces": np.zeros(6, int), "bare": 0, "normals": 0})
                g["hits"] += int(hit.sum())
                g["misses"] += int((~hit).sum())
                g["S"] += S
                g["faces"] += np.bincount(_exit_faces(R, t)[~hit], minlength=6)
                g["bare"] += int((hit & np.isnan(n[:ROWS])).sum())
                g["normals"] += int((hit & np.isfinite(n[:ROWS])).sum())
                assert S > ROWS * COLS, (kind, N, wrap, name, S)
                if group == "outside":
                    assert (t < 0).any()
            for group, g in groups.items():
                msg = f"{kind} N={N} wrap={wrap} {group}: {g}"
                assert g["hits"] >= 25 and g["misses"] >= 40, msg
                if group == "faces":
                    assert (g["faces"] >= 5).all(), msg
                if group == "edge":
                    assert g["bare"] >= 10 and g["normals"] >= 20, msg


def _bits_differ(a, b):
    return (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))   # (NaN words: tests/test_gpu_bricks.py _bits_differ)


def _cast_dev(ctx, dvol, dcol, N, wrap, R, t, dflags):
    from kintinuous_amd.abi import Intr
    v0, n0, c0 = _prefill()
    dv, dn, dc = ctx.upload(v0), ctx.upload(n0), ctx.upload(c0)
    counts = ctx.raycast_bricks(Intr(*_intr()), R, t, _trunc(N), [SIZE] * 3, dvol, dv, dn, COLS, ROWS, wrap, dc, dcol, N, dflags)
    return ctx.download(dv, f32, v0.shape), ctx.download(dn, f32, n0.shape), ctx.download(dc, np.uint8, c0.shape), counts


def run_cases(ctx, oracle, kind, N, check=True):
    """{case key: samples replaced by hops}; with check, every output against the oracle's"""
    hops = {}
    for wrap in wraps(N):
        rvol, rcol = _ref_volume(oracle, kind, N, wrap)
        dvol, dcol, dfl, gvol, gcol, flags = _dev_volume(ctx, oracle, kind, N, wrap)
        assert np.array_equal(gvol, rvol) and np.array_equal(gcol, rcol), (kind, N, wrap)
        assert flags.any() and not flags.all(), (kind, N, wrap, flags.ravel().tolist())
        group_hops = {}
        for (group, name, R, t) in cases(kind):
            key = f"{kind}/N={N}/wrap={wrap}/{name}"
            ref = _oracle_cast(oracle, (kind, N, tuple(wrap), name), rvol, rcol, N, wrap, R, t)
            for skip in (False, True):
                gv, gn, gc, (S, hopped, hop_iters, batch_iters) = _cast_dev(ctx, dvol, dcol, N, wrap, R, t, dfl if skip else None)
                if skip:
                    hops[key] = hopped
                    group_hops[group] = group_hops.get(group, 0) + hopped
                if not check:
                    continue
                msg = f"{key} {'SKIP' if skip else 'no-SKIP'}"
                assert not _bits_differ(ref[0], gv).any(), f"{msg}: vertex map"
                assert not _bits_differ(ref[1], gn).any(), f"{msg}: normal map"
                assert np.array_equal(ref[2], gc), f"{msg}: colour image"
                assert S == ref[3], f"{msg}: S {S} vs the oracle's {ref[3]}"
                assert (hopped > 0 and hop_iters > 0) if skip and hopped else hopped == 0, msg
                assert hopped <= S
        for group, h in group_hops.items():
            assert h > 0, f"{kind} N={N} wrap={wrap} {group}: no sample was replaced by a hop"
    return hops


@gpu
@pytest.mark.parametrize("kind,N", ALL)
def test_raycast_equals_oracle(ctx, oracle_mod, kind, N):
    hops = run_cases(ctx, oracle_mod, kind, N)
    golden = json.load(open(HOPS_GOLDEN))
    for key, h in hops.items():
        assert golden[key] == h, f"{key}: {h} samples replaced by hops, {golden[key]} before the indexing change"
