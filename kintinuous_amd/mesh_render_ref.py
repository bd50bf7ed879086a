"""numpy restatement of the rasteriser of the -m mesh (kt_mesh_render.hip, kt_mesh_render / kt_mesh_render_device): the definition the
device equals on every byte, on every call.

The definition (include/kt_abi.h).  Everything is in double unless stated; every product, sum, quotient and conversion is rounded once, in
the order written, nothing contracted; rint rounds ties to even.
  - input: n vertices (16 bytes each), m triangles (uint32[3]), the intrinsics (fx, fy, cx, cy), cols, rows, the camera as
    kt_tracker_get_pose gives it (R camera-to-world, row-major; t the camera centre) and near (float, metres);
  - vertex: d = (double)p - (double)t, c_k = (R[0][k] d.x + R[1][k] d.y) + R[2][k] d.z; valid under kt_mesh_simplify's rule; visible when
    valid, c_z >= near and, with sx = (c_x fx) / c_z + cx and sy likewise, |sx 256| < 2^22 and |sy 256| < 2^22; then X = (int32)rint(sx 256),
    Y likewise, iz = 1.0 / c_z; pixel (i, j) is sampled at X = 256 i, Y = 256 j;
  - triangle: an index >= n and a referenced vertex that is not valid are errors; two equal indices: degenerate; a vertex that is not
    visible: clipped (the whole triangle; there is no clipping); A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) in int64: 0 degenerate,
    negative: vertices 1 and 2 change places; any other triangle is drawn;
  - coverage: w0 = edge(v1, v2, P), w1 = edge(v2, v0, P), w2 = edge(v0, v1, P), edge(a, b, P) = (bx - ax)(Py - ay) - (by - ay)(Px - ax);
    P is inside when every w_k > 0, or w_k = 0 and its edge a -> b is inclusive: by - ay > 0, or by - ay = 0 and bx - ax < 0;
  - depth: S = ((double)w0 iz0 + (double)w1 iz1) + (double)w2 iz2, z = (double)A / S, zq = min((int64)rint(z 65536), 2^32 - 2); the pixel's
    word is the minimum over the covering triangles of zq << 32 | triangle index, all ones when empty;
  - planes: index (0xFFFFFFFF empty); depth uint16 mm = min(65535, (zq 1000 + 32768) >> 16), 0 empty; color rgb24, per channel
    rint(((b0 c0 + b1 c1) + b2 c2) / S) clamped to [0, 255] with b_k = (double)w_k iz_k and red the rgb word's bits 16-23; model rgb24
    grey g = rint(255 (0.2 + 0.8 q)), q = (nrm . c0)^2 / ((nrm . nrm)(c0 . c0)) (0 with a zero denominator), nrm = (c1 - c0) x (c2 - c0)
    of the camera-space vertices, a cross product as (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), a dot product as
    (x x' + y y') + z z'; empty pixels are (0, 0, 0);
  - stats: drawn, clipped and degenerate triangles, covered pixels.
"""
from __future__ import annotations

import numpy as np

from .mesh_holes_ref import valid_vertices
from .mesh_ref import MESH_VERTEX_DTYPE

MAX_VERTICES = 1 << 29
MAX_TRIANGLES = 1 << 29
MAX_SIDE = 8192
NEAR_MIN, NEAR_MAX = 0.001, 8192.0
GUARD = float(1 << 22)                                    # |sx 256| and |sy 256| stay below it
SUB = 256                                                 # sub-pixel steps per pixel
ZQ_MAX = (1 << 32) - 2
EMPTY = np.uint64((1 << 64) - 1)
NO_TRIANGLE = 0xFFFFFFFF
STAT_NAMES = ("drawn_triangles", "clipped_triangles", "degenerate_triangles", "covered_pixels")
_BATCH = 1 << 21                                          # pixels of one vectorised batch


def check_params(intr, cols, rows, R, t, near):
    """((fx, fy, cx, cy) as doubles, R float64 [3, 3], t float64 [3], (double)near) of a valid call"""
    k = np.asarray(intr, np.float32).reshape(4)
    R = np.asarray(R, np.float32).reshape(3, 3)
    t = np.asarray(t, np.float32).reshape(3)
    near = np.float32(near)
    if not (int(cols) == cols and int(rows) == rows and 1 <= cols <= MAX_SIDE and 1 <= rows <= MAX_SIDE):
        raise ValueError("cols and rows lie in [1, 8192]")
    if not (np.isfinite(k).all() and k[0] > 0 and k[1] > 0):
        raise ValueError("the intrinsics are finite, fx and fy positive")
    if not (np.isfinite(R).all() and np.isfinite(t).all() and (np.abs(t) < np.float32(8192.0)).all()):
        raise ValueError("R and t are finite, |t| < 8192")
    if not (np.float32(NEAR_MIN) <= near < np.float32(NEAR_MAX)):
        raise ValueError("near lies in [0.001, 8192)")
    return tuple(float(a) for a in k), R.astype(np.float64), t.astype(np.float64), float(near)


def project(v, k, R, t, near):
    """(valid bool [n], visible bool [n], X int64 [n], Y int64 [n], iz float64 [n], c float64 [n, 3])"""
    fx, fy, cx, cy = k
    with np.errstate(all="ignore"):
        d = v["xyz"].astype(np.float64) - t
        c = np.stack([(R[0, a] * d[:, 0] + R[1, a] * d[:, 1]) + R[2, a] * d[:, 2] for a in range(3)], axis=1)
        valid = valid_vertices(v)
        ax = ((c[:, 0] * fx) / c[:, 2] + cx) * float(SUB)
        ay = ((c[:, 1] * fy) / c[:, 2] + cy) * float(SUB)
        visible = valid & (c[:, 2] >= near) & (np.abs(ax) < GUARD) & (np.abs(ay) < GUARD)
        X = np.rint(np.where(visible, ax, 0.0)).astype(np.int64)
        Y = np.rint(np.where(visible, ay, 0.0)).astype(np.int64)
        iz = np.where(visible, 1.0 / np.where(visible, c[:, 2], 1.0), 0.0)
    return valid, visible, X, Y, iz, c


def setup(v, tri, k, R, t, near):
    """The drawn triangles: (ids int64 [T], corners int64 [T, 3] after the swap, A int64 [T], (clipped, degenerate) counts, the projection)"""
    n = len(v)
    if tri.size and int(tri.max()) >= n:
        raise ValueError("a triangle index out of range")
    pr = project(v, k, R, t, near)
    valid, visible, X, Y = pr[:4]
    idx = tri.astype(np.int64)
    if not valid[idx].all():
        raise ValueError("a triangle's vertex that is not finite or has a coordinate of 8192 m or more")
    equal = (idx[:, 0] == idx[:, 1]) | (idx[:, 1] == idx[:, 2]) | (idx[:, 0] == idx[:, 2])
    seen = visible[idx].all(axis=1)
    clipped = ~equal & ~seen
    x, y = X[idx], Y[idx]
    A = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    drawn = ~equal & seen & (A != 0)
    ids = np.flatnonzero(drawn)
    corners, A = idx[ids], A[ids]
    swap = A < 0
    corners[swap] = corners[swap][:, [0, 2, 1]]
    return ids, corners, np.abs(A), (int(clipped.sum()), int(len(tri) - clipped.sum() - len(ids))), pr


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _inclusive(ax, ay, bx, by):
    return (by - ay > 0) | ((by - ay == 0) & (bx - ax < 0))


def weights(x, y, px, py):
    """(w0, w1, w2 int64, inside bool) of pixels (px, py) against corners x, y int64 [..., 3]; everything broadcasts"""
    PX, PY = px * SUB, py * SUB
    w, inside = [], True
    for a, b in ((1, 2), (2, 0), (0, 1)):
        e = _edge(x[..., a], y[..., a], x[..., b], y[..., b], PX, PY)
        inside = inside & ((e > 0) | ((e == 0) & _inclusive(x[..., a], y[..., a], x[..., b], y[..., b])))
        w.append(e)
    return w[0], w[1], w[2], inside


def covering(corners, X, Y, cols, rows):
    """Every (triangle, pixel) pair of the coverage rule: (row of `corners` int64 [K], pixel j * cols + i int64 [K], w0, w1, w2 int64 [K])"""
    x, y = X[corners], Y[corners]
    x0, x1 = np.maximum(-(-x.min(axis=1) // SUB), 0), np.minimum(x.max(axis=1) // SUB, cols - 1)
    y0, y1 = np.maximum(-(-y.min(axis=1) // SUB), 0), np.minimum(y.max(axis=1) // SUB, rows - 1)
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    live = np.flatnonzero((bw > 0) & (bh > 0))
    out = []

    def batch(rows_, W, H):
        oy, ox = np.mgrid[0:H, 0:W]
        px, py = x0[rows_, None, None] + ox, y0[rows_, None, None] + oy
        w0, w1, w2, inside = weights(x[rows_][:, None, None, :], y[rows_][:, None, None, :], px, py)
        inside &= (px <= x1[rows_, None, None]) & (py <= y1[rows_, None, None])
        r = np.broadcast_to(rows_[:, None, None], inside.shape)
        out.append((r[inside], (py * cols + px)[inside], w0[inside], w1[inside], w2[inside]))

    pw = 1 << np.ceil(np.log2(np.maximum(bw[live], 1))).astype(np.int64)
    ph = 1 << np.ceil(np.log2(np.maximum(bh[live], 1))).astype(np.int64)
    small = (pw <= 32) & (ph <= 32)
    for W, H in sorted(set(zip(pw[small].tolist(), ph[small].tolist()))):
        group = live[small][(pw[small] == W) & (ph[small] == H)]
        step = max(1, _BATCH // (W * H))
        for s in range(0, len(group), step):
            batch(group[s:s + step], W, H)
    for r in live[~small]:
        batch(np.array([r]), int(bw[r]), int(bh[r]))
    if not out:
        z = np.zeros(0, np.int64)
        return z, z, z, z, z
    return tuple(np.concatenate([o[a] for o in out]) for a in range(5))


def _prepare(vertices, triangles, intr, cols, rows, R, t, near):
    v = np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3)
    if len(v) > MAX_VERTICES or len(tri) > MAX_TRIANGLES:
        raise ValueError("n <= 2^29 vertices and m <= 2^29 triangles")
    k, R, t, near = check_params(intr, cols, rows, R, t, near)
    if len(v) == 0:
        tri = tri[:0]
    return v, tri, setup(v, tri, k, R, t, near)


def coverage(vertices, triangles, intr, cols, rows, R, t, near):
    """How many drawn triangles cover each pixel: int64 [rows, cols]"""
    v, tri, (ids, corners, A, _, pr) = _prepare(vertices, triangles, intr, cols, rows, R, t, near)
    _, pix, _, _, _ = covering(corners, pr[2], pr[3], cols, rows)
    return np.bincount(pix, minlength=cols * rows).reshape(rows, cols)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def words(vertices, triangles, intr, cols, rows, R, t, near):
    """(the pixel words uint64 [rows * cols], zq of every (triangle, pixel) pair with its pixel, the set-up)"""
    v, tri, su = _prepare(vertices, triangles, intr, cols, rows, R, t, near)
    ids, corners, A, _, pr = su
    iz = pr[4]
    r, pix, w0, w1, w2 = covering(corners, pr[2], pr[3], cols, rows)
    c = corners[r]
    S = (w0.astype(np.float64) * iz[c[:, 0]] + w1.astype(np.float64) * iz[c[:, 1]]) + w2.astype(np.float64) * iz[c[:, 2]]
    z = A[r].astype(np.float64) / S
    zq = np.minimum(np.rint(z * 65536.0).astype(np.int64), ZQ_MAX)
    word = zq.astype(np.uint64) << np.uint64(32) | ids[r].astype(np.uint64)
    px = np.full(cols * rows, EMPTY, np.uint64)
    np.minimum.at(px, pix, word)
    return px, (zq, pix), (v, tri, su)


def render(vertices, triangles, intr, cols, rows, R, t, near):
    """(index uint32 [rows, cols], depth uint16 [rows, cols], color uint8 [rows, cols, 3], model uint8 [rows, cols, 3], stats: the four of
    STAT_NAMES)"""
    px, _, (v, tri, (ids, corners, A, (clipped, degenerate), pr)) = words(vertices, triangles, intr, cols, rows, R, t, near)
    _, _, X, Y, iz, cam = pr
    index = (px & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    depth = np.zeros(cols * rows, np.uint16)
    color, model = np.zeros((cols * rows, 3), np.uint8), np.zeros((cols * rows, 3), np.uint8)
    p = np.flatnonzero(px != EMPTY)
    if len(p):
        zq = (px[p] >> np.uint64(32)).astype(np.int64)
        depth[p] = np.minimum(65535, (zq * 1000 + 32768) >> 16).astype(np.uint16)
        c = corners[np.searchsorted(ids, index[p].astype(np.int64))]
        w0, w1, w2, inside = weights(X[c], Y[c], p % cols, p // cols)
        assert inside.all()
        b = [w.astype(np.float64) * iz[c[:, a]] for a, w in enumerate((w0, w1, w2))]
        S = (b[0] + b[1]) + b[2]
        for ch, shift in enumerate((16, 8, 0)):
            col = [((v["rgb"][c[:, a]] >> np.uint32(shift)) & np.uint32(255)).astype(np.float64) for a in range(3)]
            color[p, ch] = np.clip(np.rint(((b[0] * col[0] + b[1] * col[1]) + b[2] * col[2]) / S), 0.0, 255.0).astype(np.uint8)
        c0, c1, c2 = cam[c[:, 0]], cam[c[:, 1]], cam[c[:, 2]]
        nrm = _cross(c1 - c0, c2 - c0)
        nc = _dot(nrm, c0)
        den = _dot(nrm, nrm) * _dot(c0, c0)
        with np.errstate(all="ignore"):
            q = np.where(den == 0.0, 0.0, (nc * nc) / np.where(den == 0.0, 1.0, den))
        model[p] = np.clip(np.rint(255.0 * (0.2 + 0.8 * q)), 0.0, 255.0).astype(np.uint8)[:, None]
    stats = (len(ids), clipped, degenerate, len(p))
    return index.reshape(rows, cols), depth.reshape(rows, cols), color.reshape(rows, cols, 3), model.reshape(rows, cols, 3), stats
