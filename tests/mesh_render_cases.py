"""Cases shared by the rasteriser's CPU and GPU tests (test_mesh_render_ref.py, test_gpu_mesh_render.py): named scenes of a few triangles
built so that their image positions are exact multiples of 1 / 256 px (an image-filling triangle that reaches far outside the image, a
sub-pixel triangle between centres, triangles on pixel centres, a rectangle of four triangles, a closed fan, duplicates, two depth layers,
every kind of rejected triangle, vertices near the coordinate bound, a sweep of box sizes across the kernels' small / large threshold),
the N = 32 marching-cubes sphere from inside and outside, and a random soup of 4099 small triangles with its shuffle."""
import functools

import numpy as np

import mesh_normals_cases as nc
from kintinuous_amd import mesh_ref, mesh_render_ref as ref

V = mesh_ref.MESH_VERTEX_DTYPE
IMAGES = ((1, 1), (7, 5), (67, 43), (160, 120))
SMALL = 4                                       # KT_REN_SMALL of kt_mesh_render.hip: a box of at most 4 px each way is drawn by one lane
NEAR = 0.05
I3 = np.eye(3, dtype=np.float32)
ZERO = np.zeros(3, np.float32)
FAR_OFFSET = (8000.0, -8000.0, 7998.0)
PLANES = ("index", "depth", "color", "model")


def intr_of(cols, rows, f=64.0):
    """(fx, fy, cx, cy): a power-of-two focal length and an integer principal point, so that x = (sx - cx) z / f is exact for small sx, z"""
    return (f, f, float(cols // 2), float(rows // 2))


def at_pixels(sxy, z, intr, rgb=None):
    """vertices whose images are exactly sxy (pixels, multiples of 1 / 256) at depths z (powers of two or small dyadic numbers), with the
    camera at the origin looking along +z"""
    sxy = np.asarray(sxy, np.float64).reshape(-1, 2)
    z = np.broadcast_to(np.asarray(z, np.float64), (len(sxy),))
    v = np.zeros(len(sxy), V)
    x, y = (sxy[:, 0] - intr[2]) * z / intr[0], (sxy[:, 1] - intr[3]) * z / intr[1]
    v["xyz"] = np.stack([x, y, z], axis=1).astype(np.float32)
    assert np.array_equal(v["xyz"].astype(np.float64), np.stack([x, y, z], axis=1))           # exact in float
    v["rgb"] = (np.arange(len(v), dtype=np.uint32) * np.uint32(2654435761)) & np.uint32(0xFFFFFF) if rgb is None else rgb
    return v


def scene(v, tri, cols, rows, intr=None, R=I3, t=ZERO, near=NEAR):
    return dict(v=v, tri=np.asarray(tri, np.uint32).reshape(-1, 3), intr=intr_of(cols, rows) if intr is None else intr, cols=cols, rows=rows,
                R=np.asarray(R, np.float32), t=np.asarray(t, np.float32), near=near)


def fill_case(cols, rows):
    """one triangle over the whole image and far outside it, inside the guard band of 16384 px, at three depths"""
    k = intr_of(cols, rows)
    return scene(at_pixels([(-3000, -2000), (9000, -2500), (-1000, 7000)], (1.0, 2.0, 4.0), k, rgb=[0xFF0000, 0x00FF00, 0x0000FF]), [[0, 1, 2]], cols, rows, k)


def subpixel_case():
    k = intr_of(67, 43)
    return scene(at_pixels([(10.25, 7.25), (10.75, 7.25), (10.5, 7.75)], 2.0, k), [[0, 1, 2]], 67, 43, k)


def centres_case(cols, rows):
    """every vertex on a pixel centre; one edge along a row of centres, one along a column, one through centres on the diagonal"""
    k = intr_of(cols, rows)
    a = min(cols, rows) - 2
    return scene(at_pixels([(1, 1), (1 + a, 1), (1, 1 + a)], 2.0, k), [[0, 1, 2]], cols, rows, k)


RECT = (5.0, 4.0, 23.0, 40.0, 30.0)             # x of the left edge, y of the top edge, x of the shared vertical edge, x right, y bottom: all on centres


def rectangle_case():
    """a fronto-parallel rectangle at z = 2 m of two quads that share a vertical edge, each of two triangles that share a diagonal"""
    k = intr_of(67, 43)
    xa, ya, xm, xb, yb = RECT
    v = at_pixels([(xa, ya), (xm, ya), (xb, ya), (xa, yb), (xm, yb), (xb, yb)], 2.0, k)
    return scene(v, [[0, 1, 4], [0, 4, 3], [1, 2, 5], [5, 4, 1]], 67, 43, k)


FAN_HUB = (33.0, 21.0)
FAN_RIM = ((52.0, 21.0), (45.5, 33.25), (33.0, 38.0), (20.125, 30.5), (14.0, 21.0), (22.75, 8.5), (33.0, 3.0), (46.0, 9.0))


def fan_case(offset=(0.0, 0.0, 0.0)):
    """a closed fan around a hub on a pixel centre, some spokes along rows, columns and diagonals of centres; `offset` moves the scene
    and the camera"""
    k = intr_of(67, 43)
    v = at_pixels((FAN_HUB,) + FAN_RIM, (2.0,) + (2.0, 2.5, 2.0, 3.0, 2.0, 1.5, 2.0, 2.5), k)
    n = len(FAN_RIM)
    tri = [[0, 1 + i, 1 + (i + 1) % n] for i in range(n)]
    tri[2], tri[5] = tri[2][::-1], tri[5][::-1]             # two of them wound the other way
    v["xyz"] = (v["xyz"].astype(np.float64) + np.asarray(offset)).astype(np.float32)
    return scene(v, tri, 67, 43, k, t=np.asarray(offset, np.float32))


def twice_case():
    k = intr_of(67, 43)
    return scene(at_pixels([(3.5, 2.25), (60.0, 10.0), (20.0, 41.5)], (1.0, 2.0, 1.5), k), [[0, 1, 2], [0, 1, 2], [0, 2, 1]], 67, 43, k)


def layers_case(gap):
    """two overlapping triangles `gap` metres apart, the far one first"""
    k = intr_of(67, 43)
    back = at_pixels([(2.0, 2.0), (64.0, 3.0), (30.0, 41.0)], 2.0, k)
    front = at_pixels([(10.0, 40.0), (66.0, 30.0), (34.5, 1.0)], 2.0, k)
    back["xyz"] = (back["xyz"].astype(np.float64) * ((2.0 + gap) / 2.0)).astype(np.float32)     # the same image, farther away
    return scene(np.concatenate([back, front]), [[0, 1, 2], [3, 4, 5]], 67, 43, k)


def rejects_case():
    """one triangle behind the camera, one across `near`, one beyond the guard band, one with two equal indices, one with three collinear
    vertices, and one that is drawn"""
    k = intr_of(67, 43)
    v = at_pixels([(10, 10), (50, 12), (30, 40),                       # drawn
                   (1, 1), (2, 2), (3, 3),                             # collinear, on centres
                   (20, 20), (40, 20), (30, 30),                       # 6-8: across near (8 moved below)
                   (30, 5), (20000, 5), (30, 25)], 2.0, k)             # 9-11: 10 lies beyond the guard band
    behind = v[:3].copy()
    behind["xyz"][:, 2] = -1.0
    v["xyz"][8] = (0.0, 0.0, 0.03125)
    return scene(np.concatenate([v, behind]), [[12, 13, 14], [6, 7, 8], [9, 10, 11], [0, 1, 1], [3, 4, 5], [0, 1, 2]], 67, 43, k)


SWEEP = tuple((w, h) for h in range(1, SMALL + 3) for w in range(1, SMALL + 3))


def sweep_case():
    """a triangle for every box of 1 .. SMALL + 2 pixels each way, its own cell of 12 x 12 px in a 160 x 120 image"""
    k = intr_of(160, 120)
    pts, tri = [], []
    for w, h in SWEEP:
        x0, y0 = 3 + 12 * (w - 1), 3 + 12 * (h - 1)
        pts += [(x0 - 0.25, y0 - 0.25), (x0 + w - 1 + 0.25, y0 - 0.125), (x0 - 0.125, y0 + h - 1 + 0.25)]
        tri.append([len(pts) - 3, len(pts) - 2, len(pts) - 1])
    return scene(at_pixels(pts, 2.0, k), tri, 160, 120, k)


def look_at(centre, distance, yaw):
    """(R camera-to-world, t): a camera `distance` from `centre`, turned by `yaw` about y, looking at it"""
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    return R, (np.asarray(centre) - distance * R[:, 2].astype(np.float64)).astype(np.float32)


SPHERE_INTR = (100.0, 100.0, 79.5, 59.5)


def sphere_case(outside):
    v, tri = nc.sphere_mesh()
    R, t = look_at(nc.SPHERE_CENTRE, 3.0 if outside else 0.0, 0.3)
    return scene(v.copy(), tri.copy(), 160, 120, SPHERE_INTR, R, t)


@functools.lru_cache(maxsize=None)
def _soup():
    rng = np.random.default_rng(4099)
    m = 4099
    k = intr_of(160, 120)
    centre = rng.uniform((-6, -6), (166, 126), (m, 1, 2))
    sxy = np.round((centre + rng.uniform(-2.5, 2.5, (m, 3, 2))) * 256) / 256
    z = 2.0 ** rng.integers(0, 3, (m, 3)).astype(np.float64) * rng.integers(4, 8, (m, 3)) / 4.0
    v = at_pixels(sxy.reshape(-1, 2), z.reshape(-1), k, rgb=rng.integers(0, 1 << 24, 3 * m).astype(np.uint32))
    return v, np.arange(3 * m, dtype=np.uint32).reshape(m, 3), rng.permutation(m)


def soup_case(shuffled):
    v, tri, perm = _soup()
    return scene(v.copy(), tri[perm] if shuffled else tri.copy(), 160, 120)


SOUP_PERMUTATION = lambda: _soup()[2]

CASES = {"subpixel": subpixel_case, "rectangle": rectangle_case, "fan": fan_case, "twice": twice_case, "layers 1 cm": lambda: layers_case(0.01),
         "layers 1 m": lambda: layers_case(1.0), "rejects": rejects_case, "far": lambda: fan_case(FAR_OFFSET), "sweep": sweep_case,
         "sphere inside": lambda: sphere_case(False), "sphere outside": lambda: sphere_case(True), "soup": lambda: soup_case(False),
         "soup shuffled": lambda: soup_case(True)}
for _c, _r in IMAGES:
    CASES["fill %dx%d" % (_c, _r)] = functools.partial(fill_case, _c, _r)
    if min(_c, _r) >= 5:
        CASES["centres %dx%d" % (_c, _r)] = functools.partial(centres_case, _c, _r)


def names():
    return sorted(CASES)


def case(name):
    return CASES[name]()


def args(s):
    """a scene as the restatement's arguments"""
    return s["v"], s["tri"], s["intr"], s["cols"], s["rows"], s["R"], s["t"], s["near"]


@functools.lru_cache(maxsize=None)
def want(name):
    """the restatement's (index, depth, color, model, stats) of a case, computed once and read-only"""
    out = ref.render(*args(case(name)))
    for a in out[:4]:
        a.setflags(write=False)
    return out


def camera_space(s):
    """float64 [n, 3]: R^T (p - t), by numpy's own matrix product"""
    return (s["v"]["xyz"].astype(np.float64) - s["t"].astype(np.float64)) @ s["R"].astype(np.float64)
