"""CPU: the restatement of the rasteriser (kintinuous_amd/mesh_render_ref.py) against things it was not written from -- the pixel count and
depth of a rectangle worked out from its corners, exactly-once coverage inside closed outlines, invariance under a shuffle of the triangle
list, and an independent float64 ray-triangle intersection through every pixel centre."""
import numpy as np
import pytest

import mesh_render_cases as cases
from kintinuous_amd import mesh_render_ref as ref

# Measured with this file (profiles/mesh_render.md): the largest |depth difference| between the restatement and the ray-triangle
# intersection over the compared pixels of the four cases below -- 0.0000 mm on the two layers (planes at whole millimetres), 0.5124 mm
# on the sphere from inside (the rounding of the depth plane to whole millimetres), 2.1936 mm on the sphere from outside, where the
# snapping of the vertices to 1 / 256 px moves the surface along the steep slopes next to the silhouette.  The asserted bound is ten
# times the largest: the margin leaves room for other slopes, not for bugs.
MEASURED_MAX_MM = 2.1936
DEPTH_BOUND_MM = 10 * MEASURED_MAX_MM
EDGE_MARGIN_PX = 1.0 / 128
EXCLUDED_SHARE = 0.05


def _render(name):
    return cases.want(name)


def test_rectangle_count_and_depth():
    """A triangle's oriented edge a -> b is inclusive when it runs down the image (by > ay) or, if level, to the left.  After the swap a
    triangle has A > 0, which in an image whose y grows downwards is: top edge to the right, right edge down, bottom edge to the left,
    left edge up.  So the right and bottom edges of the rectangle own their centres and the left and top ones do not: pixel (i, j) is
    covered when xa < i <= xb and ya < j <= yb, once, whatever the triangulation inside"""
    s = cases.case("rectangle")
    xa, ya, xm, xb, yb = cases.RECT
    i, j = np.arange(s["cols"]), np.arange(s["rows"])
    inside = ((j > ya) & (j <= yb))[:, None] & ((i > xa) & (i <= xb))[None, :]
    index, depth, color, model, stats = _render("rectangle")
    assert inside.sum() == (xb - xa) * (yb - ya) and stats == (4, 0, 0, int(inside.sum()))
    assert np.array_equal(index != ref.NO_TRIANGLE, inside)
    assert (depth[inside] == 2000).all() and (depth[~inside] == 0).all()
    assert np.array_equal(ref.coverage(*cases.args(s)), inside.astype(np.int64))
    assert (model[inside] > 0).all() and (model[~inside] == 0).all() and (color[~inside] == 0).all()


def _strictly_inside(outline, cols, rows):
    """pixel centres strictly inside a convex or star-shaped polygon given as [k, 2] in order: the even-odd rule on float64, minus the
    centres within 1e-9 px of an outline edge"""
    jj, ii = np.mgrid[0:rows, 0:cols].astype(np.float64)
    inside = np.zeros((rows, cols), bool)
    on_edge = np.zeros((rows, cols), bool)
    for a, b in zip(outline, np.roll(outline, -1, axis=0)):
        with np.errstate(all="ignore"):
            crosses = ((a[1] > jj) != (b[1] > jj)) & (ii < (b[0] - a[0]) * (jj - a[1]) / (b[1] - a[1]) + a[0])
        inside ^= crosses
        d = b - a
        u = np.clip(((ii - a[0]) * d[0] + (jj - a[1]) * d[1]) / (d @ d), 0.0, 1.0)
        on_edge |= np.hypot(ii - (a[0] + u * d[0]), jj - (a[1] + u * d[1])) < 1e-9
    return inside & ~on_edge


def test_coverage_is_one_strictly_inside_the_outlines():
    xa, ya, xm, xb, yb = cases.RECT
    for name, outline in (("rectangle", [(xa, ya), (xb, ya), (xb, yb), (xa, yb)]), ("fan", cases.FAN_RIM), ("far", cases.FAN_RIM)):
        s = cases.case(name)
        inside = _strictly_inside(np.array(outline, np.float64), s["cols"], s["rows"])
        cov = ref.coverage(*cases.args(s))
        assert inside.sum() > 500 and (cov[inside] == 1).all(), name
        assert cov.max() == 1 and cov[int(cases.FAN_HUB[1]), int(cases.FAN_HUB[0])] == 1       # the hub and the spokes through centres: once
    # the front faces of the sphere seen from outside: one triangle on every pixel whose eight neighbours are covered as well
    s = cases.case("sphere outside")
    c = cases.camera_space(s)
    t = s["tri"].astype(np.int64)
    faces = s["tri"][_front_faces(c, t)]
    index = ref.render(s["v"], faces, *cases.args(s)[2:])[0]
    covered = index != ref.NO_TRIANGLE
    inner = covered.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner &= np.roll(np.roll(covered, dy, axis=0), dx, axis=1)
    cov = ref.coverage(s["v"], faces, *cases.args(s)[2:])
    assert inner.sum() > 2000 and (cov[inner] == 1).all()


def _front_faces(c, t):
    """the triangles of an outward-oriented closed mesh that face the camera at the origin of c: the ones on the near side, told by depth --
    a front face lies nearer than the centroid of all vertices"""
    n = np.cross(c[t[:, 1]] - c[t[:, 0]], c[t[:, 2]] - c[t[:, 0]])
    facing = np.einsum("ij,ij->i", n, c[t[:, 0]])
    near_side = c[t].mean(axis=1)[:, 2] < c[:, 2].mean()
    sign = np.sign(facing[near_side].sum())                  # the orientation the near side has
    return np.flatnonzero(np.sign(facing) == sign)


def test_shuffled_soup():
    a, b = cases.case("soup"), cases.case("soup shuffled")
    perm = cases.SOUP_PERMUTATION()
    assert np.array_equal(b["tri"], a["tri"][perm])
    ia, da, ca, ma, sa = _render("soup")
    ib, db, cb, mb, sb = _render("soup shuffled")
    assert sa == sb and sa[0] > 3000 and sa[3] > 5000
    px, (zq, pix), _ = ref.words(*cases.args(a))
    best = (px >> np.uint64(32)).astype(np.int64)
    ties = np.bincount(pix[zq == best[pix]], minlength=len(px)).reshape(ia.shape) > 1
    assert ties.sum() < 0.01 * sa[3]
    assert np.array_equal(da, db)                                                    # (the depth of a tie is the same too)
    assert np.array_equal(ca[~ties], cb[~ties]) and np.array_equal(ma[~ties], mb[~ties])
    covered = ia != ref.NO_TRIANGLE
    assert np.array_equal(perm[ib[covered & ~ties]], ia[covered & ~ties])            # the same triangles under their new numbers


# ---- an independent intersection: Moeller-Trumbore in float64 through every pixel centre, the nearest hit -------------------------------
def _ray_cast(s):
    """(index int64 [rows, cols] (-1: no hit), z float64 [rows, cols], near_edge bool [rows, cols]: the centre lies within EDGE_MARGIN_PX
    of a projected edge).  A triangle with a vertex at or behind z = near is dropped whole, which is the rasteriser's rule"""
    cols, rows = s["cols"], s["rows"]
    fx, fy, cx, cy = s["intr"]
    c = cases.camera_space(s)
    best_z = np.full((rows, cols), np.inf)
    best_i = np.full((rows, cols), -1, np.int64)
    near_edge = np.zeros((rows, cols), bool)
    for ti, (i0, i1, i2) in enumerate(s["tri"].astype(np.int64)):
        p = c[[i0, i1, i2]]
        if len({i0, i1, i2}) < 3 or (p[:, 2] < s["near"]).any():
            continue
        sx, sy = p[:, 0] * fx / p[:, 2] + cx, p[:, 1] * fy / p[:, 2] + cy
        x0, x1 = max(int(np.floor(sx.min())) - 1, 0), min(int(np.ceil(sx.max())) + 1, cols - 1)
        y0, y1 = max(int(np.floor(sy.min())) - 1, 0), min(int(np.ceil(sy.max())) + 1, rows - 1)
        if x0 > x1 or y0 > y1:
            continue
        jj, ii = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.float64)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            ex, ey = sx[b] - sx[a], sy[b] - sy[a]
            L = ex * ex + ey * ey
            u = np.clip(((ii - sx[a]) * ex + (jj - sy[a]) * ey) / L, 0.0, 1.0) if L > 0 else 0.0
            near_edge[y0:y1 + 1, x0:x1 + 1] |= np.hypot(ii - (sx[a] + u * ex), jj - (sy[a] + u * ey)) <= EDGE_MARGIN_PX
        d = np.stack([(ii - cx) / fx, (jj - cy) / fy, np.ones_like(ii)], axis=-1)
        e1, e2 = p[1] - p[0], p[2] - p[0]
        h = np.cross(d, e2)
        det = h @ e1
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            sv = -p[0]                                        # the ray starts at the origin
            u = (h @ sv) * inv
            q = np.cross(sv, e1)
            v = (d @ q) * inv
            z = (e2 @ q) * inv                                # the ray parameter, which is the depth: d_z = 1
            hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (z > 0) & (z < best_z[y0:y1 + 1, x0:x1 + 1])
        best_z[y0:y1 + 1, x0:x1 + 1][hit] = z[hit]
        best_i[y0:y1 + 1, x0:x1 + 1][hit] = ti
    return best_i, best_z, near_edge


@pytest.mark.parametrize("name", ["layers 1 cm", "layers 1 m", "sphere inside", "sphere outside"])
def test_against_ray_triangle_intersection(name):
    s = cases.case(name)
    index, depth, _, _, stats = _render(name)
    hit_i, hit_z, near_edge = _ray_cast(s)
    share = near_edge.mean()
    assert share < EXCLUDED_SHARE, share
    keep = ~near_edge
    got = np.where(index == ref.NO_TRIANGLE, -1, index.astype(np.int64))
    assert np.array_equal(got[keep], hit_i[keep])
    both = keep & (hit_i >= 0)
    assert both.sum() > {"layers 1 cm": 1000, "layers 1 m": 1000, "sphere inside": 15000, "sphere outside": 3000}[name]
    diff = np.abs(depth[both].astype(np.float64) - hit_z[both] * 1000.0)
    print("%s: %d pixels compared, %.2f %% excluded, max |depth difference| %.4f mm" % (name, both.sum(), 100 * share, diff.max()))
    assert diff.max() <= DEPTH_BOUND_MM


# ---- the errors and the empty cases -------------------------------------------------------------------------------------------------------
def test_errors_and_empty_cases():
    s = cases.case("fan")
    v, tri, intr, cols, rows, R, t, near = cases.args(s)
    for bad, cause in ((dict(tri=np.array([[0, 1, len(v)]], np.uint32)), "index out of range"), (dict(cols=0), "cols and rows"), (dict(rows=8193), "cols and rows"),
                       (dict(intr=(0.0, 64.0, 1.0, 1.0)), "intrinsics"), (dict(intr=(64.0, -1.0, 1.0, 1.0)), "intrinsics"), (dict(intr=(64.0, 64.0, np.nan, 1.0)), "intrinsics"),
                       (dict(R=np.full((3, 3), np.inf)), "R and t"), (dict(t=(0.0, 8192.0, 0.0)), "R and t"), (dict(t=(np.nan, 0.0, 0.0)), "R and t"),
                       (dict(near=0.0009), "near"), (dict(near=8192.0), "near"), (dict(near=np.nan), "near")):
        kw = {**s, **bad}
        with pytest.raises(ValueError, match=cause):
            ref.render(*cases.args(kw))
    for axis, val in ((0, np.nan), (1, np.inf), (2, 8192.0), (0, -8192.0)):
        vb = v.copy()
        vb["xyz"][3, axis] = val
        with pytest.raises(ValueError, match="not finite or has a coordinate"):
            ref.render(vb, tri, intr, cols, rows, R, t, near)
        vu = np.concatenate([v, vb[3:4]])                                             # the same vertex unreferenced: accepted
        assert ref.render(vu, tri, intr, cols, rows, R, t, near)[4] == cases.want("fan")[4]
    for vv, tt in ((v[:0], tri[:0]), (v, tri[:0]), (v[:0], tri)):                      # n = 0 or m = 0: an empty image
        index, depth, color, model, stats = ref.render(vv, tt, intr, cols, rows, R, t, near)
        assert stats == (0, 0, 0, 0) and (index == ref.NO_TRIANGLE).all() and not depth.any() and not color.any() and not model.any()
        assert index.shape == (rows, cols) and depth.dtype == np.uint16 and color.shape == (rows, cols, 3) and model.dtype == np.uint8
    # the bounds themselves are allowed
    assert ref.render(v, tri, intr, cols, rows, R, t, 0.001)[4] == cases.want("fan")[4]
    assert ref.render(v, tri, intr, 8192, 1, R, t, near)[4][0] == len(tri)


def test_stats_of_the_named_cases():
    assert _render("rejects")[4][:3] == (1, 3, 2)                                     # drawn; behind, across near, beyond the guard band; equal indices, collinear
    assert _render("subpixel")[4] == (1, 0, 0, 0)                                     # drawn, yet it covers nothing
    index = _render("twice")[0]
    assert _render("twice")[4][0] == 3 and set(np.unique(index)) == {0, ref.NO_TRIANGLE}  # equal depth goes to the smaller index
    for name in ("layers 1 cm", "layers 1 m"):
        index, depth = _render(name)[:2]
        overlap = (ref.coverage(*cases.args(cases.case(name))) == 2)
        assert overlap.sum() > 300 and (index[overlap] == 1).all()                    # the near layer, listed second, wins
    for cols, rows in cases.IMAGES:
        index, depth, color, model, stats = _render("fill %dx%d" % (cols, rows))
        assert stats == (1, 0, 0, cols * rows) and (index == 0).all() and depth.min() >= 1000 and depth.max() <= 4000
    cov = ref.coverage(*cases.args(cases.case("sweep")))
    for w, h in cases.SWEEP:                                                          # every box of the sweep has the size it is named for
        x0, y0 = 3 + 12 * (w - 1), 3 + 12 * (h - 1)
        cell = cov[y0 - 3:y0 + 9, x0 - 3:x0 + 9]
        ys, xs = np.nonzero(cell)
        assert xs.max() - xs.min() + 1 <= w and ys.max() - ys.min() + 1 <= h and cell[3, 3] == 1
    s = cases.case("centres 7x5")                                                     # vertices (1, 1), (4, 1), (1, 4): the tie rule by hand
    want = np.zeros((5, 7), np.int64)
    want[2, 2], want[2, 3], want[3, 2] = 1, 1, 1                                      # the top and left edges do not own their centres, the hypotenuse (running down-left) does
    assert np.array_equal(ref.coverage(*cases.args(s)), want)
