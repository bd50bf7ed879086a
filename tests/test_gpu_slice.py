"""The per-slice stage (kt_slice_process / kt_slice_process_device, csrc/kt_slice.hip) against the oracle (kto_slice_process) on inputs
built to reach each of its data-dependent paths, bit for bit: the output count, the leaf order, the xyz bits, bgra (the pass-through
alpha byte included), the NaN mask of the normals and the bits of the normals and curvatures.

 - the three algorithms rocPRIM's radix_sort_pairs picks by size (one block sort <= 1024 (u32, u32) pairs, merge sort <= 2^20, onesweep
   above), on a workspace that grows once and is then reused for every smaller size, and on one fixed-capacity workspace with a device
   count below the host's bound; clouds with many points per leaf, so that the in-order centroid sums see any instability of the sort;
 - the neighbour search in stages (cell cubes of radius 2, 3, 4, 8, 16; the z-window when a cube holds more than KT_SLICE_MAXC leaves;
   the window grown to all leaves; fewer leaves than k; the pass-through cloud with more leaves than slice_normals' bounded grid has
   waves), each from a geometry that must take it -- the CPU test test_case_table_covers_the_search_paths checks that with a model of
   the search rule;
 - the (distance, index) tie rule on exact lattices, duplicate points, points on cell faces, negative coordinates and -0.0, a
   non-power-of-two leaf;
 - the whole range of k and weight_cull the C-ABI accepts;
 - the grid's integer edges: the largest overflow-check product a float cloud can reach below INT32_MAX, INT32_MAX + 1, and clouds whose
   32-bit leaf key reaches 0xffffffff (the key of a culled point on the GPU);
 - the stage behind the tracker's shift path with a capacity above 2^20."""
import ctypes as C

import numpy as np
import pytest

INT32_MAX = 2147483647
MAXC = 729                       # KT_SLICE_MAXC: leaves a cell cube may list before the search hands over to the z-window
BLOCK_SORT_MAX = 256 * 4         # rocPRIM: (u32, u32) pairs, radix_sort_block_sort_config_base -> kernel_config<256, 4>
MERGE_SORT_MAX = 1 << 20         # rocPRIM: radix_sort_config<>::merge_sort_limit
SORT_SIZES = [1, 2, 3, 1023, 1024, 1025, 65535, 65536, 65537, 1 << 20, (1 << 20) + 1, 1_500_000]
DEVICE_BOUNDS = [(1000, 997), (1024, 700), (65537, 65000), (1_048_576, 1_000_003), (1_500_000, 1_499_999)]   # (n_max, *n_dev)
DEVICE_CAP = 1_600_000
TRACKER_CAP = 1_200_000


# ---- clouds ---------------------------------------------------------------------------------------------------------------------
def _cloud(xyz, rng, alpha=(0, 256)):
    from oracle.oracle import POINT_DTYPE
    p = np.zeros(len(xyz), POINT_DTYPE)
    p["xyz"] = np.asarray(xyz, np.float32)
    p["bgra"][:, :3] = rng.integers(0, 256, (len(xyz), 3))
    p["bgra"][:, 3] = rng.integers(alpha[0], alpha[1], len(xyz))
    return p


def _in_cells(cells, leaf, per, rng, spread=0.1):
    """`per` points in each of the given integer cells, near the cell's centre (centroids close to a lattice), in random order"""
    c = np.repeat(np.asarray(cells, np.float64), per, axis=0)
    xyz = (c + 0.5 + rng.uniform(-spread, spread, c.shape)) * leaf
    return xyz[rng.permutation(len(xyz))]


def _grid2(nx, ny, z=0):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), np.full(i.size, z)], axis=1)


def _plane(seed, per):
    rng = np.random.default_rng(seed)
    cells = _grid2(60, 60, 40) - [30, 30, 0]
    return _cloud(_in_cells(cells, 0.05, per, rng), rng)


def _strip(seed):
    """a strip 2 cells wide (the interior needs ~5 cells along it for 20 neighbours, its ends ~10) and, far from it, a line 1 cell wide
    (~10 cells, its ends ~20): the slab-edge geometry that needs r = 8 and 16 and the window"""
    rng = np.random.default_rng(seed)
    a = np.array([[x, y, 0] for x in range(300) for y in range(2)])
    b = np.array([[x, 60, 50] for x in range(200)])
    return _cloud(_in_cells(np.concatenate([a, b]) + [-150, -30, 20], 0.04, 3, rng), rng)


def _blob(seed):
    """a quarter of the cells of a 24 x 24 x 40 block occupied: for k = 64 the 64th neighbour lies beyond 3.5 cells and the r = 8 cube
    holds ~1200 leaves (> KT_SLICE_MAXC): the windowed search"""
    rng = np.random.default_rng(seed)
    i, j, k = np.meshgrid(np.arange(24), np.arange(24), np.arange(40), indexing="ij")
    cells = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
    cells = cells[rng.random(len(cells)) < 0.25] + [-12, -12, 30]
    return _cloud(_in_cells(cells, 0.03, 2, rng, 0.3), rng)


def _outliers(seed):
    """a dense 30 x 30 patch and 12 points 20 - 25 m away at the corners and ends of the bounding box: their k-th neighbour is in the
    patch, further than any window short of the whole list"""
    rng = np.random.default_rng(seed)
    patch = _in_cells(_grid2(30, 30, 40) - [15, 15, 0], 0.05, 4, rng)
    far = [[sx * 22, sy * 22, 2 + sz * 22] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    far += [[0, 0, 25], [0, 0, -21], [24, 0, 2], [-24, 1, 2]]
    return _cloud(np.concatenate([patch, np.asarray(far, np.float64) + rng.uniform(-0.01, 0.01, (12, 3))]), rng)


def _few(seed, n_leaves):
    rng = np.random.default_rng(seed)
    cells = rng.choice(1000, n_leaves, replace=False)
    cells = np.stack([cells % 10, (cells // 10) % 10, cells // 100], axis=1) + [0, 0, 30]
    return _cloud(_in_cells(cells, 0.05, 3, rng, 0.4), rng)


def _box_corners(e, leaf, rng, n):
    """n points at cell centres of a box of e = (ex, ey, ez) cells, its two extreme corners included: PCL's check product is prod(e)"""
    e = np.asarray(e, np.int64)
    cells = np.concatenate([[[0, 0, 0], e - 1], rng.integers(0, e, (n - 2, 3))])
    return _cloud((cells + 0.5) * leaf, rng)


def _lattice(seed, side=12, leaf=1.0 / 16, dup=(1, 2), neg_zero=True):
    """points exactly on the lattice of cell corners (on cell faces, coordinates exact binary multiples of a power-of-two leaf, squared
    distances tie exactly), centred on the origin: negative coordinates, 0 and -0.0; each point repeated dup[0] .. dup[1] - 1 times"""
    rng = np.random.default_rng(seed)
    r = np.arange(side) - side // 2
    i, j, k = np.meshgrid(r, r, r, indexing="ij")
    cells = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
    cells = np.repeat(cells, rng.integers(dup[0], dup[1], len(cells)), axis=0)
    xyz = (cells * leaf)[rng.permutation(len(cells))].astype(np.float32)
    if neg_zero:
        z = xyz == 0
        xyz[z & (rng.random(xyz.shape) < 0.5)] = np.float32(-0.0)
    return _cloud(xyz, rng)


def _faces(seed):
    """random points, a half of their coordinates snapped to cell faces (multiples of the leaf), the other half to cell centres"""
    rng = np.random.default_rng(seed)
    leaf = 1.0 / 32
    xyz = rng.uniform(-0.6, 0.6, (6000, 3)) + [0, 0, 1.5]
    snap = rng.random(xyz.shape) < 0.5
    xyz = np.where(snap, np.round(xyz / leaf) * leaf, (np.floor(xyz / leaf) + 0.5) * leaf)
    return _cloud(xyz, rng)


def _tenth(seed):
    """leaf 0.1: coordinates float32(i * 0.1) and their float neighbours, where p * inv_leaf rounds across an integer"""
    rng = np.random.default_rng(seed)
    i = rng.integers(-25, 25, (8000, 3))
    xyz = (i * 0.1).astype(np.float32)
    nudge = rng.integers(-1, 2, xyz.shape)
    xyz = np.where(nudge == 0, xyz, np.nextafter(xyz, np.where(nudge > 0, np.float32(np.inf), np.float32(-np.inf))))
    return _cloud(xyz, rng)


def _key_ffffffff(seed, wide):
    """PCL's check multiplies the truncated extents, the keys use div_b = floor(max / leaf) - floor(min / leaf) + 1, one larger per axis.
    wide: extents (1, 46340, 46340) pass the check (46340^2 <= INT32_MAX) while div_b = (2, 46341, 46341): the keys wrap past 2^32, and
    the point in cell (1, 41707, 46340) has the key 1 + 2 * 41707 + 92682 * 46340 = 0xffffffff; the point in (1, 41710, 46340) wraps onto
    the key of cell (1, 2, 0).  not wide: extents (1, 32768, 65535), div_b = (2, 32768, 65536): 2^32 cells, the last one's key is
    0xffffffff without any wrap.  Every coordinate is exact (a power-of-two leaf, indices < 2^17).  Some points are culled (alpha 0),
    before, between and after the 0xffffffff ones in the input."""
    rng = np.random.default_rng(seed)
    leaf = 1.0 / 64
    if wide:   # (x, y, z) in leaf sizes
        cells = [[0.75, 0.5, 0.5], [1.25, 46340.25, 46340.25], [1.25, 41707.5, 46340.25], [1.25, 41707.2, 46340.1],
                 [1.25, 41710.5, 46340.25], [1.25, 2.5, 0.5], [1.0, 100.5, 7.5], [1.0, 101.5, 7.5], [1.0, 100.5, 8.5], [1.25, 45000.5, 46000.5]]
        target = 2
    else:
        cells = [[0.75, 0.5, 0.75], [1.25, 32767.5, 65535.25], [1.25, 32767.2, 65535.1], [1.0, 10.5, 20.5], [1.0, 11.5, 20.5],
                 [1.0, 10.5, 21.5], [1.25, 32000.5, 65000.5]]
        target = 1
    xyz = np.asarray(cells) * leaf
    p = _cloud(xyz, rng, alpha=(5, 256))
    culled = _cloud(xyz[[target, target, 3, 0]] + [0, 0, leaf / 8], rng, alpha=(0, 1))
    return np.concatenate([culled[:1], p[:target + 1], culled[1:3], p[target + 1:], culled[3:]])


def _window_planes(seed):
    """Two probes of the z-window's bounds.  A point P near the top of its cell with, 7.25 leaf sizes straight above it, one leaf Q in
    the plane c2 + 8, near its cell's bottom; in P's own plane two leaves at 7.4 and 7.45; and > 729 leaves of a shell of the r = 8 cube
    further than 9 leaf sizes, so that the cube search hands P over to the window.  With k = 3 the window R = 8 settles P on (P, Q, 7.4):
    a window that left out the plane c2 + 8 would settle it on (P, 7.4, 7.45), within its reach of 7.5 as well.  The second probe is
    the mirror image (Q in the plane c2 - 8).  Two far leaves widen the z-range, so the windows are not the whole list."""
    rng = np.random.default_rng(seed)
    r = np.arange(-8, 9)
    i, j, k = np.meshgrid(r, r, r, indexing="ij")
    cube = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
    shell = cube[(cube ** 2).sum(axis=1) > 81]
    shell = shell + 0.5 + rng.uniform(-0.05, 0.05, shell.shape)
    pts = []
    for x0, up in ((0, 1), (60, -1)):
        z0 = 0.875 if up > 0 else 0.125
        probe = [[0.5, 0.5, z0], [0.5, 0.5, z0 + up * 7.25], [7.9, 0.5, z0], [0.5, -6.95, z0]]
        pts += [np.asarray(probe) + [x0, 0, 0], shell + [x0, 0, 0]]
    pts.append(np.array([[30.5, 30.5, 30.5], [30.5, 30.5, -30.5]]))
    xyz = np.concatenate(pts) * (1.0 / 16) + [1.0, -0.5, 2.0]
    return _cloud(xyz, rng)


def _passthrough(seed):
    """extents (1024, 1024, 2048): a check product of 2^31 = INT32_MAX + 1, the cloud passes through unfiltered; 20 000 points, more than
    slice_normals' 4096 x 4 waves, so the grid strides"""
    return _box_corners((1024, 1024, 2048), 1.0 / 16, np.random.default_rng(seed), 20000)


def _int32max_gridded(seed):
    """INT32_MAX = 2^31 - 1 is prime: a check product equal to it needs two factors 1 and an extent of 2^31 - 2 leaves, which the float
    (max - min) * inv_leaf cannot hold (floats are multiples of 128 there).  The largest product a cloud can reach is INT32_MAX - 1 =
    558 * 1661 * 2317: gridded, the keys below 2^31"""
    return _box_corners((558, 1661, 2317), 1.0 / 16, np.random.default_rng(seed), 400)


# name -> (builder, leaf, k, weight_cull, the search classes the case is there to reach)
_CASES = {
    "plane_k7": (lambda: _plane(1, 4), 0.05, 7, 0, {"r2"}),
    "plane_dense": (lambda: _plane(2, 8), 0.05, 20, 100, {"r3", "r4"}),
    "strip": (lambda: _strip(3), 0.04, 20, 0, {"r8", "r16"}),
    "blob_k64": (lambda: _blob(4), 0.03, 64, -1, {"window"}),
    "outliers": (lambda: _outliers(5), 0.05, 20, 0, {"window_all"}),
    "few_leaves": (lambda: _few(6, 15), 0.05, 20, 0, {"exhaustion"}),
    "two_leaves": (lambda: _few(7, 2), 0.05, 20, 0, set()),
    "one_leaf": (lambda: _few(8, 1), 0.05, 1, 0, set()),
    "lattice_k20": (lambda: _lattice(9), 1.0 / 16, 20, 0, set()),
    "lattice_k7": (lambda: _lattice(10), 1.0 / 16, 7, 0, set()),
    "lattice_k8": (lambda: _lattice(11), 1.0 / 16, 8, 0, set()),
    "lattice_dupes": (lambda: _lattice(12, side=10, dup=(1, 6)), 1.0 / 16, 20, 30, set()),
    "window_planes": (lambda: _window_planes(19), 1.0 / 16, 3, 0, set()),
    "faces": (lambda: _faces(13), 1.0 / 32, 20, 0, set()),
    "leaf_tenth": (lambda: _tenth(14), 0.1, 20, 0, set()),
    "passthrough_2p31": (lambda: _passthrough(15), 1.0 / 16, 20, 0, {"passthrough"}),
    "gridded_int32max_minus1": (lambda: _int32max_gridded(16), 1.0 / 16, 8, 0, set()),
    "key_ffffffff_wrapped": (lambda: _key_ffffffff(17, True), 1.0 / 64, 3, 1, {"wide"}),
    "key_ffffffff_last_cell": (lambda: _key_ffffffff(18, False), 1.0 / 64, 3, 1, {"wide"}),
}
_PARAM_CLOUDS = ["lattice_dupes", "plane_k7"]
_KS = [1, 2, 3, 7, 8, 20, 21, 63, 64]
_CULLS = [-1, 0, 1, 255]


def _sort_cloud(n=1_500_000, seed=21):
    """1.5 M points on a height field over 120 x 120 cells of 5 cm (~29 k leaves, ~40 points each), in random order (every prefix hits
    most leaves), a fifth of them below the weight cull of 2"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 6.0, (n, 2))
    z = 2.0 + 0.3 * np.sin(xy[:, 0]) * np.cos(0.7 * xy[:, 1]) + rng.normal(0, 0.01, n)
    return _cloud(np.stack([xy[:, 0] - 3.0, xy[:, 1] - 3.0, z], axis=1), rng, alpha=(0, 10))


# ---- a model of the search rule (coverage only; never used for the comparison) --------------------------------------------------
def _grid(p, cull, leaf):
    """the leaves of the stage (numpy restatement of the grid): dict with the per-leaf cell, centroid, the grid's div_b and flags"""
    kept = p if cull <= 0 else p[p["bgra"][:, 3] >= cull]
    xyz = kept["xyz"]
    inv = np.float32(1) / np.float32(leaf)
    mn, mx = xyz.min(axis=0), xyz.max(axis=0)
    e = ((mx - mn) * inv).astype(np.int64) + 1
    min_b = np.floor(mn * inv).astype(np.int64)
    div = np.floor(mx * inv).astype(np.int64) - min_b + 1
    g = dict(e=e, div=div, gridded=int(np.prod(e)) <= INT32_MAX, n_kept=len(kept))
    g["wide"] = g["gridded"] and int(np.prod(div)) >= 1 << 32
    ijk = (np.floor(xyz * inv) - min_b.astype(np.float32)).astype(np.int64)
    key = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    g["key32"] = key % (1 << 32)
    if not g["gridded"]:
        g["cen"], g["cell"] = xyz.astype(np.float64), None
        return g
    uniq, inverse = np.unique(g["key32"], return_inverse=True)
    cnt = np.bincount(inverse)
    g["cen"] = np.stack([np.bincount(inverse, xyz[:, a].astype(np.float64)) / cnt for a in range(3)], axis=1)
    g["cell"] = np.stack([uniq % div[0], (uniq // div[0]) % div[1], uniq // (div[0] * div[1])], axis=1)
    return g


def _classify(p, leaf, k, cull, margin=0.1):
    """per leaf: the search stage that settles it (r2 r3 r4 r8 r16 window window_all), or None when the leaf sits within `margin` leaf
    sizes (or 5 % of KT_SLICE_MAXC leaves) of a threshold; whole-cloud classes: passthrough, wide, exhaustion.  The rule of slice_normals:
    radii 3 (2 for k <= 7), 4, 8, 16 while a cube lists at most KT_SLICE_MAXC leaves, settled when the k-th distance is <= (r - 0.5)
    leaf sizes; then z-windows of R = 8, 16, ... cells, settled when the k-th distance is <= (R - 0.5) leaf sizes or the window is all."""
    from scipy.spatial import cKDTree
    g = _grid(p, cull, leaf)
    L = len(g["cen"])
    kk = min(k, L)
    out = {"leaves": L}
    if not g["gridded"]:
        out["passthrough"] = L
    if g["wide"]:
        out["wide"] = L
    if L < k:
        out["exhaustion"] = L
    if not g["gridded"] or g["wide"]:
        return out
    d, _ = cKDTree(g["cen"] / leaf).query(g["cen"] / leaf, k=kk)
    dk = d.reshape(L, -1)[:, kk - 1]                       # the k-th distance in leaf sizes (the leaf itself first, at 0)
    cell_tree = cKDTree(g["cell"])
    todo = np.ones(L, bool)
    clear = np.ones(L, bool)
    prev, handed = -np.inf, []
    for r in ([2, 3, 4, 8, 16] if kk <= 7 else [3, 4, 8, 16]):
        idx = np.nonzero(todo)[0]
        if not len(idx):
            break
        n = cell_tree.query_ball_point(g["cell"][idx], r, p=np.inf, return_length=True)
        over = n > MAXC                                    # listed past KT_SLICE_MAXC: handed to the window
        clear[idx[np.abs(n - MAXC) <= 0.05 * MAXC]] = False
        done = ~over & (dk[idx] <= r - 0.5)
        clear[idx[done & ((dk[idx] > r - 0.5 - margin) | (dk[idx] <= prev + margin))]] = False
        out[f"r{r}"] = int(clear[idx[done]].sum())
        todo[idx[done | over]] = False
        handed.extend(idx[over].tolist())
        prev = r - 0.5
    window = np.array(sorted(handed + np.nonzero(todo)[0].tolist()), np.int64)
    c2, d2 = g["cell"][:, 2], int(g["div"][2])
    for q in window:
        R, prev = 8, -np.inf
        while True:
            every = c2[q] - R <= 0 and c2[q] + R >= d2 - 1
            if dk[q] <= R - 0.5 or every:
                name = "window_all" if every else "window"
                ok = clear[q] and dk[q] > prev + margin and (every or dk[q] <= R - 0.5 - margin)
                out[name] = out.get(name, 0) + bool(ok)
                break
            prev = R - 0.5
            R *= 2
    return out


def _sort_band(n):
    return "block" if n <= BLOCK_SORT_MAX else "merge" if n <= MERGE_SORT_MAX else "onesweep"


# ---- CPU: the table reaches what it claims ----------------------------------------------------------------------------------------
def test_case_table_covers_the_search_paths():
    """Every search class of slice_normals holds at least 10 leaves, well clear of its thresholds, in the cases the table names for it;
    every sort band holds sizes on both sides of its limits; the grid-edge clouds have the products and keys they are built for."""
    reached = {}
    for name, (build, leaf, k, cull, classes) in _CASES.items():
        got = _classify(build(), leaf, k, cull)
        for c in classes:
            assert got.get(c, 0) >= (3 if c == "wide" else 10), (name, c, got)
            reached[c] = reached.get(c, 0) + got[c]
    assert set(reached) == {"r2", "r3", "r4", "r8", "r16", "window", "window_all", "exhaustion", "passthrough", "wide"}, reached
    assert _classify(_passthrough(15), 1.0 / 16, 20, 0)["passthrough"] > 4096 * 4          # more leaves than slice_normals has waves
    # the sort bands (rocPRIM picks the algorithm by the n_max of the call)
    bands = [_sort_band(n) for n in SORT_SIZES]
    assert bands.count("block") >= 5 and bands.count("merge") >= 4 and bands.count("onesweep") >= 2, bands
    assert {_sort_band(n) for n, _ in DEVICE_BOUNDS} == {"block", "merge", "onesweep"} and all(c < n <= DEVICE_CAP for n, c in DEVICE_BOUNDS)
    assert _sort_band(TRACKER_CAP) == "onesweep"
    assert {_sort_band(b - 1) + _sort_band(b) + _sort_band(b + 1) for b in (BLOCK_SORT_MAX, MERGE_SORT_MAX)} == {"blockblockmerge", "mergemergeonesweep"}
    # the grid edges
    assert int(np.prod(_grid(_int32max_gridded(16), 0, 1.0 / 16)["e"])) == INT32_MAX - 1
    assert int(np.prod(_grid(_passthrough(15), 0, 1.0 / 16)["e"])) == INT32_MAX + 1
    for wide in (True, False):
        g = _grid(_key_ffffffff(17, wide), 1, 1.0 / 64)
        assert g["gridded"] and g["wide"] and int(np.prod(g["e"])) <= INT32_MAX and (g["key32"] == 0xffffffff).sum() == 2, g


def test_sort_cloud_has_many_points_per_leaf():
    p = _sort_cloud()
    g = _grid(p, 2, 0.05)
    assert 20_000 <= len(g["cen"]) <= 30_000 and g["n_kept"] / len(g["cen"]) >= 30
    assert 0.15 < (p["bgra"][:, 3] < 2).mean() < 0.25


def test_oracle_keeps_the_leaf_of_key_ffffffff(oracle_mod):
    """PCL 1.7 voxel_grid.hpp computes the leaf index in int, stores it as unsigned int and keeps every leaf, 0xffffffff included (its
    cull runs before, on the cloud): the oracle's count is the number of distinct wrapped keys of the kept points, and the two points of
    key 0xffffffff make one leaf, the last of the list."""
    for wide in (True, False):
        p = _key_ffffffff(17, wide)
        g = _grid(p, 1, 1.0 / 64)
        out = oracle_mod.slice_process(p, 1, 1.0 / 64, 3)
        assert len(out) == len(np.unique(g["key32"]))
        kept = p[p["bgra"][:, 3] >= 1]
        two = kept["xyz"][g["key32"] == 0xffffffff]
        assert np.array_equal(out["xyz"][-1], (two[0] + two[1]) * np.float32(0.5))


def test_oracle_tie_rule_picks_the_lowest_index_of_the_sqrt3_shell(oracle_mod):
    """Known answer of the (squared distance, index) order: the centre of a 3 x 3 x 3 lattice block without its (+1, 0, 0) cell, k = 20,
    takes itself, its 5 face and 12 edge neighbours and TWO of the 8 corners, all at exactly sqrt(3) leaf sizes.  The leaf order is the
    key order (z-major): the two lowest-index corners are (-1, -1, -1) and (1, -1, -1).  The centre's normal and curvature equal, bit for
    bit, those of the centre of the 20-point cloud that holds only those two corners (same neighbours, same order of the sums); not
    those of the cloud with the two highest-index corners, which a reversed tie-break would pick (the block without (+1, 0, 0) is not
    symmetric: the two choices give mirrored covariances).  The same for k = 8 (two of the 12 edge neighbours at sqrt(2))."""
    from oracle.oracle import POINT_DTYPE
    leaf = 1.0 / 16
    r = np.arange(-1, 2)
    i, j, k = np.meshgrid(r, r, r, indexing="ij")
    cube = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
    cube = cube[~(cube == [1, 0, 0]).all(axis=1)]
    base = np.array([1.0, -0.5, 2.0], np.float32)

    def centre(cells, kn):
        p = np.zeros(len(cells), POINT_DTYPE)
        p["xyz"] = base + (np.asarray(cells, np.float32) * np.float32(leaf))
        out = oracle_mod.slice_process(p, 0, leaf, kn)
        q = np.nonzero((out["xyz"] == base).all(axis=1))[0]
        assert len(q) == 1
        return out[q[0]]

    def same(a, b):
        return a["normal"].tobytes() == b["normal"].tobytes() and a["curvature"].tobytes() == b["curvature"].tobytes()

    shell = np.abs(cube).sum(axis=1)
    for kn, ring in ((20, 3), (8, 2)):
        inner = cube[shell < ring]
        members = cube[shell == ring]
        members = sorted(members.tolist(), key=lambda c: (c[2], c[1], c[0]))
        m = kn - len(inner)
        assert m == 2
        full = centre(cube, kn)
        assert not np.isnan(full["normal"]).any()
        assert same(full, centre(np.concatenate([inner, members[:m]]), kn)), kn
        assert not same(full, centre(np.concatenate([inner, members[-m:]]), kn)), kn


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _point_set(p):
    return sorted(bytes(r) for r in np.ascontiguousarray(p).view(np.uint8).reshape(len(p), -1)) if len(p) else []


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same(got, want, what):
    """the stage's output against the oracle's: count, leaf order and positions (xyz bits), bgra with the alpha byte, the constant
    fields, the NaN mask of the normals and curvatures, and the bits of every normal and curvature that is not NaN"""
    assert len(got) == len(want), (what, len(got), len(want))
    if not len(want):
        return
    assert np.array_equal(_bits(got["xyz"]), _bits(want["xyz"])), what
    assert np.array_equal(got["bgra"], want["bgra"]), what
    assert np.array_equal(_bits(got["one"]), _bits(want["one"])) and np.array_equal(_bits(got["zero"]), _bits(want["zero"])), what
    nan = np.isnan(want["normal"])
    assert np.array_equal(np.isnan(got["normal"]), nan) and np.array_equal(np.isnan(got["curvature"]), np.isnan(want["curvature"])), what
    ok = ~nan.any(axis=1)
    bad = np.nonzero((_bits(got["normal"][ok]) != _bits(want["normal"][ok])).any(axis=1) | (_bits(got["curvature"][ok]) != _bits(want["curvature"][ok])))[0]
    assert not len(bad), (what, len(bad), int(ok.sum()), got[ok][bad[:3]], want[ok][bad[:3]])


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(_CASES))
def test_slice_case(ctx, oracle_mod, case):
    from kintinuous_amd import abi
    build, leaf, k, cull, _ = _CASES[case]
    p = build()
    want = oracle_mod.slice_process(p, cull, leaf, k)
    assert len(want) > 0
    _assert_same(abi.slice_process(ctx, p, cull, leaf, k), want, case)


@pytest.mark.gpu
@pytest.mark.parametrize("cloud", _PARAM_CLOUDS)
def test_k_and_weight_cull_range(ctx, oracle_mod, cloud):
    """k over 1 .. 64 (k = 1, 2: NaN normals; k <= 7: the cube starts at r = 2; k = 64: every lane of the pick fetch) and weight_cull
    -1, 0 (no cull), 1 and 255 (a few points left)"""
    from kintinuous_amd import abi
    build, leaf, _, _, _ = _CASES[cloud]
    p = build()
    for cull in _CULLS:
        for k in _KS:
            want = oracle_mod.slice_process(p, cull, leaf, k)
            _assert_same(abi.slice_process(ctx, p, cull, leaf, k), want, (cloud, cull, k))
            if k <= 2:
                assert np.isnan(want["normal"]).all()


@pytest.fixture(scope="module")
def sort_cloud():
    return _sort_cloud()


@pytest.fixture(scope="module")
def sort_want(oracle_mod, sort_cloud):
    return {n: oracle_mod.slice_process(sort_cloud[:n], 2, 0.05, 20) for n in SORT_SIZES}


@pytest.mark.gpu
def test_sort_bands_on_one_growing_workspace(ctx, sort_cloud, sort_want):
    """kt_slice_process on the context's workspace (grown once, by the first and largest call, then reused): every size of SORT_SIZES,
    descending, then ascending -- the block sort, the merge sort and onesweep, each on a workspace sized for 1.5 M points"""
    from kintinuous_amd import abi
    assert len(sort_want[SORT_SIZES[-1]]) > 15_000
    for n in sorted(SORT_SIZES, reverse=True) + sorted(SORT_SIZES):
        _assert_same(abi.slice_process(ctx, sort_cloud[:n], 2, 0.05, 20), sort_want[n], n)


@pytest.mark.gpu
def test_sort_bands_device_entry_on_a_fixed_workspace(ctx, oracle_mod, sort_cloud):
    """kt_slice_process_device on one workspace of capacity 1.6 M: n_max in each sort band, the count on the device below it (the sort
    then runs over n_max keys, the culled ones and those past the count sorted behind every leaf)"""
    from kintinuous_amd import abi
    ws = C.c_void_p()
    abi._chk(abi.lib().kt_slice_ws_create(ctx.h, DEVICE_CAP, None, C.byref(ws)))
    try:
        pts = ctx.upload(sort_cloud)
        for n_max, count in sorted(DEVICE_BOUNDS, reverse=True) + sorted(DEVICE_BOUNDS):
            n_dev = ctx.upload(np.array([count], np.uint32))
            abi._chk(abi.lib().kt_slice_process_device(ws, pts.ptr, n_dev.ptr, n_max, 2, C.c_float(0.05), 20))
            n = C.c_size_t(0)
            abi._chk(abi.lib().kt_slice_ws_count(ws, C.byref(n)))
            got = np.zeros(n.value, abi.NPOINT_DTYPE)
            if n.value:
                abi._chk(abi.lib().kt_download(ctx.h, got.ctypes.data_as(C.c_void_p), abi.lib().kt_slice_ws_output(ws), got.nbytes))
            _assert_same(got, oracle_mod.slice_process(sort_cloud[:count], 2, 0.05, 20), (n_max, count))
    finally:
        abi._chk(abi.lib().kt_slice_ws_destroy(ws))


@pytest.mark.gpu
def test_stage_behind_the_tracker_with_onesweep(ctx, oracle_mod):
    """The stage behind the shift path with max_slice_points above 2^20 (the sort runs as onesweep over the whole capacity), k = 9 and a
    weight cull of 3, a shift on nearly every frame (voxel_shift 1, 6 cm steps at 5.5 cm voxels: both slab buffers in flight).  Every
    processed slice equals, byte for byte, the host-array stage on the raw slice, and the oracle's; raw slices, poses and volumes do not
    notice the stage."""
    from kintinuous_amd import abi, synth
    cam = synth.Camera.small(160, 120)
    scene = synth.Scene("wall")
    traj = synth.crabwalk_trajectory(420)
    frames = [synth.render(scene, cam, *traj[4 * i]) for i in range(50)]
    cfg = abi.TrackerConfig(cam.cols, cam.rows, 128, cam.fx, cam.fy, cam.cx, cam.cy, 7.0, 1, 2, 0, 0, 0, 0, 0, TRACKER_CAP, 0, 0)
    cull, k, leaf = 3, 9, 7.0 / 128

    def run(stage):
        trk = abi.Tracker(ctx, cfg)
        try:
            if stage:
                trk.enable_slice_stage(True, weight_cull=cull, k=k)
            for i, (d, rgb) in enumerate(frames):
                trk.process_frame_host(d, rgb, 33333 * i)
            trk.finalise()
            return dict(raw=[trk.slice(i) for i in range(trk.num_slices())], proc=[trk.slice_processed(i) for i in range(trk.num_slices())],
                        pose=trk.pose(), vol=trk.volume().copy(), col=trk.color_volume().copy())
        finally:
            trk.close()

    a, b = run(True), run(False)
    assert len(a["raw"]) == len(b["raw"]) >= 40 and all(p is not None for p in a["proc"])
    assert np.array_equal(a["vol"], b["vol"]) and np.array_equal(a["col"], b["col"]) and all(np.array_equal(x, y) for x, y in zip(a["pose"], b["pose"]))
    nonempty = 0
    for i, ((raw, dim), proc, (raw_b, dim_b)) in enumerate(zip(a["raw"], a["proc"], b["raw"])):
        assert dim == dim_b and _point_set(raw) == _point_set(raw_b)       # (the extraction appends in no fixed order)
        want = abi.slice_process(ctx, raw, cull, leaf, k) if len(raw) else np.zeros(0, abi.NPOINT_DTYPE)
        assert len(proc) == len(want) and proc.tobytes() == want.tobytes(), i
        _assert_same(proc, oracle_mod.slice_process(raw.view(oracle_mod.POINT_DTYPE), cull, leaf, k), i)
        nonempty += len(proc) > 0
    assert nonempty >= 15
