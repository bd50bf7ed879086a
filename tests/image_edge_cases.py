"""Inputs for the image-side edge tests (tests/test_image_edge_cases.py on the CPU, tests/test_gpu_image_edges.py on the GPU): seeded,
deterministic builders keyed by name, and `tile_classes`, a numpy restatement of the per-tile decision of kt_bilateral2_kernel
(csrc/kt_image.hip).  No GPU and no pytest in here.  Shapes are (rows, cols) unless a name says otherwise."""
import zlib

import numpy as np

TILE_X, TILE_Y, RADIUS = 16, 32, 6      # KT_BIL2_TX, KT_BIL2_TY, KT_BIL_R
WRAP = 46341                            # smallest d whose int d * d wraps: 46341^2 = 2^31 + 4633
WALK = 768                              # workgroups of a launch: tile t belongs to workgroup t % WALK once there are more tiles than that


def _rng(name, *shape):
    return np.random.default_rng([zlib.crc32(name.encode())] + [int(s) for s in shape])


# ---- the kernel's per-tile decision ---------------------------------------------------------------------------------------------------
def tile_spreads(depth):
    """int (tiles_y, tiles_x): max - min over what the kernel looks at per tile: the tile's taps -- the cells of the tile plus a 6-pixel
    halo, cut to [0, cols - 1) x [0, rows - 1): the last column and row are taps of nobody -- and its centres (the tile's own pixels, last
    column and row included)."""
    d = np.asarray(depth).astype(np.int64)
    rows, cols = d.shape
    ty, tx = -(-rows // TILE_Y), -(-cols // TILE_X)
    out = np.zeros((ty, tx), np.int64)
    for j in range(ty):
        for i in range(tx):
            y0, x0 = j * TILE_Y, i * TILE_X
            centres = d[y0:min(y0 + TILE_Y, rows), x0:min(x0 + TILE_X, cols)]
            taps = d[max(y0 - RADIUS, 0):min(y0 + TILE_Y + RADIUS, rows - 1), max(x0 - RADIUS, 0):min(x0 + TILE_X + RADIUS, cols - 1)]
            out[j, i] = max(centres.max(), taps.max(initial=-1)) - min(centres.min(), taps.min(initial=1 << 40))
    return out


def tile_classes(depth):
    """bool (tiles_y, tiles_x): True where the tile takes the tap-by-tap path, i.e. where its spread is 46341 or more"""
    return tile_spreads(depth) >= WRAP


def walk_positions(ntiles):
    """position of every tile in its workgroup's walk: 0 for the first tile a workgroup filters, 1 for its second, ..."""
    return np.arange(ntiles) // WALK if ntiles > WALK else np.zeros(ntiles, np.int64)


def walk_transitions(classes):
    """{(class before, class after): count} over consecutive tiles (t, t + 768) of every workgroup"""
    c = np.asarray(classes).reshape(-1)
    n = {(a, b): 0 for a in (False, True) for b in (False, True)}
    if c.size > WALK:
        for a, b in zip(c[:-WALK], c[WALK:]):
            n[(bool(a), bool(b))] += 1
    return n


def tile_of_pixels(shape):
    """int (rows, cols): the flat tile index of every pixel"""
    rows, cols = shape
    tx = -(-cols // TILE_X)
    return (np.arange(rows)[:, None] // TILE_Y) * tx + np.arange(cols)[None, :] // TILE_X


# ---- bilateral filter -----------------------------------------------------------------------------------------------------------------
MIXED_WALK_RECTANGLES = 150
MIXED_WALK_EDGE_TILES = 48      # table tiles that get one pixel at the edge of the decision: half at 46341 (they become general), half at 46340


def mixed_walk(with_edge_pixels=True):
    """(2016, 400): 25 x 63 = 1575 tiles, so workgroups 0-38 walk three tiles and the others two.  A smooth surface of 1-2 m with
    +-30 mm noise and 3 % holes (table path), and small rectangles of 50000..65535 (their tiles and the tiles whose halo they touch
    take the general path).  Rectangles alone never put a tile AT the decision's edge, so 48 of the remaining table tiles get a hole
    beside their middle and next to it one pixel of 46341 (spread exactly 46341: general; the hole's weight for it is +inf and 0 * inf makes
    it 0) or of 46340 (spread 46340: table; an ordinary zero weight, the pixel keeps its value and is clamped to 32767)."""
    rows, cols = 2016, 400
    rng = _rng("mixed_walk")
    y, x = np.mgrid[0:rows, 0:cols]
    d = 1500 + 450 * np.sin(x / 61.0) * np.cos(y / 173.0) + rng.integers(-30, 31, (rows, cols))
    d[rng.random((rows, cols)) < 0.03] = 0
    for _ in range(MIXED_WALK_RECTANGLES):
        h, w = int(rng.integers(1, 21)), int(rng.integers(1, 13))
        y0, x0 = int(rng.integers(0, rows - h + 1)), int(rng.integers(0, cols - w + 1))
        d[y0:y0 + h, x0:x0 + w] = rng.integers(50000, 65536, (h, w))
    d = np.ascontiguousarray(d, np.uint16)
    if with_edge_pixels:
        for k, (r, c) in enumerate(mixed_walk_edge_pixels(d)):
            d[r, c - 1] = 0
            d[r, c] = WRAP if k % 2 == 0 else WRAP - 1
    return d


def mixed_walk_edge_pixels(d):
    """(row, col) of the edge pixels: the middle of every `stride`-th tile that is a table tile without them, spread over all three walk positions"""
    classes = tile_classes(d).reshape(-1)
    tx = -(-d.shape[1] // TILE_X)
    table = np.flatnonzero(~classes)
    picks = table[::len(table) // MIXED_WALK_EDGE_TILES][:MIXED_WALK_EDGE_TILES]
    return [(int(t // tx) * TILE_Y + TILE_Y // 2, int(t % tx) * TILE_X + TILE_X // 2) for t in picks]


GAP_FAR_PIXELS = ((10, 5), (31, 15), (37, 20))   # (row, col): inside tile (0, 0); its last row and column, in every tile's halo; next to the clipped corner


def gap(g):
    """(40, 24), 2 x 2 tiles: constant 1000 with three isolated pixels at 1000 + g"""
    d = np.full((40, 24), 1000, np.uint16)
    for r, c in GAP_FAR_PIXELS:
        d[r, c] = 1000 + g
    return d


def high_clamp():
    """(48, 40), uniform in 30000..33999: the table path on both sides of the 32767 clamp"""
    return _rng("high_clamp").integers(30000, 34000, (48, 40)).astype(np.uint16)


def top_of_range():
    """(48, 40), uniform in 65000..65535: the table path with tile values next to the sentinel"""
    return _rng("top_of_range").integers(65000, 65536, (48, 40)).astype(np.uint16)


def isolated_border():
    """(40, 40): constant 1000, last column 3000, last row 5000, every second pixel of column cols - 2 at 1400.  A pixel of the last
    column or row is a centre and never a tap, and here every real tap is 395 or more away from it: sum2 == 0."""
    d = np.full((40, 40), 1000, np.uint16)
    d[0::2, -2] = 1400
    d[:, -1] = 3000
    d[-1, :] = 5000
    return d


BILATERAL_SHAPES = ((1, 1), (1, 9), (9, 1), (2, 2), (7, 7), (13, 15), (33, 17), (31, 33), (45, 201))


def shape_noise(rows, cols):
    """+-200 mm noise around 1100"""
    return (1100 + _rng("shapes", rows, cols).integers(-200, 201, (rows, cols))).astype(np.uint16)


def bilateral_cases():
    """{name: depth}; `BILATERAL_NOISE` names the ones with noise in them (the __expf allowance of the oracle-versus-reference check)"""
    cases = {"mixed_walk": mixed_walk(), "gap_46340": gap(46340), "gap_46341": gap(46341), "high_clamp": high_clamp(),
             "top_of_range": top_of_range(), "isolated_border": isolated_border()}
    for r, c in BILATERAL_SHAPES:
        cases[f"shapes_{r}x{c}"] = shape_noise(r, c)
    return cases


BILATERAL_NOISE = ("mixed_walk", "high_clamp", "top_of_range") + tuple(f"shapes_{r}x{c}" for r, c in BILATERAL_SHAPES)

# ---- the other kernels ----------------------------------------------------------------------------------------------------------------
PYR_DOWN_ODD_SHAPES = ((2, 2), (3, 3), (5, 7), (9, 16), (121, 161))


def _patches(rng, rows, cols, near_zero):
    """full-range u16 levels in patches of 3 x 3 pixels with +-40 mm noise: the pixels of a patch are within the pyramid's 90 mm cut-off of
    each other, those of different patches almost never -- white noise would cut every tap but the centre off, and no window's extent
    would matter.  The patch grid is anchored at the last row and column, so the last window centre of a line (cols - 2 or cols - 3) shares
    its patch with the last column whatever the parity.  A share `near_zero` of the patches lies within 90 mm of zero (of the -1 an LDS tile holds outside the image)."""
    pr, pc = -(-rows // 3), -(-cols // 3)
    base = rng.integers(0, 65536, (pr, pc))
    low = rng.random((pr, pc)) < near_zero
    base[low] = rng.integers(1, 45, int(low.sum()))
    d = np.kron(base, np.ones((3, 3), np.int64))[-rows:, -cols:] + rng.integers(-40, 41, (rows, cols))
    return np.clip(d, 0, 65535)


def pyr_down_odd(rows, cols):
    """full-range u16 noise, in patches (`_patches`)"""
    return _patches(_rng("pyr_down_odd", rows, cols), rows, cols, 0.0).astype(np.uint16)


PYRAMID_FUSED_SIZES = ((8, 8), (40, 24), (24, 40), (72, 56))   # (cols, rows): multiples of 8, none a multiple of 16 in both directions


def pyramid_fused(cols, rows):
    """full-range u16 noise in patches (`_patches`, 25 % of them near zero) with 20 % zeros, not bilateral-filtered: the 90 mm cut-off
    falls both ways, holes are window centres, and border windows have centres within 90 mm of the -1 cells beside them"""
    rng = _rng("pyramid_fused", cols, rows)
    d = _patches(rng, rows, cols, 0.25)
    d[rng.random((rows, cols)) < 0.2] = 0
    return d.astype(np.uint16)


def pyr_down_model(src, outside_counts=False, last_column=True):
    """numpy restatement of pyrDown for the CPU test's case conditions (not a reference: float64 sums).  `outside_counts`: a cell outside
    the source is a -1 that is compared with the centre like any tap, instead of being skipped; `last_column=False`: the window stops one
    column short of the source's last.  Either slip must change outputs of a case that claims to reach it."""
    src = np.asarray(src).astype(np.int64)
    srows, scols = src.shape
    w = (0.375, 0.25, 0.0625)
    dst = np.zeros((srows // 2, scols // 2), np.int64)
    for y in range(srows // 2):
        for x in range(scols // 2):
            centre, s, wall = src[2 * y, 2 * x], 0.0, 0.0
            for yi in range(-2, 3):
                for xi in range(-2, 3):
                    yy, xx = 2 * y + yi, 2 * x + xi
                    inside = 0 <= yy < srows and 0 <= xx < (scols if last_column else scols - 1)
                    if not inside and not (outside_counts and not (0 <= yy < srows and 0 <= xx < scols)):
                        continue
                    val = src[yy, xx] if inside else -1
                    if abs(val - centre) < 90:
                        s += val * w[abs(xi)] * w[abs(yi)]
                        wall += w[abs(xi)] * w[abs(yi)]
            dst[y, x] = int(s / wall) & 0xffff if wall else 0
    return dst.astype(np.uint16)


TINY_U8_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5))


def tiny_u8(rows, cols):
    return _rng("tiny_u8", rows, cols).integers(0, 256, (rows, cols)).astype(np.uint8)


GAUSS_SMALL_SHAPES = ((2, 2), (3, 5), (5, 3), (4, 6), (9, 13))


def gauss_small_u8(rows, cols):
    return _rng("gauss_small_u8", rows, cols).integers(0, 256, (rows, cols)).astype(np.uint8)


def gauss_small_f32(rows, cols):
    """uniform 0.4..6 m with 30 % NaN"""
    rng = _rng("gauss_small_f32", rows, cols)
    d = rng.uniform(0.4, 6.0, (rows, cols)).astype(np.float32)
    d[rng.random((rows, cols)) < 0.3] = np.nan
    return d


RESIZE_ODD_ROWS = (7, 10)   # (in_rows, in_cols)


def resize_odd_rows():
    """a (3 * 7, 10) map with 20 % NaN in the x plane, for the vertex and the normal form"""
    rows, cols = RESIZE_ODD_ROWS
    rng = _rng("resize_odd_rows")
    m = rng.uniform(-2.0, 2.0, (3 * rows, cols)).astype(np.float32)
    m[:rows][rng.random((rows, cols)) < 0.2] = np.nan
    return m
