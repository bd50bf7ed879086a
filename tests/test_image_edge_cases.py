"""CPU: the cases of tests/image_edge_cases.py are what they claim to be -- so that a later change of a seed or a builder cannot empty
one -- and, where oracle/_ref can be had, the oracle agrees with the reference's own kernels on every one of them, so the expectations
that tests/test_gpu_image_edges.py holds the HIP kernels to are the reference's."""
import numpy as np
import pytest

import image_edge_cases as E

needs_ref = pytest.mark.skipif(not __import__("oracle.ref", fromlist=["available"]).available(), reason="oracle/_ref is not built and the reference's sources are not here to build it from")


@pytest.fixture(scope="module")
def R():
    from oracle import ref
    ref.build()
    ref.lib()
    return ref


@pytest.fixture(scope="module")
def bilateral():
    return E.bilateral_cases()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_builders_are_deterministic_and_typed(bilateral):
    again = E.bilateral_cases()
    assert list(again) == list(bilateral) and len(bilateral) == 6 + len(E.BILATERAL_SHAPES)
    for name, d in bilateral.items():
        assert d.dtype == np.uint16 and d.flags.c_contiguous and same(d, again[name]), name
    assert bilateral["mixed_walk"].shape == (2016, 400) and bilateral["gap_46340"].shape == bilateral["gap_46341"].shape == (40, 24)
    assert bilateral["high_clamp"].shape == bilateral["top_of_range"].shape == (48, 40) and bilateral["isolated_border"].shape == (40, 40)
    for r, c in E.BILATERAL_SHAPES:
        d = bilateral[f"shapes_{r}x{c}"]
        assert d.shape == (r, c) and 900 <= d.min() and d.max() <= 1300
    # odd cols (the unpacked store), cols < 16, rows < 32, and one more than a tile in each direction
    assert any(c % 2 for _, c in E.BILATERAL_SHAPES) and any(c < 16 for _, c in E.BILATERAL_SHAPES) and any(r < 32 for r, _ in E.BILATERAL_SHAPES)
    assert (33, 17) in E.BILATERAL_SHAPES and (1, 1) in E.BILATERAL_SHAPES
    for builder, shapes, dtype in ((E.pyr_down_odd, E.PYR_DOWN_ODD_SHAPES, np.uint16), (E.tiny_u8, E.TINY_U8_SHAPES, np.uint8),
                                   (E.gauss_small_u8, E.GAUSS_SMALL_SHAPES, np.uint8), (E.gauss_small_f32, E.GAUSS_SMALL_SHAPES, np.float32)):
        for r, c in shapes:
            a = builder(r, c)
            assert a.shape == (r, c) and a.dtype == dtype and a.flags.c_contiguous and same(a, builder(r, c)), (builder.__name__, r, c)
    assert any(r % 2 and c % 2 for r, c in E.PYR_DOWN_ODD_SHAPES) and all(r % 2 or c % 2 or (r, c) == (2, 2) for r, c in E.PYR_DOWN_ODD_SHAPES)
    for c, r in E.PYRAMID_FUSED_SIZES:
        d = E.pyramid_fused(c, r)
        assert d.shape == (r, c) and d.dtype == np.uint16 and c % 8 == 0 and r % 8 == 0 and (c % 16 or r % 16) and same(d, E.pyramid_fused(c, r))
        assert 0.1 <= (d == 0).mean() <= 0.35 and d.max() > 60000
    m = E.resize_odd_rows()
    rows, cols = E.RESIZE_ODD_ROWS
    assert m.shape == (3 * rows, cols) and m.dtype == np.float32 and rows % 2 == 1 and cols % 2 == 0 and same(m, E.resize_odd_rows())
    assert 0.1 <= np.isnan(m[:rows]).mean() <= 0.35 and not np.isnan(m[rows:]).any()
    f = E.gauss_small_f32(9, 13)
    assert 0.15 <= np.isnan(f).mean() <= 0.45 and np.nanmin(f) >= 0.4 and np.nanmax(f) <= 6.0


def test_tile_classes_restates_the_decision():
    """hand-made tiles: the halo counts, the last column and row count as centres only, 46340 is table and 46341 is general"""
    d = np.full((64, 48), 1000, np.uint16)
    assert E.tile_classes(d).shape == (2, 3) and not E.tile_classes(d).any()
    d[5, 21] = 1000 + 46341                       # column 21 = tile column 1, and the last halo column (15 + 6) of tile column 0
    assert E.tile_classes(d).tolist() == [[True, True, False], [False, False, False]]
    d[5, 21] = 1000 + 46340
    assert not E.tile_classes(d).any()
    d[5, 21] = 1000
    d[5, 22] = 60000                              # one past the halo of tile column 0
    assert E.tile_classes(d).tolist() == [[False, True, False], [False, False, False]]
    d[5, 22] = 1000
    d[38, 26] = 60000                             # tile (1, 1); first halo column of tile column 2 (32 - 6), first row past the halo of tile row 0 (31 + 6 + 1)
    assert E.tile_classes(d).tolist() == [[False, False, False], [False, True, True]]
    d[38, 26] = 1000
    d[37, 47] = 60000                             # last column: a centre of tile (1, 2), a tap of nobody -- although it lies in the halo of tile (0, 2)
    assert E.tile_classes(d).tolist() == [[False, False, False], [False, False, True]]
    d[37, 47] = 1000
    d[63, 15] = 60000                             # last row, last column of tile column 0: in tile (1, 1)'s halo columns, but no tap
    assert E.tile_classes(d).tolist() == [[False, False, False], [True, False, False]]
    assert E.tile_classes(np.zeros((1, 1), np.uint16)).tolist() == [[False]]
    assert E.walk_positions(1575).tolist() == [0] * 768 + [1] * 768 + [2] * 39 and not E.walk_positions(768).any()
    assert E.tile_of_pixels((33, 17)).max() == 3 and E.tile_of_pixels((33, 17))[32, 16] == 3 and E.tile_of_pixels((33, 17))[31, 15] == 0


def test_mixed_walk_conditions(bilateral, oracle_mod):
    classes = E.tile_classes(bilateral["mixed_walk"])
    n = classes.size
    assert classes.shape == (63, 25) and n > E.WALK
    general = int(classes.sum())
    trans = E.walk_transitions(classes)
    print("mixed_walk: tiles", n, "general", general, "table", n - general, "transitions", trans)
    assert general >= 0.1 * n and n - general >= 0.1 * n
    assert sum(trans.values()) == n - E.WALK
    for k, v in trans.items():
        assert v >= 20, (k, v)
    d = bilateral["mixed_walk"]
    base = d[(d < 40000) & (d > 0)]
    assert 0.02 <= (d == 0).mean() <= 0.04 and base.min() >= 1000 and base.max() <= 2000 and 0.001 < (d >= 50000).mean() < 0.05
    # the decision's own edge inside the walk: tiles whose spread is exactly 46341 (general) and exactly 46340 (table), at more than one walk position
    spreads = E.tile_spreads(d).reshape(-1)
    pos = E.walk_positions(n)
    for s in (E.WRAP, E.WRAP - 1):
        assert int((spreads == s).sum()) >= 20 and len(set(pos[spreads == s])) >= 2, (s, int((spreads == s).sum()))
    plain = E.tile_classes(E.mixed_walk(with_edge_pixels=False))
    assert np.array_equal(plain.reshape(-1) != classes.reshape(-1), spreads == E.WRAP)      # an edge pixel changes the class of its own tile only
    o = oracle_mod.bilateral_filter(d)
    for k, (r, c) in enumerate(E.mixed_walk_edge_pixels(E.mixed_walk(with_edge_pixels=False))):
        assert d[r, c] == (E.WRAP if k % 2 == 0 else E.WRAP - 1) and d[r, c - 1] == 0
        # the hole weighs +inf for a centre of 46341 (0 * inf: the pixel becomes 0) and an ordinary zero for one of 46340 (it keeps its value, clamped)
        assert o[r, c] == (0 if k % 2 == 0 else 32767) and o[r, c - 1] == 0, (k, r, c, o[r, c], o[r, c - 1])


def test_gap_conditions(bilateral, oracle_mod):
    lo, hi = bilateral["gap_46340"], bilateral["gap_46341"]
    assert int((lo != 1000).sum()) == int((hi != 1000).sum()) == 3 and lo.max() == 47340 and hi.max() == 47341
    assert not E.tile_classes(lo).any()
    far_tiles = {int(E.tile_of_pixels(hi.shape)[r, c]) for r, c in E.GAP_FAR_PIXELS}
    assert len(far_tiles) >= 2 and all(E.tile_classes(hi).reshape(-1)[t] for t in far_tiles)
    olo, ohi = oracle_mod.bilateral_filter(lo), oracle_mod.bilateral_filter(hi)
    rows, cols = lo.shape
    near = np.zeros(lo.shape, bool)
    for r, c in E.GAP_FAR_PIXELS:
        assert 0 < r < rows - 1 and 0 < c < cols - 1            # a tap of its neighbours, not only a centre
        assert olo[r, c] == 32767 and ohi[r, c] == 0, (r, c, olo[r, c], ohi[r, c])
        box = np.s_[max(r - 6, 0):r + 7, max(c - 6, 0):c + 7]
        near[box] = True
        assert (olo[box] != ohi[box]).any(), (r, c)
        # at 46340 the far tap weighs an ordinary zero: the neighbours keep 1000; at 46341 it weighs +inf: inf / inf makes them 0
        assert ((olo[box] == 1000) | (lo[box] != 1000)).all() and (ohi[box] == 0).all(), (r, c)
    assert same(olo[~near], ohi[~near]) and (olo[~near] == 1000).all()


def test_other_bilateral_conditions(bilateral, oracle_mod):
    d = bilateral["high_clamp"]
    assert not E.tile_classes(d).any() and d.min() >= 30000 and d.max() <= 33999
    o = oracle_mod.bilateral_filter(d)
    assert (o == 32767).mean() >= 0.1 and ((o < 32767) & (o > 0)).mean() >= 0.1 and o.max() == 32767
    d = bilateral["top_of_range"]
    assert not E.tile_classes(d).any() and d.min() >= 65000 and d.max() > 65500
    assert (oracle_mod.bilateral_filter(d)[:-1, :-1] == 32767).all()
    d = bilateral["isolated_border"]
    rows, cols = d.shape
    assert not E.tile_classes(d).any() and (d[:-1, -1] == 3000).all() and (d[-1] == 5000).all() and (d[0:-1:2, -2] == 1400).all() and (d[1:-1:2, -2] == 1000).all()
    o = oracle_mod.bilateral_filter(d)
    assert int((o[:, -1] == 0).sum()) >= rows // 2      # 0 / 0: every real tap is 395 or more away from the centre
    assert (o[:-8, :-8] == 1000).all()
    for name in bilateral:
        if name.startswith("shapes_"):
            assert not E.tile_classes(bilateral[name]).any(), name


def test_pyramid_case_conditions(oracle_mod):
    """`pyr_down_model` equals the oracle on every case, and the two slips it can make change outputs of the cases that claim to reach them:
    a window that stops short of the last column (every pyr_down_odd shape) and outside cells that count as -1 taps (every level of every
    pyramid_fused size)"""
    for r, c in E.PYR_DOWN_ODD_SHAPES:
        d = E.pyr_down_odd(r, c)
        m = E.pyr_down_model(d)
        assert same(oracle_mod.pyr_down(d), m), (r, c)
        assert (E.pyr_down_model(d, last_column=False) != m).any(), (r, c)
        assert d.max() - d.min() > 30000 or d.size <= 9
    for c, r in E.PYRAMID_FUSED_SIZES:
        cur = E.pyramid_fused(c, r)
        for l in range(3):
            m = E.pyr_down_model(cur)
            assert same(oracle_mod.pyr_down(cur), m), (c, r, l)
            assert (E.pyr_down_model(cur, outside_counts=True) != m).any(), (c, r, l)
            centres = cur[0::2, 0::2]
            assert l > 0 or (centres == 0).sum() >= 2                      # holes as window centres
            cur = m


# ---- the oracle against the reference's own kernels on every case -------------------------------------------------------------------------------
@needs_ref
def test_oracle_vs_ref_bilateral(bilateral, oracle_mod, R):
    for name, d in bilateral.items():
        o, r = oracle_mod.bilateral_filter(d), R.bilateral_filter(d)
        bad = int((o != r).sum())
        print(name, "oracle != reference in", bad, "of", d.size)
        if name in E.BILATERAL_NOISE:
            # the __expf allowance test_oracle_vs_ref.py states for noise: the last bit of a weight flips a tie of rn(sum1 / sum2)
            assert bad <= max(2, d.size // 2000) and int(np.abs(o.astype(int) - r.astype(int)).max(initial=0)) <= 1, (name, bad)
        else:
            assert same(o, r), (name, bad)


@needs_ref
def test_oracle_vs_ref_other_kernels(oracle_mod, R):
    O = oracle_mod
    from oracle.oracle import OIntr
    for r, c in E.PYR_DOWN_ODD_SHAPES:
        d = E.pyr_down_odd(r, c)
        assert same(O.pyr_down(d), R.pyr_down(d)), ("pyr_down_odd", r, c)
    for c, r in E.PYRAMID_FUSED_SIZES:
        cur = E.pyramid_fused(c, r)
        for l in range(4):
            intr = OIntr(0.9 * c, 0.9 * c, 0.5 * c - 0.5, 0.5 * r - 0.5).level(l)
            v = O.create_vmap(intr, cur)
            assert same(v, R.create_vmap(intr, cur)) and same(O.create_nmap(v), R.create_nmap(v)), ("pyramid_fused maps", c, r, l)
            if l < 3:
                nxt = O.pyr_down(cur)
                assert same(nxt, R.pyr_down(cur)), ("pyramid_fused", c, r, l)
                cur = nxt
    for r, c in E.TINY_U8_SHAPES:
        img = E.tiny_u8(r, c)
        (a, b), (a2, b2) = O.derivative_images(img), R.derivative_images(img)
        assert same(a, a2) and same(b, b2), ("tiny_u8", r, c)
    for r, c in E.GAUSS_SMALL_SHAPES:
        u, f = E.gauss_small_u8(r, c), E.gauss_small_f32(r, c)
        assert same(O.pyr_down_gauss_u8(u), R.pyr_down_gauss_u8(u)), ("gauss_small u8", r, c)
        a, b = O.pyr_down_gauss_f32(f), R.pyr_down_gauss_f32(f)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and same(a[~np.isnan(a)], b[~np.isnan(b)]), ("gauss_small f32", r, c)
    m = E.resize_odd_rows()
    pre = np.full((3 * (E.RESIZE_ODD_ROWS[0] // 2), E.RESIZE_ODD_ROWS[1] // 2), 7.0, np.float32)
    for normalize in (False, True):
        assert same(O.resize_map(m, normalize, out=pre.copy()), R.resize_map(m, normalize, out=pre.copy())), ("resize_odd_rows", normalize)
