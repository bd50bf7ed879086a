"""GPU parity at the edges of the image side (csrc/kt_image.hip, csrc/kt_pyramid.hpp) on the cases of tests/image_edge_cases.py, bit for
bit against the oracle: the bilateral filter's two paths in one image and in one workgroup's walk, the 46340 / 46341 decision, the table
path above 32767 and on 0 / 0, odd and tiny shapes; pyrDown on odd sources; the fused pyramid on unfiltered full-range depth down to 8 x 8;
the derivative images, the Gauss pyramids and the map resize on their smallest shapes.  Every output buffer is a pattern with 64 guard
elements behind it.  tests/test_image_edge_cases.py (CPU) asserts that the cases reach what they are meant to reach and that the oracle
equals the reference's own kernels on them."""
import numpy as np
import pytest

import image_edge_cases as E

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN16 = 0xA5A5     # above 32767: no output of the bilateral filter


@pytest.fixture(scope="module")
def bilateral(oracle_mod):
    """{name: (depth, the oracle's output)}, computed once"""
    return {name: (d, oracle_mod.bilateral_filter(d)) for name, d in E.bilateral_cases().items()}


def _guarded(ctx, n, dtype, pattern):
    return ctx.upload(np.full(n + GUARD, pattern, dtype))


def _take(ctx, buf, shape, dtype, pattern, what):
    n = int(np.prod(shape))
    out = ctx.download(buf, dtype, (n + GUARD,))
    assert np.array_equal(out[n:].view(np.uint8), np.full(GUARD, pattern, dtype).view(np.uint8)), f"{what}: guard behind the output overwritten"
    return out[:n].reshape(shape)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _same_maps(a, b):
    """float maps: the same NaN positions (sign and payload of a NaN are the machine's) and the same bits everywhere else"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _launch_bilateral(ctx, d):
    rows, cols = d.shape
    dst = _guarded(ctx, d.size, np.uint16, PATTERN16)
    ctx.bilateral_filter(ctx.upload(d), dst, cols, rows)
    return dst


def _bilateral_report(name, d, ref, got):
    """where the mismatches and the surviving pattern values are: per tile class and per position in a workgroup's walk"""
    bad, stale = ref != got, got == PATTERN16
    classes = E.tile_classes(d).reshape(-1)
    tile = E.tile_of_pixels(d.shape)
    general, pos = classes[tile], E.walk_positions(classes.size)[tile]
    msg = [f"{name} {d.shape}: {int(bad.sum())} mismatches, {int(stale.sum())} pattern values left, {int(classes.sum())} of {classes.size} tiles general"]
    msg.append(f"table path {int((bad & ~general).sum())} / {int((~general).sum())} pixels, general path {int((bad & general).sum())} / {int(general.sum())}")
    for p in range(int(pos.max()) + 1):
        msg.append(f"walk position {p}: {int((bad & (pos == p)).sum())} mismatches ({int((bad & (pos == p) & general).sum())} general), "
                   f"{int((stale & (pos == p)).sum())} pattern values, of {int((pos == p).sum())} pixels")
    if bad.any():
        y, x = np.argwhere(bad)[0]
        msg.append(f"first at (row {y}, col {x}): input {d[y, x]}, oracle {ref[y, x]}, kernel {got[y, x]}, bad tiles {np.unique(tile[bad])[:12].tolist()}")
    return "; ".join(msg)


def _check_bilateral(ctx, name, d, ref, dst):
    got = _take(ctx, dst, d.shape, np.uint16, PATTERN16, name)
    assert not (got == PATTERN16).any() and np.array_equal(ref.view(np.uint8), got.view(np.uint8)), _bilateral_report(name, d, ref, got)
    return got


BILATERAL_NAMES = ["mixed_walk", "gap_46340", "gap_46341", "high_clamp", "top_of_range", "isolated_border"] + [f"shapes_{r}x{c}" for r, c in E.BILATERAL_SHAPES]


@pytest.mark.parametrize("name", BILATERAL_NAMES)
def test_bilateral_case(ctx, bilateral, name):
    d, ref = bilateral[name]
    _check_bilateral(ctx, name, d, ref, _launch_bilateral(ctx, d))


def test_bilateral_case_list_is_complete(bilateral):
    assert sorted(bilateral) == sorted(BILATERAL_NAMES)


def test_mixed_walk_twice(ctx, bilateral):
    """two launches on one context: a missing barrier between a workgroup's tiles shows as a difference between runs or against the oracle"""
    d, ref = bilateral["mixed_walk"]
    a, b = _launch_bilateral(ctx, d), _launch_bilateral(ctx, d)
    ga = _check_bilateral(ctx, "mixed_walk (first run)", d, ref, a)
    gb = _check_bilateral(ctx, "mixed_walk (second run)", d, ref, b)
    assert _same(ga, gb)


@pytest.mark.parametrize("order", [("gap_46341", "gap_46340"), ("gap_46340", "gap_46341")])
def test_gap_back_to_back(ctx, bilateral, order):
    """nothing of one launch's tile class leaks into the next launch on the same context"""
    bufs = [_launch_bilateral(ctx, bilateral[name][0]) for name in order]
    for name, buf in zip(order, bufs):
        _check_bilateral(ctx, f"{name} in {order}", *bilateral[name], buf)
    # ... and the two do differ where they should: the 13 x 13 neighbourhood of a far pixel
    lo, hi = bilateral["gap_46340"][1], bilateral["gap_46341"][1]
    r, c = E.GAP_FAR_PIXELS[0]
    assert lo[r, c] == 32767 and hi[r, c] == 0 and (lo[r - 6:r + 7, max(c - 6, 0):c + 7] != hi[r - 6:r + 7, max(c - 6, 0):c + 7]).all()


@pytest.mark.parametrize("shape", E.PYR_DOWN_ODD_SHAPES)
def test_pyr_down_odd(ctx, oracle_mod, shape):
    rows, cols = shape
    d = E.pyr_down_odd(rows, cols)
    ref = oracle_mod.pyr_down(d)
    assert ref.shape == (rows // 2, cols // 2)
    for pattern in (0xA5A5, 0x5A5A):        # full-range noise: an output may equal one pattern, not both
        dst = _guarded(ctx, ref.size, np.uint16, pattern)
        ctx.pyr_down(ctx.upload(d), cols, rows, dst)
        got = _take(ctx, dst, ref.shape, np.uint16, pattern, f"pyr_down {shape}")
        assert _same(ref, got), (shape, int((ref != got).sum()), np.argwhere(ref != got)[:4].tolist())


@pytest.mark.parametrize("size", E.PYRAMID_FUSED_SIZES)
def test_pyramid_fused(ctx, oracle_mod, size):
    """kt_build_pyramid == pyrDown x 3 + createVMap x 4 + createNMap x 4 of the oracle over pre-filled planes (stale-plane semantics), on
    unfiltered full-range depth with holes: the LDS form's skipped -1 cells against the reference's clipped windows"""
    from kintinuous_amd.abi import Intr
    from oracle.oracle import OIntr
    cols, rows = size
    fx, fy, cx, cy = 0.9 * cols, 0.9 * cols, 0.5 * cols - 0.5, 0.5 * rows - 0.5
    depths = [E.pyramid_fused(cols, rows)]
    for l in range(3):
        depths.append(oracle_mod.pyr_down(depths[-1]))
    rng = np.random.default_rng(cols * 1000 + rows)
    pre = [rng.uniform(-1, 1, (3 * (rows >> l), cols >> l)).astype(np.float32) for l in range(4)]
    vref = [oracle_mod.create_vmap(OIntr(fx, fy, cx, cy).level(l), depths[l], out=pre[l].copy()) for l in range(4)]
    nref = [oracle_mod.create_nmap(vref[l], out=pre[l].copy()) for l in range(4)]
    tail = np.full(GUARD, -7.0, np.float32)
    gd = [_guarded(ctx, depths[l].size, np.uint16, 0xA5A5) for l in range(1, 4)]
    gv = [ctx.upload(np.concatenate([pre[l].reshape(-1), tail])) for l in range(4)]
    gn = [ctx.upload(np.concatenate([pre[l].reshape(-1), tail])) for l in range(4)]
    ctx.build_pyramid(Intr(fx, fy, cx, cy), ctx.upload(depths[0]), cols, rows, gd, gv, gn)
    ctx.sync()
    for l in range(1, 4):
        got = _take(ctx, gd[l - 1], depths[l].shape, np.uint16, 0xA5A5, f"{size} depth level {l}")
        assert _same(depths[l], got), (size, f"depth level {l}", int((depths[l] != got).sum()), np.argwhere(depths[l] != got)[:4].tolist())
    for l in range(4):
        v = _take(ctx, gv[l], pre[l].shape, np.float32, -7.0, f"{size} vmap level {l}")
        n = _take(ctx, gn[l], pre[l].shape, np.float32, -7.0, f"{size} nmap level {l}")
        assert _same_maps(vref[l], v), (size, f"vmap level {l}")
        assert _same_maps(nref[l], n), (size, f"nmap level {l}")
    if size == (8, 8):      # level 3 is one pixel: the last column and row at once, its normal is NaN
        assert depths[3].shape == (1, 1) and np.isnan(nref[3][0, 0]) and _same(nref[3][1:], pre[3][1:])


@pytest.mark.parametrize("shape", E.TINY_U8_SHAPES)
def test_derivative_images_tiny(ctx, oracle_mod, shape):
    rows, cols = shape
    img = E.tiny_u8(rows, cols)
    dx, dy = oracle_mod.derivative_images(img)
    gx, gy = _guarded(ctx, img.size, np.int16, 0x5A5A), _guarded(ctx, img.size, np.int16, 0x5A5A)
    ctx.derivative_images(ctx.upload(img), cols, rows, gx, gy)
    hx, hy = _take(ctx, gx, shape, np.int16, 0x5A5A, f"dx {shape}"), _take(ctx, gy, shape, np.int16, 0x5A5A, f"dy {shape}")
    assert _same(dx, hx) and _same(dy, hy), (shape, img.tolist(), dx.tolist(), hx.tolist(), dy.tolist(), hy.tolist())


@pytest.mark.parametrize("shape", E.GAUSS_SMALL_SHAPES)
def test_gauss_pyramids_small(ctx, oracle_mod, shape):
    rows, cols = shape
    u = E.gauss_small_u8(rows, cols)
    ref = oracle_mod.pyr_down_gauss_u8(u)
    for pattern in (0xA5, 0x5A):
        dst = _guarded(ctx, ref.size, np.uint8, pattern)
        ctx.pyr_down_gauss_u8(ctx.upload(u), cols, rows, dst)
        got = _take(ctx, dst, ref.shape, np.uint8, pattern, f"gauss u8 {shape}")
        assert _same(ref, got), (shape, ref.tolist(), got.tolist())
    f = E.gauss_small_f32(rows, cols)
    ref = oracle_mod.pyr_down_gauss_f32(f)
    dst = _guarded(ctx, ref.size, np.float32, -7.0)
    ctx.pyr_down_gauss_f32(ctx.upload(f), cols, rows, dst)
    got = _take(ctx, dst, ref.shape, np.float32, -7.0, f"gauss f32 {shape}")
    assert _same_maps(ref, got) and not (got == -7.0).any(), (shape, ref.tolist(), got.tolist())


@pytest.mark.parametrize("normalize", [False, True])
def test_resize_odd_rows(ctx, oracle_mod, normalize):
    """in_rows = 7: the planes of the input are 7 rows apart, those of the output 3"""
    rows, cols = E.RESIZE_ODD_ROWS
    m = E.resize_odd_rows()
    pre = np.random.default_rng(3).uniform(-1, 1, (3 * (rows // 2), cols // 2)).astype(np.float32)
    ref = oracle_mod.resize_map(m, normalize, out=pre.copy())
    dst = ctx.upload(np.concatenate([pre.reshape(-1), np.full(GUARD, -7.0, np.float32)]))
    (ctx.resize_nmap if normalize else ctx.resize_vmap)(ctx.upload(m), cols, rows, dst)
    got = _take(ctx, dst, pre.shape, np.float32, -7.0, f"resize normalize={normalize}")
    assert _same_maps(ref, got), (normalize, int((ref.view(np.uint32) != got.view(np.uint32)).sum()))
    assert np.isnan(ref[:rows // 2]).any() and np.isfinite(ref[:rows // 2]).any()


def test_refused_sizes_write_nothing(ctx):
    """odd in_cols for the resize and a size that is no multiple of 8 for the fused pyramid are refused by contract: KT_ERR_ARG, no launch"""
    from kintinuous_amd import abi
    src = ctx.upload(np.ones((3 * 6, 9), np.float32))
    for call in (ctx.resize_vmap, ctx.resize_nmap):
        dst = _guarded(ctx, 3 * 3 * 4, np.float32, -7.0)
        with pytest.raises(abi.KtError) as e:
            call(src, 9, 6, dst)
        assert e.value.status == abi.KT_ERR_ARG
        assert (_take(ctx, dst, (9, 4), np.float32, -7.0, "refused resize") == -7.0).all()
    for cols, rows in ((12, 8), (8, 12)):
        d0 = ctx.upload(np.full((rows, cols), 1000, np.uint16))
        gd = [_guarded(ctx, (rows >> l) * (cols >> l), np.uint16, 0xA5A5) for l in range(1, 4)]
        gv = [_guarded(ctx, 3 * (rows >> l) * (cols >> l), np.float32, -7.0) for l in range(4)]
        gn = [_guarded(ctx, 3 * (rows >> l) * (cols >> l), np.float32, -7.0) for l in range(4)]
        with pytest.raises(abi.KtError) as e:
            ctx.build_pyramid(abi.Intr(10.0, 10.0, 5.5, 3.5), d0, cols, rows, gd, gv, gn)
        assert e.value.status == abi.KT_ERR_ARG
        ctx.sync()
        for l in range(1, 4):
            assert (_take(ctx, gd[l - 1], ((rows >> l) * (cols >> l),), np.uint16, 0xA5A5, "refused pyramid") == 0xA5A5).all()
        for l in range(4):
            for b in (gv[l], gn[l]):
                assert (_take(ctx, b, (3 * (rows >> l) * (cols >> l),), np.float32, -7.0, "refused pyramid") == -7.0).all()
