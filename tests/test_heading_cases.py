"""CPU: the cases of tests/heading_cases.py are what they claim to be -- so that a later change of a seed or a builder cannot empty one -- and,
where oracle/_ref can be had, the oracle agrees with the reference's own kernels on every one of them, so what tests/test_gpu_headings.py
holds the HIP kernels to is the reference's."""
import numpy as np
import pytest

import heading_cases as H

needs_ref = pytest.mark.skipif(not __import__("oracle.ref", fromlist=["available"]).available(), reason="oracle/_ref is not built and the reference's sources are not here to build it from")


@pytest.fixture(scope="module")
def R():
    from oracle import ref
    ref.build()
    ref.lib()
    return ref


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_maps(a, b):
    """float maps: the same NaN positions (a NaN's sign and payload are the machine's) and the same bits everywhere else"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def test_table_covers_its_classes(oracle_mod):
    cases = H.cases()
    assert 36 <= len(cases) <= 48 and H.cases() is cases
    per_class = {cls: [c for c in cases if c.cls == cls] for cls in H.CLASSES}
    assert all(per_class[cls] for cls in H.CLASSES) and sum(len(v) for v in per_class.values()) == len(cases)
    # sizes: 160 x 120 at N = 64 and 96, the ragged 173 x 97 at N = 80, one integer principal point among the axis cases; both wraps
    shapes = {(c.cam, c.N) for c in cases}
    assert {("s", 64), ("s", 96), ("r", 80), ("i", 64)} <= shapes and all(N == 80 for cam, N in shapes if cam == "r")
    ipp = H.camera("i")
    assert any(c.cam == "i" for c in per_class["axis"]) and ipp.cx == int(ipp.cx) and ipp.cy == int(ipp.cy) and (ipp.cols, ipp.rows) == (160, 120)
    assert (H.camera("r").cols, H.camera("r").rows) == (173, 97) and H.camera("s").cy != int(H.camera("s").cy)
    for N in (64, 80, 96):
        wraps = {tuple(c.wrap) for c in cases if c.N == N}
        assert (0, 0, 0) in wraps and any(N - 1 in w for w in wraps), N
    for c in cases:
        assert c.R.dtype == np.float32 and c.t.dtype == np.float32 and c.R.shape == (3, 3) and c.t.shape == (3,)
        R64 = c.R.astype(np.float64)
        assert np.abs(R64 @ R64.T - np.eye(3)).max() < 1e-6 and np.linalg.det(R64) > 0.999, c.name
        assert H.trunc(c.N) == max(0.06, 2.1 * 6.0 / c.N) and H.neighbour(c).cls == c.cls and H.neighbour(c) is not c
        # the branch of kt_clip_halfline that the near plane takes, from the float32 product -- with the transpose's element and with the
        # element of the inverse that the kernels are handed
        Rinv = oracle_mod.mat33_inverse(c.R)
        assert H.clip_branch(c.R[2, 2], c.N) == c.expect["branch"] == H.clip_branch(Rinv[2, 2], c.N) if "branch" in c.expect else c.cls == "oblique", c.name
        if "facing" in c.expect:
            assert np.array_equal(c.R[:, 2], np.asarray(H.AXIS_DIR[c.expect["facing"]], np.float32)) and set(np.unique(np.abs(c.R))) == {0.0, 1.0}, c.name
            assert np.array_equal(Rinv, c.R.T)
        if c.cls == "roll":
            assert np.array_equal(c.R[:, 2], [0, 0, 1]) and set(np.unique(np.abs(c.R))) == {0.0, 1.0} and not np.array_equal(c.R, np.eye(3))
        if c.expect.get("nonzero"):
            assert c.R[2, 2] != 0 and Rinv[2, 2] != 0, c.name
        if "octant" in c.expect:
            assert np.array_equal(np.sign(c.R[:, 2]), c.expect["octant"]) and np.abs(c.R[:, 2]).min() > 0.2 and c.expect["octant"] != (1, 1, 1), c.name
        if "on_voxel" in c.expect:
            k = c.t / np.float32(H.SIZE / 64) - np.float32(0.5)     # exact: the cell is 3 / 32
            assert c.N == 64 and np.array_equal(k, np.round(k)) == c.expect["on_voxel"] and (c.expect["on_voxel"] or np.array_equal(k - np.floor(k), [0.25] * 3)), c.name
        if c.expect.get("outside"):
            off = np.where(c.t < 0, -c.t, np.where(c.t > H.SIZE, c.t - np.float32(H.SIZE), 0))
            assert np.count_nonzero(off) == 1 and abs(off.max() - 0.45) < 1e-6 and not H.inside(c), c.name
            inward = -np.sign(c.t - np.float32(H.SIZE / 2))[np.argmax(off)]
            assert c.R[:, 2][np.argmax(off)] == (-inward if c.expect.get("away") else inward), c.name
        else:
            assert H.inside(c), c.name
    assert {c.expect["facing"] for c in per_class["axis"]} == set(H.AXIS) and {c.expect["facing"] for c in per_class["on_voxel"] if c.expect["on_voxel"]} == set(H.AXIS)
    assert sum(not c.expect["on_voxel"] for c in per_class["on_voxel"]) >= 3
    assert sorted(c.expect["octant"] for c in per_class["oblique"]) == sorted(H.OCTANTS) and len(set(H.OCTANTS)) == 7
    assert len(per_class["roll"]) == 3 and len({c.R.tobytes() for c in per_class["roll"]}) == 3
    for kind in ("yaw", "pitch"):
        got = [c for c in per_class["near_quarter"] if c.name.startswith(kind)]
        assert {c.expect["branch"] for c in got} == {"lo", "hi", "mid"}, kind
        for c in got:   # +-1e-10: the dividing branch with a quotient near 1e11
            bz = abs(float(np.float32(c.R[2, 2]) * (np.float32(H.SIZE) / np.float32(c.N))))
            assert (1e-12 < bz < 2e-11) if "1e-10" in c.name else (5e-6 < bz < 2e-5) if "1e-04" in c.name else (0 < bz < 1e-16), (c.name, bz)
    assert {c.expect["facing"] for c in per_class["outside"] if not c.expect.get("away")} == {"+x", "-x", "+y", "-y", "-z"}
    assert sum(bool(c.expect.get("away")) for c in cases) == 1


def test_frames_are_deterministic():
    for c in H.cases()[::7]:
        for which in (0, 1):
            H._frame.cache_clear()
            R, t, d, rgb = H.frame(c, which)
            H._frame.cache_clear()
            R2, t2, d2, rgb2 = H.frame(c, which)
            cam = H.camera(c.cam)
            assert same(d, d2) and same(rgb, rgb2) and d.shape == (cam.rows, cam.cols) and d.dtype == np.uint16 and rgb.shape == (cam.rows, cam.cols, 3)
            pose = c if which == 0 else H.neighbour(c)
            assert np.array_equal(R, pose.R) and np.array_equal(t, pose.t)
            assert 0.005 < (d == 0).mean()      # the seeded holes are there


def test_cases_are_not_vacuous(oracle_mod):
    """A condition, not a tolerance: every case's own frame updates at least U_FLOOR voxels of an empty volume (looking away: none, and
    nothing changes), and the ray cast of the fused volume from the case's pose finds a surface."""
    smallest = {}
    for c in H.cases():
        (vol, col, scaled, U), (vol2, col2, _, U2) = H.fused(oracle_mod, c)
        assert U == int((col[..., 3] != 0).sum()), c.name      # into an empty volume an update is a weight byte that left 0
        if c.expect.get("away"):
            assert U == 0 and not vol.any() and not col.any(), c.name
            continue
        smallest[c.cls] = min(smallest.get(c.cls, U), U)
        assert U >= H.U_FLOOR, (c.name, U)
        assert (vol < 0).any() and U2 >= 0
        if H.inside(c):     # a camera inside the volume sees what it fused
            cam = H.camera(c.cam)
            v, n, img, S = H.cast(oracle_mod, oracle_mod, c, False, vol2, col2, key="empty")
            assert np.isfinite(v[:cam.rows]).sum() > 1000, (c.name, int(np.isfinite(v[:cam.rows]).sum()))
    print("smallest U per class:", smallest, "cases per class:", {cls: sum(c.cls == cls for c in H.cases()) for cls in H.CLASSES})
    assert set(smallest) == set(H.CLASSES)


@needs_ref
@pytest.mark.parametrize("name", H.names())
def test_oracle_equals_reference(oracle_mod, R, name):
    """integrate (volume, colour volume, scaled depth; both frames) and the ray cast from the case's pose and from a quarter turn on: the maps by
    the NaN-position rule, b / g / r exact, the heat byte outside border voxels (the rule of test_oracle_vs_ref.py::test_raycast)"""
    O = oracle_mod
    c = H.by_name(name)
    N, cam = c.N, H.camera(c.cam)
    vr, cr = np.zeros((N, N, N), np.int16), np.zeros((N, N, N, 4), np.uint8)
    for which, (vo, co, so, U) in enumerate(H.fused(O, c)):
        depth, rgb, nmap, Rinv, t = H.inputs(O, c, which)
        sr = R.integrate_tsdf(depth, H.intr(O, c), [H.SIZE] * 3, Rinv, t, H.trunc(N), vr, c.wrap, cr, rgb, nmap, True)
        assert same(so, sr), f"{name} frame {which}: scaled depth"
        assert same(vo, vr), f"{name} frame {which}: {int((vo != vr).sum())} tsdf words differ"
        assert same(co, cr), f"{name} frame {which}: {int((co != cr).any(axis=-1).sum())} colour / weight words differ"
    cell = np.float32(H.SIZE / N)
    for turned in (False, True):
        (vo_, no_, co_, _), (vr_, nr_, cr_, _) = H.cast(O, O, c, turned, vr, cr), H.cast(R, O, c, turned, vr, cr)
        assert same_maps(vo_, vr_) and same_maps(no_, nr_), (name, turned)
        assert same(co_[..., :3], cr_[..., :3]), (name, turned)
        hit = np.isfinite(vo_[:cam.rows])
        g = np.floor(np.stack([vo_[:cam.rows], vo_[cam.rows:2 * cam.rows], vo_[2 * cam.rows:]], -1) / cell)
        border = hit & ((g <= 0) | (g >= N - 1)).any(axis=-1)
        assert same(co_[..., 3][~border], cr_[..., 3][~border]), (name, turned, int((co_[..., 3] != cr_[..., 3]).sum()))
