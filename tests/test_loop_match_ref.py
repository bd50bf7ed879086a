"""CPU.  The numpy restatement of the loop-closure bootstrap stage (kintinuous_amd/loop_match_ref.py): its table against
the generator, its matcher and inlier count against the independent implementation of tests/loop_match_cases.py, and the whole stage
against the reference's gates on the room pairs -- at least 40 matches, an inlier share above 0.35, a registration score below 0.01 from
its bootstrap for (A, B); a gate's rejection for (A, C).  tests/test_gpu_loop_match.py holds the GPU to this restatement."""
import os

import numpy as np
import pytest

import loop_icp_cases as lc
import loop_match_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_brief_table_matches_generator():
    from kintinuous_amd import brief_table as bt
    text = open(bt.HEADER).read()
    assert text == bt.header_text()
    tab = bt.parse_header(text)
    assert tab.shape == (256, 4) and np.array_equal(tab, bt.build_table())
    assert tab.min() >= -bt.REACH and tab.max() <= bt.REACH and tab.min() == -bt.REACH and tab.max() == bt.REACH
    assert not ((tab[:, 0] == tab[:, 2]) & (tab[:, 1] == tab[:, 3])).any()
    assert len({tuple(r) for r in tab.tolist()}) == 256
    # splitmix64's published first outputs for seed 1234567
    s, a = bt.splitmix64(1234567)
    s, b = bt.splitmix64(s)
    assert (a, b) == (6457827717110365317, 3203168211198807973)


def test_draws_are_distinct_and_spread():
    from kintinuous_amd import loop_match_ref as ref
    for m in (3, 4, 5, 40, 777):
        tri = ref.draw_triples(1, 2000, m)
        assert tri.min() == 0 and tri.max() == m - 1
        assert ((tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])).all()
    assert len({tuple(sorted(t)) for t in ref.draw_triples(1, 2000, 4).tolist()}) == 4      # every triple of four is drawn


def test_matcher_equals_brute_force():
    """random descriptors with planted duplicates, near copies and ties of d1 and d2: index, d1, d2 and the verdict"""
    from kintinuous_amd import loop_match_ref as ref
    rng = np.random.default_rng(4)
    old = rng.integers(0, 2 ** 32, (700, 8), dtype=np.uint64).astype(np.uint32)
    new = rng.integers(0, 2 ** 32, (300, 8), dtype=np.uint64).astype(np.uint32)
    for i in range(0, 120):
        new[i] = old[5 * i]
        new[i, i % 8] ^= np.uint32((1 << (i % 32)) | (1 << ((i * 7) % 32)))
    old[650] = old[10]                       # a duplicate of a matched descriptor: d1 == d2, lowest index
    old[3] = old[651] = new[200] ^ np.array([0, 0, 16, 0, 0, 0, 0, 0], np.uint32)      # two copies one bit away: d1 == d2 == 1
    old[4] = old[652] = new[201]             # exact copies: d1 == d2 == 0, which no ratio accepts
    for kw in (dict(), dict(ratio_num=2, ratio_den=1), dict(max_hamming=1), dict(ratio_num=1, ratio_den=1)):
        p = ref.Params(**kw)
        want = mc.brute_match(new, old, p.max_hamming, p.ratio_num, p.ratio_den)
        got = ref.descriptor_match(new, old, p)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), kw
    assert list(ref.descriptor_match(new, old, ref.Params(ratio_num=2, ratio_den=1))[0][200:202]) == [3, -1]
    got = ref.descriptor_match(new, old[7:8], ref.Params())
    want = mc.brute_match(new, old[7:8], 64, 4, 5)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and (got[2] == ref.NO_SECOND).all()
    # the cross-check: a match list in new order whose pairs are mutual nearest neighbours
    m = ref.match_keypoints(new, old, ref.Params())
    dist = ref.hamming(new, old)
    assert len(m) > 50 and (np.diff(m[:, 0]) > 0).all()
    assert (dist.argmin(axis=1)[m[:, 0]] == m[:, 1]).all() and (dist.argmin(axis=0)[m[:, 1]] == m[:, 0]).all()


PAIR_SIZES = [(160, 120), (640, 480)]


@pytest.mark.parametrize("cols,rows", PAIR_SIZES)
def test_pair_a_b_passes_the_reference_gates(cols, rows):
    from kintinuous_amd import loop_icp_ref, loop_match_ref as ref
    res = mc.restated(cols, rows)
    cam, d_old, _ = mc.frame(cols, rows, "A")
    _, d_new, _ = mc.frame(cols, rows, "B")
    info = res["info"]
    err = lc.pose_error(res["bootstrap"], lc.truth())
    print(f"{cols}x{rows} (A, B): {info}, share {info['n_inliers'] / info['n_matches']:.3f}, bootstrap to the truth {err[0]:.3e} rad {err[1]:.3e} m")
    assert info["n_matches"] >= 40 and info["n_inliers"] / info["n_matches"] > 0.35
    # the final inlier flags against the independent float64 count for the final T, and the winning hypothesis's score likewise
    m = res["match_index"]
    Pn = ref.points3d(res["keypoints_new"][0][m[:, 0]], d_new, cam.fx, cam.fy, cam.cx, cam.cy)
    Po = ref.points3d(res["keypoints_old"][0][m[:, 1]], d_old, cam.fx, cam.fy, cam.cx, cam.cy)
    uv_old = res["matches"][:, :2]
    flags = mc.count_inliers64(res["pose"].astype(np.float64), Pn, uv_old, (cam.fx, cam.fy, cam.cx, cam.cy), 2.0)
    assert int((flags != res["inlier"]).sum()) <= 1          # (the pose went through float32 on its way here: one borderline match may flip)
    tri = ref.draw_triples(1, 500, len(m))[res["info"]["best_hypothesis"]][None]
    R, t, deg = ref.fit_triples(Pn, Po, tri)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R[0], t[0]
    assert not deg[0] and int(mc.count_inliers64(T, Pn, uv_old, (cam.fx, cam.fy, cam.cx, cam.cy), 2.0).sum()) == res["best_score"]
    # the rigid inverse
    assert np.abs(res["bootstrap"].astype(np.float64) @ res["pose"].astype(np.float64) - np.eye(4)).max() < 1e-6
    # the reference's last gate: the registration stage from this bootstrap
    M, score, icp_info = loop_icp_ref.icp_depth_frames(d_old, d_new, cam.fx, cam.fy, cam.cx, cam.cy, res["bootstrap"], lc.LEAF, 4.0, 10)
    print(f"  registration from the bootstrap: score {score:.3e}, {icp_info}")
    assert score < 0.01


@pytest.mark.parametrize("cols,rows", PAIR_SIZES)
def test_pair_a_c_is_rejected(cols, rows):
    res = mc.restated(cols, rows, "A", "C")
    info = res["info"]
    print(f"{cols}x{rows} (A, C): {info}")
    assert info["n_matches"] < 40 or info["n_inliers"] <= 0.35 * info["n_matches"]


def test_selection_order_and_tie_rule():
    """max_keypoints cuts inside a run of equal scores: the kept ones are the first in raster order, and the output is sorted by (score
    descending, raster index ascending)"""
    from kintinuous_amd import loop_match_ref as ref
    grid = [(u, v) for v in range(20, 100, 12) for u in range(20, 140, 12)]
    rgb, depth = mc.blob_frame(160, 120, grid), np.full((120, 160), 1500, np.uint16)
    uv_all, sc_all, _ = ref.frame_keypoints(rgb, depth, ref.Params(max_keypoints=4096))
    uv, sc, desc = ref.frame_keypoints(rgb, depth, ref.Params(max_keypoints=100))
    assert len(uv_all) > 100 and len(set(sc_all.tolist())) == 1 and len(uv) == 100 and desc.shape == (100, 8)
    raster = uv_all[:, 1] * 160 + uv_all[:, 0]
    assert (np.diff(raster) > 0).all() and np.array_equal(uv, uv_all[:100])
    _, d, tex = mc.frame(160, 120, "A")
    uv, sc, _ = ref.frame_keypoints(tex, d, ref.Params())
    key = sc.astype(np.int64) * -(1 << 32) + (uv[:, 1] * 160 + uv[:, 0])
    assert (np.diff(key) > 0).all()
    assert uv[:, 0].min() >= ref.MARGIN and uv[:, 0].max() <= 159 - ref.MARGIN and uv[:, 1].min() >= ref.MARGIN and uv[:, 1].max() <= 119 - ref.MARGIN
    assert (d[uv[:, 1], uv[:, 0]] != 0).all()
